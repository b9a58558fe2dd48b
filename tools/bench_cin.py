#!/usr/bin/env python3
"""Isolated timing of the CIN kernels (ops.wd_cin_*, csrc/kernels/cin.hip) against the eager PyTorch composition --
the einsum that materialises Z [B, H_{k-1} m, D] per layer, and autograd's backward of it -- on random bf16 inputs
of `--batch` samples x `--fields` embeddings of `--dim`, `--layers` feature maps. Both arms run in one process,
alternated `--rounds` times; device-event time per call over `--iters` back-to-back calls, median and min..max over
the rounds. Counted FLOPs per layer, 2 per multiply-add: forward 2 B D H_k H_{k-1} m; data backward twice that plus
the two contractions 4 B D H_{k-1} m; weight gradient 2 B D H_k H_{k-1} m. An eager arm that runs out of memory is
reported as such; the fused side is never shrunk.
The eager arm's gradients are dropped before every call, and dX and the gradient block are cleared before every timed
run of an arm (the fused backward and the folds add into them).
    python tools/bench_cin.py [--batch 16384] [--fields 26] [--dim 32] [--layers 64,64] [--iters 5] [--rounds 5]
    python tools/bench_cin.py --losses     # |CPU - GPU| of the mean loss over six steps of a small model, with and
                                           # without the CIN, the DeepFM term and a cross layer
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minips_amd import ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def eager_step(x0, Ws, w_out, dz):
    """Forward and backward of the CIN term in eager bf16 PyTorch (Z materialised per layer)."""
    B, m, D = x0.shape
    for t in (x0, w_out, *Ws):
        t.grad = None
    xp, pooled = x0, []
    for W in Ws:
        z = (xp[:, :, None, :] * x0[:, None, :, :]).reshape(B, -1, D)  # [B, Hp m, D]
        xp = torch.matmul(W.reshape(W.shape[0], -1), z)                # [B, H, D]
        pooled.append(xp.float().sum(2))
    out = torch.cat(pooled, 1) @ w_out.float()
    out.backward(dz)
    return out


def loss_table(steps=6, B=320):
    """profiles/cin/cpu_vs_gpu_losses.txt: the same batches on the CPU references and on the GPU kernels."""
    from minips_amd.data.synthetic import CriteoSynth
    from minips_amd.models.widedeep import WideDeep, WideDeepConfig
    from minips_amd.ps.comm import Comm

    cards = [100, 50, 3000, 7, 300, 20, 5, 60, 90, 10, 11, 12]

    def run(device, cin, fm, cross):
        m = WideDeep(WideDeepConfig(cards=cards, hidden=(128, 64, 64), emb_dim=16, row_width=20, cin_layers=cin,
                                    fm_term=fm, cross_layers=cross), Comm(device=torch.device(device)))
        data = CriteoSynth(B, cards=cards, device="cpu", seed=3)
        return [float(m.train_step(*(t.to(device) for t in data.next())).item()) / B for _ in range(steps)]

    for name, cin, fm, cross in (("cin+fm+cross", (32, 16), True, 1), ("fm+cross only", (), True, 1),
                                 ("cin only", (32, 16), False, 0), ("plain", (), False, 0)):
        diffs = [abs(a - b) for a, b in zip(run("cpu", cin, fm, cross), run("cuda:0", cin, fm, cross))]
        print(name, ["%.1e" % d for d in diffs], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--layers", default="64,64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--losses", action="store_true")
    args = ap.parse_args()
    if args.losses:
        return loss_table()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D = args.batch, args.fields, args.dim
    layers = tuple(int(h) for h in args.layers.split(","))
    g = torch.Generator().manual_seed(0)
    X = torch.randn(B, F * D + 64, generator=g).to(torch.bfloat16).to(dev)
    n = ops.wd_cin_layout(F, layers)[1]
    Pc = torch.zeros(n, dtype=torch.bfloat16)
    Ws, w_out = ops.wd_cin_views(Pc, F, layers)
    for W in Ws:
        W[:, :, :F] = (torch.randn(W.shape[0], W.shape[1], F, generator=g) / (W.shape[1] * F) ** 0.5).to(torch.bfloat16)
    w_out.copy_(torch.randn(sum(layers), generator=g).to(torch.bfloat16))
    Pc = Pc.to(dev)
    Ws, w_out = ops.wd_cin_views(Pc, F, layers)
    dz = torch.randn(B, generator=g).to(dev)
    bufs = ops.wd_cin_buffers(B, F, D, layers, dev)
    wide, dX, Gc = torch.zeros(B, device=dev), torch.zeros(B * F, D, dtype=torch.bfloat16, device=dev), torch.zeros(
        n, device=dev)
    nch = ops.wd_cin_nchunks(B)
    hps = (F,) + layers[:-1]
    arms, flops = {}, {}
    for k, (H, hp) in enumerate(zip(layers, hps), 1):
        W = Ws[k - 1]
        part = bufs["part"][: nch * W.numel()].view(nch, H, hp * W.shape[2])
        mac = 2.0 * B * D * H * hp * F
        arms[f"fwd{k}"] = lambda W=W, k=k: ops.wd_cin_layer_forward(X, F, D, W, layers, k, bufs["XK"])
        arms[f"bwd{k}"] = lambda W=W, k=k: ops.wd_cin_layer_backward(X, F, D, W, layers, k, bufs["XK"], bufs["dXK"],
                                                                     w_out, dz, bufs["g0"], dX)
        arms[f"wgrad{k}"] = lambda k=k, part=part: ops.wd_cin_layer_wgrad(X, F, D, layers, k, bufs["XK"], bufs["dXK"],
                                                                          w_out, dz, part)
        arms[f"fold{k}"] = lambda k=k, part=part: ops.wd_cin_fold(part, ops.wd_cin_views(Gc, F, layers)[0][k - 1])
        flops.update({f"fwd{k}": mac, f"bwd{k}": mac + 4.0 * B * D * hp * F, f"wgrad{k}": mac})
    arms["output"] = lambda: ops.wd_cin_output(bufs["XK"], w_out, wide, bufs["p"])
    arms["fused_step"] = lambda: (ops.wd_cin_forward(X, F, D, Pc, layers, wide, bufs),
                                  ops.wd_cin_backward(X, F, D, Pc, layers, dz, dX, bufs, Gc))
    flops["fused_step"] = sum(v for k, v in flops.items())
    x0 = X[:, : F * D].reshape(B, F, D).clone().requires_grad_(True)
    We = [W[:, :, :F].clone().requires_grad_(True) for W in Ws]
    woe = w_out.clone().requires_grad_(True)
    eager_ok = True
    try:
        eager_step(x0, We, woe, dz)
        torch.cuda.synchronize()
        arms["eager_step"] = lambda: eager_step(x0, We, woe, dz)
        flops["eager_step"] = flops["fused_step"]
    except torch.OutOfMemoryError as e:
        eager_ok = False
        print(f"eager arm: out of memory ({str(e).splitlines()[0]})")
        torch.cuda.empty_cache()
    for fn in arms.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            dX.zero_(), Gc.zero_()
            times[k].append(timed(fn, args.iters))
    res = {}
    for k, ts in times.items():
        med = statistics.median(ts)
        res[k] = dict(us=round(med, 1), min=round(min(ts), 1), max=round(max(ts), 1),
                      **({"tflops": round(flops[k] / med / 1e6, 1)} if k in flops else {}))
        print(f"{k:11s} {med:10.1f} us  ({min(ts):.1f} .. {max(ts):.1f})"
              + (f"  {flops[k] / med / 1e6:7.1f} TFLOP/s counted" if k in flops else ""))
    print(json.dumps(dict(batch=B, fields=F, dim=D, layers=list(layers), eager="ran" if eager_ok else "out of memory",
                          **res)))


if __name__ == "__main__":
    main()
