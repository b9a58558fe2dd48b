#!/usr/bin/env python
"""AutoInt's kernels on one GPU: every wd_attn_* kernel per layer (device-event median, min .. max, counted TFLOP/s),
the fused forward + backward of the term, and beside them the eager PyTorch composition of the same rule on GPU
tensors (bf16 matmuls, fp32 softmax, autograd backward), the two arms alternated in one process.

  python tools/bench_attn.py --batch 16384 --layers 3 --heads 2 --dim 32 [--fields 26 --emb 32 --reps 20]

FLOPs are counted from the shapes (2 per multiply-add), once per product of the rule: forward per sample and layer
2 m Din 4A (projections) + 2 . 2 m m A (scores, P V); backward 2 m Din 4A (dE) + 2 m Din 4A (dW) + 4 . 2 m m A
(dV, dP, dQ, dK) -- the recomputation and the second orientation of a product are not counted as useful work."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minips_amd import ops  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def eager_term(X, Ws, w_out, F, D, H, d):
    """The same rule in eager PyTorch: bf16 operands, fp32 softmax; returns the wide term [B]."""
    B, A = X.shape[0], H * d
    E = X[:, : F * D].view(B, F, D)
    for W in Ws:
        Y = E @ W
        Q, K, V = (Y[..., i * A:(i + 1) * A].view(B, F, H, d).transpose(1, 2) for i in range(3))
        P = torch.softmax((Q @ K.transpose(-1, -2)).float(), -1).to(torch.bfloat16)
        E = torch.relu((P @ V).transpose(1, 2).reshape(B, F, A) + Y[..., 3 * A:])
    return E.reshape(B, -1).float() @ w_out.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--emb", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, F, D, cfg = a.batch, a.fields, a.emb, (a.layers, a.heads, a.dim)
    T, H, d = ops.wd_attn_check(F, D, cfg)
    A = H * d
    g = torch.Generator().manual_seed(0)
    n = ops.wd_attn_layout(F, D, cfg)[1]
    Pc = torch.zeros(n, dtype=torch.bfloat16)
    Ws, w_out = ops.wd_attn_views(Pc, F, D, cfg)
    for W in Ws:
        W.copy_(torch.randn(W.shape, generator=g) / W.shape[0] ** 0.5)
    w_out.copy_(torch.randn(w_out.shape, generator=g) / w_out.numel() ** 0.5)
    Pc = Pc.to(dev)
    Ws, w_out = ops.wd_attn_views(Pc, F, D, cfg)
    X = torch.randn(B, F * D + 13, generator=g).to(torch.bfloat16).to(dev)
    dwide, wide = torch.randn(B, generator=g).to(dev), torch.zeros(B, device=dev)
    dX, Gc = torch.zeros(B * F, D, dtype=torch.bfloat16, device=dev), torch.zeros(n, device=dev)
    bufs = ops.wd_attn_buffers(B, F, D, cfg, dev)
    nch, Gs = ops.wd_attn_nchunks(B), ops.wd_attn_views(Gc, F, D, cfg)[0]
    ops.wd_attn_forward(X, F, D, Pc, cfg, wide, bufs)
    rows = []

    def row(name, fn, flops):
        med, lo, hi = timed(fn, a.reps)
        rows.append(dict(kernel=name, ms=round(med, 4), min=round(lo, 4), max=round(hi, 4),
                         tflops=round(flops / med / 1e9, 2) if flops else None))

    for l in range(1, T + 1):
        din, W = (D if l == 1 else A), Ws[l - 1]
        part = bufs["part"][: nch * W.numel()].view(nch, W.shape[0], W.shape[1])
        row(f"attn_fwd l={l}", lambda: ops.wd_attn_layer_forward(X, F, D, W, cfg, l, bufs["EK"]),
            B * (2 * F * din * 4 * A + 4 * F * F * A))
        row(f"attn_bwd l={l}", lambda: ops.wd_attn_layer_backward(X, F, D, W, cfg, l, bufs["EK"], bufs["dEK"], w_out,
                                                                  dwide, dX, part),
            B * (4 * F * din * 4 * A + 8 * F * F * A))
        row(f"attn_fold l={l}", lambda: ops.wd_attn_fold(part, Gs[l - 1]), 0)
    row("attn_out", lambda: ops.wd_attn_output(bufs["EK"], d, w_out, wide), 2 * B * F * A)
    row("attn_wout", lambda: ops.wd_attn_wout_partial(bufs["EK"], d, dwide, bufs["part_o"]), 2 * B * F * A)

    def fused():
        ops.wd_attn_forward(X, F, D, Pc, cfg, wide, bufs)
        ops.wd_attn_backward(X, F, D, Pc, cfg, dwide, dX, bufs, Gc)

    Xe = X.clone().requires_grad_()
    We, woe = [W.clone().requires_grad_() for W in Ws], w_out.clone().requires_grad_()

    def eager():
        Xe.grad = None
        eager_term(Xe, We, woe, F, D, H, d).backward(dwide)

    arms = {"fused": [], "eager": []}
    for _ in range(3):  # alternated
        arms["fused"].append(timed(fused, a.reps)[0])
        arms["eager"].append(timed(eager, a.reps)[0])
    for r in rows:
        print(json.dumps(r))
    print(json.dumps(dict(B=B, F=F, D=D, cfg=cfg, fused_fwd_bwd_ms=[round(t, 4) for t in arms["fused"]],
                          eager_fwd_bwd_ms=[round(t, 4) for t in arms["eager"]])))


if __name__ == "__main__":
    main()
