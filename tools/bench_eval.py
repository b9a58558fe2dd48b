#!/usr/bin/env python3
"""Timing of the held-out evaluation path on the GPU (profiles/eval/eval_head.txt).

  * ops.eval_head (fused last layer + histogram + log loss) against the eager composition it
    replaces -- H.float() @ w + b + wide, two torch.histc, BCE-with-logits -- at B = 16384,
    Hd = 256 and 1024, on randn logits and on a skewed input (every logit in one bin: the
    hottest possible LDS / global bin). The two are timed alternately, device events around
    ``iters`` back-to-back calls, best and median of ``reps`` windows.
  * one WideDeep.evaluate batch against one training step of the same model (B = 16384, the
    benchmark's cardinalities), host clock around synchronised windows.

    python tools/bench_eval.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minips_amd import ops  # noqa: E402


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def _ab(fns: dict, iters=200, reps=9):
    for fn in fns.values():  # warm up every shape
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():  # alternating
            t[k].append(_window(fn, iters))
    return {k: (min(v), statistics.median(v)) for k, v in t.items()}


def bench_head(dev, out):
    NB = 4096
    B = 16384
    g = torch.Generator().manual_seed(0)
    for Hd in (256, 1024):
        for kind in ("randn", "one-bin"):
            H = torch.randn(B, Hd, generator=g)
            w = torch.randn(Hd, generator=g) / Hd ** 0.5
            if kind == "one-bin":
                H, w = torch.zeros(B, Hd), torch.zeros(Hd)
            H, w = H.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16)
            b0 = torch.tensor([0.25], dtype=torch.bfloat16, device=dev)
            wide = (torch.randn(B, generator=g) * (0.0 if kind == "one-bin" else 0.1)).to(dev)
            y = (torch.rand(B, generator=g) < 0.25).float().to(dev)
            acc = torch.zeros(2 * NB + 2, dtype=torch.int64, device=dev)
            z = torch.empty(B, device=dev)
            wf = w.float()

            def fused():
                ops.eval_head(H, w, b0, wide, y, acc)

            def eager():
                zz = H.float() @ wf + b0.float() + wide
                pos = y > 0.5
                zc = zz.clamp(-16, 16)
                torch.histc(zc[pos], NB, -16, 16)
                torch.histc(zc[~pos], NB, -16, 16)
                torch.nn.functional.binary_cross_entropy_with_logits(zz, y, reduction="sum")

            def hist_only():
                ops.binary_hist(z, y, acc)

            ops.eval_head(H, w, b0, wide, y, acc, z)
            r = _ab(dict(fused=fused, eager=eager, hist_only=hist_only))
            mb = B * Hd * 2 / 1e6
            out(f"eval_head B={B} Hd={Hd} {kind:8s} us/call (best, median): "
                + "  ".join(f"{k} {a:7.2f} {m:7.2f}" for k, (a, m) in r.items())
                + f"   [H = {mb:.1f} MB: fused reads it at {mb / r['fused'][0] * 1e3:.0f} GB/s]")


def bench_model(dev, out):
    from minips_amd.data.synthetic import CriteoSynth
    from minips_amd.models.widedeep import WideDeep, WideDeepConfig
    from minips_amd.ps.comm import Comm

    B = 16384
    cfg = WideDeepConfig()
    m = WideDeep(cfg, Comm(device=dev))
    data = CriteoSynth(B, cards=cfg.cards, device=dev, seed=0)
    held = data.holdout(1)
    batches = [data.next() for _ in range(8)]
    hb = [held.next() for _ in range(8)]

    def train():
        for b in batches:
            m.train_step(*b)

    def evaluate():
        m.evaluate(hb)  # (ends in the host copy of the accumulator: synchronised)

    for _ in range(3):
        train()
        evaluate()
    t = dict(train=[], evaluate=[])
    for _ in range(7):
        for k, fn in (("train", train), ("evaluate", evaluate)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3 / 8)
    m.drain()
    out(f"WideDeep B={B}, per batch, ms (best, median of 7 windows of 8 batches): "
        + "  ".join(f"{k} {min(v):.3f} {statistics.median(v):.3f}" for k, v in t.items())
        + "   [train: op-by-op train_step without the look-ahead feeder; evaluate: plan + Get + forward + "
          "eval_head, one reduce and host copy per 8 batches]")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU: timings are taken on the device only")
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/bench_eval.py on {torch.cuda.get_device_name(0)}")
    bench_head(dev, out)
    bench_model(dev, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
