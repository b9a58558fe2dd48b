#!/usr/bin/env python3
"""Isolated timings of the gradient-clipping kernels at a dense table's size (default: GPT-2 small):

  grad_sumsq            next to torch.linalg.vector_norm on the same tensor (what a user would write)
  adam_clip_apply       next to adam_apply (the clipping prologue folds the partial sums in every workgroup)

Device-event time per call over `--iters` back-to-back calls, the variants alternated `--rounds` times.
    python tools/bench_gradclip.py [--n 124475904] [--L 1024]
"""
from __future__ import annotations

import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=124_475_904, help="fp32 elements (GPT-2 small's padded table)")
    ap.add_argument("--L", default="256,512,1024", help="grad_sumsq workgroup counts")
    ap.add_argument("--bucket", type=int, default=7_087_872, help="elements of one layer bucket (GPT-2 small)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n // 4 * 4
    g = torch.randn(n, device=dev)
    w, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    wb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    Ls = [int(x) for x in args.L.split(",")]
    part = torch.zeros(max(Ls), dtype=torch.float64, device=dev)
    bucket = g[: args.bucket // 4 * 4]  # one GPT-2 layer's bucket: few workgroups on a small stream
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    variants = {f"grad_sumsq L={L}": (lambda L=L: ops.grad_sumsq(g, part, L)) for L in Ls}
    for L in (64, 128, 256, 315):
        variants[f"grad_sumsq bucket n={bucket.numel()} L={L}"] = lambda L=L: ops.grad_sumsq(bucket, part, L)
    variants["torch.linalg.vector_norm (fp32)"] = lambda: torch.linalg.vector_norm(g)
    variants["torch.linalg.vector_norm (dtype=float64)"] = lambda: torch.linalg.vector_norm(g, dtype=torch.float64)
    variants["adam_apply"] = lambda: ops.adam_apply(w, m, v, g, 1e-4, step=3, w_bf16=wb)
    for np_ in (512, 1024, 4096):
        p = torch.ones(np_, dtype=torch.float64, device=dev)
        variants[f"adam_clip_apply np={np_}"] = \
            lambda p=p: ops.adam_clip_apply(w, m, v, g, 1e-4, p, 1.0, stats, step=3, w_bf16=wb)
    nb = bucket.numel()
    variants["adam_apply bucket"] = lambda: ops.adam_apply(w[:nb], m[:nb], v[:nb], bucket, 1e-4, step=3, w_bf16=wb[:nb])
    for np_ in (1024, 2048, 4096):
        p = torch.ones(np_, dtype=torch.float64, device=dev)
        variants[f"adam_clip_apply bucket np={np_}"] = \
            lambda p=p: ops.adam_clip_apply(w[:nb], m[:nb], v[:nb], bucket, 1e-4, p, 1.0, stats, step=3, w_bf16=wb[:nb])
    times = {k: [] for k in variants}
    for fn in variants.values():  # warm up every variant
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    read = 4 * n
    adam = 4 * n * 7 + 2 * n  # 4 reads + 3 writes (+ the bf16 copy)
    for k, ts in times.items():
        nbytes = (adam if k.startswith("adam") else read) * (nb / n if "bucket" in k else 1.0)
        print(json.dumps({"kernel": k, "n": n, "us": [round(t, 1) for t in ts],
                          "tb_per_s": round(nbytes / (min(ts) * 1e-6) / 1e12, 3)}), flush=True)
    ops.grad_sumsq(g, part, Ls[-1])
    ref = float(torch.linalg.vector_norm(g, dtype=torch.float64))
    got = float(part[: Ls[-1]].sum()) ** 0.5
    print(json.dumps({"norm_grad_sumsq": got, "norm_torch_fp64": ref, "rel": abs(got - ref) / ref}))


if __name__ == "__main__":
    main()
