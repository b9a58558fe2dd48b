#!/usr/bin/env python3
"""K-Means' fused step beside the classic composition, one shape a line (README "K-Means: fused step").

For every (K, D) at --n points: ops.km_nearest, ops.km_sums and the classic composition (ops.kmeans_assign(mfma=True) +
scatter_add_rows + bincount), alternated round by round in one run and timed by device events. Prints the median and
the min .. max spread of each in ms, the fused sweep's rate counting 2 n K D FLOPs, and whether the two paths agree on
the assignment. A GPU is required: there is no CPU timing.

  python tools/bench_kmeans.py --n 65536 --shapes 16x16,100x128,1000x128,4096x256 --rounds 30
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


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stat(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="16x16,100x128,1000x128,4096x256", help="K x D, comma separated")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans: needs a GPU")
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        K, D = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(K * 1000 + D)
        C = 3 * torch.randn(K, D, generator=g, device=dev)
        X = C[torch.randint(0, K, (args.n,), generator=g, device=dev)] + 0.5 * torch.randn(args.n, D, generator=g,
                                                                                             device=dev)

        def classic():
            dist = torch.empty(args.n, dtype=torch.float32, device=dev)
            assign = ops.kmeans_assign(X, C, dist=dist, mfma=True)
            idx = assign.to(torch.int64)
            sums = torch.zeros(K, D, dtype=torch.float32, device=dev)
            ops.scatter_add_rows(X, idx, sums)
            return assign, sums, torch.bincount(idx, minlength=K)

        ts = dict(km_nearest=[], km_sums=[], classic=[])
        for r in range(args.warmup + args.rounds):
            tn, (assign, _, _, _) = _timed(lambda: ops.km_nearest(X, C))
            tsum, (sums, counts) = _timed(lambda: ops.km_sums(X, assign, K))
            tc, (assign_c, sums_c, counts_c) = _timed(classic)
            if r >= args.warmup:
                ts["km_nearest"].append(tn), ts["km_sums"].append(tsum), ts["classic"].append(tc)
        out = dict(n=args.n, K=K, D=D, rounds=args.rounds, **{k: _stat(v) for k, v in ts.items()})
        out["fused_ms"] = round(out["km_nearest"]["median_ms"] + out["km_sums"]["median_ms"], 4)
        out["km_nearest_tflops"] = round(2.0 * args.n * K * D / (out["km_nearest"]["median_ms"] * 1e-3) / 1e12, 2)
        out["assign_agree"] = round(float((assign == assign_c).float().mean()), 6)
        out["sums_maxdiff"] = float((sums - sums_c).abs().max())
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
