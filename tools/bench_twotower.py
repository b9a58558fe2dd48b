#!/usr/bin/env python3
"""Isolated timing of the in-batch sampled softmax kernels (ops.ibs_forward / ibs_backward, csrc/kernels/ibs.hip) next
to the eager torch composition of the same math (gather, A B^T, masked log-softmax, G B and G^T A, index_add_), in one
process, at P in `--pairs` x d in `--dims`: users uniform over P ids, items Zipf(`--zipf`) over P / 4 ids (accidental
hits and hot item rows).

Device-event time per call over `--iters` back-to-back calls, fused and eager alternated `--rounds` times. Counted
FLOPs: 2 P^2 d forward, 8 P^2 d for the two gradient sweeps (each recomputes the logits and multiplies G).
    python tools/bench_twotower.py [--pairs 4096 16384] [--dims 32 64 128] [--iters 10] [--rounds 5] [--once]
`--once` runs each fused op a few times and exits (for a kernel trace).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minips_amd import ops  # noqa: E402
from tools.bench_fm import draw_keys, timed  # noqa: E402


def eager(inv, rows, d, tau, logq, gscale, cap):
    """The eager composition: three P x P matrices in HBM (logits, mask, gradient)."""
    P = inv.numel() // 2
    u, it = inv.view(P, 2)[:, 0], inv.view(P, 2)[:, 1]
    A, B = rows[u], rows[it]
    s = (A @ B.t()) / tau - logq[None, :]
    dead = (it[:, None] == it[None, :]) & ~torch.eye(P, dtype=torch.bool, device=rows.device)
    s = s.masked_fill(dead, -math.inf)
    lse = torch.logsumexp(s, 1)
    loss = lse - s.diagonal()
    G = torch.exp(s - lse[:, None])
    G.diagonal().sub_(1.0)
    G *= gscale / tau
    grad = torch.zeros(cap, d, device=rows.device)
    grad.index_add_(0, u, G @ B)
    grad.index_add_(0, it, G.t() @ A)
    return loss, lse, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--tau", type=float, default=0.25)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    for P in args.pairs:
        for d in args.dims:
            users = torch.randint(0, P, (P,), device=dev, generator=gen)
            items = P + draw_keys("zipf", P, max(P // 4, 1), args.zipf, gen, dev)
            uniq, inv = torch.unique(torch.stack([users, items], 1).reshape(-1), return_inverse=True)
            cap = uniq.numel()
            rows = torch.randn(cap, d, device=dev, generator=gen) * math.sqrt(0.5 / math.sqrt(d))
            logq = torch.randn(P, device=dev, generator=gen) * 0.5 - 3.0
            csr = ops.emb_build_csr(inv, 1, cap)[:2]
            gscale = 1.0 / P
            grad = torch.zeros(cap, d, device=dev)
            loss, lse = ops.ibs_forward(inv, rows, d, args.tau, logq)
            fns = {"ibs_forward": lambda: ops.ibs_forward(inv, rows, d, args.tau, logq),
                   "ibs_backward": lambda: ops.ibs_backward(inv, rows, d, args.tau, lse, grad, logq, gscale, csr=csr),
                   "eager_fwd_bwd": lambda: eager(inv, rows, d, args.tau, logq, gscale, cap)}
            if args.once:
                del fns["eager_fwd_bwd"]
            for fn in fns.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            if args.once:
                continue
            el, es, eg = fns["eager_fwd_bwd"]()
            agree = {"loss": float((loss - el).abs().max()),
                     "grad_rel": float((grad - eg).abs().max() / eg.abs().max())}
            times = {name: [] for name in fns}
            for _ in range(args.rounds):
                for name, fn in fns.items():
                    times[name].append(timed(fn, args.iters))
            print(json.dumps({"P": P, "d": d, "unique_rows": cap, "max_members": int(torch.bincount(inv).max()),
                              "max_abs_diff": agree}), flush=True)
            flops = {"ibs_forward": 2.0 * P * P * d, "ibs_backward": 8.0 * P * P * d, "eager_fwd_bwd": 6.0 * P * P * d}
            for name, ts in times.items():
                med = statistics.median(ts)
                print(json.dumps({"P": P, "d": d, "kernel": name, "us_median": round(med, 1),
                                  "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                                  "spread": round((max(ts) - min(ts)) / med, 4),
                                  "counted_tflop_per_s": round(flops[name] / (med * 1e-6) / 1e12, 2)}), flush=True)


if __name__ == "__main__":
    main()
