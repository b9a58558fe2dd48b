#!/usr/bin/env python3
"""Isolated timing of the Gaussian-mixture E-step (ops.gmm_estep, csrc/kernels/gmm.hip) next to the eager torch
composition of the same math (X * X, two matmuls for the scores, logsumexp, exp, three matmuls for the statistics; the
[n, K] responsibilities go through HBM), in one process: `--n` planted points at each `--shapes` K x D, both in fp32.

Device-event time per call over `--iters` back-to-back calls, fused and eager alternated `--rounds` times. Counted
work per call: FLOPs 8 n K D (two products of 2 n K (2D) each), bytes 4 n D (the points, read once).
    python tools/bench_gmm.py [--n 1048576] [--shapes 16x16,64x64,128x64] [--iters 10] [--rounds 5]

`--covariance full` times ops.gmm_full_estep (csrc/kernels/gmm_full.hip) on rotated planted points against its eager
composition (a batched matmul for the whitened residuals, logsumexp, an einsum for the weighted second moments).
Counted work per call: FLOPs 2 n K D^2 for the scores (the dense product; the kernel skips the tiles above the
diagonal) and 2 n K (D^2 + D) for the statistics (the full second moment; the kernel computes its lower triangle).
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
from minips_amd.data.synthetic import GMMSynth  # noqa: E402
from tools.bench_fm import timed  # noqa: E402


def eager_estep(X, shift, ca, cb, cst):
    x = X - shift
    xx = x * x
    t = cst + xx @ ca.t() + x @ cb.t()
    lse = torch.logsumexp(t, 1)
    r = torch.exp(t - lse[:, None])
    rt = r.t()
    return torch.cat([rt @ x, rt @ xx, rt @ torch.ones(X.shape[0], 1, device=X.device)], 1), lse.double().sum()


def eager_full_estep(X, shift, Wh, b, cst):
    x = X - shift
    y = torch.matmul(Wh, x.t()) - b[:, :, None]          # [K, D, n]
    t = (cst[:, None] - 0.5 * (y * y).sum(1)).t()
    lse = torch.logsumexp(t, 1)
    r = torch.exp(t - lse[:, None])
    S2 = torch.einsum("nk,nd,ne->kde", r, x, x)
    rt = r.t()
    return torch.cat([rt @ x, S2.reshape(S2.shape[0], -1), rt.sum(1, keepdim=True)], 1), lse.double().sum()


def setup_full(K, D, n, dev):
    """The operands and the three timed calls of the full-covariance E-step, and its counted FLOPs per call."""
    syn = GMMSynth(n, dims=D, K_teacher=K, sep=0.5, seed=1, device=dev, rotate=True)
    X = syn.next()
    shift = X.mean(0)
    mu = syn.centres - shift
    cov = torch.einsum("kde,ke,kfe->kdf", syn.rot, syn.sigma ** 2, syn.rot)
    cov = torch.tril(cov) + torch.tril(cov, -1).transpose(1, 2)
    s = torch.cat([mu, (cov + mu[:, :, None] * mu[:, None, :]).reshape(K, D * D), torch.ones(K, 1, device=dev)], 1)
    Wh, b, cst = ops.gmm_full_prepare((s * syn.weights[:, None]).contiguous(), 1e-6)
    We, be = Wh[:, :D, :D].contiguous(), b[:, :D].contiguous()
    fns = {"gmm_full_estep": lambda: ops.gmm_full_estep(X, shift, Wh, b, cst),
           "gmm_full_estep_predict": lambda: ops.gmm_full_estep(X, shift, Wh, b, cst, accumulate=False,
                                                                want_assign=True, want_logp=True),
           "eager": lambda: eager_full_estep(X, shift, We, be, cst)}
    return fns, {"predict": 2 * n * K * D * D, "full": 2 * n * K * D * D + 2 * n * K * (D * D + D)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--covariance", choices=["diag", "full"], default="diag")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--shapes", default="16x16,64x64,128x64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        K, D = (int(v) for v in shape.split("x"))
        if args.covariance == "full":
            fns, work = setup_full(K, D, args.n, dev)
            report(args, K, D, fns, "gmm_full_estep", work)
            continue
        syn = GMMSynth(args.n, dims=D, K_teacher=K, sep=0.5, seed=1, device=dev)
        X = syn.next()
        shift = X.mean(0)
        mu, var = syn.centres - shift, syn.sigma ** 2
        s = (torch.cat([mu, var + mu * mu, torch.ones(K, 1, device=dev)], 1) * syn.weights[:, None]).contiguous()
        coef, cst = ops.gmm_prepare(s, 1e-4)
        dp = ops.gmm_pad(D)
        ca, cb = coef[:, :D].contiguous(), coef[:, dp:dp + D].contiguous()
        fns = {"gmm_estep": lambda: ops.gmm_estep(X, shift, coef, cst),
               "gmm_estep_predict": lambda: ops.gmm_estep(X, shift, coef, cst, accumulate=False, want_assign=True,
                                                          want_logp=True),
               "eager": lambda: eager_estep(X, shift, ca, cb, cst)}
        report(args, K, D, fns, "gmm_estep", {"predict": 4 * args.n * K * D, "full": 8 * args.n * K * D})


def report(args, K, D, fns, fused, work):
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    S, ll = fns[fused]()[:2]
    Se, lle = fns["eager"]()
    agree = dict(S_rel=float((S - Se).abs().max() / Se.abs().max()), ll_rel=float((ll - lle).abs() / lle.abs()))
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, args.iters))
    print(json.dumps({"K": K, "D": D, "n": args.n, "max_rel_diff": agree}), flush=True)
    for name, ts in times.items():
        med = statistics.median(ts)
        flops = work["predict" if name.endswith("predict") else "full"]
        print(json.dumps({"K": K, "D": D, "kernel": name, "us_median": round(med, 1), "us_min": round(min(ts), 1),
                          "us_max": round(max(ts), 1), "spread": round((max(ts) - min(ts)) / med, 4),
                          "counted_gflop_per_s": round(flops / (med * 1e-6) / 1e9, 1),
                          "counted_gb_per_s": round(4 * args.n * D / (med * 1e-6) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
