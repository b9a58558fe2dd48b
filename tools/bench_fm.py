#!/usr/bin/env python3
"""Isolated timing of the factorization-machine kernels (ops.fm_forward / ops.fm_backward, csrc/kernels/fm.hip)
next to the eager torch composition of the same math (gather, multiply, index_add_ -- the CPU reference's
formula run on the GPU), in one process, on a CSR batch of `--batch` samples x `--nnz` lookups, k = `--k`,
with keys drawn uniformly or Zipf(`--zipf`) from `--features` ids (Zipf: a few rows own most of the lookups,
the backward's wave and workgroup paths).

Device-event time per call over `--iters` back-to-back calls, fused and eager alternated `--rounds` times.
Counted bytes, whole 64-byte lines (a gathered row or S row of W or k floats starts on a 16-byte boundary and
touches ceil(bytes / 64) lines, taken as the minimum; the streams are counted as they are):
  forward   per lookup: inv 8 + vals 4 + rowid 4 + one row of W floats; per sample: rowptr 8, labels 4,
            S 4 k, z / dz / loss 12
  backward  per lookup: members 4 + memrow 4 (twice: the two binary searches end in it) + rowid 4 + vals 4 +
            dz 4 (one line each when gathered: counted as 64) + one S row; per unique row: one row read, one
            gradient row written
    python tools/bench_fm.py [--batch 65536] [--nnz 64] [--k 16] [--iters 10] [--rounds 10]
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


def lines(nbytes):
    return (nbytes + 63) // 64 * 64


def draw_keys(kind, n, features, zipf, gen, dev):
    if kind == "uniform":
        return torch.randint(0, features, (n,), generator=gen, device=dev)
    # Zipf(s) over [1, features] by inverse transform of the continuous envelope x^-s
    u = torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    a = 1.0 - zipf
    x = ((features ** a - 1.0) * u + 1.0) ** (1.0 / a)
    return (x.long() - 1).clamp_(0, features - 1)


def eager_forward(rowptr, rowid, inv, vals, labels, rows, k, w0, gscale):
    B = labels.numel()
    p = rows[inv, :k] * vals[:, None]
    S = torch.zeros(B, k, device=rows.device).index_add_(0, rowid, p)
    Q = torch.zeros(B, device=rows.device).index_add_(0, rowid, (p * p).sum(1))
    lin = torch.zeros(B, device=rows.device).index_add_(0, rowid, rows[inv, k] * vals)
    z = w0 + lin + 0.5 * ((S * S).sum(1) - Q)
    y = (labels > 0.5).float()
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    return S, z, (torch.sigmoid(z) - y) * gscale, loss


def eager_backward(inv, rowid, vals, dz, S, rows, k, grad):
    c = dz[rowid] * vals
    grad.zero_()
    grad[:, :k].index_add_(0, inv, c[:, None] * (S[rowid] - rows[inv, :k] * vals[:, None]))
    grad[:, k].index_add_(0, inv, c)
    return grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--nnz", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--features", type=int, default=16_777_216)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, nnz, k = args.batch, args.nnz, args.k
    W, n = k + 4, B * nnz
    gen = torch.Generator(device=dev).manual_seed(0)
    for kind in ("uniform", "zipf"):
        keys = draw_keys(kind, n, args.features, args.zipf, gen, dev)
        uniq, inv = torch.unique(keys, return_inverse=True)
        U = uniq.numel()
        counts = torch.bincount(inv, minlength=U)
        rows = torch.randn(U, W, device=dev, generator=gen) * 0.01
        rows[:, k + 1:] = 0
        vals = torch.rand(n, device=dev, generator=gen)
        labels = (torch.rand(B, device=dev, generator=gen) < 0.5).float()
        rowptr = torch.arange(0, n + 1, nnz, device=dev, dtype=torch.int64)
        w0 = torch.zeros(1, device=dev)
        csr = ops.emb_build_csr(inv, 1, U)
        gscale = 1.0 / B
        S, z, dz, loss, rowid = ops.fm_forward(rowptr, inv, vals, labels, rows, k, w0, gscale)
        rowid64 = rowid.long()
        grad, grad_e = torch.empty(U, W, device=dev), torch.empty(U, W, device=dev)
        fns = {
            "fm_forward": lambda: ops.fm_forward(rowptr, inv, vals, labels, rows, k, w0, gscale),
            "eager_forward": lambda: eager_forward(rowptr, rowid64, inv, vals, labels, rows, k, w0, gscale),
            "fm_backward": lambda: ops.fm_backward(inv, rowid, vals, dz, S, rows, k, grad, csr=csr),
            "eager_backward": lambda: eager_backward(inv, rowid64, vals, dz, S, rows, k, grad_e),
        }
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the two compositions agree (reordered fp32 sums: to rounding)
        Se, ze, dze, _ = eager_forward(rowptr, rowid64, inv, vals, labels, rows, k, w0, gscale)
        agree = dict(z=float((z - ze).abs().max()), S=float((S - Se).abs().max()),
                     grad=float((grad - grad_e).abs().max()), grad_scale=float(grad_e.abs().max()))
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, args.iters))
        row_b, s_b = lines(4 * W), lines(4 * k)
        nbytes = {"fm_forward": n * (16 + row_b) + B * (24 + 4 * k),
                  "fm_backward": n * (12 + 3 * 64 + s_b) + U * (row_b + 4 * W)}
        nbytes["eager_forward"], nbytes["eager_backward"] = nbytes["fm_forward"], nbytes["fm_backward"]
        med = {name: statistics.median(ts) for name, ts in times.items()}
        print(json.dumps({"keys": kind, "batch": B, "nnz": nnz, "k": k, "lookups": n, "unique_rows": U,
                          "max_members": int(counts.max()), "rows_over_32": int((counts > 32).sum()),
                          "rows_over_2048": int((counts > 2048).sum()), "max_abs_diff": agree}), flush=True)
        for name, ts in times.items():
            print(json.dumps({"keys": kind, "kernel": name, "us_median": round(med[name], 1),
                              "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                              "spread": round((max(ts) - min(ts)) / med[name], 4),
                              "counted_gb_per_s": round(nbytes[name] / (med[name] * 1e-6) / 1e9, 1)}), flush=True)
        print(json.dumps({"keys": kind, "fused_pair_us": round(med["fm_forward"] + med["fm_backward"], 1),
                          "eager_pair_us": round(med["eager_forward"] + med["eager_backward"], 1),
                          "fused_faster": bool(med["fm_forward"] + med["fm_backward"]
                                               < med["eager_forward"] + med["eager_backward"])}), flush=True)
        del rows, grad, grad_e, S, keys, inv


if __name__ == "__main__":
    main()
