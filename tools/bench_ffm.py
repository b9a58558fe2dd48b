#!/usr/bin/env python3
"""Isolated timing of the field-aware factorization-machine kernels (ops.ffm_forward / ops.ffm_backward,
csrc/kernels/ffm.hip) next to the eager torch composition of the same math (the CPU reference's formula run on
the GPU: a [B, F, F, k] gather, multiply, index_add_), and beside the FM kernels (ops.fm_forward /
ops.fm_backward, the same k) on the same batch, in one process: `--batch` samples with one feature per field,
`--fields` fields of `--card` ids, key = field * card + id, ids drawn uniformly or Zipf(`--zipf`).

Device-event time per call over `--iters` back-to-back calls, the kernels alternated `--rounds` times. Counted
gathered bytes (the slots the rule needs, nothing else): forward 2 * 4 k per pair, backward 4 k per (member,
partner) term plus the gradient rows written once.
    python tools/bench_ffm.py [--batch 16384] [--fields 26] [--k 4] [--card 262144] [--iters 10] [--rounds 10]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minips_amd import _native, ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def draw_ids(kind, n, card, zipf, gen, dev):
    if kind == "uniform":
        return torch.randint(0, card, (n,), generator=gen, device=dev)
    # Zipf(s) over [1, card] by inverse transform of the continuous envelope x^-s
    u = torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    a = 1.0 - zipf
    x = ((card ** a - 1.0) * u + 1.0) ** (1.0 / a)
    return (x.long() - 1).clamp_(0, card - 1)


def eager_forward(inv2, x2, labels, rows, F, k, w0, gscale, upper):
    """The regular batch (F lookups per sample, lookup f has field f): A[b, i, j] = v_{inv[b, i], j}."""
    cap = rows.shape[0]
    slots = rows[:, :F * k].reshape(cap * F, k)
    A = slots[inv2[:, :, None] * F + torch.arange(F, device=rows.device)[None, None, :]]
    P = (A * A.transpose(1, 2)).sum(-1) * (x2[:, :, None] * x2[:, None, :])
    z = w0 + (rows[inv2, F * k] * x2).sum(1) + (P * upper).sum((1, 2))
    y = (labels > 0.5).float()
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    return z, (torch.sigmoid(z) - y) * gscale, loss


def eager_backward(inv2, x2, dz, rows, F, k, grad, off):
    """Member i of row inv[b, i] receives, in slot j, c_i x_j v_{inv[b, j], i} for j != i."""
    cap = rows.shape[0]
    slots = rows[:, :F * k].reshape(cap * F, k)
    ar = torch.arange(F, device=rows.device)
    c = dz[:, None] * x2
    At = slots[inv2[:, None, :] * F + ar[None, :, None]]  # At[b, i, j] = v_{inv[b, j], i}
    T = At * ((c[:, :, None] * x2[:, None, :]) * off)[..., None]
    dst = (inv2[:, :, None] * F + ar[None, None, :]).expand(-1, F, F)
    acc = torch.zeros(cap * F, k, device=rows.device).index_add_(0, dst.reshape(-1), T.reshape(-1, k))
    grad.zero_()
    grad[:, :F * k] = acc.reshape(cap, F * k)
    grad[:, F * k].index_add_(0, inv2.reshape(-1), c.reshape(-1))
    return grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--card", type=int, default=262144)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,zipf")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    K_ = _native.ffmk()  # the member counts at which the backward switches paths
    B, F, k = args.batch, args.fields, args.k
    W, n = F * k + 4, B * F
    gen = torch.Generator(device=dev).manual_seed(0)
    upper = torch.triu(torch.ones(F, F, device=dev), diagonal=1)
    off = 1.0 - torch.eye(F, device=dev)
    for kind in args.kinds.split(","):
        ids = draw_ids(kind, n, args.card, args.zipf, gen, dev).reshape(B, F)
        keys = (ids + torch.arange(F, device=dev)[None, :] * args.card).reshape(-1)
        uniq, inv = torch.unique(keys, return_inverse=True)
        U = uniq.numel()
        counts = torch.bincount(inv, minlength=U)
        rows = torch.randn(U, W, device=dev, generator=gen) * 0.01
        rows[:, F * k + 1:] = 0
        vals = torch.rand(n, device=dev, generator=gen)
        fields = torch.arange(F, device=dev, dtype=torch.int32).repeat(B)
        labels = (torch.rand(B, device=dev, generator=gen) < 0.5).float()
        rowptr = torch.arange(0, n + 1, F, device=dev, dtype=torch.int64)
        w0 = torch.zeros(1, device=dev)
        csr = ops.emb_build_csr(inv, 1, U)
        gscale = 1.0 / B
        z, dz, loss, rowid = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, gscale)
        inv2, x2 = inv.reshape(B, F), vals.reshape(B, F)
        grad, grad_e = torch.empty(U, W, device=dev), torch.empty(U, W, device=dev)
        # the FM on the same lookups: rows of k + 4
        rows_fm = torch.randn(U, k + 4, device=dev, generator=gen) * 0.01
        S_fm, _, dz_fm, _, rowid_fm = ops.fm_forward(rowptr, inv, vals, labels, rows_fm, k, w0, gscale)
        grad_fm = torch.empty(U, k + 4, device=dev)
        fns = {
            "ffm_forward": lambda: ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, gscale),
            "eager_forward": lambda: eager_forward(inv2, x2, labels, rows, F, k, w0, gscale, upper),
            "ffm_backward": lambda: ops.ffm_backward(inv, rowid, rowptr, vals, fields, dz, rows, F, k, grad, csr=csr),
            "eager_backward": lambda: eager_backward(inv2, x2, dz, rows, F, k, grad_e, off),
            "fm_forward": lambda: ops.fm_forward(rowptr, inv, vals, labels, rows_fm, k, w0, gscale),
            "fm_backward": lambda: ops.fm_backward(inv, rowid_fm, vals, dz_fm, S_fm, rows_fm, k, grad_fm, csr=csr),
        }
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ze, _, _ = eager_forward(inv2, x2, labels, rows, F, k, w0, gscale, upper)
        agree = dict(z=float((z - ze).abs().max()), grad=float((grad - grad_e).abs().max()),
                     grad_scale=float(grad_e.abs().max()))
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, args.iters))
        pairs = B * F * (F - 1) // 2
        nbytes = {"ffm_forward": pairs * 2 * 4 * k, "ffm_backward": 2 * pairs * 4 * k + U * W * 4}
        med = {name: statistics.median(ts) for name, ts in times.items()}
        print(json.dumps({"keys": kind, "batch": B, "fields": F, "k": k, "lookups": n, "unique_rows": U, "pairs": pairs,
                          "max_members": int(counts.max()),
                          "rows_over_group_max": int((counts > K_.GROUP_MAX).sum()),
                          "rows_over_wave_max": int((counts > K_.WAVE_MAX).sum()), "max_abs_diff": agree}), flush=True)
        for name, ts in times.items():
            rec = {"keys": kind, "kernel": name, "us_median": round(med[name], 1), "us_min": round(min(ts), 1),
                   "us_max": round(max(ts), 1), "spread": round((max(ts) - min(ts)) / med[name], 4)}
            if name in nbytes:
                rec["gathered_gb_per_s"] = round(nbytes[name] / (med[name] * 1e-6) / 1e9, 1)
            print(json.dumps(rec), flush=True)
        fused, eager = med["ffm_forward"] + med["ffm_backward"], med["eager_forward"] + med["eager_backward"]
        print(json.dumps({"keys": kind, "fused_pair_us": round(fused, 1), "eager_pair_us": round(eager, 1),
                          "eager_over_fused": round(eager / fused, 2),
                          "forward_ratio": round(med["eager_forward"] / med["ffm_forward"], 2),
                          "backward_ratio": round(med["eager_backward"] / med["ffm_backward"], 2),
                          "fm_pair_us": round(med["fm_forward"] + med["fm_backward"], 1)}), flush=True)
        del rows, grad, grad_e, keys, inv, rows_fm, grad_fm


if __name__ == "__main__":
    main()
