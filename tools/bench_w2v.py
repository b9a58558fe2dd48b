#!/usr/bin/env python3
"""Isolated timing of the skip-gram negative-sampling kernels (ops.sgns_lookups / sgns_forward / sgns_backward,
csrc/kernels/sgns.hip) next to the eager torch composition of the same math (the integer draws as int64 tensor
arithmetic; gather, multiply, reduce, index_add_ -- the CPU references' formulas run on the GPU), in one process,
on `--pairs` pairs with `--negatives` negatives of `--dim` floats, with centre and context words drawn uniformly
or Zipf(`--zipf`) from `--vocab` words (Zipf: a few rows own most of the lookups -- the backward's wave and
workgroup paths; the negatives follow the unigram^0.75 of the same counts).

Device-event time per call over `--iters` back-to-back calls, fused and eager alternated `--rounds` times.
Counted bytes (the minimum a pass has to move; a gathered row of d floats is 4 d bytes, whole 64-byte lines):
  lookups   per pair: centre 8 + context 8 + keys 8 (N + 2); per draw: thr 8 + alias 4 (one line each: 128)
  forward   per pair: inv 8 (N + 2) + (N + 2) rows + e 4 (N + 1) + loss 4 + h 4 d
  backward  per lookup: members 4 + memrow 4 + inv 8 + e 4 (one line each when gathered: 64) + one row (v or h);
            per unique row: one gradient row written
    python tools/bench_w2v.py [--pairs 65536] [--negatives 5] [--dim 128] [--iters 10] [--rounds 10]
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
from tools.bench_fm import draw_keys, lines, timed  # noqa: E402


def eager_lookups(cen, ctx, thr, alias, T, seed, epoch, pair_base, N):
    P, V = cen.numel(), thr.numel()
    base = ops.lda_mix_int(seed + epoch * 0x9E3779B97F4A7C15)
    base = base - (1 << 64) if base >> 63 else base
    g = torch.arange(P, dtype=torch.int64, device=cen.device) + pair_base
    r = ops._lda_mix((g[:, None] * 64 + torch.arange(N, dtype=torch.int64, device=cen.device)[None, :]) ^ base)
    i = ops.mulhi_u64(r, torch.full_like(r, V))
    x = ops.mulhi_u64(ops._lda_mix(r), torch.full_like(r, T))
    neg = torch.where(x < thr[i], i, alias[i].long())
    return torch.cat([2 * cen[:, None], 2 * ctx[:, None] + 1, 2 * neg + 1], 1)


def eager_forward(inv, rows, N, gscale):
    iv = inv.view(-1, N + 2)
    a, b = iv[:, 0], iv[:, 1:]
    va, u = rows[a], rows[b]
    s = torch.bmm(u, va[:, :, None]).squeeze(2)
    live = torch.ones_like(s)
    live[:, 1:] = (b[:, 1:] != b[:, :1]).float()
    y = torch.zeros_like(s)
    y[:, 0] = 1
    e = (torch.sigmoid(s) - y) * gscale * live
    loss = ((s.clamp(min=0) - s * y + torch.log1p(torch.exp(-s.abs()))) * live).sum(1)
    h = torch.bmm(e[:, None, :], u).squeeze(1)
    return e, loss, h


def eager_backward(inv, e, h, rows, N, grad):
    iv = inv.view(-1, N + 2)
    a, b = iv[:, 0], iv[:, 1:]
    grad.zero_()
    grad.index_add_(0, a, h)
    grad.index_add_(0, b.reshape(-1), (e[:, :, None] * rows[a][:, None, :]).reshape(-1, rows.shape[1]))
    return grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1 << 20)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    P, N, d, V = args.pairs, args.negatives, args.dim, args.vocab
    K2, n = N + 2, P * (N + 2)
    gen = torch.Generator(device=dev).manual_seed(0)
    for kind in ("uniform", "zipf"):
        cen, ctx = draw_keys(kind, P, V, args.zipf, gen, dev), draw_keys(kind, P, V, args.zipf, gen, dev)
        # the corpus the pairs came from: 256 draws of the same law per pair
        counts = torch.bincount(draw_keys(kind, 256 * P, V, args.zipf, gen, dev), minlength=V) + 1
        thr, alias, T, _ = ops.sgns_alias(counts.cpu())
        thr, alias = thr.to(dev), alias.to(dev)
        keys = ops.sgns_lookups(cen, ctx, thr, alias, T, 1, 0, 0, N)
        same = bool(torch.equal(keys, eager_lookups(cen, ctx, thr, alias, T, 1, 0, 0, N)))
        uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
        U = uniq.numel()
        members = torch.bincount(inv, minlength=U)
        group_max, wave_max = _native.w2vk().GROUP_MAX, _native.w2vk().WAVE_MAX  # the backward's switches
        rows = torch.randn(U, d, device=dev, generator=gen) * d ** -0.25
        csr = ops.emb_build_csr(inv, 1, U)
        gscale = 1.0 / P
        e, loss, h = ops.sgns_forward(inv, rows, N, gscale)
        grad, grad_e = torch.empty(U, d, device=dev), torch.empty(U, d, device=dev)
        fns = {
            "sgns_lookups": lambda: ops.sgns_lookups(cen, ctx, thr, alias, T, 1, 0, 0, N),
            "eager_lookups": lambda: eager_lookups(cen, ctx, thr, alias, T, 1, 0, 0, N),
            "sgns_forward": lambda: ops.sgns_forward(inv, rows, N, gscale),
            "eager_forward": lambda: eager_forward(inv, rows, N, gscale),
            "sgns_backward": lambda: ops.sgns_backward(inv, e, h, rows, N, grad, csr=csr),
            "eager_backward": lambda: eager_backward(inv, e, h, rows, N, grad_e),
        }
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the two compositions agree (reordered fp32 sums: to rounding)
        ee, le, he = eager_forward(inv, rows, N, gscale)
        agree = dict(lookups_equal=same, e=float((e - ee).abs().max()), loss=float((loss - le).abs().max()),
                     h=float((h - he).abs().max()), grad=float((grad - grad_e).abs().max()),
                     grad_scale=float(grad_e.abs().max()))
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, args.iters))
        row_b = lines(4 * d)
        nbytes = {"sgns_lookups": P * (16 + 8 * K2) + P * N * 128,
                  "sgns_forward": P * (8 * K2 + K2 * row_b + 4 * (N + 1) + 4 + 4 * d),
                  "sgns_backward": n * (8 + 2 * 64 + row_b) + U * 4 * d}
        for k in ("lookups", "forward", "backward"):
            nbytes["eager_" + k] = nbytes["sgns_" + k]
        med = {name: statistics.median(ts) for name, ts in times.items()}
        print(json.dumps({"words": kind, "pairs": P, "negatives": N, "dim": d, "vocab": V, "lookups": n,
                          "unique_rows": U, "max_members": int(members.max()),
                          "rows_over_group_max": int((members > group_max).sum()),
                          "rows_over_wave_max": int((members > wave_max).sum()), "wave_max": wave_max,
                          "max_abs_diff": agree}), flush=True)
        for name, ts in times.items():
            print(json.dumps({"words": kind, "kernel": name, "us_median": round(med[name], 1),
                              "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                              "spread": round((max(ts) - min(ts)) / med[name], 4),
                              "counted_gb_per_s": round(nbytes[name] / (med[name] * 1e-6) / 1e9, 1)}), flush=True)
        fused = sum(med["sgns_" + k] for k in ("lookups", "forward", "backward"))
        eager = sum(med["eager_" + k] for k in ("lookups", "forward", "backward"))
        print(json.dumps({"words": kind, "fused_us": round(fused, 1), "eager_us": round(eager, 1),
                          "fused_faster": bool(fused < eager)}), flush=True)
        del rows, grad, grad_e, e, h, keys, inv


if __name__ == "__main__":
    main()
