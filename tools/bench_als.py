#!/usr/bin/env python3
"""Isolated timing of the ALS kernels (ops.als_solve / als_gram, csrc/kernels/als.hip) next to the eager torch
composition of the same math (gather to [B, n, k], baddbmm for the Gram matrices, linalg.cholesky_ex,
cholesky_solve), in one process: one clock of `--entities` entities with `--per` lookups each (the user half) and one
clock of the item half of the same ratings with Zipf(`--zipf`) items, whose popular items take the multi-chunk path
(the eager composition pads every entity to the longest, so it runs the item half on the entities of at most 512
lookups only and its time there is a lower bound).

Device-event time per call over `--iters` back-to-back calls, fused and eager alternated `--rounds` times.
Counted work per clock: FLOPs n k^2 + k^3 / 3 an entity (n its lookups; a multiply-add counts 2: 2 n k^2 would be the
full SYRK, the lower triangle is half of it), bytes 4 k (n + 3) + 16 n an entity (gathered rows, old row, new row,
delta; inv, a, c).
    python tools/bench_als.py [--entities 4096] [--per 64] [--k 32] [--items 32768] [--iters 10] [--rounds 5]
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
from tools.bench_fm import draw_keys, timed  # noqa: E402


def eager_solve(rowptr, inv, a, c, rows, reg, slot, x_old, nmax):
    """The padded eager composition: [B, nmax, k] gathers and [B, k, k] Gram matrices in HBM."""
    B, k = rowptr.numel() - 1, rows.shape[1]
    ne = rowptr[1:] - rowptr[:-1]
    pos = torch.arange(nmax, device=rows.device)[None, :]
    live = pos < ne[:, None]
    j = (rowptr[:-1, None] + pos).clamp(max=inv.numel() - 1)
    Y = rows[inv[j]] * live[:, :, None]
    A = torch.baddbmm(torch.diag_embed(reg[:, None].expand(B, k)), (Y * a[j][:, :, None]).transpose(1, 2), Y)
    b = torch.bmm((c[j] * live)[:, None, :], Y).squeeze(1)
    L, _ = torch.linalg.cholesky_ex(A)
    x = torch.cholesky_solve(b[:, :, None], L).squeeze(2)
    return x, x - x_old[slot]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=4096)
    ap.add_argument("--per", type=int, default=64)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--items", type=int, default=32768)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--chunk", type=int, default=ops.ALS_CHUNK)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, per, k, I = args.entities, args.per, args.k, args.items
    gen = torch.Generator(device=dev).manual_seed(0)
    users_total = 32 * B  # the item half sees the ratings of 32 user batches
    cases = {}
    # user half: B users, per lookups each, over I item rows
    cases["users"] = (torch.arange(B + 1, device=dev) * per, draw_keys("zipf", B * per, I, args.zipf, gen, dev), I)
    # item half: the first B items of the transpose of users_total x per Zipf ratings (the popular ones)
    cols = draw_keys("zipf", users_total * per, I, args.zipf, gen, dev)
    cnt = torch.bincount(cols, minlength=I)[:B]
    rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(cnt, 0)
    cases["items"] = (rp, torch.randint(0, users_total, (int(rp[-1]),), device=dev, generator=gen), users_total)
    for side, (rowptr, keys, R) in cases.items():
        n = keys.numel()
        uniq, inv = torch.unique(keys, return_inverse=True)
        rows = torch.randn(uniq.numel(), k, device=dev, generator=gen) * k ** -0.25
        a = torch.ones(n, device=dev)
        c = torch.randn(n, device=dev, generator=gen)
        ne = rowptr[1:] - rowptr[:-1]
        reg = 0.05 * ne.float().clamp(min=1.0)
        slot = torch.randperm(B, device=dev, generator=gen)
        x_old = torch.randn(B, k, device=dev, generator=gen)
        x_out, delta = torch.empty_like(x_old), torch.empty_like(x_old)
        desc, multi, nmd = ops.als_chunks(rowptr.cpu(), args.chunk)
        chunks = (desc.to(dev), multi.to(dev), nmd)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"als_solve": lambda: ops.als_solve(rowptr, inv, a, c, rows, reg, slot, x_old, x_out, delta, chunks,
                                                  bad=bad)}
        small = ne <= min(args.chunk, 512)   # what the padded composition holds
        if side == "users" or bool(small.any()):
            keep = torch.nonzero(small).reshape(-1)
            srp = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=dev)
            srp[1:] = torch.cumsum(ne[keep], 0)
            eid = torch.repeat_interleave(torch.arange(B, device=dev), ne)
            sj = torch.nonzero(small[eid]).reshape(-1)
            nmax = int(ne[keep].max())
            eargs = (srp, inv[sj], a[sj], c[sj], rows, reg[keep], slot[keep], x_old, nmax)
            fns["eager_solve"] = lambda: eager_solve(*eargs)
        table = torch.randn(R, k, device=dev, generator=gen)
        fns["als_gram"] = lambda: ops.als_gram(table)
        fns["eager_gram"] = lambda: table.t() @ table
        for fn in fns.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        agree = {}
        if "eager_solve" in fns:
            xe, _ = fns["eager_solve"]()
            agree["x"] = float((x_out[slot[keep]] - xe).abs().max())
        agree["gram_rel"] = float(((ops.als_gram(table) - table.t() @ table).abs().max() / R))
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, args.iters))
        flops = float((ne.double() * k * k + k ** 3 / 3).sum())
        nbytes = float((4 * k * (ne.double() + 3) + 16 * ne.double()).sum())
        print(json.dumps({"side": side, "entities": B, "lookups": n, "k": k, "unique_rows": uniq.numel(),
                          "max_lookups": int(ne.max()), "multi_chunk_entities": int(multi.shape[0]),
                          "descriptors": int(desc.shape[0]), "eager_entities": int(small.sum()), "bad": int(bad),
                          "max_abs_diff": agree}), flush=True)
        for name, ts in times.items():
            med = statistics.median(ts)
            out = {"side": side, "kernel": name, "us_median": round(med, 1), "us_min": round(min(ts), 1),
                   "us_max": round(max(ts), 1), "spread": round((max(ts) - min(ts)) / med, 4)}
            if name == "als_solve":
                out.update(counted_gflop_per_s=round(flops / (med * 1e-6) / 1e9, 1),
                           counted_gb_per_s=round(nbytes / (med * 1e-6) / 1e9, 1))
            if name.endswith("gram"):
                out.update(counted_gflop_per_s=round(R * k * k / (med * 1e-6) / 1e9, 1),
                           counted_gb_per_s=round(4 * R * k / (med * 1e-6) / 1e9, 1))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
