#!/usr/bin/env python3
"""Isolated timing of the three Deep & Cross kernels (ops.wd_cross_forward / wd_cross_backward / wd_cross_fold,
csrc/kernels/dcn.hip) on one Criteo-shaped batch of `--batch` samples x `--fields` lookups of `--dim` bf16 values
plus 13 dense features, X padded as the model pads it, `--layers` cross layers. The backward runs on dX in lookup
order (no perm) and in the planner's row-sorted order (perm = the position of every lookup in the lookup CSR).
Beside them, as yardsticks at the same shape in the same run: ops.wd_assemble (which writes the X they read) and
DeepFM's ops.wd_fm_forward / ops.wd_fm_backward.

Device-event time per call over `--iters` back-to-back calls, the arms alternated `--rounds` times; median and
min..max over the rounds. Counted bytes are whole 128-byte lines of every row a kernel must touch:
  cross forward   B lines(2 d) (X) + 4 B (L+1) (p) + 8 B (wide read and written)
  cross backward  B lines(2 d) (X) + 4 B F D (dX read and written) + 4 B (L+2) (p, dwide) + the partials
                  4 nchunks ((L+1) dp + 8) [+ 4 B F (perm)]
  fold            the partials read + 8 (2L+1) d (Gc read and written)
  fm forward      B lines(2 F D) (X) + 4 B D (S) + 8 B;  fm backward  B lines(2 F D) + 4 B F D + 4 B D + 4 B
    python tools/bench_dcn.py [--batch 16384] [--fields 26] [--dim 32] [--layers 3] [--iters 20] [--rounds 10]
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
    return (nbytes + 127) // 128 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    from minips_amd.data.synthetic import CRITEO_KAGGLE_CARDS, CriteoSynth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D, L = args.batch, args.fields, args.dim, args.layers
    W = D + 4
    cards = list(CRITEO_KAGGLE_CARDS)[:F] if F <= len(CRITEO_KAGGLE_CARDS) else [100000] * F
    dense, keys, _ = CriteoSynth(B, cards=cards, device=dev, seed=0).next()
    uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
    U = uniq.numel()
    g = torch.Generator(device=dev).manual_seed(1)
    rows = (torch.randn(U, W, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    d = F * D + dense.shape[1]
    dp = (d + 7) // 8 * 8
    ldx = (d + 1 + 63) // 64 * 64
    X = torch.zeros(B, ldx, dtype=torch.bfloat16, device=dev)
    wide = torch.zeros(B, device=dev)
    S = torch.empty(B, D, device=dev)
    dwide = torch.randn(B, generator=g, device=dev) / B
    dX = (torch.randn(B * F, D, generator=g, device=dev) / B).to(torch.bfloat16)
    members, _ = ops.emb_build_csr(inv, F, U)
    perm = ops.emb_csr_positions(members)
    Pc = torch.zeros(2 * L + 1, dp, dtype=torch.bfloat16, device=dev)
    Pc[0::2, :d] = ((torch.rand(L + 1, d, generator=g, device=dev) * 2 - 1) / d ** 0.5).to(torch.bfloat16)
    Pc[1::2, :d] = (0.01 * torch.randn(L, d, generator=g, device=dev)).to(torch.bfloat16)
    p = torch.empty(B, L + 1, device=dev)
    k = torch.empty(L + 1, device=dev)
    part = torch.empty(ops.wd_cross_part_shape(B, d, L), device=dev)
    Gc = torch.zeros(2 * L + 1, dp, device=dev)

    fns = {
        "wd_assemble": lambda: ops.wd_assemble(dense, rows, inv, F, D, X, wide, ones_col=d),
        "wd_fm_forward": lambda: ops.wd_fm_forward(X, F, D, wide, S),
        "wd_cross_forward": lambda: ops.wd_cross_forward(X, d, Pc, L, wide, p, k),
        "wd_fm_backward natural": lambda: ops.wd_fm_backward(X, S, dwide, dX, F, D),
        "wd_cross_backward natural": lambda: ops.wd_cross_backward(X, d, p, k, dwide, Pc, L, dX, F, D, part),
        "wd_fm_backward sorted": lambda: ops.wd_fm_backward(X, S, dwide, dX, F, D, perm=perm),
        "wd_cross_backward sorted": lambda: ops.wd_cross_backward(X, d, p, k, dwide, Pc, L, dX, F, D, part, perm=perm),
        "wd_cross_fold": lambda: ops.wd_cross_fold(part, Pc, d, L, Gc),
    }
    part_bytes = 4 * part.numel()
    fm_f = B * lines(2 * F * D) + 4 * B * D + 8 * B
    fm_b = B * lines(2 * F * D) + 4 * B * F * D + 4 * B * D + 4 * B
    cr_f = B * lines(2 * d) + 4 * B * (L + 1) + 8 * B
    cr_b = B * lines(2 * d) + 4 * B * F * D + 4 * B * (L + 2) + part_bytes
    counted = {"wd_fm_forward": fm_f, "wd_cross_forward": cr_f, "wd_fm_backward natural": fm_b,
               "wd_cross_backward natural": cr_b, "wd_fm_backward sorted": fm_b + 4 * B * F,
               "wd_cross_backward sorted": cr_b + 4 * B * F, "wd_cross_fold": part_bytes + 8 * (2 * L + 1) * d}
    for fn in fns.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, args.iters))
    print(f"B {B} F {F} D {D} n_dense {dense.shape[1]} d {d} ldx {ldx} L {L} chunks {part.shape[0]} partials "
          f"{part_bytes / 1e6:.2f} MB; {args.iters} calls x {args.rounds} rounds, us per call")
    out = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        tb = f"  {counted[name] / med / 1e6:6.2f} TB/s of {counted[name] / 1e6:.1f} MB counted" if name in counted \
            else ""
        print(f"  {name:26s} median {med:8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}{tb}")
        out[name] = dict(us=round(med, 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2),
                         **({"tb_s": round(counted[name] / med / 1e6, 3), "mb": round(counted[name] / 1e6, 2)}
                            if name in counted else {}))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    ratios = {"forward": med["wd_cross_forward"] / med["wd_fm_forward"],
              "backward natural": med["wd_cross_backward natural"] / med["wd_fm_backward natural"],
              "backward sorted": med["wd_cross_backward sorted"] / med["wd_fm_backward sorted"]}
    for name, r in ratios.items():
        print(f"  cross / fm {name:18s} {r:5.2f} x  (aim: at most 1.25)")
    print(json.dumps(dict(batch=B, fields=F, dim=D, d=d, ldx=ldx, layers=L, iters=args.iters, rounds=args.rounds,
                          kernels=out, ratios={n: round(r, 3) for n, r in ratios.items()})))


if __name__ == "__main__":
    main()
