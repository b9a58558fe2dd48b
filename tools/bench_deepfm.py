#!/usr/bin/env python3
"""Isolated timing of DeepFM's two kernels (ops.wd_fm_forward / ops.wd_fm_backward, csrc/kernels/deepfm.hip) on
one Criteo-shaped batch of `--batch` samples x `--fields` lookups of `--dim` bf16 values, X padded as the model
pads it. The backward runs on dX in lookup order (no perm) and in the planner's row-sorted order (perm = the
position of every lookup in the lookup CSR, what linear_dgrad(perm=...) writes). Beside them, as yardsticks on
the same batch in the same run: ops.wd_assemble (which writes the X the forward reads) and the row-wise Adagrad
apply of the batch's unique rows.

Device-event time per call over `--iters` back-to-back calls, the five ops alternated `--rounds` times; median
and min..max over the rounds. Counted bytes (what each kernel must move at least):
  forward   2 B F D (X) + 4 B D (S) + 8 B (wide read and written)
  backward  6 B F D (X read, dX read and written) + 4 B D (S, once per sample) + 4 B (dwide) + 4 B F (perm)
    python tools/bench_deepfm.py [--batch 16384] [--fields 26] [--dim 32] [--iters 20] [--rounds 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    from minips_amd.data.synthetic import CRITEO_KAGGLE_CARDS, CriteoSynth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, F, D = args.batch, args.fields, args.dim
    W = D + 4
    cards = list(CRITEO_KAGGLE_CARDS)[:F] if F <= len(CRITEO_KAGGLE_CARDS) else [100000] * F
    dense, keys, _ = CriteoSynth(B, cards=cards, device=dev, seed=0).next()
    uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
    U = uniq.numel()
    g = torch.Generator(device=dev).manual_seed(1)
    rows = (torch.randn(U, W, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    k_in = F * D + dense.shape[1]
    ldx = (k_in + 1 + 63) // 64 * 64
    X = torch.zeros(B, ldx, dtype=torch.bfloat16, device=dev)
    wide = torch.zeros(B, device=dev)
    S = torch.empty(B, D, device=dev)
    dwide = torch.randn(B, generator=g, device=dev) / B
    dX = (torch.randn(B * F, D, generator=g, device=dev) / B).to(torch.bfloat16)
    members, _ = ops.emb_build_csr(inv, F, U)
    perm = ops.emb_csr_positions(members)
    # the row-wise Adagrad apply of the batch's unique rows (split rows [D | 1 | 3], two accumulators)
    table = torch.randn(U, W, generator=g, device=dev) * 0.01
    st, st2 = torch.zeros(U, device=dev), torch.zeros(U, device=dev)
    ukeys = torch.arange(U, device=dev)
    grads = torch.randn(U, W, generator=g, device=dev) / B

    fns = {
        "wd_assemble": lambda: ops.wd_assemble(dense, rows, inv, F, D, X, wide, ones_col=k_in),
        "wd_fm_forward": lambda: ops.wd_fm_forward(X, F, D, wide, S),
        "wd_fm_backward natural": lambda: ops.wd_fm_backward(X, S, dwide, dX, F, D),
        "wd_fm_backward sorted": lambda: ops.wd_fm_backward(X, S, dwide, dX, F, D, perm=perm),
        "rowwise_adagrad": lambda: ops.sparse_rowwise_adagrad(table, st, ukeys, 0, grads, 0.02, state2=st2, split=D),
    }
    fwd_bytes = 2 * B * F * D + 4 * B * D + 8 * B
    bwd_bytes = 6 * B * F * D + 4 * B * D + 4 * B
    counted = {"wd_fm_forward": fwd_bytes, "wd_fm_backward natural": bwd_bytes,
               "wd_fm_backward sorted": bwd_bytes + 4 * B * F}
    for fn in fns.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.iters))
    print(f"B {B} F {F} D {D} ldx {ldx} unique rows {U}; {args.iters} calls x {args.rounds} rounds, us per call")
    out = {}
    for k, ts in times.items():
        med = statistics.median(ts)
        tb = f"  {counted[k] / med / 1e6:6.2f} TB/s of {counted[k] / 1e6:.1f} MB counted" if k in counted else ""
        print(f"  {k:24s} median {med:8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}{tb}")
        out[k] = dict(us=round(med, 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2),
                      **({"tb_s": round(counted[k] / med / 1e6, 3)} if k in counted else {}))
    print(json.dumps(dict(batch=B, fields=F, dim=D, ldx=ldx, unique_rows=U, iters=args.iters, rounds=args.rounds,
                          kernels=out)))


if __name__ == "__main__":
    main()
