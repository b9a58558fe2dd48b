#!/usr/bin/env python3
"""Isolated timing of the split-row apply with two rules (ops.sparse_adagrad_ftrl, csrc/kernels/wideftrl.hip)
next to the row-wise Adagrad apply it stands in for (ops.sparse_rowwise_adagrad with split 32, width 36), in
one process, on the unique routed keys of one Wide & Deep batch (CriteoSynth, default cards) over a table
of the model's size.

Device-event time per call over `--iters` back-to-back calls, the two kernels alternated `--rounds` times.
Counted bytes per row, in whole 64-byte lines: the Adagrad moves 448 (g 144, w 2 x 144, two 4-byte states read
and written), the new kernel 504 (the same without state2, plus 2 x 32 of zn). The yardstick of the new
kernel is the Adagrad's time x 504 / 448, widened by the spread of the Adagrad's own rounds.
    python tools/bench_wideftrl.py [--batch 16384] [--iters 20] [--rounds 30]
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

ADAGRAD_BYTES, WIDE_BYTES = 448, 504


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def main():
    from minips_amd.data.synthetic import CRITEO_KAGGLE_CARDS, CriteoSynth
    from minips_amd.ps.tables import _route_multiplier

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--l1", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, D1 = 36, 32
    cards = list(CRITEO_KAGGLE_CARDS)
    rows = int(sum(cards))
    raw = CriteoSynth(args.batch, cards=cards, device=dev, seed=0).next()[1]
    keys = torch.unique((raw.reshape(-1) * _route_multiplier(rows)) % rows)  # the table's "mix" placement, sorted
    n = keys.numel()
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(rows, W, device=dev, generator=gen) * 0.01
    table[:, D1:] = 0
    state, state2 = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
    zn = torch.zeros(rows, 2 * (W - D1), device=dev)
    g = torch.randn(n, W, device=dev, generator=gen) * (1.0 / args.batch)
    g[:, D1 + 1:] = 0
    fns = {
        "sparse_rowwise_adagrad": lambda: ops.sparse_rowwise_adagrad(table, state, keys, 0, g, 0.02, 1e-8,
                                                                     state2=state2, split=D1),
        "sparse_adagrad_ftrl": lambda: ops.sparse_adagrad_ftrl(table, state, zn, D1, keys, 0, g, 0.02, 1e-8, 0.1, 1.0,
                                                               args.l1, 0.0, grad_scale=float(args.batch)),
    }
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.iters))
    nbytes = {"sparse_rowwise_adagrad": n * ADAGRAD_BYTES, "sparse_adagrad_ftrl": n * WIDE_BYTES}
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        print(json.dumps({"kernel": k, "keys": n, "rows": rows, "us_median": round(med[k], 2),
                          "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                          "spread": round((max(ts) - min(ts)) / med[k], 4),
                          "tb_per_s": round(nbytes[k] / (med[k] * 1e-6) / 1e12, 3)}), flush=True)
    ya = times["sparse_rowwise_adagrad"]
    yard = med["sparse_rowwise_adagrad"] * WIDE_BYTES / ADAGRAD_BYTES
    wide = yard * (1.0 + (max(ya) - min(ya)) / med["sparse_rowwise_adagrad"])
    print(json.dumps({"yardstick_us": round(yard, 2), "yardstick_widened_us": round(wide, 2),
                      "sparse_adagrad_ftrl_us": round(med["sparse_adagrad_ftrl"], 2),
                      "ratio_to_yardstick": round(med["sparse_adagrad_ftrl"] / yard, 4),
                      "within": bool(med["sparse_adagrad_ftrl"] <= wide)}), flush=True)


if __name__ == "__main__":
    main()
