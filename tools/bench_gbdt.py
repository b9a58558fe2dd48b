#!/usr/bin/env python3
"""Isolated timing of the histogram GBDT kernels (ops.gbdt_*, csrc/kernels/gbdt.hip) next to the eager torch
composition of the same step run on the GPU (the CPU references' formulas: index_add_ into int64 for the
histogram, cumsum + the fp64 gain + the first maximum for the split, gathers for the advance), in one process:
`--rows` samples of `--features` features in `--bins` bins, the levels 0 .. `--levels` - 1 with uniformly
random node ids.

Device-event time per call over `--iters` back-to-back calls, the arms alternated `--rounds` times. gbdt_hist is
reported per level and per path with its counted bytes per second -- the bins row (ldb bytes), the node id (4) and
the gradient pair (8) of every sample, nothing else -- beside a device copy of the same byte count measured in
the same run (the card's streaming rate).
    python tools/bench_gbdt.py [--rows 4194304] [--features 32] [--bins 64] [--levels 6] [--iters 5] [--rounds 5]
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


def alternate(fns, iters, rounds, eager_iters=1):
    """{name: [us per call] * rounds}, the arms alternated; the eager arms run `eager_iters` calls a round."""
    for name, fn in fns.items():
        for _ in range(1 if name.startswith("eager") else 2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, eager_iters if name.startswith("eager") else iters))
    return times


def report(tag, times, nbytes=None, **extra):
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        rec = dict(tag, kernel=name, us_median=round(med[name], 1), us_min=round(min(ts), 1), us_max=round(max(ts), 1),
                   spread=round((max(ts) - min(ts)) / med[name], 4))
        if nbytes and name in nbytes:
            rec["counted_gb_per_s"] = round(nbytes[name] / (med[name] * 1e-6) / 1e9, 1)
        rec.update(extra)
        print(json.dumps(rec), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    K_ = _native.gbdtk()
    N, F, NB = args.rows, args.features, args.bins
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(N, F, device=dev, generator=gen) * 2 - 1
    cuts = (torch.arange(1, NB, device=dev, dtype=torch.float32) / NB * 2 - 1)[None, :].repeat(F, 1).contiguous()
    labels = (torch.rand(N, device=dev, generator=gen) < 0.5).float()
    z = torch.randn(N, device=dev, generator=gen)
    gh = torch.zeros(N, 2, dtype=torch.int32, device=dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)
    bins = ops.gbdt_bin(X, cuts)
    ldb = bins.shape[1]
    ops.gbdt_grad(z, labels, gh, acc)
    print(json.dumps(dict(rows=N, features=F, bins=NB, ldb=ldb, levels=args.levels, flush_rows=K_.FLUSH_ROWS,
                          lds_bytes=K_.LDS_BYTES)), flush=True)

    # the card's streaming rate on the histogram's byte count: a device copy reads and writes it once each
    hist_bytes = N * (ldb + 4 + 8)
    src = torch.empty(hist_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    t = alternate({"copy": lambda: dst.copy_(src)}, args.iters, args.rounds)
    copy_us = statistics.median(t["copy"])
    print(json.dumps(dict(kernel="device_copy", bytes_read=hist_bytes, us_median=round(copy_us, 1),
                          read_plus_write_gb_per_s=round(2 * hist_bytes / (copy_us * 1e-6) / 1e9, 1))), flush=True)
    del src, dst

    # element-wise kernels against their compositions
    XT = X.t().contiguous()

    def eager_bin():
        return torch.searchsorted(cuts, XT, right=False).t().to(torch.uint8)  # #{j : cuts[j] < x}

    def eager_grad():
        y = (labels > 0.5).float()
        p = torch.sigmoid(z.clamp(-30, 30))
        g = torch.stack([torch.round((p - y) * 1048576.0),
                         torch.round((p * (1 - p)).clamp(min=2.0 ** -20) * 1048576.0)], 1).to(torch.int32)
        zl = z.clamp(-64, 64)
        l = zl.clamp(min=0) - zl * y + torch.log1p(torch.exp(-zl.abs()))
        return g, torch.round(l * 16777216.0).to(torch.int64).sum()

    assert torch.equal(eager_bin(), bins[:, :F])
    out = torch.empty_like(bins)
    t = alternate({"gbdt_bin": lambda: ops.gbdt_bin(X, cuts, out=out), "eager_bin": eager_bin,
                   "gbdt_grad": lambda: ops.gbdt_grad(z, labels, gh, acc), "eager_grad": eager_grad},
                  args.iters, args.rounds, eager_iters=2)
    med = report({}, t, nbytes={"gbdt_bin": N * (4 * F + ldb), "gbdt_grad": N * 16})
    print(json.dumps(dict(bin_eager_over_kernel=round(med["eager_bin"] / med["gbdt_bin"], 2),
                          grad_eager_over_kernel=round(med["eager_grad"] / med["gbdt_grad"], 2))), flush=True)
    del XT, out

    # per level: hist on each path, split, advance
    sums = dict(kernel=0.0, eager=0.0)
    for d in range(args.levels):
        nodes = 1 << d
        node = torch.randint(0, nodes, (N,), device=dev, generator=gen).to(torch.int32)
        hist = torch.zeros(nodes, F, NB, 3, dtype=torch.int64, device=dev)
        ref = torch.zeros_like(hist)
        ops._gbdt_hist_ref(bins, node, gh, ref)
        paths = {"auto": 0, "lds": 1, "global": 2}
        if K_.LDS_BYTES < nodes * NB * 12:
            del paths["lds"]
        for name, p in paths.items():
            hist.zero_()
            ops.gbdt_hist(bins, node, gh, hist, path=p)
            assert torch.equal(hist, ref), (d, name)
        fns = {f"gbdt_hist_{name}": (lambda p=p: ops.gbdt_hist(bins, node, gh, hist, path=p))
               for name, p in paths.items()}
        fns["eager_hist"] = lambda: ops._gbdt_hist_ref(bins, node, gh, hist)
        outs = (torch.empty(nodes, dtype=torch.int32, device=dev), torch.empty(nodes, dtype=torch.int32, device=dev),
                torch.empty(nodes, dtype=torch.float64, device=dev),
                torch.empty(nodes, 2, 3, dtype=torch.int64, device=dev))
        eouts = tuple(torch.empty_like(o) for o in outs)
        fns["gbdt_split"] = lambda: ops.gbdt_split(ref, 1.0, 1, 0.0, *outs)
        fns["eager_split"] = lambda: ops._gbdt_split_ref(ref, 1.0, 1, 0.0, *eouts)
        nd, nde = node.clone(), node.clone()

        def adv(fn, n):
            n.copy_(node)
            fn(bins, n, outs[0], outs[1], F)

        fns["gbdt_advance"] = lambda: adv(ops.gbdt_advance, nd)
        fns["eager_advance"] = lambda: adv(ops._gbdt_advance_ref, nde)
        t = alternate(fns, args.iters, args.rounds)
        for a, b in zip(outs, eouts):
            assert torch.equal(a, b), d
        assert torch.equal(nd, nde), d
        med = report(dict(level=d, nodes=nodes), t,
                     nbytes={k: hist_bytes for k in fns if k.startswith("gbdt_hist")},
                     tile=min(F, K_.LDS_BYTES // (nodes * NB * 12)))
        k = med["gbdt_hist_auto"] + med["gbdt_split"] + med["gbdt_advance"]
        e = med["eager_hist"] + med["eager_split"] + med["eager_advance"]
        sums["kernel"] += k
        sums["eager"] += e
        print(json.dumps(dict(level=d, kernel_level_us=round(k, 1), eager_level_us=round(e, 1),
                              eager_over_kernel=round(e / k, 2),
                              hist_ratio=round(med["eager_hist"] / med["gbdt_hist_auto"], 2),
                              split_ratio=round(med["eager_split"] / med["gbdt_split"], 2),
                              advance_ratio=round(med["eager_advance"] / med["gbdt_advance"], 2))), flush=True)
        del node, hist, ref, nd, nde
    print(json.dumps(dict(levels=args.levels, kernel_tree_us=round(sums["kernel"], 1),
                          eager_tree_us=round(sums["eager"], 1),
                          eager_over_kernel=round(sums["eager"] / sums["kernel"], 2))), flush=True)

    # predict: 20 trees of depth 6 (random splits)
    T, depth = 20, 6
    nn = (1 << depth) - 1
    feat = torch.randint(0, F, (T, nn), device=dev, generator=gen).to(torch.int32)
    thr = torch.randint(0, NB - 1, (T, nn), device=dev, generator=gen).to(torch.uint8)
    leaf = torch.randn(T, nn + 1, device=dev, generator=gen)
    zo = torch.empty(N, device=dev)
    t = alternate({"gbdt_predict": lambda: ops.gbdt_predict(bins, feat, thr, leaf, F, depth, 0.0, zo)}, args.iters,
                  args.rounds)
    report(dict(trees=T, depth=depth), t, nbytes={"gbdt_predict": N * (ldb + 4)})


if __name__ == "__main__":
    main()
