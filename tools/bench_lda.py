#!/usr/bin/env python3
"""Isolated timing of the LDA Gibbs kernels (ops.lda_*, csrc/kernels/lda.hip) and of a one-rank sweep of the model,
in one process: a synthetic corpus of `--tokens` tokens in documents of `--doc_len`, words drawn from a power law
over `--vocab` words (a few hot words with more members than lda_delta's wave path takes), topics uniform, and
the snapshot the corpus implies (rows = the word-topic counts of the batch, nk their column sums).

Device-event time per call over `--iters` back-to-back calls, the arms alternated `--rounds` times, after two
warm-up calls each. Every kernel is reported with tokens per second and its counted bytes per second:
  lda_sample  n * (4 W + 8 + 2 + 2): a row of W floats, inv, z_old and z_new per token
  lda_loglik  n * (4 W + 8 + 2)
  lda_delta   n * (4 + 4 + 2 + 2) + U * 4 W: members, memrow, both topics per token and every unique row written
beside a device copy of lda_sample's byte count measured in the same run (the card's streaming rate).
    python tools/bench_lda.py [--tokens 4194304] [--topics 64,256,1024] [--iters 3] [--rounds 5] [--sweep 1]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_gbdt import alternate, report  # noqa: E402  (the timing discipline of the GBDT tool)
from minips_amd import _native, ops  # noqa: E402


def make_corpus(tokens, doc_len, vocab, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    docs = max(tokens // doc_len, 1)
    p = 1.0 / (torch.arange(vocab, device=dev, dtype=torch.float32) + 10.0)
    words = torch.multinomial(p, docs * doc_len, replacement=True, generator=gen)
    rowptr = torch.arange(docs + 1, dtype=torch.int64, device=dev) * doc_len
    return rowptr, words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 22)
    ap.add_argument("--doc_len", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1 << 16)
    ap.add_argument("--topics", default="64,256,1024")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", type=int, default=1, help="also time sweeps of the model on one rank (0: kernels only)")
    ap.add_argument("--batch_docs", type=int, default=8192)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    K_ = _native.ldak()
    rowptr, words = make_corpus(args.tokens, args.doc_len, args.vocab, dev)
    n, B = words.numel(), rowptr.numel() - 1
    uniq, inv = torch.unique(words, return_inverse=True)
    U = uniq.numel()
    members = torch.bincount(inv)
    csr = ops.emb_build_csr(inv, 1, U)
    gid = torch.arange(B, dtype=torch.int64, device=dev)
    print(json.dumps(dict(tokens=n, docs=B, doc_len=args.doc_len, vocab=args.vocab, unique_rows=U,
                          hottest_row_members=int(members.max()),
                          rows_above_wave_max=int((members > K_.WAVE_MAX).sum()), wave_max=K_.WAVE_MAX,
                          chunk=K_.CHUNK)), flush=True)
    for K in (int(k) for k in args.topics.split(",")):
        W = (K + 3) & ~3
        gen = torch.Generator(device=dev).manual_seed(K)
        z_old = torch.randint(0, K, (n,), device=dev, generator=gen).to(torch.int16)
        rows = torch.zeros(U * W, device=dev).index_add_(0, inv * W + z_old.long(),
                                                         torch.ones(n, device=dev)).view(U, W)
        nk = rows[:, :K].sum(0).long()
        alpha, beta, Vbeta = 0.1, 0.01, args.vocab * 0.01
        z_new = torch.empty_like(z_old)
        dk = torch.zeros(K, dtype=torch.int64, device=dev)
        delta = torch.empty(U, W, device=dev)
        acc = torch.zeros(2, dtype=torch.int64, device=dev)
        nbytes = {"lda_sample": n * (4 * W + 12), "lda_loglik": n * (4 * W + 10), "lda_delta": n * 12 + U * 4 * W}
        src = torch.empty(nbytes["lda_sample"], dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        fns = {"copy": lambda: dst.copy_(src),
               "lda_sample": lambda: ops.lda_sample(rowptr, gid, inv, z_old, rows, nk, alpha, beta, Vbeta, 1, 1,
                                                    z_new=z_new, dk=dk),
               "lda_delta": lambda: ops.lda_delta(inv, z_old, z_new, K, delta, csr=csr),
               "lda_loglik": lambda: ops.lda_loglik(rowptr, inv, z_old, rows, nk, alpha, beta, Vbeta, acc)}
        t = alternate(fns, args.iters, args.rounds)
        copy_us = statistics.median(t.pop("copy"))
        print(json.dumps(dict(K=K, kernel="device_copy", bytes_read=nbytes["lda_sample"], us_median=round(copy_us, 1),
                              read_plus_write_gb_per_s=round(2 * nbytes["lda_sample"] / (copy_us * 1e-6) / 1e9, 1))),
              flush=True)
        med = report(dict(K=K, W=W), t, nbytes=nbytes)
        print(json.dumps(dict(K=K, **{f"{k}_mtokens_per_s": round(n / v, 2) for k, v in med.items()},
                              changed=int((z_new != z_old).sum()))), flush=True)
        del src, dst, rows, delta
        if args.sweep:
            from minips_amd.models.lda import LDA, LDAConfig
            from minips_amd.ps.comm import Comm

            m = LDA(LDAConfig(num_topics=K, vocab=args.vocab, alpha=alpha, beta=beta, batch_docs=args.batch_docs,
                              seed=0), Comm(device=dev))
            m.attach(rowptr, words, 0)
            m.init()
            m.sweep()  # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                m.sweep()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            s = statistics.median(ts)
            print(json.dumps(dict(K=K, sweep="one rank", batch_docs=args.batch_docs, clocks=len(m._batches),
                                  ms_median=round(s * 1e3, 2), ms_min=round(min(ts) * 1e3, 2),
                                  ms_max=round(max(ts) * 1e3, 2), mtokens_per_s=round(n / s / 1e6, 2),
                                  loglik=round(m.loglik(), 4))), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
