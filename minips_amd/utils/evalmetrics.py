"""Held-out evaluation of the binary (CTR) models: exact binned AUC and log loss.

``BinaryEvaluator`` owns one int64 accumulator on the model's device (``ops.binary_hist``:
neg[NB] | pos[NB] | loss_fx | n_nan) that ``update_logits`` / ``update_head`` add to, sums it over
the ranks (``reduce``) and turns it into metrics on the host with Python integers (``result``).

Everything accumulated is an integer, so the metrics are bit-reproducible: they do not depend on
the order of the samples, the launch shape, the batch split or the number of ranks. The scores are
the LOGITS binned on a fixed grid over [-16, 16] (AUC is invariant under monotone maps, and the
bin of a logit needs no transcendental, so CPU and GPU agree on every bin); pairs that share a bin
count 1/2, so ``auc`` is the Mann-Whitney statistic of the binned scores and ``auc_slack`` bounds
its distance from the unbinned AUC of the same data.
"""
from __future__ import annotations

from fractions import Fraction

import torch

from .. import ops


class BinaryEvaluator:
    def __init__(self, device, bins: int = 4096):
        if not 32 <= bins <= 8192 or bins & (bins - 1):
            raise ValueError(f"bins must be a power of two in [32, 8192], got {bins}")
        self.device = torch.device(device)
        self.bins = int(bins)
        self.acc = torch.zeros(2 * self.bins + 2, dtype=torch.int64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def update_logits(self, z: torch.Tensor, y: torch.Tensor):
        """fp32 logits [n] and 0/1 float labels [n]."""
        ops.binary_hist(z, y, self.acc)

    def update_head(self, H, w, b0, wide, y, logits_out=None):
        """The model's last layer fused with the update: z = H . w + b0 + wide (ops.eval_head)."""
        ops.eval_head(H, w, b0, wide, y, self.acc, logits_out)

    def reduce(self, comm):
        """Sum the accumulator over the ranks (collective; exact). int64 sums are carried by every
        path of Comm.all_reduce_: c10d gloo (also the staged GPU-over-gloo test harness), c10d
        RCCL and the native RCCL plane (ncclInt64); an emulated LoopbackComm keeps its own rank's
        counts, as its all-reduce is a no-op by design."""
        comm.all_reduce_(self.acc)
        return self

    def result(self) -> dict:
        """One host copy of the accumulator, then exact integer arithmetic."""
        NB = self.bins
        a = self.acc.tolist()
        neg, pos, loss_fx, n_nan = a[:NB], a[NB:2 * NB], a[2 * NB], a[2 * NB + 1]
        P, N = sum(pos), sum(neg)
        num = ties = below = 0
        for b in range(NB):
            if pos[b]:
                num += pos[b] * (2 * below + neg[b])
                ties += pos[b] * neg[b]
            below += neg[b]
        n = P + N
        out = dict(auc=None, auc_exact=None, auc_slack=None, logloss=None, n=n, n_pos=P, n_nan=n_nan, bins=NB)
        if P and N:
            out["auc_exact"] = Fraction(num, 2 * P * N)
            out["auc"] = num / (2 * P * N)
            out["auc_slack"] = ties / (2 * P * N)
        if n:
            out["logloss"] = loss_fx / ops.EVAL_LOSS_SCALE / n
        return out
