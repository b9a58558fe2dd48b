"""Gradient-boosted decision trees (binary logistic objective) on the parameter-server data plane, in exact fixed
point: histogram GBDT whose trees are the same bits on the CPU and the GPU and on 1, 2 or 4 ranks.

Data      a rank's shard stays resident after ``attach``: bins uint8 [N, align16(F)] (every feature quantised once
          against ``cuts`` fp32 [F, NB - 1]), labels, the running logits z, the node of every sample, and the
          round's fixed-point gradients gh int32 [N, 2].
Round     ``boost()``: ops.gbdt_grad (gradients quantised to multiples of 2^-20, the loss in fixed point) and then,
          level by level, zero hist -> ops.gbdt_hist (this rank's samples) -> ONE Comm.all_reduce_ of the int64
          hist -> ops.gbdt_split -> ops.gbdt_advance. Everything summed is an integer, so the reduced histogram
          does not depend on how the samples are split over ranks, and every rank derives the same tree from it.
          The last level's child sums give the leaves (ops.gbdt_leaf) and the advance adds them to z. Split
          results stay on the device: a steady one-rank round issues no host sync.
Trees     complete binary trees of fixed depth, level-major (node n of level d at 2^d - 1 + n), preallocated for
          ``max_trees``: feat int32 [T, 2^depth - 1] (-1: a pass-through node, everything goes left), thr uint8
          likewise (right: bin > thr), leaf fp32 [T, 2^depth].
The rule is stated in csrc/kernels/gbdt.h; ``leaf_csr`` turns the trees into the sparse one-hot features of the
classic GBDT + LR pipeline (keys t * 2^depth + leaf, values 1: what SparseLR.train_step takes).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional

import torch

from .. import ops
from ..ps.comm import Comm

MAX_SAMPLES = (1 << 33) - 1   # the fp64 conversions of the split are exact below 2^33 samples
MAX_HIST_BYTES = 1 << 30


@dataclass
class GBDTConfig:
    num_features: int = 8
    num_bins: int = 64
    depth: int = 6
    lr: float = 0.1
    reg_lambda: float = 1.0
    min_child_count: int = 1
    min_gain: float = 0.0
    base_score: float = 0.0
    max_trees: int = 256
    transport: str = "collective"

    def __post_init__(self):
        F, NB, D = self.num_features, self.num_bins, self.depth
        if not 2 <= NB <= ops.GBDT_MAX_BINS:
            raise ValueError(f"gbdt: num_bins is {NB}, expected 2 <= num_bins <= {ops.GBDT_MAX_BINS}")
        if not 1 <= D <= ops.GBDT_MAX_DEPTH:
            raise ValueError(f"gbdt: depth is {D}, expected 1 <= depth <= {ops.GBDT_MAX_DEPTH}")
        if not 1 <= F <= ops.GBDT_MAX_F:
            raise ValueError(f"gbdt: num_features is {F}, expected 1 <= num_features <= {ops.GBDT_MAX_F}")
        if not self.reg_lambda > 0:
            raise ValueError(f"gbdt: reg_lambda is {self.reg_lambda}, expected > 0 (every denominator stays positive)")
        if self.min_child_count < 1:
            raise ValueError(f"gbdt: min_child_count is {self.min_child_count}, expected >= 1")
        if not self.min_gain >= 0:
            raise ValueError(f"gbdt: min_gain is {self.min_gain}, expected >= 0")
        if not self.lr > 0:
            raise ValueError(f"gbdt: lr is {self.lr}, expected > 0")
        if not 1 <= self.max_trees <= 1 << 16:
            raise ValueError(f"gbdt: max_trees is {self.max_trees}, expected 1 <= max_trees <= 65536")
        if not abs(self.base_score) < float("inf"):
            raise ValueError(f"gbdt: base_score is {self.base_score}, expected a finite logit")
        hist = (1 << (D - 1)) * F * NB * 3 * 8
        if hist > MAX_HIST_BYTES:
            raise ValueError(f"gbdt: the last level's hist [2^{D - 1}, {F}, {NB}, 3] int64 is {hist} bytes, above "
                             f"1 GiB")
        if self.transport != "collective":
            raise ValueError(f"gbdt: transport {self.transport!r} is not supported (the histograms are summed by an "
                             f"all-reduce; there is no gbdt on the one-sided transport); use 'collective'")


class GBDT:
    def __init__(self, cfg: GBDTConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        dev, D = comm.device, cfg.depth
        self.F, self.NB = cfg.num_features, cfg.num_bins
        self.ldb = (self.F + 15) & ~15
        nn = (1 << D) - 1
        self.feat = torch.full((cfg.max_trees, nn), -1, dtype=torch.int32, device=dev)
        self.thr = torch.zeros(cfg.max_trees, nn, dtype=torch.uint8, device=dev)
        self.leaf = torch.zeros(cfg.max_trees, nn + 1, dtype=torch.float32, device=dev)
        self.num_trees = 0
        self.cuts: Optional[torch.Tensor] = None
        # one level's outputs each, and the hist of the widest level (a level takes a prefix of it)
        self._hist = torch.zeros((1 << (D - 1)) * self.F * self.NB * 3, dtype=torch.int64, device=dev)
        self._lvl = [(torch.empty(1 << d, dtype=torch.int32, device=dev),
                      torch.empty(1 << d, dtype=torch.int32, device=dev),
                      torch.empty(1 << d, dtype=torch.float64, device=dev),
                      torch.empty(1 << d, 2, 3, dtype=torch.int64, device=dev)) for d in range(D)]
        self._loss = torch.zeros(1, dtype=torch.int64, device=dev)
        self.bins = self.labels = self.z = self.node = self.gh = None

    # -- cuts and bins ----------------------------------------------------------------------
    def make_cuts(self, X: torch.Tensor) -> torch.Tensor:
        """Quantile cuts of this rank's X [N, F], on the host, once: per feature the fp64 torch.quantile at j / NB
        (NaN left out), cast to fp32, duplicates dropped, padded with +inf. On several ranks rank 0's cuts reach
        every rank through one all-reduce of a buffer that is zero elsewhere (an exact sum). Sets and returns
        them."""
        F, NB = self.F, self.NB
        if X.dim() != 2 or X.shape[1] != F:
            raise ValueError(f"gbdt: make_cuts takes X [N, {F}], got {tuple(X.shape)}")
        cuts = torch.full((F, NB - 1), float("inf"), dtype=torch.float32)
        if self.comm.rank == 0:
            q = torch.arange(1, NB, dtype=torch.float64) / NB
            Xh = X.detach().to("cpu", torch.float64)
            for f in range(F):
                col = Xh[:, f]
                col = col[~torch.isnan(col)]
                if col.numel() > (1 << 24):  # torch.quantile's input limit: an even subsample
                    col = col[:: -(-col.numel() // (1 << 24))]
                if col.numel():
                    c = torch.unique(torch.quantile(col, q).float())  # sorted, duplicates dropped
                    c = c[torch.isfinite(c)]
                    cuts[f, : c.numel()] = c
        if self.comm.world > 1:
            if self.comm.rank != 0:
                cuts.zero_()
            buf = cuts.to(self.comm.device)
            self.comm.all_reduce_(buf)
            cuts = buf
        return self.set_cuts(cuts)

    def set_cuts(self, cuts: torch.Tensor) -> torch.Tensor:
        if cuts.shape != (self.F, self.NB - 1):
            raise ValueError(f"gbdt: cuts must be [{self.F}, {self.NB - 1}], got {tuple(cuts.shape)}")
        self.cuts = cuts.detach().to(self.comm.device, torch.float32).contiguous()
        return self.cuts

    def bin(self, X: torch.Tensor) -> torch.Tensor:
        """bins uint8 [N, align16(F)] of X [N, F] (ops.gbdt_bin)."""
        if self.cuts is None:
            raise ValueError("gbdt: no cuts yet: make_cuts(X) or set_cuts(cuts) first")
        if X.dim() != 2 or X.shape[1] != self.F:
            raise ValueError(f"gbdt: X must be [N, {self.F}], got {tuple(X.shape)}")
        return ops.gbdt_bin(X.to(self.comm.device, torch.float32), self.cuts)

    def _as_bins(self, X: torch.Tensor) -> torch.Tensor:
        if X.dtype == torch.uint8:
            if X.dim() != 2 or X.shape[1] < self.F:
                raise ValueError(f"gbdt: bins must be uint8 [N, >= {self.F}], got {tuple(X.shape)}")
            return X.to(self.comm.device)
        return self.bin(X)

    # -- training ---------------------------------------------------------------------------
    def attach(self, X_or_bins: torch.Tensor, labels: torch.Tensor):
        """Keeps this rank's shard resident: bins (uint8 as given, anything else is binned), labels, z (the
        logits of the trees so far), node, gh."""
        if self.cuts is None:
            raise ValueError("gbdt: attach before the cuts exist: make_cuts(X) or set_cuts(cuts) first")
        dev = self.comm.device
        bins = self._as_bins(X_or_bins)
        N = bins.shape[0]
        if labels.numel() != N:
            raise ValueError(f"gbdt: {labels.numel()} labels for {N} samples")
        total = N
        if self.comm.world > 1:
            t = torch.tensor([N], dtype=torch.int64, device=dev)
            self.comm.all_reduce_(t)
            total = int(t)
        if total > MAX_SAMPLES:
            raise ValueError(f"gbdt: {total} samples over all ranks, expected at most 2^33 - 1 (the split's fp64 "
                             f"conversions are exact below that)")
        self.bins = bins
        self.labels = labels.detach().to(dev, torch.float32).reshape(N).contiguous()
        self.node = torch.zeros(N, dtype=torch.int32, device=dev)
        self.gh = torch.zeros(N, 2, dtype=torch.int32, device=dev)
        self.z = self._predict_bins(bins)
        return self

    def _level_hist(self, d: int) -> torch.Tensor:
        nodes = 1 << d
        return self._hist[: nodes * self.F * self.NB * 3].view(nodes, self.F, self.NB, 3)

    def boost(self, gh: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Adds one tree. ``gh`` (int32 [N, 2]) replaces the round's gradients of this rank's samples (how the
        tests replay GPU gradients on the CPU). Returns the round's summed training loss of all ranks (before the
        tree; a device value, summed in fixed point: equal for every rank count)."""
        cfg = self.cfg
        if self.bins is None:
            raise ValueError("gbdt: boost before attach(X, labels)")
        if self.num_trees >= cfg.max_trees:
            raise ValueError(f"gbdt: {self.num_trees} trees already, max_trees is {cfg.max_trees}")
        t, D = self.num_trees, cfg.depth
        self._loss.zero_()
        ops.gbdt_grad(self.z, self.labels, self.gh, self._loss)
        if gh is not None:
            if gh.shape != self.gh.shape or gh.dtype != torch.int32:
                raise ValueError(f"gbdt: gh must be int32 {tuple(self.gh.shape)}, got {gh.dtype} {tuple(gh.shape)}")
            self.gh.copy_(gh)
        self.node.zero_()
        for d in range(D):
            nodes, off = 1 << d, (1 << d) - 1
            hist = self._level_hist(d)
            hist.zero_()
            ops.gbdt_hist(self.bins, self.node, self.gh, hist)
            self.comm.all_reduce_(hist)
            feat, thr, gain, child = self._lvl[d]
            ops.gbdt_split(hist, cfg.reg_lambda, cfg.min_child_count, cfg.min_gain, feat, thr, gain, child)
            self.feat[t, off: off + nodes].copy_(feat)
            self.thr[t, off: off + nodes].copy_(thr)
            if d == D - 1:
                ops.gbdt_leaf(child, cfg.reg_lambda, cfg.lr, self.leaf[t])
                ops.gbdt_advance(self.bins, self.node, feat, thr, self.F, self.leaf[t], self.z)
            else:
                ops.gbdt_advance(self.bins, self.node, feat, thr, self.F)
        self.num_trees = t + 1
        loss = self._loss.clone()
        self.comm.all_reduce_(loss)
        return loss.double().mul_(2.0 ** -24).reshape(())

    # -- inference --------------------------------------------------------------------------
    def _predict_bins(self, bins: torch.Tensor, leaf_index: Optional[torch.Tensor] = None) -> torch.Tensor:
        T = self.num_trees
        z = torch.empty(bins.shape[0], dtype=torch.float32, device=self.comm.device)
        ops.gbdt_predict(bins, self.feat[:T], self.thr[:T], self.leaf[:T], self.F, self.cfg.depth, self.cfg.base_score,
                         z, leaf_index)
        return z

    def predict_logits(self, X: torch.Tensor) -> torch.Tensor:
        """Logits [N] of X [N, F] (or of uint8 bins): base_score plus every tree's leaf, in fp32 in tree order."""
        return self._predict_bins(self._as_bins(X))

    def leaf_index(self, X: torch.Tensor) -> torch.Tensor:
        """int32 [N, T]: the leaf every sample reaches in every tree."""
        bins = self._as_bins(X)
        li = torch.zeros(bins.shape[0], self.num_trees, dtype=torch.int32, device=self.comm.device)
        self._predict_bins(bins, li)
        return li

    def leaf_csr(self, X: torch.Tensor):
        """(rowptr, cols, vals): the trees as sparse one-hot features, keys t * 2^depth + leaf and values 1, over
        num_dims = num_trees * 2^depth -- the CSR batch SparseLR.train_step takes."""
        li = self.leaf_index(X).long()
        N, T = li.shape
        dev = li.device
        cols = (li + (torch.arange(T, dtype=torch.int64, device=dev) << self.cfg.depth)[None, :]).reshape(-1)
        rowptr = torch.arange(N + 1, dtype=torch.int64, device=dev) * T
        return rowptr, cols, torch.ones(N * T, dtype=torch.float32, device=dev)

    def evaluate(self, batches, evaluator=None) -> dict:
        """Held-out evaluation: ``batches`` yields (X, labels); every rank calls it with the same number of
        batches. Binning and ops.gbdt_predict only: no model state is written. Returns BinaryEvaluator.result()
        over all ranks' samples."""
        from ..utils.evalmetrics import BinaryEvaluator

        ev = evaluator if evaluator is not None else BinaryEvaluator(self.comm.device)
        for X, labels in batches:
            z = self.predict_logits(X)
            ev.update_logits(z, (labels.to(z.device) > 0.5).float())
        ev.reduce(self.comm)
        return ev.result()

    def drain(self):
        """Nothing is in flight between rounds (the driver's common epilogue calls it)."""

    # -- state ------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        T = self.num_trees
        return dict(config=dataclasses.asdict(self.cfg), num_trees=T,
                    cuts=None if self.cuts is None else self.cuts.cpu().clone(), feat=self.feat[:T].cpu().clone(),
                    thr=self.thr[:T].cpu().clone(), leaf=self.leaf[:T].cpu().clone())

    def load_state_dict(self, sd: dict):
        c, mine = sd["config"], dataclasses.asdict(self.cfg)
        for k in ("num_features", "num_bins", "depth"):
            if c[k] != mine[k]:
                raise ValueError(f"gbdt: the state was saved with {k} = {c[k]}, this model has {mine[k]}")
        T = int(sd["num_trees"])
        if T > self.cfg.max_trees:
            raise ValueError(f"gbdt: the state holds {T} trees, max_trees is {self.cfg.max_trees}")
        # the hyperparameters travel with the trees: a continued run adds the trees the saved one would have
        self.cfg = dataclasses.replace(self.cfg, **{k: c[k] for k in ("lr", "reg_lambda", "min_child_count",
                                                                      "min_gain", "base_score")})
        if sd["cuts"] is not None:
            self.set_cuts(sd["cuts"])
        self.feat.fill_(-1)
        self.thr.zero_()
        self.leaf.zero_()
        self.feat[:T].copy_(sd["feat"])
        self.thr[:T].copy_(sd["thr"])
        self.leaf[:T].copy_(sd["leaf"])
        self.num_trees = T
        if self.bins is not None:  # the resident logits follow the loaded trees
            self.z = self._predict_bins(self.bins)
        return self

    def save(self, path: str):
        torch.save(self.state_dict(), path)

    def load(self, path: str):
        return self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
