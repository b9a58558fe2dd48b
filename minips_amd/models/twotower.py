"""Two-tower retrieval with the in-batch sampled softmax (Yi et al., 2019, "Sampling-bias-corrected neural modeling
for large corpus item recommendations") on the GPU parameter server: the candidate generator in front of the ranking
models -- a user embedding and an item embedding, every pair of a batch using the other pairs' items as negatives.

Parameters
  sparse table  users + items fp32 rows of dim floats, row-wise Adagrad, N(0, init_std): key u is user u's row, key
                users + i item i's (ALS's key space with word2vec's optimizer). The table is plain: save / restore /
                N -> M resharding go through the name-generic checkpoint code.
Clock: the key matrix [P, 2] -> plan (with the lookup CSR) -> sparse Get -> ops.ibs_forward (one launch: loss, lse)
-> ops.ibs_backward (two fused sweeps and a row reduce: every unique row's gradient written once, no atomics) ->
sparse Add -> Clock. The loss is the mean over the global batch of lse_p - s_pp (the gradient carries 1 / (P *
world)); the negatives are the rank's own batch, as in data-parallel practice. Nothing is read back: a steady
one-rank clock issues no host sync. The rule is stated in csrc/kernels/ibs.h.

``set_item_counts`` gives the bias correction its log sampling probabilities: logq_i = log((count_i + 1) / (total +
items)); without it, or with ``correct_bias=False``, the logits are not corrected.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .. import _native, ops
from ..ps.comm import Comm
from ..ps.tables import SparseTable


@dataclass
class TwoTowerConfig:
    users: int = 1 << 16
    items: int = 1 << 16
    dim: int = 64
    tau: float = 0.1
    lr: float = 0.05
    init_std: float = 0.0   # 0.0: 1 / sqrt(dim)
    eps: float = 1e-8
    correct_bias: bool = True
    seed: int = 0
    consistency: str = "bsp"
    staleness: int = 0
    transport: str = "collective"
    storage: str = "vector"
    value_dtype: torch.dtype = torch.float32
    pull_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        if self.users < 1 or self.items < 1 or self.users + self.items >= 1 << 31:
            raise ValueError(f"twotower: users {self.users} and items {self.items}, expected both >= 1 and users + "
                             f"items < 2^31")
        if self.dim % 4 or not ops.IBS_MIN_D <= self.dim <= ops.IBS_MAX_D:
            raise ValueError(f"twotower: dim is {self.dim}, expected dim % 4 == 0 and {ops.IBS_MIN_D} <= dim <= "
                             f"{ops.IBS_MAX_D}")
        if not (self.tau > 0 and math.isfinite(self.tau)):
            raise ValueError(f"twotower: tau is {self.tau}, expected a positive finite temperature")
        if not self.init_std >= 0:
            raise ValueError(f"twotower: init_std is {self.init_std}, expected >= 0 (0: 1 / sqrt(dim))")
        if self.transport != "collective":
            raise ValueError(f"twotower: transport {self.transport!r} is not supported (the one-sided owners apply "
                             f"the row-wise Adagrad of W&D's rows only); use 'collective'")
        if self.storage.lower() != "vector":
            raise ValueError(f"twotower: storage {self.storage!r} is not supported (user u and item i are the keys u "
                             f"and users + i of a range table); use 'vector'")
        if self.value_dtype != torch.float32 or self.pull_dtype != torch.float32:
            raise ValueError(f"twotower: rows are stored and pulled in fp32, not {self.value_dtype} / "
                             f"{self.pull_dtype}")


class TwoTower:
    def __init__(self, cfg: TwoTowerConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        self.U, self.I, self.d = cfg.users, cfg.items, cfg.dim
        if comm.device.type == "cuda":  # a missing kernel is an error, here and not at the first clock
            try:
                _native.ibsk()
            except RuntimeError as e:
                raise ValueError(f"twotower: the model runs on {comm.device} and needs the _ibsk extension: {e}") from e
        std = cfg.init_std if cfg.init_std > 0 else cfg.dim ** -0.5
        self.table = SparseTable(comm, self.U + self.I, self.d, optimizer="rowwise_adagrad", lr=cfg.lr, eps=cfg.eps,
                                 pull_dtype=torch.float32, push_dtype=torch.float32, value_dtype=torch.float32,
                                 init_std=std, seed=cfg.seed + 1234, consistency=cfg.consistency,
                                 staleness=cfg.staleness, table_id=0)
        self.logq = None

    def set_item_counts(self, counts: torch.Tensor):
        """The bias correction's log sampling probabilities from the int64 item counts [items] of the training
        stream: logq_i = log((count_i + 1) / (total + items)) in fp64, rounded to fp32. On several ranks rank 0's
        counts reach every rank through one all-reduce of a buffer that is zero elsewhere."""
        c = counts.detach().to("cpu", torch.int64).reshape(-1)
        if c.numel() != self.I or bool((c < 0).any()):
            raise ValueError(f"twotower: set_item_counts takes {self.I} counts >= 0, got {c.numel()}")
        if self.comm.world > 1 and not self.comm.emulated:
            if self.comm.rank != 0:
                c = torch.zeros_like(c)
            c = c.to(self.comm.device)
            self.comm.all_reduce_(c)
            c = c.cpu()
        q = torch.log((c.double() + 1.0) / (float(c.sum()) + self.I))
        self.logq = q.float().to(self.comm.device)
        return self

    def _lookups(self, users, items):
        """(keys int64 [2 P], logq [P] or None) of the pairs: an id outside its range gives the key -1."""
        dev = self.comm.device
        u = users.to(dev, torch.int64).reshape(-1)
        i = items.to(dev, torch.int64).reshape(-1)
        if u.numel() != i.numel():
            raise ValueError(f"twotower: {u.numel()} users for {i.numel()} items")
        ku = torch.where((u >= 0) & (u < self.U), u, torch.full_like(u, -1))
        ok = (i >= 0) & (i < self.I)
        ki = torch.where(ok, i + self.U, torch.full_like(i, -1))
        logq = None
        if self.cfg.correct_bias and self.logq is not None and u.numel():
            logq = torch.where(ok, self.logq[i.clamp(0, self.I - 1)], torch.zeros((), device=dev))
        return torch.stack([ku, ki], 1).reshape(-1), logq

    def train_step(self, users, items) -> torch.Tensor:
        """One clock on P pairs (users / items int64 [P] ids): Get, forward, backward, Add, Clock. Returns the summed
        loss of this rank's pairs (a device tensor; no host sync). P may be 0: the rank plans zero keys, pushes zero
        rows and clocks."""
        cfg, dev = self.cfg, self.comm.device
        keys, logq = self._lookups(users, items)
        P = keys.numel() // 2
        plan = self.table.plan(keys, csr=True)
        rows, plan = self.table.get(keys, plan=plan)
        if plan.keys_n:
            gscale = 1.0 / (P * self.comm.world)
            loss, lse = ops.ibs_forward(plan.inv, rows, self.d, cfg.tau, logq, gscale)
            grad_rows = (torch.empty if dev.type == "cuda" else torch.zeros)(max(plan.cap, 1), self.d,
                                                                             dtype=torch.float32, device=dev)
            ops.ibs_backward(plan.inv, rows, self.d, cfg.tau, lse, grad_rows, logq, gscale,
                             csr=plan.csr[:2] if plan.csr is not None else None)
            self.table.add(plan, grad_rows)
            out = loss.sum()
        else:
            if self.comm.world > 1:  # the push is a collective: a rank without pairs pushes zero rows
                self.table.add(plan, torch.zeros(max(plan.cap, 1), self.d, dtype=torch.float32, device=dev))
            out = torch.zeros((), dtype=torch.float32, device=dev)
        self.table.clock()
        return out

    def evaluate(self, batches) -> float:
        """The mean in-batch loss of ``batches`` (an iterable of (users, items)) over all ranks: forward only -- no
        Add, no Clock, no table bit written. Collective (every rank passes the same number of batches)."""
        dev = self.comm.device
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        for users, items in batches:
            keys, logq = self._lookups(users, items)
            rows, plan = self.table.get(keys)
            if plan.keys_n:
                loss, _ = ops.ibs_forward(plan.inv, rows, self.d, self.cfg.tau, logq)
                acc[0] += loss.sum().double()
                acc[1] += keys.numel() // 2
        if self.comm.world > 1:
            self.comm.all_reduce_(acc)
        return float(acc[0]) / max(float(acc[1]), 1.0)

    def user_vectors(self) -> torch.Tensor:
        """The user embeddings fp32 [users, dim] (collective: a Get of every user key)."""
        return self.table.get_rows(torch.arange(self.U, dtype=torch.int64, device=self.comm.device))

    def item_vectors(self) -> torch.Tensor:
        """The item embeddings fp32 [items, dim] (collective: a Get of every item key)."""
        return self.table.get_rows(torch.arange(self.U, self.U + self.I, dtype=torch.int64, device=self.comm.device))

    def drain(self):
        self.table.drain()
