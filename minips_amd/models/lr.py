"""Sparse logistic regression on the GPU parameter server (BASELINE config 1, reference
examples/lr_example.cpp): one width-1 fp32 SparseTable row per feature, the server apply is the
reference's plain ``w += delta`` ("add"), and the worker computes
delta[col] = alpha * sum_rows x * (y - sigmoid(w . x)) for the features present in its batch
(lr_example.cpp:291-312) with the fused ``lr_sparse_step`` kernel over the pulled rows.

``optimizer="ftrl"``: the table applies per-coordinate FTRL-Proximal (ops.sparse_ftrl) to the batch's
summed logistic gradient instead; with ``l1`` > 0 most weights end at exactly zero (``nnz()``).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..ps.comm import Comm
from ..ps.tables import HashSparseTable, SparseTable


@dataclass
class SparseLRConfig:
    num_dims: int = 16_609_143  # webspam trigram feature count (reference default num_dims)
    alpha: float = 0.1
    consistency: str = "bsp"
    staleness: int = 0
    storage: str = "vector"  # reference kStorageType: "vector" (dense key range) or "map" (hash)
    value_dtype: torch.dtype = torch.float32  # float64: the reference's CreateTable<double>
    optimizer: str = "add"  # "add": the reference's w += alpha * delta; "ftrl": FTRL-Proximal (vector, fp32)
    ftrl_alpha: float = 0.1
    ftrl_beta: float = 1.0
    l1: float = 0.0
    l2: float = 0.0

    def __post_init__(self):
        if self.optimizer not in ("add", "ftrl"):
            raise ValueError(f"sparse LR optimizer {self.optimizer!r}: add | ftrl")
        if self.optimizer == "ftrl":
            if self.storage.lower() != "vector":
                raise ValueError(f"optimizer 'ftrl' needs storage 'vector', not {self.storage!r}")
            if self.value_dtype != torch.float32:
                raise ValueError(f"optimizer 'ftrl' keeps fp32 weights, not {self.value_dtype}")


class SparseLR:
    def __init__(self, cfg: SparseLRConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        # the worker's delta = scale * x * (y - p): the reference's step, or (scale -1) the plain gradient
        self._delta_scale = cfg.alpha
        if cfg.optimizer == "ftrl":
            self._delta_scale = -1.0
            self.table = SparseTable(comm, cfg.num_dims, 1, optimizer="ftrl", lr=cfg.ftrl_alpha,
                                     ftrl_beta=cfg.ftrl_beta, l1=cfg.l1, l2=cfg.l2, init_std=0.0,
                                     pull_dtype=torch.float32, push_dtype=torch.float32,
                                     consistency=cfg.consistency, staleness=cfg.staleness)
        elif cfg.storage.lower() == "map":  # MapStorage: rows created on first touch, zero-initialised
            self.table = HashSparseTable(comm, 1, optimizer="add", pull_dtype=torch.float32, init_std=0.0,
                                         consistency=cfg.consistency, staleness=cfg.staleness)
        elif cfg.storage.lower() == "vector":
            self.table = SparseTable(comm, cfg.num_dims, 1, optimizer="add", pull_dtype=torch.float32, init_std=0.0,
                                     consistency=cfg.consistency, staleness=cfg.staleness,
                                     value_dtype=cfg.value_dtype)
        else:
            raise ValueError(f"kStorageType {cfg.storage!r}: Map or Vector")

    def train_step(self, rowptr, cols, vals, labels):
        """CSR batch (rowptr [B+1], cols/vals [nnz], labels [B] in {0,1} or {-1,1}).
        Returns the number of correctly classified rows (before the update)."""
        dev = self.comm.device
        rows, plan = self.table.get(cols)
        delta = torch.zeros(max(plan.cap, 1), dtype=rows.dtype, device=dev)
        correct = torch.zeros(1, dtype=torch.float32, device=dev)
        if plan.cap:
            ops.lr_sparse_step(rowptr, plan.inv, vals, labels, rows.view(-1)[: plan.cap], self._delta_scale,
                               delta[: plan.cap], correct)
            self.table.add(plan, delta.view(-1, 1))
        self.table.clock()
        return correct

    def evaluate(self, rowptr, cols, vals, labels):
        w = self.table.get_rows(cols).view(-1)
        correct = torch.zeros(1, dtype=torch.float32, device=self.comm.device)
        idx = torch.arange(cols.numel(), device=cols.device)
        ops.lr_sparse_step(rowptr, idx, vals, labels, w, 0.0, None, correct)
        return correct

    def drain(self):
        self.table.drain()

    def nnz(self) -> int:
        """Non-zero weights of the model (a host read that drains the table: for reports)."""
        return self.table.nnz()
