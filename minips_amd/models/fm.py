"""2-way factorization machine (Rendle, 2010) on the GPU parameter server: the second-order model over the
same general CSR (libsvm) input as sparse LR, one short row per feature.

Parameters
  sparse table  one fp32 split row per feature, [k factors | 1 linear weight | 3 pad] (Wide&Deep's row layout):
                row-wise Adagrad on the factors, and on the linear column either its own Adagrad accumulator
                (``linear_optimizer="adagrad"``) or FTRL-Proximal with L1 / L2 (``"ftrl"``,
                SparseTable(wide_optimizer="ftrl")).
  dense table   the bias w0: a minimal DenseTable (Adagrad), padded by the table to its kernels' and its
                sharding's granularity; the pad's gradient is 0.
Step: plan (with the lookup CSR) -> sparse Get -> ops.fm_forward (one launch: S, z, loss, dz, the lookups'
samples) -> ops.fm_backward (every unique row's gradient written once, no atomics) -> sparse Add + the bias
gradient dz.sum() -> Clocks. z = w0 + sum_j w_j x_j + (sum_f (sum_j v_jf x_j)^2 - sum_j sum_f (v_jf x_j)^2) / 2;
the loss is the mean logistic loss over the global batch (dz carries 1 / (B * world)).

``init_std=0.0`` makes the model exactly linear forever: the factor gradient c (S - v x) stays 0.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..ps.comm import Comm
from ..ps.tables import DenseTable, SparseTable


@dataclass
class FMConfig:
    num_dims: int = 16_609_143
    k: int = 16
    lr: float = 0.05
    init_std: float = 0.01
    eps: float = 1e-8
    consistency: str = "bsp"
    staleness: int = 0
    use_bias: bool = True
    lr_bias: float = 0.05
    # the linear column's rule: "adagrad" (the row's second accumulator) or "ftrl" (FTRL-Proximal, L1 / L2)
    linear_optimizer: str = "adagrad"
    linear_alpha: float = 0.1
    linear_beta: float = 1.0
    linear_l1: float = 0.0
    linear_l2: float = 0.0
    # multiplies the pushed (mean-loss) gradient of the FTRL linear column; 0.0: batch size x world, the
    # summed-loss gradient that alpha 0.1, beta 1, l1 about 1 assume
    linear_grad_scale: float = 0.0
    seed: int = 0
    transport: str = "collective"
    storage: str = "vector"
    value_dtype: torch.dtype = torch.float32
    pull_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        if self.k % 4 or not 4 <= self.k <= 60:
            raise ValueError(f"fm: k is {self.k}, expected k % 4 == 0 and 4 <= k <= 60 (rows of k + 4 floats)")
        if self.transport != "collective":
            raise ValueError(f"fm: transport {self.transport!r} is not supported (the one-sided owners apply the "
                             f"row-wise Adagrad of W&D's rows only); use 'collective'")
        if self.storage.lower() != "vector":
            raise ValueError(f"fm: storage {self.storage!r} is not supported (hash / map rows have no split "
                             f"layout); use 'vector'")
        if self.value_dtype != torch.float32 or self.pull_dtype != torch.float32:
            raise ValueError(f"fm: rows are stored and pulled in fp32, not {self.value_dtype} / {self.pull_dtype}")
        if self.linear_optimizer not in ("adagrad", "ftrl"):
            raise ValueError(f"fm: linear_optimizer {self.linear_optimizer!r}: adagrad | ftrl")


class FM:
    def __init__(self, cfg: FMConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        k = cfg.k
        self._ftrl = cfg.linear_optimizer == "ftrl"
        self._ftrl_auto = self._ftrl and not cfg.linear_grad_scale > 0
        ftrl = dict(wide_optimizer="ftrl", wide_lr=cfg.linear_alpha, ftrl_beta=cfg.linear_beta, l1=cfg.linear_l1,
                    l2=cfg.linear_l2, ftrl_grad_scale=cfg.linear_grad_scale if cfg.linear_grad_scale > 0 else 1.0) \
            if self._ftrl else {}
        self.table = SparseTable(comm, cfg.num_dims, k + 4, optimizer="rowwise_adagrad", lr=cfg.lr, eps=cfg.eps,
                                 split=k, pull_dtype=torch.float32, push_dtype=torch.float32,
                                 init_std=cfg.init_std, seed=cfg.seed + 1234, consistency=cfg.consistency,
                                 staleness=cfg.staleness, table_id=0, **ftrl)
        self.table.shard[:, k:].zero_()  # the linear weights and the pad start at zero
        self.bias = DenseTable(comm, 1, optimizer="adagrad", lr=cfg.lr_bias, pull_dtype=torch.float32,
                               consistency=cfg.consistency, staleness=cfg.staleness, eps=cfg.eps, table_id=1) \
            if cfg.use_bias else None

    # -- forward ----------------------------------------------------------------------------
    def _w0(self):
        return self.bias.get() if self.bias is not None else None  # fm_forward reads element 0

    def _forward(self, rowptr, cols, vals, labels, csr: bool):
        plan = self.table.plan(cols, csr=csr)
        rows, plan = self.table.get(cols, plan=plan)
        B = labels.numel()
        out = ops.fm_forward(rowptr, plan.inv, vals, labels, rows, self.cfg.k, self._w0(),
                             1.0 / (max(B, 1) * self.comm.world))
        return rows, plan, out

    def train_step(self, rowptr, cols, vals, labels) -> torch.Tensor:
        """One superstep on a CSR batch (rowptr [B+1], cols / vals [nnz], labels [B] in {0,1} or {-1,1}): Get,
        forward, backward, Add, Clock. Returns the summed loss of this rank's samples (a device tensor; no
        host sync)."""
        k = self.cfg.k
        dev = self.comm.device
        B = labels.numel()
        if self._ftrl_auto:  # the FTRL column sees the summed-loss gradient: batch size x world
            self.table.ftrl_grad_scale = float(max(B, 1) * self.comm.world)
        rows, plan, (S, z, dz, loss, rowid) = self._forward(rowptr, cols, vals, labels, csr=True)
        if plan.keys_n:
            grad_rows = (torch.empty if dev.type == "cuda" else torch.zeros)(max(plan.cap, 1), k + 4,
                                                                             dtype=torch.float32, device=dev)
            csr = plan.csr[:2] if plan.csr is not None else None
            ops.fm_backward(plan.inv, rowid, vals, dz, S, rows, k, grad_rows, csr=csr)
            self.table.add(plan, grad_rows)
        self.table.clock()
        if self.bias is not None:
            self.bias.grad[:1] += dz.sum().reshape(1)
            self.bias.add()
            self.bias.clock()
        return loss.sum()

    def predict_logits(self, rowptr, cols, vals) -> torch.Tensor:
        """Logits [B] of a CSR batch: forward only (a collective Get on several ranks)."""
        labels = torch.zeros(rowptr.numel() - 1, dtype=torch.float32, device=self.comm.device)
        return self._forward(rowptr, cols, vals, labels, csr=False)[2][1]

    def evaluate(self, batches, evaluator=None) -> dict:
        """Held-out evaluation: ``batches`` yields (rowptr, cols, vals, labels); every rank calls it with the
        same number of batches. Forward only -- plan, Get, ops.fm_forward -- with no Add and no Clock:
        training continues afterwards bit for bit as without it. Returns BinaryEvaluator.result() over all
        ranks' samples (``evaluator``: accumulate into this one)."""
        from ..utils.evalmetrics import BinaryEvaluator

        ev = evaluator if evaluator is not None else BinaryEvaluator(self.comm.device)
        for rowptr, cols, vals, labels in batches:
            z = self._forward(rowptr, cols, vals, labels, csr=False)[2][1]
            ev.update_logits(z, (labels > 0.5).float())
        ev.reduce(self.comm)
        return ev.result()

    def linear_nnz(self) -> int:
        """Non-zero linear weights of the whole table (SparseTable.wide_nnz: drains, one all-reduce)."""
        self.drain()
        return self.table.wide_nnz()

    def drain(self):
        self.table.drain()
        if self.bias is not None:
            self.bias.drain()
