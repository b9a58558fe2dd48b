"""Field-aware factorization machine (Juan et al., 2016) on the GPU parameter server: the FM whose features
keep one vector per partner field, over the same general CSR (libsvm) input as sparse LR and the FM.

Parameters
  sparse table  one fp32 split row per feature, [F slots of k factors | 1 linear weight | 3 pad]: slot g is the
                vector the feature uses against a partner of field g. Row-wise Adagrad on the F k factors, and on
                the linear column either its own Adagrad accumulator (``linear_optimizer="adagrad"``) or
                FTRL-Proximal with L1 / L2 (``"ftrl"``, SparseTable(wide_optimizer="ftrl")).
  dense table   the bias w0: a minimal DenseTable (Adagrad).
Fields: a lookup's field is given with the batch (``fields``, int32 per lookup) or derived from its key:
``field_bounds`` (F - 1 ascending key boundaries, torch.bucketize) or, by default, equal key ranges of
ceil(num_dims / F) keys.
Step: plan (with the lookup CSR) -> sparse Get -> ops.ffm_forward (one launch: z, loss, dz, the lookups'
samples) -> ops.ffm_backward (every unique row's gradient written once, no atomics, recomputed from the rows)
-> sparse Add + the bias gradient dz.sum() -> Clocks. z = w0 + sum_j w_j x_j + sum_{i<j} <v_{i, f_j}, v_{j, f_i}>
x_i x_j; the loss is the mean logistic loss over the global batch (dz carries 1 / (B * world)).

``init_std=0.0`` makes the model exactly linear forever: every factor gradient is a sum of other factors.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import ops
from ..ps.comm import Comm
from ..ps.tables import DenseTable, SparseTable


@dataclass
class FFMConfig:
    num_dims: int = 16_609_143
    num_fields: int = 8
    k: int = 4
    # F - 1 ascending key boundaries: a key's field is the number of boundaries <= key (None: equal ranges)
    field_bounds: Optional[Sequence[int]] = None
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
    # multiplies the pushed (mean-loss) gradient of the FTRL linear column; 0.0: batch size x world
    linear_grad_scale: float = 0.0
    seed: int = 0
    transport: str = "collective"
    storage: str = "vector"
    value_dtype: torch.dtype = torch.float32
    pull_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        F, k = self.num_fields, self.k
        if k % 4 or not 4 <= k <= ops.FFM_MAX_K:
            raise ValueError(f"ffm: k is {k}, expected k % 4 == 0 and 4 <= k <= {ops.FFM_MAX_K}")
        if not 1 <= F <= ops.FFM_MAX_F or F * k > ops.FFM_MAX_FK:
            raise ValueError(f"ffm: num_fields is {F} (k {k}), expected 1 <= num_fields <= {ops.FFM_MAX_F} and "
                             f"num_fields * k <= {ops.FFM_MAX_FK} (rows of num_fields * k + 4 floats)")
        if self.field_bounds is not None:
            fb = [int(v) for v in self.field_bounds]
            if len(fb) != F - 1 or any(b <= a for a, b in zip(fb, fb[1:])):
                raise ValueError(f"ffm: field_bounds needs num_fields - 1 = {F - 1} ascending keys, got {fb}")
        if self.transport != "collective":
            raise ValueError(f"ffm: transport {self.transport!r} is not supported (the one-sided owners apply the "
                             f"row-wise Adagrad of W&D's rows only); use 'collective'")
        if self.storage.lower() != "vector":
            raise ValueError(f"ffm: storage {self.storage!r} is not supported (hash / map rows have no split "
                             f"layout); use 'vector'")
        if self.value_dtype != torch.float32 or self.pull_dtype != torch.float32:
            raise ValueError(f"ffm: rows are stored and pulled in fp32, not {self.value_dtype} / {self.pull_dtype}")
        if self.linear_optimizer not in ("adagrad", "ftrl"):
            raise ValueError(f"ffm: linear_optimizer {self.linear_optimizer!r}: adagrad | ftrl")


class FFM:
    def __init__(self, cfg: FFMConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        F, k = cfg.num_fields, cfg.k
        self.FK = F * k
        self._ftrl = cfg.linear_optimizer == "ftrl"
        self._ftrl_auto = self._ftrl and not cfg.linear_grad_scale > 0
        ftrl = dict(wide_optimizer="ftrl", wide_lr=cfg.linear_alpha, ftrl_beta=cfg.linear_beta, l1=cfg.linear_l1,
                    l2=cfg.linear_l2, ftrl_grad_scale=cfg.linear_grad_scale if cfg.linear_grad_scale > 0 else 1.0) \
            if self._ftrl else {}
        self.table = SparseTable(comm, cfg.num_dims, self.FK + 4, optimizer="rowwise_adagrad", lr=cfg.lr, eps=cfg.eps,
                                 split=self.FK, pull_dtype=torch.float32, push_dtype=torch.float32,
                                 init_std=cfg.init_std, seed=cfg.seed + 1234, consistency=cfg.consistency,
                                 staleness=cfg.staleness, table_id=0, **ftrl)
        self.table.shard[:, self.FK:].zero_()  # the linear weights and the pad start at zero
        self.bias = DenseTable(comm, 1, optimizer="adagrad", lr=cfg.lr_bias, pull_dtype=torch.float32,
                               consistency=cfg.consistency, staleness=cfg.staleness, eps=cfg.eps, table_id=1) \
            if cfg.use_bias else None
        self._bounds = torch.tensor([int(v) for v in cfg.field_bounds], dtype=torch.int64, device=comm.device) \
            if cfg.field_bounds is not None else None
        self._span = -(-cfg.num_dims // F)  # the default: equal key ranges

    # -- fields -----------------------------------------------------------------------------
    def fields_of(self, cols: torch.Tensor) -> torch.Tensor:
        """The field (int32) of every key: the number of ``field_bounds`` <= key, or key // ceil(num_dims / F)
        clamped to F - 1."""
        if self._bounds is not None:
            return torch.bucketize(cols, self._bounds, right=True).to(torch.int32)
        return torch.div(cols, self._span, rounding_mode="floor").clamp_(0, self.cfg.num_fields - 1).to(torch.int32)

    # -- forward ----------------------------------------------------------------------------
    def _w0(self):
        return self.bias.get() if self.bias is not None else None  # ffm_forward reads element 0

    def _forward(self, rowptr, cols, vals, labels, fields, csr: bool):
        fields = self.fields_of(cols) if fields is None else fields.to(torch.int32)
        plan = self.table.plan(cols, csr=csr)
        rows, plan = self.table.get(cols, plan=plan)
        B = labels.numel()
        out = ops.ffm_forward(rowptr, plan.inv, vals, fields, labels, rows, self.cfg.num_fields, self.cfg.k,
                              self._w0(), 1.0 / (max(B, 1) * self.comm.world))
        return rows, plan, fields, out

    def train_step(self, rowptr, cols, vals, labels, fields=None) -> torch.Tensor:
        """One superstep on a CSR batch (rowptr [B+1], cols / vals [nnz], labels [B] in {0,1} or {-1,1},
        ``fields`` int32 [nnz] or None: derived from the keys): Get, forward, backward, Add, Clock. Returns the
        summed loss of this rank's samples (a device tensor; no host sync)."""
        F, k = self.cfg.num_fields, self.cfg.k
        dev = self.comm.device
        B = labels.numel()
        if self._ftrl_auto:  # the FTRL column sees the summed-loss gradient: batch size x world
            self.table.ftrl_grad_scale = float(max(B, 1) * self.comm.world)
        rows, plan, fields, (z, dz, loss, rowid) = self._forward(rowptr, cols, vals, labels, fields, csr=True)
        if plan.keys_n:
            grad_rows = (torch.empty if dev.type == "cuda" else torch.zeros)(max(plan.cap, 1), self.FK + 4,
                                                                             dtype=torch.float32, device=dev)
            csr = plan.csr[:2] if plan.csr is not None else None
            ops.ffm_backward(plan.inv, rowid, rowptr, vals, fields, dz, rows, F, k, grad_rows, csr=csr)
            self.table.add(plan, grad_rows)
        self.table.clock()
        if self.bias is not None:
            self.bias.grad[:1] += dz.sum().reshape(1)
            self.bias.add()
            self.bias.clock()
        return loss.sum()

    def predict_logits(self, rowptr, cols, vals, fields=None) -> torch.Tensor:
        """Logits [B] of a CSR batch: forward only (a collective Get on several ranks)."""
        labels = torch.zeros(rowptr.numel() - 1, dtype=torch.float32, device=self.comm.device)
        return self._forward(rowptr, cols, vals, labels, fields, csr=False)[3][0]

    def evaluate(self, batches, evaluator=None) -> dict:
        """Held-out evaluation: ``batches`` yields (rowptr, cols, vals, labels) or (rowptr, cols, vals, labels,
        fields); every rank calls it with the same number of batches. Forward only -- plan, Get,
        ops.ffm_forward -- with no Add and no Clock: training continues afterwards bit for bit as without it.
        Returns BinaryEvaluator.result() over all ranks' samples (``evaluator``: accumulate into this one)."""
        from ..utils.evalmetrics import BinaryEvaluator

        ev = evaluator if evaluator is not None else BinaryEvaluator(self.comm.device)
        for batch in batches:
            rowptr, cols, vals, labels = batch[:4]
            fields = batch[4] if len(batch) > 4 else None
            z = self._forward(rowptr, cols, vals, labels, fields, csr=False)[3][0]
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
