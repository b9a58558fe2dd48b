"""Collaborative filtering by alternating least squares on the GPU parameter server (Zhou et al. 2008, "ALS-WR";
Hu, Koren and Volinsky 2008 for implicit feedback): the sparse-table model that is not trained by gradients. A clock
pulls the rows of one side, forms one small normal-equation system per entity (a k x k Gram matrix of gathered rows),
solves it and pushes the new row as x_new - x_old.

Parameters
  sparse table  U + I fp32 rows of k floats, optimizer "add" (the reference server's w += delta), range-routed: key
                u < U is user u's factor, key U + i item i's (N(0, init_std)). The table is plain: save / restore /
                N -> M resharding go through the name-generic checkpoint code.
Half-sweep: the entities of one side, ``batch_entities`` consecutive ones per clock. Clock: plan + Get of the batch's
other-side keys -> plan + Get of the entity keys (the old rows; slot = the plan's inv) -> ops.als_solve (one fused
launch, a fold launch when an entity has several chunks) -> sparse Add of delta -> Clock. Only entity rows are pushed.
Nothing is read back: a steady one-rank clock issues no host sync; the count of entities whose factorisation failed
is read at drain(). The rule is stated in csrc/kernels/als.h.

``attach_users`` / ``attach_items`` keep a rank's slice of the rating matrix (CSR by user) and of its transpose (CSR
by item) resident and fix the batches, their weights and their chunk descriptors -- the only host read of rowptr.
Every rank owns a disjoint slice of each side and runs the all-reduced maximum number of clocks.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _native, ops
from ..ps.comm import Comm
from ..ps.tables import SparseTable


@dataclass
class ALSConfig:
    users: int = 1 << 12
    items: int = 1 << 10
    k: int = 32
    reg: float = 0.05
    weighted_reg: bool = True
    implicit: bool = False
    alpha: float = 40.0
    batch_entities: int = 4096
    init_std: float = 0.1
    seed: int = 0
    chunk: int = ops.ALS_CHUNK
    consistency: str = "bsp"
    staleness: int = 0
    transport: str = "collective"
    storage: str = "vector"
    value_dtype: torch.dtype = torch.float32
    pull_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        if self.users < 1 or self.items < 1 or self.users + self.items >= 1 << 31:
            raise ValueError(f"als: users {self.users} and items {self.items}, expected >= 1 and fewer than 2^31 rows")
        if self.k % 4 or not ops.ALS_MIN_K <= self.k <= ops.ALS_MAX_K:
            raise ValueError(f"als: k is {self.k}, expected k % 4 == 0 and {ops.ALS_MIN_K} <= k <= {ops.ALS_MAX_K}")
        if not self.reg > 0:  # (a NaN fails the comparison)
            raise ValueError(f"als: reg is {self.reg}, expected > 0 (it makes every system positive definite)")
        if not self.alpha > 0:
            raise ValueError(f"als: alpha is {self.alpha}, expected > 0")
        if not self.init_std > 0:
            raise ValueError(f"als: init_std is {self.init_std}, expected > 0 (zero rows never leave zero)")
        if self.batch_entities < 1 or not 1 <= self.chunk <= ops.ALS_MAX_CHUNK:
            raise ValueError(f"als: batch_entities {self.batch_entities} and chunk {self.chunk}, expected >= 1 and "
                             f"chunk <= {ops.ALS_MAX_CHUNK}")
        if self.transport != "collective":
            raise ValueError(f"als: transport {self.transport!r} is not supported (the one-sided owners apply the "
                             f"row-wise Adagrad of W&D's rows only); use 'collective'")
        if self.consistency.lower() != "bsp" or self.staleness:
            raise ValueError(f"als: consistency {self.consistency!r} (staleness {self.staleness}) is not supported: a "
                             f"half-sweep reads one side while it writes the other; use 'bsp'")
        if self.storage.lower() != "vector":
            raise ValueError(f"als: storage {self.storage!r} is not supported (users and items are the two key ranges "
                             f"of a range table); use 'vector'")
        if self.value_dtype != torch.float32 or self.pull_dtype != torch.float32:
            raise ValueError(f"als: rows are stored and pulled in fp32, not {self.value_dtype} / {self.pull_dtype}")


def transpose_csr(rowptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor, n_cols: int):
    """The transpose of a full CSR matrix with one stable sort: (rowptr [n_cols + 1], rows, vals) by column, the
    entries of a column in row order."""
    rowptr, cols = rowptr.to(torch.int64).reshape(-1), cols.to(torch.int64).reshape(-1)
    rid = torch.repeat_interleave(torch.arange(rowptr.numel() - 1, dtype=torch.int64, device=cols.device),
                                  rowptr[1:] - rowptr[:-1])
    order = torch.sort(cols, stable=True).indices
    tp = torch.zeros(n_cols + 1, dtype=torch.int64, device=cols.device)
    tp[1:] = torch.cumsum(torch.bincount(cols, minlength=n_cols), 0)
    return tp, rid[order], vals.reshape(-1)[order]


class ALS:
    def __init__(self, cfg: ALSConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        self.U, self.I, self.k = cfg.users, cfg.items, cfg.k
        if comm.device.type == "cuda":  # a missing kernel is an error, here and not at the first clock
            try:
                _native.alsk()
            except RuntimeError as e:
                raise ValueError(f"als: the model runs on {comm.device} and needs the _alsk extension: {e}") from e
        self.table = SparseTable(comm, self.U + self.I, self.k, optimizer="add", pull_dtype=torch.float32,
                                 push_dtype=torch.float32, value_dtype=torch.float32, init_std=cfg.init_std,
                                 seed=cfg.seed + 1234, consistency="bsp", route="range", table_id=0)
        self.sides = {}          # "users" / "items": the attached slice and its batches
        self.bad = torch.zeros(1, dtype=torch.int32, device=comm.device)
        self.bad_total = 0       # entities whose factorisation failed, as of the last drain()
        self.sweeps = 0

    # -- data -------------------------------------------------------------------------------
    def attach_users(self, rowptr, cols, vals, user_base: int = 0):
        """Keeps this rank's slice of the rating matrix by user: user user_base + e rated the items
        cols[rowptr[e]:rowptr[e + 1]] with vals. Collective (the clock count is all-reduced)."""
        return self._attach("users", rowptr, cols, vals, user_base)

    def attach_items(self, rowptr, cols, vals, item_base: int = 0):
        """Keeps this rank's slice of the transpose: item item_base + e was rated by the users cols[...]."""
        return self._attach("items", rowptr, cols, vals, item_base)

    def _attach(self, side, rowptr, cols, vals, base):
        cfg, dev = self.cfg, self.comm.device
        n_own, n_other = (self.U, self.I) if side == "users" else (self.I, self.U)
        rp = rowptr.detach().to("cpu", torch.int64).reshape(-1)
        co = cols.detach().to("cpu", torch.int64).reshape(-1)
        va = vals.detach().to("cpu", torch.float32).reshape(-1)
        E, n = rp.numel() - 1, co.numel()
        if E < 0 or int(rp[0]) != 0 or int(rp[-1]) != n or bool((rp[1:] < rp[:-1]).any()) or va.numel() != n:
            raise ValueError(f"als: attach_{side}: rowptr must ascend from 0 to the {n} ratings it indexes")
        if base < 0 or base + E > n_own:
            raise ValueError(f"als: attach_{side}: entities {base} .. {base + E} must lie in [0, {n_own}]")
        if n and (int(co.min()) < 0 or int(co.max()) >= n_other):
            raise ValueError(f"als: attach_{side}: ids must lie in [0, {n_other}), found {int(co.min())} .. "
                             f"{int(co.max())}")
        if cfg.implicit and n and float(va.min()) < 0:
            raise ValueError(f"als: attach_{side}: implicit feedback takes ratings >= 0")
        key0, other0 = (0, self.U) if side == "users" else (self.U, 0)
        batches = []
        for e0 in range(0, E, cfg.batch_entities):
            e1 = min(e0 + cfg.batch_entities, E)
            lo, hi = int(rp[e0]), int(rp[e1])
            brp = rp[e0:e1 + 1] - lo
            r = va[lo:hi]
            a, c = (cfg.alpha * r, 1.0 + cfg.alpha * r) if cfg.implicit else (torch.ones_like(r), r)
            ne = (brp[1:] - brp[:-1]).float()
            reg = cfg.reg * ne if (cfg.weighted_reg and not cfg.implicit) else torch.full_like(ne, cfg.reg)
            desc, multi, nmd = ops.als_chunks(brp, cfg.chunk)
            batches.append(dict(rowptr=brp.to(dev), okeys=(co[lo:hi] + other0).to(dev), a=a.to(dev), c=c.to(dev),
                                reg=reg.to(dev), ekeys=(torch.arange(e0, e1, dtype=torch.int64) + key0 + base).to(dev),
                                chunks=(desc.to(dev), multi.to(dev), nmd)))
        clocks = torch.tensor([len(batches)], dtype=torch.int64, device=dev)
        if self.comm.world > 1 and not self.comm.emulated:
            self.comm.all_reduce_(clocks, op=torch.distributed.ReduceOp.MAX)
        self.sides[side] = dict(batches=batches, clocks=int(clocks), rowptr=rp.to(dev), cols=co.to(dev),
                                vals=va.to(dev), base=base, E=E)
        return self

    # -- one clock --------------------------------------------------------------------------
    def _clock(self, b, gram0=None):
        """One clock of a half-sweep on the batch ``b`` (None: this rank's slice is exhausted; it plans zero keys
        and clocks)."""
        dev, t, k = self.comm.device, self.table, self.k
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        okeys, ekeys = (b["okeys"], b["ekeys"]) if b is not None else (empty, empty)
        plan_o = t.plan(okeys)
        rows, plan_o = t.get(okeys, plan=plan_o)
        plan_e = t.plan(ekeys)
        x_old, plan_e = t.get(ekeys, plan=plan_e)
        m = x_old.shape[0]
        if b is not None and m:
            assert m >= plan_e.cap
            x_out = torch.empty_like(x_old)
            delta = torch.zeros_like(x_old)
            ops.als_solve(b["rowptr"], plan_o.inv, b["a"], b["c"], rows, b["reg"], plan_e.inv, x_old, x_out, delta,
                          b["chunks"], gram0=gram0, bad=self.bad)
            t.add(plan_e, delta)
        elif self.comm.world > 1:  # the push is a collective: a rank without entities pushes zero rows
            t.add(plan_e, torch.zeros(max(plan_e.cap, 1), k, dtype=torch.float32, device=dev))
        t.clock()

    def _gram(self, side):
        """Y^T Y over all rows of the other side: ops.als_gram over the owned shard rows of its key range, then one
        all-reduce of k * k floats."""
        lo, hi = (self.U, self.U + self.I) if side == "users" else (0, self.U)
        G = ops.als_gram(self.table.local_rows(lo, hi))
        if self.comm.world > 1 and not self.comm.emulated:
            self.comm.all_reduce_(G)
        return G

    def half_sweep(self, side: str):
        """Solves every attached entity of ``side`` ("users" | "items") from the other side's rows."""
        if side not in self.sides:
            raise ValueError(f"als: half_sweep({side!r}) before attach_{side}(rowptr, cols, vals)")
        s = self.sides[side]
        gram0 = self._gram(side) if self.cfg.implicit else None
        for c in range(s["clocks"]):
            self._clock(s["batches"][c] if c < len(s["batches"]) else None, gram0)

    def sweep(self):
        """The user half, then the item half. Returns nothing from the device."""
        for side in ("users", "items"):
            if side not in self.sides:
                raise ValueError(f"als: sweep before attach_{side}(rowptr, cols, vals)")
        self.half_sweep("users")
        self.half_sweep("items")
        self.sweeps += 1

    # -- reports (torch code, not the hot path) -------------------------------------------------
    def _dots(self, u, i):
        """fp32 <x_u, y_i> per pair (collective: two Gets)."""
        dev = self.comm.device
        X = self.table.get_rows(u.to(dev, torch.int64))
        Y = self.table.get_rows(i.to(dev, torch.int64) + self.U)
        return (X * Y).sum(1)

    def _sum(self, v: torch.Tensor) -> torch.Tensor:
        v = v.double().reshape(-1)
        if self.comm.world > 1 and not self.comm.emulated:
            self.comm.all_reduce_(v)
        return v

    def rmse(self, u, i, r) -> float:
        """Root mean squared error of the ratings (u, i, r) of every rank (collective): fp32 gathered dot products,
        summed in fp64."""
        dev = self.comm.device
        err = self._dots(u, i).double() - r.to(dev).double()
        s = self._sum(torch.stack([(err * err).sum(), torch.tensor(float(err.numel()), dtype=torch.float64,
                                                                   device=dev)]))
        return float((s[0] / s[1].clamp(min=1.0)).sqrt())

    def objective(self) -> float:
        """The regularised objective ALS minimises, over all ranks (collective). Explicit: sum (r - <x, y>)^2 +
        lambda sum_e w_e |x_e|^2 over both sides, w_e = n_e (weighted_reg) or 1. Implicit: sum over every (u, i) of
        c_ui (p_ui - <x, y>)^2 + lambda (|X|^2 + |Y|^2), the unobserved pairs through <X^T X, Y^T Y>."""
        for side in ("users", "items"):
            if side not in self.sides:
                raise ValueError(f"als: objective before attach_{side}(rowptr, cols, vals)")
        cfg, dev, su = self.cfg, self.comm.device, self.sides["users"]
        uid = torch.repeat_interleave(torch.arange(su["E"], dtype=torch.int64, device=dev),
                                      su["rowptr"][1:] - su["rowptr"][:-1]) + su["base"]
        s, r = self._dots(uid, su["cols"]).double(), su["vals"].double()
        if cfg.implicit:
            fit = ((1.0 + cfg.alpha * r) * (1.0 - s) ** 2 - s * s).sum()
        else:
            fit = ((r - s) ** 2).sum()
        pen = torch.zeros((), dtype=torch.float64, device=dev)
        grams = []
        for side, key0 in (("users", 0), ("items", self.U)):
            sd = self.sides[side]
            X = self.table.get_rows(torch.arange(sd["E"], dtype=torch.int64, device=dev) + key0 + sd["base"]).double()
            w = (sd["rowptr"][1:] - sd["rowptr"][:-1]).double() if (cfg.weighted_reg and not cfg.implicit) \
                else torch.ones(sd["E"], dtype=torch.float64, device=dev)
            pen = pen + cfg.reg * (w * (X * X).sum(1)).sum()
            grams.append(self._sum(X.t() @ X))
        total = self._sum(torch.stack([fit, pen])).sum()
        if cfg.implicit:
            total = total + (grams[0] * grams[1]).sum()
        return float(total)

    def drain(self):
        self.table.drain()
        self.bad_total += int(self.bad.item())
        self.bad.zero_()
