"""Gaussian mixture model with diagonal covariances on the GPU parameter server, fitted by stepwise EM (Cappe and
Moulines 2009): the soft counterpart of models/kmeans.py. The table holds the normalised sufficient statistics, not
the parameters; a clock runs the E-step on the local batch and pushes a step towards the batch's statistics.

Parameters
  dense table   K (2D + 1) + D fp32 values, optimizer "add", pulled in fp32: s [K, 2D + 1] (s[k, 0:D] = E[r_k x],
                s[k, D:2D] = E[r_k x^2], s[k, 2D] = E[r_k]) followed by shift [D]. x always means point - shift. shift
                is fixed at construction and never receives a delta; it lives in the table so checkpoints carry it.
Clock: Get -> ops.gmm_prepare (coef, cst from s) -> ops.gmm_estep on the local batch (S, ll) -> push
    rho_t (S / (B world) - s / world),   rho_t = rho0 (t + t0)^-kappa
-> Add -> Clock. The update is linear in each rank's statistics, so the table's own sum over the ranks is the whole
reduction: s <- (1 - rho_t) s + rho_t mean-statistics of the global batch, with no extra collective. Every rank must
bring the same batch size B (the gscale convention of Wide & Deep). rho0 = 1, kappa = 0 on the full data is exact
batch EM. t is the table's own clock count (DenseTable.step, on the host, saved and restored with every checkpoint
and rolled back with the table), so a restored run continues with the step size of an uninterrupted one. Nothing is
read back: a steady one-rank clock issues no host sync; the count of points that were skipped (non-finite lse) is
read at drain(). The rule is stated in csrc/kernels/gmm.h.

covariance="full" gives every component a full covariance matrix (the rule: csrc/kernels/gmm_full.h). The clock, the
step size, the reduction and the checkpoints are the same; the table is K (D + D*D + 1) + D values, s [K, D + D*D + 1]
(E[r_k x] | E[r_k x x^T] row-major | E[r_k]) followed by shift, the operands come from ops.gmm_full_prepare (a
Cholesky factor's inverse per component, reg_covar added to the diagonal; var_floor is unused) and the E-step is
ops.gmm_full_estep. The start is the seeding's centres with Sigma = diag(data variance). D <= 64.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _native, ops
from ..ps.comm import Comm
from ..ps.tables import DenseTable
from .kmeans import init_centres


@dataclass
class GMMConfig:
    K: int = 8
    dims: int = 16
    var_floor: float = 1e-4
    rho0: float = 1.0
    kappa: float = 0.0
    t0: float = 1.0
    consistency: str = "bsp"
    staleness: int = 0
    seed: int = 0
    init_mode: str = "kmeans++"
    transport: str = "collective"
    covariance: str = "diag"
    reg_covar: float = 1e-6

    def __post_init__(self):
        if self.covariance not in ("diag", "full"):
            raise ValueError(f"gmm: unknown covariance {self.covariance!r}, expected 'diag' or 'full'")
        if self.covariance == "full":
            if not ops.gmm_full_shape_ok(self.K, self.dims):
                raise ValueError(f"gmm: covariance 'full' with K = {self.K}, dims = {self.dims}, expected 1 <= K <= "
                                 f"{ops.GMM_FULL_MAX_K} and 1 <= dims <= {ops.GMM_FULL_MAX_D}")
            if not (self.reg_covar >= 0 and self.reg_covar < float("inf")):  # (a NaN fails the comparison)
                raise ValueError(f"gmm: reg_covar is {self.reg_covar}, expected a finite value >= 0")
        if not ops.gmm_shape_ok(self.K, self.dims):
            raise ValueError(f"gmm: K = {self.K}, dims = {self.dims}, expected 1 <= K <= {ops.GMM_MAX_K}, 1 <= dims <= "
                             f"{ops.GMM_MAX_D} and 16 ceil(K / 16) * 16 ceil(dims / 16) <= {ops.GMM_MAX_KD}")
        if not (self.var_floor > 0 and self.var_floor < float("inf")):  # (a NaN fails the comparison)
            raise ValueError(f"gmm: var_floor is {self.var_floor}, expected a finite value > 0")
        if not 0 < self.rho0 <= 1 or not 0 <= self.kappa <= 1 or not self.t0 > 0:
            raise ValueError(f"gmm: rho0 {self.rho0}, kappa {self.kappa}, t0 {self.t0}: expected 0 < rho0 <= 1, "
                             f"0 <= kappa <= 1 and t0 > 0")
        if self.transport != "collective":
            raise ValueError(f"gmm: transport {self.transport!r} is not supported (the one-sided owners apply the "
                             f"optimizers of W&D's tables only); use 'collective'")
        if self.init_mode not in ("random", "kmeans++", "kmeans_parallel"):
            raise ValueError(f"gmm: unknown init_mode {self.init_mode!r}")


class GMM:
    def __init__(self, cfg: GMMConfig, comm: Comm, init_data: torch.Tensor | None = None):
        self.cfg, self.comm = cfg, comm
        K, D = cfg.K, cfg.dims
        self.full = cfg.covariance == "full"
        self.W = ops.gmm_full_width(D) if self.full else 2 * D + 1
        dev = comm.device
        if dev.type == "cuda":  # a missing kernel is an error, here and not at the first clock
            ext = "_gmmfk" if self.full else "_gmmk"
            try:
                _native.gmmfk() if self.full else _native.gmmk()
            except RuntimeError as e:
                raise ValueError(f"gmm: the model runs on {dev} and needs the {ext} extension: {e}") from e
        self.table = DenseTable(comm, K * self.W + D, optimizer="add", pull_dtype=torch.float32,
                                consistency=cfg.consistency, staleness=cfg.staleness)
        if init_data is not None:
            X = self._points(init_data)
            centres = init_centres(X, K, cfg.init_mode, cfg.seed, comm).double().cpu()
            # the data mean and per-dimension variance over every rank's seeding batch
            Xd = X.double()
            mom = torch.cat([Xd.sum(0), (Xd * Xd).sum(0), torch.tensor([float(X.shape[0])], dtype=torch.float64,
                                                                      device=X.device)])
            if comm.world > 1 and not comm.emulated:
                comm.all_reduce_(mom)
            mom = mom.cpu()
            shift = mom[:D] / mom[2 * D]
            var = (mom[D:2 * D] / mom[2 * D] - shift * shift).clamp(min=cfg.var_floor)
        else:
            centres = torch.randn(K, D, generator=torch.Generator().manual_seed(cfg.seed)).double()
            shift, var = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
        mu = centres - shift
        if self.full:
            S2 = torch.diag(var)[None] + mu[:, :, None] * mu[:, None, :]
            s = torch.cat([mu, S2.reshape(K, D * D), torch.ones(K, 1, dtype=torch.float64)], 1) / K
        else:
            s = torch.cat([mu, var + mu * mu, torch.ones(K, 1, dtype=torch.float64)], 1) / K
        self.table.load_full(torch.cat([s.reshape(-1), shift]).float())
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.bad_total = 0       # points skipped for a non-finite lse, as of the last drain()

    def _points(self, X):
        if X.dim() != 2 or X.shape[1] != self.cfg.dims or X.dtype != torch.float32:
            raise ValueError(f"gmm: points must be fp32 [n, {self.cfg.dims}], got {X.dtype} {tuple(X.shape)}")
        return X

    def _state(self):
        K, D, W = self.cfg.K, self.cfg.dims, self.W
        P = self.table.get()
        return P[: K * W].view(K, W), P[K * W: K * W + D]

    def _estep(self, X, **kw):
        s, shift = self._state()
        if self.full:
            return s, ops.gmm_full_estep(X, shift, *ops.gmm_full_prepare(s, self.cfg.reg_covar), **kw)
        return s, ops.gmm_estep(X, shift, *ops.gmm_prepare(s, self.cfg.var_floor), **kw)

    def train_step(self, X):
        """X [B, D] fp32, the same B on every rank. Returns the batch's summed log-likelihood (fp64 [1], before the
        update)."""
        X = self._points(X)
        cfg, K, W = self.cfg, self.cfg.K, self.W
        s, (S, ll, _, _) = self._estep(X, bad=self.bad)
        rho = cfg.rho0 * (self.table.step + cfg.t0) ** -cfg.kappa  # the table's clock count: checkpoints carry it
        world = self.comm.world
        G = self.table.grad
        torch.sub(S, s, alpha=float(X.shape[0]), out=G[: K * W].view(K, W)).mul_(rho / (X.shape[0] * world))
        G[K * W:].zero_()
        self.table.add()
        self.table.clock()
        return ll

    def predict(self, X):
        """(assign int32 [n], logp fp32 [n]): the most responsible component and the log density of every point."""
        X = self._points(X)
        _, (_, _, assign, logp) = self._estep(X, accumulate=False, want_assign=True, want_logp=True)
        return assign, logp

    def params(self):
        """(pi [K], mu [K, D], var [K, D]) in the points' own coordinates (torch code, not the hot path); in full mode
        the third value is cov [K, D, D]."""
        s, shift = self._state()
        D = self.cfg.dims
        if self.full:
            s0 = s[:, -1]
            mu = s[:, :D] / s0[:, None]
            cov = s[:, D:D + D * D].reshape(-1, D, D) / s0[:, None, None] - mu[:, :, None] * mu[:, None, :]
            return s0 / s0.sum(), mu + shift, cov + self.cfg.reg_covar * torch.eye(D, device=s.device)
        s0 = s[:, 2 * D]
        mu = s[:, :D] / s0[:, None]
        var = (s[:, D:2 * D] / s0[:, None] - mu * mu).clamp(min=self.cfg.var_floor)
        return s0 / s0.sum(), mu + shift, var

    def drain(self):
        self.table.drain()
        self.bad_total += int(self.bad.item())
        self.bad.zero_()
