"""The full-covariance Gaussian mixture (CPU): ops.gmm_full_* against fp64, EM, ranks, checkpoints and refusals."""
import math

import pytest
import torch

from test_gmm import CPU, F64, LOG_2PI
from test_ps_gloo import run_world

from minips_amd import _native, ops
from minips_amd.data.synthetic import GMMSynth
from minips_amd.models.gmm import GMM, GMMConfig
from minips_amd.ps.checkpoint import Checkpointer
from minips_amd.ps.comm import Comm


def prepare64(s, reg):
    """gmm_full.h's Prepare in fp64 from the fp32 statistics: (Wh [K, DP, DP], b [K, DP], cst [K], Sigma [K, D, D])."""
    s = s.double()
    K, D = s.shape[0], math.isqrt(s.shape[1] - 1)
    dp = ops.gmm_pad(D)
    s0 = s[:, -1]
    tot = s0[torch.isfinite(s0) & (s0 > 0)].sum()
    Wh, b = torch.zeros(K, dp, dp, dtype=F64), torch.zeros(K, dp, dtype=F64)
    cst = torch.full((K,), -math.inf, dtype=F64)
    sigma = torch.zeros(K, D, D, dtype=F64)
    for k in range(K):
        if bool(torch.isfinite(s[k]).all()) and s0[k] > 0:
            mu = s[k, :D] / s0[k]
            sigma[k] = s[k, D:D + D * D].view(D, D) / s0[k] - torch.outer(mu, mu) + reg * torch.eye(D, dtype=F64)
            L, info = torch.linalg.cholesky_ex(sigma[k])
            if int(info) == 0:
                Wh[k, :D, :D] = torch.linalg.solve_triangular(L, torch.eye(D, dtype=F64), upper=False)
                b[k, :D] = Wh[k, :D, :D] @ mu
                cst[k] = math.log(s0[k] / tot) - float(L.diagonal().log().sum()) - 0.5 * D * LOG_2PI
    return Wh, b, cst, sigma


def estep64(X, shift, Wh, b, cst):
    """gmm_full.h's E-step as an fp64 loop over the components; ymag [n, K, D] = sum_d |Wh_jd x_d| + |b_j|."""
    x = X.double() - shift.double()
    n, D, K = x.shape[0], x.shape[1], cst.numel()
    t, y, ymag = torch.empty(n, K, dtype=F64), torch.empty(n, K, D, dtype=F64), torch.empty(n, K, D, dtype=F64)
    for k in range(K):
        Wk, bk = Wh[k, :D, :D].double(), b[k, :D].double()
        y[:, k] = x @ Wk.t() - bk
        ymag[:, k] = x.abs() @ Wk.abs().t() + bk.abs()
        t[:, k] = cst[k].double() - 0.5 * (y[:, k] ** 2).sum(1)
    m = torch.nan_to_num(t, nan=-math.inf).max(1).values
    lse = m + (t - m[:, None]).exp().sum(1).log()
    ok = torch.isfinite(lse)
    r = torch.where(ok[:, None], (t - lse[:, None]).exp(), torch.zeros((), dtype=F64))
    xz = torch.where(ok[:, None], x, torch.zeros((), dtype=F64))
    S2 = torch.stack([(xz * r[:, k:k + 1]).t() @ xz for k in range(K)])
    S = torch.cat([r.t() @ xz, S2.reshape(K, D * D), r.sum(0)[:, None]], 1)
    return dict(t=t, y=y, ymag=ymag, lse=lse, r=r, S=S, ll=float(lse[ok].sum()), ok=ok, x=xz)


def planted(K, D, n, seed, sep=0.5):
    """Points of a planted, rotated mixture, shift = their mean and the mixture's own statistics s [K, D + D*D + 1]."""
    syn = GMMSynth(n, dims=D, K_teacher=K, sep=sep, seed=seed, rotate=True)
    X = syn.next()
    shift = X.mean(0)
    mu = syn.centres - shift
    cov = torch.einsum("kde,ke,kfe->kdf", syn.rot, syn.sigma ** 2, syn.rot)
    cov = torch.tril(cov) + torch.tril(cov, -1).transpose(1, 2)
    s = torch.cat([mu, (cov + mu[:, :, None] * mu[:, None, :]).reshape(K, D * D), torch.ones(K, 1)], 1)
    return X, shift, (s * syn.weights[:, None]).float().contiguous()


@pytest.mark.parametrize("K,D", [(1, 1), (3, 5), (5, 17)])
def test_cpu_reference_matches_the_fp64_loop(K, D):
    X, shift, s = planted(K, D, 37, seed=K + D, sep=2.0)
    Wh, b, cst = ops.gmm_full_prepare(s, 1e-6)
    W64, b64, c64, _ = prepare64(s, 1e-6)
    dp = ops.gmm_pad(D)
    assert Wh.shape == (K, dp, dp) and torch.allclose(Wh.double(), W64, rtol=1e-4, atol=1e-5)
    assert torch.allclose(b.double(), b64, rtol=1e-4, atol=1e-4) and torch.allclose(cst.double(), c64, atol=1e-4)
    assert not Wh.triu(1).any() and not Wh[:, D:].any() and not b[:, D:].any()
    bad = torch.zeros(1, dtype=torch.int32)
    S, ll, assign, logp = ops.gmm_full_estep(X, shift, Wh, b, cst, want_assign=True, want_logp=True, bad=bad)
    ref = estep64(X, shift, Wh, b, cst)
    assert torch.allclose(S.double(), ref["S"], rtol=1e-4, atol=1e-4) and int(bad) == 0
    S2 = S[:, D:D + D * D].view(K, D, D)
    assert torch.equal(S2, S2.transpose(1, 2))   # symmetric to the bit
    assert abs(float(ll) - ref["ll"]) <= 1e-5 * abs(ref["ll"]) and ll.dtype == F64
    assert torch.allclose(logp.double(), ref["lse"], rtol=1e-5, atol=1e-4)
    assert torch.equal(assign.long(), ref["t"].argmax(1)) and assign.dtype == torch.int32
    none = ops.gmm_full_estep(X, shift, Wh, b, cst, accumulate=False)
    assert none[0] is None and none[2] is None and torch.equal(none[1], ll)


def edge_case(dev=CPU):
    """Component 1 dead by its weight, component 2 by a pivot (an indefinite moment), a NaN feature in point 2."""
    X, shift, s = planted(4, 6, 9, seed=3, sep=2.0)
    s[1, -1] = 0.0
    s[2, 6 + 2 * 6 + 2] = -1.0
    X[2, 4] = float("nan")
    Wh, b, cst = ops.gmm_full_prepare(s.to(dev), 1e-6)
    return X.to(dev), shift.to(dev), Wh, b, cst


def check_edge_case(X, shift, Wh, b, cst, S, ll, assign, logp, bad):
    assert bool((cst[1:3] == -math.inf).all()) and not Wh[1:3].any() and not b[1:3].any()
    ref = estep64(X, shift, Wh, b, cst)
    assert int(bad) == 1 and int(assign[2]) == -1 and math.isnan(float(logp[2])) and not bool(ref["ok"][2])
    assert float(S[1:3].abs().sum()) == 0.0 and bool(torch.isfinite(S).all())
    assert bool(((assign[[0, 1, 3, 4, 5, 6, 7, 8]] == 0) | (assign[[0, 1, 3, 4, 5, 6, 7, 8]] == 3)).all())
    assert torch.allclose(S.double(), ref["S"], rtol=1e-3, atol=1e-3)
    assert abs(float(ll) - ref["ll"]) < 1e-5 * abs(ref["ll"]) and abs(float(S[:, -1].sum()) - 8.0) < 1e-4


def test_dead_components_and_a_bad_point():
    X, shift, Wh, b, cst = edge_case()
    bad = torch.zeros(1, dtype=torch.int32)
    S, ll, assign, logp = ops.gmm_full_estep(X, shift, Wh, b, cst, want_assign=True, want_logp=True, bad=bad)
    check_edge_case(X, shift, Wh, b, cst, S, ll, assign, logp, bad)


def test_batch_em_on_rotated_data_beats_the_diagonal_model():
    X = GMMSynth(1024, dims=6, K_teacher=3, seed=5, rotate=True).next()
    final = {}
    for cov in ("full", "diag"):
        m = GMM(GMMConfig(K=3, dims=6, covariance=cov), Comm(device=CPU), init_data=X)   # rho0 = 1, kappa = 0
        ll = [float(m.train_step(X)) for _ in range(20)]
        ll.append(float(m.predict(X)[1].double().sum()))
        m.drain()
        assert all(after >= before - 1e-5 * abs(before) for before, after in zip(ll, ll[1:])), (cov, ll)
        assert m.bad_total == 0
        final[cov] = ll[-1] / 1024
        pi, mu, var = m.params()
        assert abs(float(pi.sum()) - 1.0) < 1e-5 and var.shape == ((3, 6, 6) if cov == "full" else (3, 6))
    print(f"mean log-likelihood after 20 clocks: full {final['full']:.6f}, diag {final['diag']:.6f}")
    assert final["full"] > final["diag"]


def _gmm_full_world(rank, world, dev=CPU):
    torch.set_num_threads(1)
    comm = Comm(device=dev)
    X = GMMSynth(256, dims=6, K_teacher=3, seed=2, rotate=True).next().to(dev)
    m = GMM(GMMConfig(K=3, dims=6, rho0=0.8, kappa=0.5, covariance="full"), comm, init_data=X)
    mine = X[rank * 256 // world:(rank + 1) * 256 // world].contiguous()
    out = [(m.train_step(mine), float(m.predict(X)[1].double().mean()))[1] for _ in range(5)]
    m.drain()
    return out + [float(m.bad_total)]


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_match_one_rank(world):
    many = run_world(_gmm_full_world, world=world)
    one = _gmm_full_world(0, 1)
    print(f"world {world}: {many[0]} vs one rank {one}")
    assert all(many[r] == many[0] for r in range(1, world))
    assert all(abs(a - b) <= 3e-3 * max(1.0, abs(b)) for a, b in zip(many[0], one)), (many[0], one)   # test_gmm.py's
    assert one[5] == 0 and one[4] > one[0]


def test_save_restore_is_bit_exact(tmp_path):
    syn = GMMSynth(128, dims=5, K_teacher=3, seed=1, rotate=True)
    cfg = dict(K=3, dims=5, kappa=0.6, covariance="full")
    a = GMM(GMMConfig(seed=3, **cfg), Comm(device=CPU), init_data=syn.next())
    a.train_step(syn.next()), a.train_step(syn.next())
    a.drain()
    Checkpointer(a.comm, str(tmp_path / "ck_")).save({0: a.table}, iteration=1, blocking=True)
    b = GMM(GMMConfig(seed=9, **cfg), Comm(device=CPU))   # another start, zero shift
    assert Checkpointer(b.comm, str(tmp_path / "ck_")).load({0: b.table}) == 1
    assert torch.equal(a.table.master, b.table.master) and bool(b._state()[1].any())
    X = syn.next()
    a.train_step(X), b.train_step(X)
    a.drain(), b.drain()
    assert torch.equal(a.table.master, b.table.master) and a.table.n_params == 3 * 31 + 5


def test_refusals_name_gmm_and_diag_is_unchanged():
    from minips_amd.train import parse

    calls = [lambda kw=kw: GMMConfig(**kw) for kw in (
        dict(covariance="tied"), dict(covariance="full", dims=65), dict(covariance="full", K=129),
        dict(covariance="full", reg_covar=-1.0), dict(covariance="full", reg_covar=float("nan")))]
    calls += [lambda: ops.gmm_full_prepare(torch.ones(2, 8)), lambda: ops.gmm_full_prepare(torch.ones(2, 7), -1.0),
              lambda: ops.gmm_full_prepare(torch.ones(129, 7)),
              lambda: ops.gmm_full_prepare(torch.ones(1, 65 * 66 + 1)),
              lambda: ops.gmm_full_estep(torch.zeros(4, 3), torch.zeros(2), torch.zeros(1, 16, 16), torch.zeros(1, 16),
                                         torch.zeros(1))]
    for call in calls:
        with pytest.raises(ValueError, match="gmm"):
            call()
    for argv in ("--model gmm --gmm_covariance full --num_dims 65", "--model gmm --gmm_reg_covar 0.1",
                 "--model gmm --gmm_covariance full --gmm_reg_covar -1", "--model kmeans --gmm_covariance full"):
        with pytest.raises(SystemExit):
            parse(argv.split())
    X = GMMSynth(64, dims=5, K_teacher=3, seed=1).next()
    named, plain = (GMM(GMMConfig(K=3, dims=5, **kw), Comm(device=CPU), init_data=X) for kw in
                    (dict(covariance="diag"), {}))
    named.train_step(X), plain.train_step(X)
    named.drain(), plain.drain()
    assert torch.equal(named.table.master, plain.table.master) and named.table.n_params == 3 * 11 + 5


def test_the_binding_exports_two_ops_and_refuses_cpu_tensors():
    K_ = _native.gmmfk()   # a missing build is an error here, not a skip
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == {"gmm_full_prepare", "gmm_full_estep"} and _native.gmmfk_available()
    assert (K_.MAX_K, K_.MAX_D, K_.MAX_CHUNKS) == (ops.GMM_FULL_MAX_K, ops.GMM_FULL_MAX_D, ops.GMM_FULL_MAX_CHUNKS)
    X, shift, s = planted(2, 3, 8, seed=0)
    Wh, b, cst = ops.gmm_full_prepare(s)
    with pytest.raises(RuntimeError, match="s"):
        K_.gmm_full_prepare(s, 3, 1e-6, Wh, b, cst)
    with pytest.raises(RuntimeError, match="X"):
        K_.gmm_full_estep(X, shift, Wh, b, cst, None, torch.zeros(1, dtype=F64), None, None, None, 0)
