"""The Gaussian mixture on the dense PS (CPU): ops.gmm_* against an fp64 loop written from the formulas of
csrc/kernels/gmm.h, the EM property, the model against an fp64 EM run here on the same data and start, ranks over
gloo, checkpoints and refusals."""
import json
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import GMMSynth
from minips_amd.models.gmm import GMM, GMMConfig
from minips_amd.ps.comm import Comm

CPU = torch.device("cpu")
F64 = torch.float64
LOG_2PI = math.log(2 * math.pi)


def prepare64(s, var_floor):
    """gmm.h's Prepare in fp64 from the fp32 statistics: (coef [K, 2 DP], cst [K])."""
    s = s.double()
    K, D = s.shape[0], (s.shape[1] - 1) // 2
    dp = ops.gmm_pad(D)
    s0 = s[:, 2 * D]
    live = torch.isfinite(s).all(1) & (s0 > 0)
    tot = s0[torch.isfinite(s0) & (s0 > 0)].sum()
    coef, cst = torch.zeros(K, 2 * dp, dtype=F64), torch.full((K,), -math.inf, dtype=F64)
    for k in range(K):
        if live[k]:
            mu = s[k, :D] / s0[k]
            var = (s[k, D:2 * D] / s0[k] - mu * mu).clamp(min=var_floor)
            coef[k, :D], coef[k, dp:dp + D] = -0.5 / var, mu / var
            cst[k] = math.log(s0[k] / tot) - 0.5 * float((mu * mu / var + var.log()).sum()) - 0.5 * D * LOG_2PI
    return coef, cst


def estep64(X, shift, coef, cst):
    """gmm.h's E-step as an fp64 loop over the components: dict of t, mag [n, K], lse [n], r [n, K], S [K, 2D +
    1], ll, ok [n]. mag_ik = |cst_k| + sum_d (|coef_a| x^2 + |coef_b x|), the magnitude behind t_ik's rounding."""
    x = X.double() - shift.double()
    n, D, K = x.shape[0], x.shape[1], cst.numel()
    dp = coef.shape[1] // 2
    ca, cb, c0 = coef[:, :D].double(), coef[:, dp:dp + D].double(), cst.double()
    t, mag = torch.empty(n, K, dtype=F64), torch.empty(n, K, dtype=F64)
    for k in range(K):
        t[:, k] = c0[k] + (ca[k] * x * x + cb[k] * x).sum(1)
        mag[:, k] = (abs(c0[k]) if math.isfinite(c0[k]) else 0.0) + (ca[k].abs() * x * x + (cb[k] * x).abs()).sum(1)
    m = torch.nan_to_num(t, nan=-math.inf).max(1).values
    lse = m + (t - m[:, None]).exp().sum(1).log()
    ok = torch.isfinite(lse)
    r = torch.where(ok[:, None], (t - lse[:, None]).exp(), torch.zeros((), dtype=F64))
    xz = torch.where(ok[:, None], x, torch.zeros((), dtype=F64))
    S = torch.cat([r.t() @ xz, r.t() @ (xz * xz), r.sum(0)[:, None]], 1)
    return dict(t=t, mag=mag, lse=lse, r=r, S=S, ll=float(lse[ok].sum()), ok=ok, x=xz)


def planted(K, D, n, seed, sep=0.5):
    """Points of a planted mixture (sigma in [0.5, 2]), centred by shift = their mean, and the mixture's own
    statistics s [K, 2D + 1] in shifted coordinates."""
    syn = GMMSynth(n, dims=D, K_teacher=K, sep=sep, seed=seed)
    X = syn.next()
    shift = X.mean(0)
    mu, var = syn.centres - shift, syn.sigma ** 2
    s = torch.cat([mu, var + mu * mu, torch.ones(K, 1)], 1) * syn.weights[:, None]
    return X, shift, s.float().contiguous()


@pytest.mark.parametrize("K,D", [(1, 1), (5, 3), (17, 20)])
def test_cpu_reference_matches_the_fp64_loop(K, D):
    X, shift, s = planted(K, D, 37, seed=K + D, sep=2.0)
    coef, cst = ops.gmm_prepare(s, 1e-4)
    c64, t64 = prepare64(s, 1e-4)
    assert coef.shape == (K, 2 * ops.gmm_pad(D)) and torch.allclose(coef.double(), c64, rtol=1e-5, atol=1e-6)
    assert torch.allclose(cst.double(), t64, rtol=1e-5, atol=1e-5)
    bad = torch.zeros(1, dtype=torch.int32)
    S, ll, assign, logp = ops.gmm_estep(X, shift, coef, cst, want_assign=True, want_logp=True, bad=bad)
    ref = estep64(X, shift, coef, cst)
    assert torch.allclose(S.double(), ref["S"], rtol=1e-4, atol=1e-5) and int(bad) == 0
    assert abs(float(ll) - ref["ll"]) <= 1e-5 * abs(ref["ll"]) and ll.dtype == F64
    assert torch.allclose(logp.double(), ref["lse"], rtol=1e-5, atol=1e-5)
    assert torch.equal(assign.long(), ref["t"].argmax(1)) and assign.dtype == torch.int32
    none = ops.gmm_estep(X, shift, coef, cst, accumulate=False)
    assert none[0] is None and none[2] is None and torch.equal(none[1], ll)


def edge_case(dev=CPU):
    """(X, shift, coef, cst) with component 1 dead, point 2 holding a NaN feature and point 5 placed 1e3 standard
    deviations from every centre."""
    X, shift, s = planted(4, 6, 9, seed=3, sep=2.0)
    s[1, 12] = 0.0
    X[2, 4] = float("nan")
    X[5] = shift + 2e3
    coef, cst = ops.gmm_prepare(s.to(dev), 1e-4)
    return X.to(dev), shift.to(dev), coef, cst


def check_edge_case(X, shift, coef, cst, S, ll, assign, logp, bad):
    assert float(cst[1]) == -math.inf and not coef[1].any()
    ref = estep64(X, shift, coef, cst)
    assert int(bad) == 1 and int(assign[2]) == -1 and math.isnan(float(logp[2])) and not bool(ref["ok"][2])
    assert float(S[1].abs().sum()) == 0.0 and bool(torch.isfinite(S).all())   # the dead component: r = 0 everywhere
    assert bool((assign[[0, 1, 3, 4, 5, 6, 7, 8]] != 1).all())
    assert float(logp[5]) < -1e5 and int(assign[5]) >= 0                       # the far point is no bad point ...
    assert torch.allclose(S.double(), ref["S"], rtol=1e-3, atol=1e-3)
    assert abs(float(ll) - ref["ll"]) < 1e-5 * abs(ref["ll"])
    assert abs(float(S[:, 12].sum()) - 8.0) < 1e-4                             # ... its r sums to 1 like the other 7


def test_dead_component_and_bad_points():
    X, shift, coef, cst = edge_case()
    bad = torch.zeros(1, dtype=torch.int32)
    S, ll, assign, logp = ops.gmm_estep(X, shift, coef, cst, want_assign=True, want_logp=True, bad=bad)
    check_edge_case(X, shift, coef, cst, S, ll, assign, logp, bad)
    dead = ops.gmm_estep(X, shift, torch.zeros_like(coef), torch.full_like(cst, -math.inf), want_assign=True, bad=bad)
    assert int(bad) == 1 + 9 and not dead[0].any() and float(dead[1]) == 0.0 and bool((dead[2] == -1).all())


# ------------------------------------------------------------------------------ the model
def em64(s, shift, X, var_floor, clocks):
    """Batch EM in fp64 from the statistics s: the summed log-likelihood before each update."""
    out = []
    for _ in range(clocks):
        ref = estep64(X, shift, *prepare64(s, var_floor))
        out.append(ref["ll"])
        s = ref["S"] / X.shape[0]
    return out


def test_loglik_never_falls_and_matches_fp64_em():
    X = GMMSynth(512, dims=8, K_teacher=4).next()
    m = GMM(GMMConfig(K=4, dims=8), Comm(device=CPU), init_data=X)
    s0, shift = (v.clone() for v in m._state())
    ll = [float(m.train_step(X)) for _ in range(15)]
    final = float(m.predict(X)[1].double().sum())
    m.drain()
    print("log-likelihood per clock:", [round(v / 512, 5) for v in ll + [final]])
    for before, after in zip(ll + [final], (ll + [final])[1:]):
        assert after >= before - 1e-5 * abs(before), ll
    assert m.bad_total == 0 and final > ll[0]
    ref = em64(s0, shift, X, 1e-4, 16)
    print(f"mean log-likelihood after 15 clocks: model {final / 512:.6f}, fp64 EM {ref[15] / 512:.6f}")
    assert abs(final - ref[15]) <= 3e-3 * abs(ref[15])
    pi, mu, var = m.params()
    assert abs(float(pi.sum()) - 1.0) < 1e-5 and mu.shape == (4, 8) and bool((var >= 1e-4).all())


def _gmm_world(rank, world, dev=CPU):
    torch.set_num_threads(1)
    comm = Comm(device=dev)
    X = GMMSynth(256, dims=6, K_teacher=3, seed=2).next().to(dev)
    m = GMM(GMMConfig(K=3, dims=6, rho0=0.8, kappa=0.5), comm, init_data=X)
    mine = X[rank * 256 // world:(rank + 1) * 256 // world].contiguous()
    out = []
    for _ in range(5):
        m.train_step(mine)
        out.append(float(m.predict(X)[1].double().mean()))
    m.drain()
    return out + [float(m.bad_total)]


@pytest.mark.parametrize("world", [2, 4])
def test_gmm_ranks_match_one_rank(world):
    many = run_world(_gmm_world, world=world)
    one = _gmm_world(0, 1)
    print(f"world {world}: {many[0]} vs one rank {one}")
    for r in range(1, world):
        assert many[r] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert one[5] == 0 and one[4] > one[0]


def test_save_restore_is_bit_exact(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    syn = GMMSynth(128, dims=5, K_teacher=3, seed=1)   # kappa > 0: the step size depends on the restored clock count
    a = GMM(GMMConfig(K=3, dims=5, kappa=0.6, seed=3), Comm(device=CPU), init_data=syn.next())
    a.train_step(syn.next()), a.train_step(syn.next())
    a.drain()
    Checkpointer(a.comm, str(tmp_path / "ck_")).save({0: a.table}, iteration=1, blocking=True)
    b = GMM(GMMConfig(K=3, dims=5, kappa=0.6, seed=9), Comm(device=CPU))   # another start, zero shift
    assert Checkpointer(b.comm, str(tmp_path / "ck_")).load({0: b.table}) == 1
    assert torch.equal(a.table.master, b.table.master) and torch.equal(a._state()[1], b._state()[1])
    assert bool(b._state()[1].any())
    X = syn.next()
    a.train_step(X), b.train_step(X)
    a.drain(), b.drain()
    assert torch.equal(a.table.master, b.table.master)


def test_config_model_and_op_refusals_name_gmm():
    m = GMM(GMMConfig(K=2, dims=3), Comm(device=CPU))
    calls = [lambda kw=kw: GMMConfig(**kw) for kw in (
        dict(K=0), dict(K=129), dict(dims=0), dict(dims=129), dict(K=80, dims=112), dict(var_floor=0.0),
        dict(var_floor=float("nan")), dict(rho0=0.0), dict(kappa=2.0), dict(transport="onesided"),
        dict(init_mode="grid"))]
    calls += [lambda: m.train_step(torch.zeros(4, 3, dtype=F64)), lambda: m.predict(torch.zeros(4, 2)),
              lambda: ops.gmm_prepare(torch.ones(80, 225), 1e-4), lambda: ops.gmm_prepare(torch.ones(2, 7), 0.0)]
    for call in calls:
        with pytest.raises(ValueError, match="gmm"):
            call()


def test_driver_refusals_and_runs(tmp_path, capsys):
    from minips_amd.train import main, parse

    gmm = ("--K 129", "--num_dims 129", "--K 80 --num_dims 112", "--gmm_rho0 0", "--gmm_kappa 2", "--gmm_var_floor 0",
           "--transport onesided", "--eval_every 2", "--kStorageType Map", "--value_dtype float64")
    other = ("--gmm_rho0 0.5", "--gmm_kappa 0.5", "--gmm_var_floor 0.1")
    for argv in ["--model gmm " + f for f in gmm] + ["--model kmeans " + f for f in other]:
        with pytest.raises(SystemExit):
            parse(argv.split())
    X = GMMSynth(60, dims=5, K_teacher=2, seed=1).next()
    path = tmp_path / "points.libsvm"   # a line is a point: `label feature:value ...`, ids from 1
    path.write_text("".join("0 " + " ".join(f"{d + 1}:{float(x[d]):.4f}" for d in range(5)) + "\n" for x in X))
    for argv, K in ((["--small", "1"], 4), (["--input", str(path), "--K", "2", "--batch", "30"], 2)):
        assert main(["--model", "gmm", "--steps", "12"] + argv) == 0
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["model"] == "gmm" and out["gmm_K"] == K and math.isfinite(out["gmm_loglik"])
        assert out["losses"][-1][1] > -40
    wide = tmp_path / "wide.libsvm"
    wide.write_text("0 1:1.0 200:2.0\n0 3:1.0\n")
    with pytest.raises(ValueError, match="gmm"):
        main(["--model", "gmm", "--steps", "1", "--input", str(wide), "--K", "1"])
