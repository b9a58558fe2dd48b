"""The Gaussian-mixture kernels (csrc/kernels/gmm.hip) on the GPU against fp64, and the model against the CPU's.

The judge is derived, not fitted. The fp64 reference (test_gmm.estep64) forms t64, lse64, r64 and S64 from the same
fp32 inputs and also mag_ik = |cst_k| + sum_d (|coef_a| x^2 + |coef_b x|). A score is a sum of 2D + 1 fp32 terms in
some order, so by the tree's (n + 16) 2^-23 rule for fp32 reductions
  |t_ik - t64_ik| <= delta_i = (2D + 1 + 16) 2^-23 max_k mag_ik
(the spare 16 cover the rounding of x = point - shift, which moves t by at most 2^-23 mag, and the cst add). Then lse
is within delta_i + e, e = 8 * 2^-23 for the fp32 exp, log and adds, and r = exp(t - lse) within a factor
exp(+-(2 delta_i + e)): a relative slack rho_i = exp(2 delta_i + e) - 1. A statistic is a sum over points of r |x|,
r x^2 or r, so it is within
  sum_i rho_i a_i  +  (CHUNK + 16) 2^-23 sum_i (1 + rho_i) a_i,      a_i = r64_ik |x_ij|  (or r64 x^2, or r64)
-- the responsibilities' slack plus the fp32 accumulation of at most CHUNK terms and the chunk fold. ll is within
sum_i (delta_i + e), logp_i within delta_i + e, and assign is right when the fp64 score of the chosen component is
within 2 delta_i of the fp64 maximum. No point is left out. The inputs are conditioned so that the bound means
something: points of a planted mixture with sigma in [0.5, 2], centred by shift, with max_i 2 delta_i <= 0.05 asserted
on the fp64 reference alone (about 0.037 at D = 128). A dropped tile, a wrong pad or a missing cst moves a statistic by
the order of its own size, thousands of times the bound.

gmm_prepare: var = s2 / s0 - mu^2 cancels, so with u = 2^-24 and q = s2 / s0 + mu^2 the variance carries 4 u q and
coef a relative 4 u q / var + 4 u; cst adds the (D + 16) 2^-23 rule over its D + 2 terms."""
import math

import pytest
import torch

from test_gmm import _gmm_world, check_edge_case, edge_case, estep64, planted, prepare64
from test_multirank_gpu import run_world
from test_w2v_gpu import _layout

from minips_amd import ops
from minips_amd.data.synthetic import GMMSynth

pytestmark = pytest.mark.gpu

E23 = 2.0 ** -23
CHUNK = ops.GMM_CHUNK
WORST = [0.0]  # the largest error / bound of this run (printed by every case)
_REF = {}      # (K, D, n) -> the inputs and their fp64 reference, computed once


def _case(K, D, n):
    if (K, D, n) not in _REF:
        X, shift, s = planted(K, D, n, seed=K + 7 * D)
        coef, cst = ops.gmm_prepare(s, 1e-4)
        ref = estep64(X, shift, coef, cst)
        ref["delta"] = (2 * D + 17) * E23 * ref["mag"].max(1).values
        assert float(2 * ref["delta"].max()) <= 0.05   # the condition on the inputs, on fp64 alone
        _REF[(K, D, n)] = (X, shift, coef, cst, ref)
    return _REF[(K, D, n)]


def _run(K, D, n, dev, how="contig", blocks=0, accumulate=True):
    X, shift, coef, cst, ref = _case(K, D, n)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    S, ll, assign, logp = ops.gmm_estep(_layout(X, how, dev), shift.to(dev), coef.to(dev), cst.to(dev),
                                        accumulate=accumulate, want_assign=True, want_logp=True, bad=bad, blocks=blocks)
    assert int(bad) == 0
    return (None if S is None else S.cpu()), ll.cpu(), assign.cpu(), logp.cpu()


def _judge(K, D, n, S, ll, assign, logp):
    ref = _case(K, D, n)[4]
    delta, e = ref["delta"], 8 * E23
    rho = torch.expm1(2 * delta + e)
    worst = float(((logp.double() - ref["lse"]).abs() / (delta + e)).max())
    worst = max(worst, abs(float(ll) - ref["ll"]) / float((delta + e).sum()))
    chosen = ref["t"].gather(1, assign.long()[:, None])[:, 0]
    assert bool((assign >= 0).all()) and bool((chosen >= ref["t"].max(1).values - 2 * delta).all())
    if S is not None:
        x = ref["x"].abs()
        A = torch.cat([x, x * x, torch.ones(n, 1, dtype=torch.float64)], 1)           # |terms| [n, 2D + 1]
        bound = (ref["r"] * rho[:, None]).t() @ A + (CHUNK + 16) * E23 * ((ref["r"] * (1 + rho[:, None])).t() @ A)
        ratio = (S.double() - ref["S"]).abs() / bound
        worst = max(worst, float(ratio.max()))
    WORST[0] = max(WORST[0], worst)
    print(f"K {K} D {D} n {n}: error / bound {worst:.4f}, largest so far {WORST[0]:.4f}")
    assert worst <= 1.0


NS = [1, 63, 65, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 17]
SHAPES = [(K, D) for K in (1, 5, 16, 17, 128) for D in (1, 3, 4, 20, 64, 128) if ops.gmm_shape_ok(K, D)]


@pytest.mark.parametrize("K,D,n", sorted({(K, D, n) for K, D in ((17, 20), (64, 128)) for n in NS}
                                         | {(K, D, n) for K, D in SHAPES + [(80, 96)] for n in (65, CHUNK + 1)}))
def test_estep_against_fp64(K, D, n, dev):
    """One sweep over n at two shapes (the largest one included), one sweep over the shapes at two n; (80, 96) is the
    96 x 96 bucket, which K in {1 .. 17, 128} never reaches."""
    _judge(K, D, n, *_run(K, D, n, dev))


@pytest.mark.parametrize("how", ["contig", "strided", "odd_ld", "misaligned"])
@pytest.mark.parametrize("K,D", [(17, 20), (64, 128), (96, 80)])
def test_row_layouts(K, D, how, dev):
    """ld = D + 4 keeps the float4 loads; ld = D + 1 and a base off by 4 bytes take the scalar staging loads."""
    out = _run(K, D, 65, dev, how=how)
    _judge(K, D, 65, *out)
    same = _run(K, D, 65, dev)
    assert torch.equal(same[0], out[0]) and torch.equal(same[1], out[1])  # only the loads differ


@pytest.mark.parametrize("K,D", [(17, 20), (128, 64), (80, 96)])
def test_predict_path_and_bits(K, D, dev):
    """accumulate=False gives the same assign / logp / ll; two runs and forced grids give the same bits."""
    n = 2 * CHUNK + 17
    S, ll, assign, logp = _run(K, D, n, dev)
    _judge(K, D, n, S, ll, assign, logp)
    pred = _run(K, D, n, dev, accumulate=False)
    assert pred[0] is None and torch.equal(pred[1], ll) and torch.equal(pred[2], assign) and torch.equal(pred[3], logp)
    for blocks in (0, 1, 7):
        again = _run(K, D, n, dev, blocks=blocks)
        assert torch.equal(again[0], S) and torch.equal(again[1], ll)


def test_dead_component_and_bad_points(dev):
    X, shift, coef, cst = edge_case(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    S, ll, assign, logp = ops.gmm_estep(X, shift, coef, cst, want_assign=True, want_logp=True, bad=bad)
    check_edge_case(X.cpu(), shift.cpu(), coef.cpu(), cst.cpu(), S.cpu(), ll.cpu(), assign.cpu(), logp.cpu(), bad.cpu())
    empty = ops.gmm_estep(X[:0], shift, coef, cst, want_assign=True)
    assert not empty[0].any() and float(empty[1]) == 0.0 and empty[2].numel() == 0


@pytest.mark.parametrize("K,D", [(1, 1), (17, 20), (128, 64), (64, 128)])
def test_prepare_against_fp64(K, D, dev):
    s = planted(K, D, 8, seed=K + D)[2]
    if K > 1:
        s[K // 2, 2 * D] = 0.0   # a dead component
    coef, cst = (v.cpu().double() for v in ops.gmm_prepare(s.to(dev), 1e-4))
    c64, t64 = prepare64(s, 1e-4)
    u, dp, sd = 2.0 ** -24, ops.gmm_pad(D), s.double()
    live = torch.isfinite(t64)
    assert torch.equal(torch.isfinite(cst), live) and not coef[~live].any() and not coef[:, D:dp].any()
    mu = sd[live, :D] / sd[live, 2 * D:]
    q = sd[live, D:2 * D] / sd[live, 2 * D:] + mu * mu
    var = (q - 2 * mu * mu).clamp(min=1e-4)
    rel = 4 * u * q / var + 4 * u
    assert bool(((coef[live][:, :D] - c64[live][:, :D]).abs() <= rel * c64[live][:, :D].abs()).all())
    cb, cb64 = coef[live][:, dp:dp + D], c64[live][:, dp:dp + D]
    assert bool(((cb - cb64).abs() <= rel * cb64.abs()).all())
    pi = sd[live, 2 * D] / sd[live, 2 * D].sum()
    terms = pi.log().abs() + 0.5 * (mu * mu / var + var.log().abs()).sum(1) + 0.5 * D * math.log(2 * math.pi)
    bound = (D + 16) * E23 * terms + 0.5 * ((mu * mu / var + 1) * rel).sum(1)
    assert bool(((cst[live] - t64[live]).abs() <= bound).all()), float(((cst[live] - t64[live]).abs() / bound).max())


# ------------------------------------------------------------------------------ the model
def _models(dev):
    from minips_amd.models.gmm import GMM, GMMConfig
    from minips_amd.ps.comm import Comm

    X = GMMSynth(600, dims=20, K_teacher=5, seed=4).next()
    cfg = GMMConfig(K=17, dims=20, rho0=0.9, kappa=0.3)
    return X, GMM(cfg, Comm(device=torch.device("cpu")), init_data=X), GMM(cfg, Comm(device=dev), init_data=X.to(dev))


def test_model_gpu_matches_cpu(dev):
    X, cpu, gpu = _models(dev)
    gpu.table.load_full(cpu.table.full_master()[: cpu.table.n_params])   # the same start: seeding draws per device
    Xg = X.to(dev)
    for clock in range(5):
        lc, lg = float(cpu.train_step(X)), float(gpu.train_step(Xg))
        print(f"clock {clock}: cpu {lc / 600:.6f} gpu {lg / 600:.6f}")
        assert abs(lg - lc) <= 3e-3 * abs(lc)
    a, lp = gpu.predict(Xg)
    ac, lpc = cpu.predict(X)
    assert abs(float(lp.double().sum()) - float(lpc.double().sum())) <= 3e-3 * abs(float(lpc.double().sum()))
    assert float((a.cpu() == ac).float().mean()) > 0.99
    cpu.drain(), gpu.drain()
    assert gpu.bad_total == 0 == cpu.bad_total


def test_steady_clock_has_no_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    X, _, gpu = _models(dev)
    Xg = X.to(dev)
    gpu.train_step(Xg)  # warm-up: scratch allocations
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for _ in range(3):
            audit.step_begin()
            gpu.train_step(Xg)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep


def _gmm_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _gmm_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_match_one_rank(dev):
    many = run_world(_gmm_two_ranks_gpu, world=2)
    one = _gmm_world(0, 1, dev=dev)
    print(f"2 ranks on one card {many[0]} vs one rank {one}")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
