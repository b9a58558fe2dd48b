"""The full-covariance Gaussian-mixture kernels (csrc/kernels/gmm_full.hip) on the GPU against fp64.

The judge is derived, not fitted, as test_gmm_gpu.py's is. The fp64 reference (test_gmm_full.estep64) works from the
same fp32 inputs and returns ymag_j = sum_d |Wh_jd x_d| + |b_j|. y_j is a sum of D + 1 fp32 terms, so by the tree's
(n + 16) 2^-23 rule |y_j - y64_j| <= dy_j = (D + 17) 2^-23 ymag_j (the spare 16 cover x = point - shift). |y|^2 moves by
at most sum_j (2 |y64_j| dy_j + dy_j^2); its own D-term sum and the cst add cost (D + 17) 2^-23 (|cst| + 0.5 |y|^2):
  |t_ik - t64_ik| <= delta_i = max_k [0.5 sum_j (2 |y_j| dy_j + dy_j^2) + (D + 17) 2^-23 (|cst_k| + 0.5 |y_k|^2)].
Then as in test_gmm_gpu.py: lse within delta_i + e (e = 8 * 2^-23), r within a factor 1 + rho_i = exp(2 delta_i + e), a
statistic (a_i = r |x_d|, r |x_d x_e| or r) within sum_i rho_i a_i + (chunk_len + 16) 2^-23 sum_i (1 + rho_i) a_i.
No point is left out. Planted, rotated inputs, sigma in [0.5, 2]; max_i 2 delta_i <= 0.05 is asserted on fp64 alone.

gmm_full_prepare (u = 2^-24, gamma_n = n u / (1 - n u); Sigma and kappa = cond_2(Sigma) from the fp64 reference, Wh the
kernel's): forming Sigma costs |E0| <= 4 u (|S2 / s0| + |mu mu^T| + reg I); the computed factor has L^ L^^T = Sigma + E0
+ dA, |dA| <= gamma_{D+1} |L^| |L^^T| (Higham, Thm 10.3), whose Frobenius norm is <= tr Sigma, so ||E||_F = ||E0 +
dA||_F <= ||E0||_F + gamma_{D+1} tr Sigma. Forward substitution leaves |L^ Wh - I| <= gamma_D |L^| |Wh| (Thm 8.5), so
G = Wh L^ - I has ||G||_F <= cond(L^) gamma_D ||L^||_F ||Wh||_F, cond(L^) = sqrt(kappa), ||L^||_F^2 = tr Sigma to first
order: the test asserts kappa ||E||_F / ||Sigma||_2 <= 0.01 and carries a factor 1.01. Then
  || Wh Sigma Wh^T - I ||_F <= ||Wh||_2^2 ||E||_F + 2 ||G||_F + ||G||_F^2,
  |b - Wh mu| <= gamma_{D+2} |Wh| |mu|                                   (componentwise, against the kernel's own Wh),
  |cst - cst64| <= 0.5 * 1.01 ||Sigma^-1||_F ||E||_F + (D + 16) 2^-23 (|log pi| + sum |log L_dd| + D / 2 log 2 pi)."""
import math

import pytest
import torch

from test_gmm_full import check_edge_case, edge_case, estep64, planted, prepare64
from test_w2v_gpu import _layout

from minips_amd import ops
from minips_amd.data.synthetic import GMMSynth

pytestmark = pytest.mark.gpu

E23, U = 2.0 ** -23, 2.0 ** -24
CHUNK = ops.GMM_FULL_CHUNK
_REF = {}      # (K, D, n) -> the inputs and their fp64 reference, computed once


def _reference(X, shift, Wh, b, cst):
    D = X.shape[1]
    ref = estep64(X, shift, Wh, b, cst)
    dy = (D + 17) * E23 * ref["ymag"]
    mag = torch.nan_to_num(cst.double().abs(), posinf=0.0) + 0.5 * (ref["y"] ** 2).sum(2)
    ref["delta"] = (0.5 * (2 * ref["y"].abs() * dy + dy * dy).sum(2) + (D + 17) * E23 * mag).max(1).values
    del ref["y"], ref["ymag"]
    return ref


def _case(K, D, n):
    if (K, D, n) not in _REF:
        X, shift, s = planted(K, D, n, seed=K + 7 * D)
        Wh, b, cst = ops.gmm_full_prepare(s, 1e-6)
        ref = _reference(X, shift, Wh, b, cst)
        assert float(2 * ref["delta"].max()) <= 0.05   # the condition on the inputs, on fp64 alone
        _REF[(K, D, n)] = (X, shift, Wh, b, cst, ref)
    return _REF[(K, D, n)]


def _run(K, D, n, dev, how="contig", blocks=0, accumulate=True):
    X, shift, Wh, b, cst, _ = _case(K, D, n)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    S, ll, assign, logp = ops.gmm_full_estep(_layout(X, how, dev), shift.to(dev), Wh.to(dev), b.to(dev), cst.to(dev),
                                             accumulate=accumulate, want_assign=True, want_logp=True, bad=bad,
                                             blocks=blocks)
    assert int(bad) == 0
    return (None if S is None else S.cpu()), ll.cpu(), assign.cpu(), logp.cpu()


def _bound_S(ref, chunk):
    rho = torch.expm1(2 * ref["delta"] + 8 * E23)
    x = ref["x"].abs()
    n, D = x.shape
    A = torch.cat([x, (x[:, :, None] * x[:, None, :]).reshape(n, D * D), torch.ones(n, 1, dtype=torch.float64)], 1)
    return (ref["r"] * rho[:, None]).t() @ A + (chunk + 16) * E23 * ((ref["r"] * (1 + rho[:, None])).t() @ A)


def _judge(label, ref, K, D, n, S, ll, assign, logp):
    delta, e = ref["delta"], 8 * E23
    worst = float(((logp.double() - ref["lse"]).abs() / (delta + e)).max())
    worst = max(worst, abs(float(ll) - ref["ll"]) / float((delta + e).sum()))
    chosen = ref["t"].gather(1, assign.long()[:, None])[:, 0]
    assert bool((assign >= 0).all()) and bool((chosen >= ref["t"].max(1).values - 2 * delta).all())
    if S is not None:
        worst = max(worst, float(((S.double() - ref["S"]).abs() / _bound_S(ref, ops.gmm_full_chunk(n, K, D))).max()))
        S2 = S[:, D:D + D * D].view(K, D, D)
        assert torch.equal(S2, S2.transpose(1, 2))   # symmetric to the bit
    print(f"{label} K {K} D {D} n {n}: error / bound {worst:.4f}")
    assert worst <= 1.0


SHAPES = [(K, D) for K in (1, 5, 16, 17, 128) for D in (1, 3, 16, 17, 48, 64)]
LONG = (2, 3, ops.GMM_FULL_MAX_CHUNKS * CHUNK + 1)   # the first n whose chunks are lengthened (to 4096)


@pytest.mark.parametrize("K,D,n", sorted(
    {(K, D, n) for K, D in ((17, 20), (128, 64)) for n in (1, 63, 65, 257, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 17)}
    | {(K, D, n) for K, D in SHAPES for n in (65, CHUNK + 1)}) + [LONG])
def test_estep_against_fp64(K, D, n, dev):
    """One sweep over n at two shapes (the largest one included), one sweep over the shapes at two n, and one n just
    past the point where the chunk rule first lengthens the chunk."""
    assert ops.gmm_full_chunk(n, K, D) == (2 * CHUNK if (K, D, n) == LONG else CHUNK)
    _judge("estep", _case(K, D, n)[5], K, D, n, *_run(K, D, n, dev))


@pytest.mark.parametrize("K,D", [(17, 20), (128, 64)])
def test_layouts_predict_path_and_bits(K, D, dev):
    """Strided (float4 loads), odd-ld and misaligned (scalar loads) rows, the predict path, reruns and forced grids."""
    same = _run(K, D, 65, dev)
    for how in ("strided", "odd_ld", "misaligned"):
        assert all(torch.equal(a, b) for a, b in zip(_run(K, D, 65, dev, how=how), same))
    n = 2 * CHUNK + 17
    S, ll, assign, logp = _run(K, D, n, dev)
    pred = _run(K, D, n, dev, accumulate=False)
    assert pred[0] is None and torch.equal(pred[1], ll) and torch.equal(pred[2], assign) and torch.equal(pred[3], logp)
    for blocks in (0, 1, 7):
        again = _run(K, D, n, dev, blocks=blocks)
        assert torch.equal(again[0], S) and torch.equal(again[1], ll) and torch.equal(again[3], logp)


def test_dead_components_and_a_bad_point(dev):
    X, shift, Wh, b, cst = edge_case(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    S, ll, assign, logp = ops.gmm_full_estep(X, shift, Wh, b, cst, want_assign=True, want_logp=True, bad=bad)
    check_edge_case(*(v.cpu() for v in (X, shift, Wh, b, cst, S, ll, assign, logp, bad)))
    empty = ops.gmm_full_estep(X[:0], shift, Wh, b, cst, want_assign=True)
    assert not empty[0].any() and float(empty[1]) == 0.0 and empty[2].numel() == 0


@pytest.mark.parametrize("K,D", [(1, 1), (17, 20), (128, 64)])
def test_prepare_against_fp64(K, D, dev):
    """The bounds of the module docstring, per live component."""
    s = planted(K, D, 8, seed=K + D)[2]
    if K > 1:
        s[K // 2, -1] = 0.0   # a dead component
    Wh, b, cst = (v.cpu().double() for v in ops.gmm_full_prepare(s.to(dev), 1e-6))
    _, _, c64, sigma = prepare64(s, 1e-6)
    dp, sd = ops.gmm_pad(D), s.double()
    live = torch.isfinite(c64)
    assert torch.equal(torch.isfinite(cst), live) and not Wh[~live].any() and not b[~live].any()
    assert not Wh.triu(1).any() and not Wh[:, D:].any() and not Wh[:, :, D:].any() and not b[:, D:].any()
    gam = lambda n: n * U / (1 - n * U)  # noqa: E731
    tot, worst = float(sd[live, -1].sum()), 0.0
    for k in torch.nonzero(live)[:, 0].tolist():
        mu, sig, W = sd[k, :D] / sd[k, -1], sigma[k], Wh[k, :D, :D]
        S2 = sd[k, D:D + D * D].view(D, D) / sd[k, -1]
        E0 = 4 * U * (S2.abs() + torch.outer(mu, mu).abs() + 1e-6 * torch.eye(D))
        E = float(E0.norm()) + gam(D + 1) * float(sig.trace())
        ev = torch.linalg.eigvalsh(sig)
        kappa = float(ev[-1] / ev[0])
        assert kappa * E / float(ev[-1]) <= 0.01
        G = 1.01 * math.sqrt(kappa) * gam(D) * math.sqrt(float(sig.trace())) * float(W.norm())
        bw = float(torch.linalg.matrix_norm(W, 2)) ** 2 * E + 2 * G + G * G
        worst = max(worst, float((W @ sig @ W.t() - torch.eye(D)).norm()) / bw)
        worst = max(worst, float(((b[k, :D] - W @ mu).abs() / (gam(D + 2) * (W.abs() @ mu.abs()) + 1e-300)).max()))
        terms = abs(math.log(float(sd[k, -1]) / tot)) + float(torch.linalg.cholesky(sig).diagonal().log().abs().sum())
        terms += 0.5 * D * math.log(2 * math.pi)
        bc = 0.5 * 1.01 * float(torch.linalg.inv(sig).norm()) * E + (D + 16) * E23 * terms
        worst = max(worst, abs(float(cst[k] - c64[k])) / bc)
    print(f"prepare K {K} D {D}: error / bound {worst:.4f}")
    assert worst <= 1.0


def test_model_gpu_step(dev):
    """One clock of GMM(covariance='full') on the GPU: its log-likelihood and its table afterwards against fp64 at the
    model's own operands, within the E-step's derived bounds; the CPU model within test_gmm_gpu.py's 3e-3."""
    from minips_amd.models.gmm import GMM, GMMConfig
    from minips_amd.ps.comm import Comm

    K, D, n = 17, 20, 600
    X = GMMSynth(n, dims=D, K_teacher=5, seed=4, sep=0.5, rotate=True).next()
    cfg = GMMConfig(K=K, dims=D, rho0=0.9, kappa=0.3, covariance="full")
    cpu, gpu = GMM(cfg, Comm(device=torch.device("cpu")), init_data=X), GMM(cfg, Comm(device=dev), init_data=X.to(dev))
    gpu.table.load_full(cpu.table.full_master()[: cpu.table.n_params])   # the same start: seeding draws per device
    s, shift = (v.clone() for v in gpu._state())
    ref = _reference(X, shift.cpu(), *(v.cpu() for v in ops.gmm_full_prepare(s, cfg.reg_covar)))
    assert float(2 * ref["delta"].max()) <= 0.05
    lg, lc = float(gpu.train_step(X.to(dev))), float(cpu.train_step(X))
    gpu.drain(), cpu.drain()
    assert abs(lg - ref["ll"]) <= float((ref["delta"] + 8 * E23).sum()) and abs(lg - lc) <= 3e-3 * abs(lc)
    rho, s64 = 0.9 * (0 + 1.0) ** -0.3, s.cpu().double()
    want = s64 + rho * (ref["S"] / n - s64)
    bound = rho * _bound_S(ref, CHUNK) / n + 8 * E23 * (want.abs() + s64.abs() + ref["S"] / n)
    assert bool(((gpu._state()[0].cpu().double() - want).abs() <= bound).all()) and gpu.bad_total == 0
