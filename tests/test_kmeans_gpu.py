"""K-Means' fused step on the GPU (ops.km_nearest / km_sums, csrc/kernels/kmeans.h) against fp64, with bounds derived
from the rule: an fp32 reduction of T terms is off by at most (T + 16) 2^-23 of the sum of the terms' magnitudes. The
points are planted around the centres (centres ~ 3 N(0, 1), noise 0.5), so a structural mistake is of the order of the
magnitudes, thousands of times the bound."""
import pytest
import torch

from minips_amd import _native, ops

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23


def _planted(n, K, D, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * K + D)
    C = 3 * torch.randn(K, D, generator=g)
    X = C[torch.randint(0, K, (n,), generator=g)] + 0.5 * torch.randn(n, D, generator=g)
    return X, C


def _check_nearest(X, C, assign, dist, sse):
    """X, C on the CPU (X without the bad points), the op's outputs for them."""
    D = X.shape[1]
    X64, C64 = X.double(), C.double()
    d64 = torch.cdist(X64, C64) ** 2
    a = assign.cpu().long()
    assert bool(((a >= 0) & (a < C.shape[0])).all())
    mine = d64.gather(1, a[:, None])[:, 0]
    mag = (C64 * C64).sum(1)[None, :] + 2 * X64.abs() @ C64.abs().t()
    delta = (D + 17) * EPS * mag.max(1).values
    assert bool((mine <= d64.min(1).values + 2 * delta).all()), float((mine - d64.min(1).values - 2 * delta).max())
    err = (dist.cpu().double() - mine).abs()
    assert bool((err <= (D + 16) * EPS * mine).all()), float((err / mine.clamp_min(1e-300)).max())
    own = float(dist.cpu().double().sum())
    assert abs(float(sse) - own) <= 1e-12 * abs(own)


def _check_sums(X, assign, K, sums, counts):
    a = assign.cpu().long()
    keep = a >= 0
    S64 = torch.zeros(K, X.shape[1], dtype=torch.float64).index_add_(0, a[keep], X[keep].double())
    A64 = torch.zeros(K, X.shape[1], dtype=torch.float64).index_add_(0, a[keep], X[keep].double().abs())
    M = torch.bincount(a[keep], minlength=K)
    assert torch.equal(counts.cpu().long(), M)
    bound = (M[:, None] + 16) * EPS * A64
    assert bool(((sums.cpu().double() - S64).abs() <= bound).all())


@pytest.mark.parametrize("n,K,D,view", [
    (1, 1, 1, False), (65, 17, 20, False), (200, 63, 64, False), (200, 64, 64, False), (200, 65, 64, False),
    (200, 129, 64, False), (ops.KM_CHUNK * 32 + 1 + 70, 100, 128, False), (300, 4096, 256, False),
    (65, 17, 20, True), (130, 70, 64, True)])
def test_step_against_fp64(dev, n, K, D, view):
    X, C = _planted(n, K, D)
    Xg = X.to(dev)
    if view:  # ld > D and a misaligned base: the scalar loads
        Xg = torch.cat([torch.zeros(n, 1), X, torch.zeros(n, 2)], 1).to(dev)[:, 1:D + 1]
    assign, dist, sums, counts, sse = ops.km_step(Xg, C.to(dev))
    _check_nearest(X, C, assign, dist, sse)
    _check_sums(X, assign, K, sums, counts)


def test_heavy_centre_and_empty_centres(dev):
    kmk = _native.kmk()
    n, K, D = 2 * kmk.WAVE_MAX + kmk.ROW_CHUNK + 37, 5, 24
    g = torch.Generator().manual_seed(3)
    C = 3 * torch.randn(K, D, generator=g) + 40 * torch.arange(K)[:, None]
    X = C[2] + 0.5 * torch.randn(n, D, generator=g)
    assign, dist, sums, counts, sse = ops.km_step(X.to(dev), C.to(dev))
    assert bool((assign == 2).all()) and counts.tolist() == [0, 0, n, 0, 0]
    _check_nearest(X, C, assign, dist, sse)
    _check_sums(X, assign, K, sums, counts)
    assert not bool(sums[[0, 1, 3, 4]].any())


def test_duplicate_dead_and_bad(dev):
    kmk = _native.kmk()
    n, K, D = 150, kmk.STRIP + 9, 20
    X, C = _planted(n, K, D, seed=5)
    X[:4] = C[3] + 0.5 * torch.randn(4, D, generator=torch.Generator().manual_seed(6))
    C[kmk.STRIP + 3] = C[3]                       # the same row one strip later: never chosen
    C[7, 2] = float("inf")                        # a dead centre: never chosen
    assign, dist, sums, counts, sse = ops.km_step(X.to(dev), C.to(dev))
    assert not bool(((assign == kmk.STRIP + 3) | (assign == 7)).any()) and bool((assign == 3).any())
    live = torch.ones(K, dtype=torch.bool)
    live[7] = False
    back = torch.arange(K)[live]                  # against the live centres only
    a_live = (assign.cpu().long()[:, None] == back[None, :]).long().argmax(1).to(torch.int32)
    _check_nearest(X, C[live], a_live, dist, sse)
    Xb = X.clone()
    Xb = torch.cat([Xb[:40], Xb[:1], Xb[40:], Xb[:1]])
    Xb[40, 5], Xb[-1, 0] = float("nan"), float("inf")
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    a2, d2, s2, c2, sse2 = ops.km_step(Xb.to(dev), C.to(dev), bad=bad)
    assert int(bad) == 2 and a2[40] == -1 and a2[-1] == -1 and bool(torch.isnan(d2[[40, -1]]).all())
    keep = torch.ones(n + 2, dtype=torch.bool)
    keep[40] = keep[-1] = False
    assert torch.equal(a2.cpu()[keep], assign.cpu()) and torch.equal(d2.cpu()[keep], dist.cpu())
    assert torch.equal(s2, sums) and torch.equal(c2, counts) and torch.equal(sse2, sse)
    dead = torch.full((3, D), float("nan"))
    a3, d3, s3, c3, sse3 = ops.km_step(X.to(dev), dead.to(dev))   # no live centre at all
    assert bool((a3 == -1).all()) and float(sse3) == 0 and not bool(c3.any()) and not bool(s3.any())


@pytest.mark.parametrize("shape", ["chunks", "heavy"])
def test_same_bits_for_every_grid(dev, shape):
    kmk = _native.kmk()
    if shape == "chunks":
        X, C = _planted(kmk.CHUNK * 32 + 1 + 70, 100, 128)
    else:
        C = 3 * torch.randn(5, 24, generator=torch.Generator().manual_seed(1))
        n = 2 * kmk.WAVE_MAX + kmk.ROW_CHUNK + 37
        X = C[2] + 0.5 * torch.randn(n, 24, generator=torch.Generator().manual_seed(2))
    Xg, Cg = X.to(dev), C.to(dev)
    ref = ops.km_step(Xg, Cg)
    for blocks in (0, 1, 7):
        for a, b in zip(ref, ops.km_step(Xg, Cg, blocks=blocks)):
            assert torch.equal(a, b), blocks


def _models(dev):
    from minips_amd.models.kmeans import KMeans, KMeansConfig
    from minips_amd.ps.comm import Comm

    g = torch.Generator().manual_seed(0)   # test_nn_gpu.py::test_lr_kmeans_gpu_matches_cpu's planted data
    true = torch.randn(6, 12, generator=g) * 5
    init = true + torch.randn(6, 12, generator=g)
    Xs = [true[torch.randint(0, 6, (512,), generator=g)] + torch.randn(512, 12, generator=g) * 0.5 for _ in range(4)]
    return Xs, [KMeans(KMeansConfig(K=6, dims=12, step="fused"), Comm(device=torch.device(d)), init_centres=init)
                for d in ("cpu", dev)]


def test_model_matches_cpu_without_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    Xs, (cpu, gpu) = _models(dev)
    for X in Xs:
        lc, lg = float(cpu.train_step(X)), float(gpu.train_step(X.to(dev)))
        assert abs(lg - lc) < 1e-3 * lc
    cpu.drain(), gpu.drain()
    torch.testing.assert_close(gpu.centres().cpu(), cpu.centres(), rtol=1e-4, atol=1e-4)
    assert gpu.bad_total == 0 == cpu.bad_total
    Xg = Xs[0].to(dev)
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for _ in range(3):
            audit.step_begin()
            gpu.train_step(Xg)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep
