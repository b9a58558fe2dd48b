"""Histogram GBDT on the GPU (csrc/kernels/gbdt.hip through minips_amd.ops): every kernel against the CPU
reference of the same rule -- integers and comparisons, so torch.equal; the gain bit for bit; the fixed-point
gradients within one unit of the fp64 rule -- on every path, grid size and alignment form, the LDS flush bound,
and the model: GPU trees replayed on the CPU, determinism, no host sync, evaluation, two ranks on one card."""
import math

import pytest
import torch

from test_gbdt import (I32, I64, S, SPLIT_CASES, WORLD_ROUNDS, _gbdt_world, assert_split_equal, bits, fit, grad64,
                       grad_inputs, hist_inputs, run_split, synth, trees_of)
from test_multirank_gpu import run_world

from minips_amd import ops
from minips_amd.models.gbdt import GBDT, GBDTConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def offset_view(t, dev):
    """The same values on the device at an odd byte offset and an odd leading dimension: t = buf[:, 1:]."""
    buf = torch.zeros(t.shape[0], t.shape[1] + 1, dtype=t.dtype, device=dev)
    buf[:, 1:] = t.to(dev)
    return buf[:, 1:]


# ------------------------------------------------------------------------------ bin
@pytest.mark.parametrize("NB", [2, 16, 64, 256])
@pytest.mark.parametrize("F", [1, 7, 16, 33])
def test_bin_equals_the_cpu(F, NB, dev):
    g = torch.Generator().manual_seed(F * 1000 + NB)
    cuts = torch.sort(torch.randn(F, NB - 1, generator=g), 1).values
    if NB > 2:
        cuts[::2, (NB - 1) // 2:] = math.inf  # features with fewer distinct quantiles: padded
    for N in (1, 63, 64, 65, 5000):
        X = torch.randn(N, F, generator=g)
        X[::3, 0] = cuts[0, 0]  # equal to a cut: not above it
        X[1::5, F - 1] = cuts[F - 1, (NB - 2) // 2]
        X[2::7, 0] = math.nan
        X[3::7, F // 2] = math.inf
        X[4::7, F - 1] = -math.inf
        ref = ops.gbdt_bin(X, cuts)
        assert int(ref[:, :F].max()) <= NB - 1
        got = ops.gbdt_bin(X.to(dev), cuts.to(dev))
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
        assert torch.equal(ops.gbdt_bin(X.to(dev), cuts.to(dev), blocks=1).cpu(), ref)
        # an odd base pointer and leading dimension: the byte-per-lane form; the other columns stay untouched
        buf = torch.full((N, F + 2), 77, dtype=torch.uint8, device=dev)
        ops.gbdt_bin(X.to(dev), cuts.to(dev), out=buf[:, 1:F + 1])
        assert torch.equal(buf[:, 1:F + 1].cpu(), ref[:, :F]) and bool((buf[:, 0] == 77).all()) \
            and bool((buf[:, F + 1] == 77).all())
        # a padded X
        Xp = torch.zeros(N, F + 3, device=dev)
        Xp[:, :F] = X.to(dev)
        assert torch.equal(ops.gbdt_bin(Xp[:, :F], cuts.to(dev)).cpu(), ref)


# ------------------------------------------------------------------------------ hist
HIST_SHAPES = [(5000, 7, 16), (3000, 33, 64), (2000, 3, 256)]


def lds_fits(nodes, NB):
    return nodes * NB * 12 <= 64 * 1024


@pytest.mark.parametrize("level", [0, 3, 7])
@pytest.mark.parametrize("N,F,NB", HIST_SHAPES)
def test_hist_equals_the_cpu_on_every_path_and_grid(N, F, NB, level, dev):
    nodes = 1 << level
    bins, node, gh = hist_inputs(N, F, NB, nodes, seed=level + NB)
    ref = torch.zeros(nodes, F, NB, 3, dtype=I64)
    ops.gbdt_hist(bins, node, gh, ref)
    assert int(ref[..., 2].sum()) < N * F  # out-of-range node ids and bins were skipped
    db, dn, dg = bins.to(dev), node.to(dev), gh.to(dev)
    ub = offset_view(bins, dev)  # the byte form of the LDS path
    for path in (0, 1, 2):
        if path == 1 and not lds_fits(nodes, NB):
            with pytest.raises(RuntimeError, match="path"):
                ops.gbdt_hist(db, dn, dg, torch.zeros_like(ref, device=dev), path=1)
            continue
        for blocks in (1, 7, 0):
            for b in (db, ub):
                hist = torch.zeros_like(ref, device=dev)
                ops.gbdt_hist(b, dn, dg, hist, path=path, blocks=blocks)
                assert torch.equal(hist.cpu(), ref), (path, blocks, b is ub)
        hist = torch.zeros_like(ref, device=dev)
        ops.gbdt_hist(db, dn, dg, hist, path=path)
        ops.gbdt_hist(db, dn, dg, hist, path=path)  # a repeat run adds the same again
        assert torch.equal(hist.cpu(), 2 * ref)
    # two halves of the samples are one call
    hist = torch.zeros_like(ref, device=dev)
    h = N // 2 + 1
    ops.gbdt_hist(db[:h], dn[:h], dg[:h], hist)
    ops.gbdt_hist(db[h:], dn[h:], dg[h:], hist)
    assert torch.equal(hist.cpu(), ref)


def test_hist_lds_accumulators_cannot_overflow(dev):
    """5000 samples in node 0 and bin 0: q_g alternates in blocks of 500 between +2^20 and -2^20, then every
    q_g is +2^20. With one workgroup a 32-bit accumulator that is not flushed in time passes 2^31."""
    N, F, NB = 5000, 3, 4
    bins = torch.zeros(N, 16, dtype=torch.uint8, device=dev)
    node = torch.zeros(N, dtype=I32, device=dev)
    sign = torch.where((torch.arange(N) // 500) % 2 == 0, 1, -1)
    for qg in (sign * S, torch.full((N,), S), torch.full((N,), -S)):
        gh = torch.stack([qg, torch.full((N,), S // 4)], 1).to(I32).to(dev)
        for blocks in (1, 0):
            hist = torch.zeros(1, F, NB, 3, dtype=I64, device=dev)
            ops.gbdt_hist(bins, node, gh, hist, path=1, blocks=blocks)
            want = torch.tensor([int(qg.sum()), N * (S // 4), N])
            assert N * S > 2 ** 31 and torch.equal(hist[0, :, 0].cpu(), want[None, :].expand(F, 3)), hist[0, :, 0]
            assert not bool(hist[0, :, 1:].any())


def test_hist_is_exact_for_gradients_beyond_the_rule(dev):
    """A caller's own gh outside [-2^20, 2^20] takes the global atomics: still the exact int64 sums."""
    N, F, NB = 4000, 5, 8
    bins, node, gh = hist_inputs(N, F, NB, 2, seed=9)
    gh[::3, 0] = 2 ** 31 - 1
    gh[1::3, 0] = -2 ** 31
    gh[::4, 1] = 2 ** 31 - 1
    ref = torch.zeros(2, F, NB, 3, dtype=I64)
    ops.gbdt_hist(bins, node, gh, ref)
    for path in (1, 2):
        hist = torch.zeros_like(ref, device=dev)
        ops.gbdt_hist(bins.to(dev), node.to(dev), gh.to(dev), hist, path=path, blocks=1)
        assert torch.equal(hist.cpu(), ref)


# ------------------------------------------------------------------------------ split
@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_equals_the_cpu_on_the_cpu_tests_cases(name, dev):
    hist, lam, mc, mg = SPLIT_CASES[name]
    assert_split_equal(run_split(hist.to(dev), lam, mc, mg), run_split(hist, lam, mc, mg))


def random_hist(nodes, F, NB, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 40, (nodes, F, NB), generator=g)
    c[torch.rand(nodes, F, NB, generator=g) < 0.3] = 0
    qg = (torch.rand(nodes, F, NB, generator=g, dtype=torch.float64) * 2 - 1) * c * S
    qh = (torch.rand(nodes, F, NB, generator=g, dtype=torch.float64) * 0.25 * S).clamp(min=1) * c
    hist = torch.stack([qg.long(), qh.long(), c], -1)
    if nodes > 2:
        hist[1] = 0  # an empty node
        hist[2] = 0
        hist[2, :, 0] = torch.tensor([S // 3, S // 5, 1])  # a node with one sample
    if F > 2:
        hist[:, 2] = hist[:, 1]  # identical features: the lower index wins
    return hist


@pytest.mark.parametrize("nodes", [1, 128])
@pytest.mark.parametrize("NB", [2, 256])
@pytest.mark.parametrize("F", [1, 33])
def test_split_equals_the_cpu(F, NB, nodes, dev):
    hist = random_hist(nodes, F, NB, seed=F + NB + nodes)
    for lam, mc, mg in ((1.0, 1, 0.0), (0.25, 30, 0.5)):
        ref = run_split(hist, lam, mc, mg)
        assert_split_equal(run_split(hist.to(dev), lam, mc, mg), ref)
        assert F < 3 or not bool((ref[0] == 2).any())
    if nodes > 2:
        assert ref[0][1] == -1 and ref[0][2] == -1


@pytest.mark.parametrize("N,F,NB", HIST_SHAPES)
def test_split_and_leaf_on_the_sample_histograms(N, F, NB, dev):
    for level in (0, 3, 7):
        nodes = 1 << level
        bins, node, gh = hist_inputs(N, F, NB, nodes, seed=level + NB, dirty=False)
        hist = torch.zeros(nodes, F, NB, 3, dtype=I64)
        ops.gbdt_hist(bins, node, gh, hist)
        ref = run_split(hist, 1.0, 2, 0.0)
        got = run_split(hist.to(dev), 1.0, 2, 0.0)
        assert_split_equal(got, ref)
        lc, lg = torch.full((2 * nodes,), 9.0), torch.full((2 * nodes,), 9.0, device=dev)
        ops.gbdt_leaf(ref[3], 1.0, 0.3, lc)
        ops.gbdt_leaf(got[3], 1.0, 0.3, lg)
        assert torch.equal(bits(lg.cpu()), bits(lc))


# ------------------------------------------------------------------------------ grad
def test_gradients_are_within_one_unit_of_fp64(dev):
    z, y = grad_inputs()
    n = z.numel()
    qg, qh, _ = grad64(z, y)
    cpu_gh, cpu_acc = torch.zeros(n, 2, dtype=I32), torch.zeros(1, dtype=I64)
    ops.gbdt_grad(z, y, cpu_gh, cpu_acc)
    for blocks in (0, 1, 7):
        gh, acc = torch.zeros(n, 2, dtype=I32, device=dev), torch.zeros(1, dtype=I64, device=dev)
        ops.gbdt_grad(z.to(dev), y.to(dev), gh, acc, blocks=blocks)
        gh = gh.cpu()
        dg = (gh[:, 0].long() - torch.round(qg).long()).abs()
        dh = (gh[:, 1].long() - torch.round(qh).long()).abs()
        print(f"blocks {blocks}: max |q - round(q64)| g {int(dg.max())} ({float((dg > 0).float().mean()):.4f} differ), "
              f"h {int(dh.max())} ({float((dh > 0).float().mean()):.4f} differ); loss acc {int(acc)} vs CPU "
              f"{int(cpu_acc)}")
        assert int(dg.max()) <= 1 and int(dh.max()) <= 1
        assert int(gh[:, 1].min()) >= 1 and int(gh[:, 0].abs().max()) <= S
        assert abs(int(acc) - int(cpu_acc)) <= n  # one fixed-point unit per sample
    ops.gbdt_grad(z.to(dev), y.to(dev), torch.zeros(n, 2, dtype=I32, device=dev), acc)  # it adds
    assert abs(int(acc) - 2 * int(cpu_acc)) <= 2 * n


# ------------------------------------------------------------------------------ advance / predict
def random_trees(T, depth, F, NB, seed):
    g = torch.Generator().manual_seed(seed)
    nn = (1 << depth) - 1
    feat = torch.randint(0, F, (T, nn), generator=g).to(I32)
    feat[torch.rand(T, nn, generator=g) < 0.25] = -1  # pass-through nodes
    thr = torch.randint(0, NB - 1, (T, nn), generator=g).to(torch.uint8)
    leaf = torch.randn(T, nn + 1, generator=g)
    return feat, thr, leaf


@pytest.mark.parametrize("depth", [1, 8])
def test_advance_and_predict_equal_the_cpu(depth, dev):
    N, F, NB, T = 3001, 7, 16, 3
    bins, _, _ = hist_inputs(N, F, NB, 1, seed=depth, dirty=False)
    feat, thr, leaf = random_trees(T, depth, F, NB, seed=depth)
    for b_cpu, b_dev in ((bins, bins.to(dev)), (bins[:, :F], offset_view(bins[:, :F], dev))):
        zc, zg = torch.zeros(N), torch.zeros(N, device=dev)
        lic, lig = torch.zeros(N, T, dtype=I32), torch.zeros(N, T, dtype=I32, device=dev)
        ops.gbdt_predict(b_cpu, feat, thr, leaf, F, depth, 0.375, zc, lic)
        ops.gbdt_predict(b_dev, feat.to(dev), thr.to(dev), leaf.to(dev), F, depth, 0.375, zg, lig)
        assert torch.equal(bits(zg.cpu()), bits(zc)) and torch.equal(lig.cpu(), lic)
        z2 = torch.zeros(N, device=dev)
        ops.gbdt_predict(b_dev, feat.to(dev), thr.to(dev), leaf.to(dev), F, depth, 0.375, z2, blocks=3)
        assert torch.equal(bits(z2.cpu()), bits(zc))
        # the levels of tree 0 one by one: advance ends where predict ends, and adds the leaf at the last level
        nc, ng = torch.zeros(N, dtype=I32), torch.zeros(N, dtype=I32, device=dev)
        nc[::50] = -1  # out of range: stays out
        ng[::50] = -1
        zc, zg = torch.full((N,), 0.5), torch.full((N,), 0.5, device=dev)
        for d in range(depth):
            lo, hi = (1 << d) - 1, (1 << (d + 1)) - 1
            f, t = feat[0, lo:hi].contiguous(), thr[0, lo:hi].to(I32)
            if d == depth - 1:
                ops.gbdt_advance(b_cpu, nc, f, t, F, leaf[0], zc)
                ops.gbdt_advance(b_dev, ng, f.to(dev), t.to(dev), F, leaf[0].to(dev), zg)
            else:
                ops.gbdt_advance(b_cpu, nc, f, t, F)
                ops.gbdt_advance(b_dev, ng, f.to(dev), t.to(dev), F, blocks=2)
            assert torch.equal(ng.cpu(), nc)
        keep = nc >= 0
        assert torch.equal(nc[keep], lic[keep][:, 0]) and bool((nc[::50] == -1).all())
        assert torch.equal(bits(zg.cpu()), bits(zc)) and bool((zc[::50] == 0.5).all())


# ------------------------------------------------------------------------------ the model
def gpu_run(dev, X, y, rounds, record=None, **cfg):
    m = GBDT(GBDTConfig(**{**dict(num_features=X.shape[1], num_bins=16, depth=3, lr=0.3), **cfg}), Comm(device=dev))
    m.make_cuts(X)
    m.attach(X.to(dev), y.to(dev))
    losses = []
    for _ in range(rounds):
        losses.append(float(m.boost()))
        if record is not None:
            record.append(m.gh.cpu().clone())
    return m, losses


def test_gpu_trees_replay_on_the_cpu_bit_for_bit(dev):
    """5 rounds on the GPU, N = 2000, F = 7, depth 3, 16 bins; the GPU's gh of every round replayed through the
    CPU model gives the same trees and the same z (expf differs between the two by an ulp, so the gradients
    themselves may differ by a unit: they are the one input that is handed over)."""
    (X, y), _ = synth(2000, features=7)
    ghs = []
    g, lg = gpu_run(dev, X, y, 5, record=ghs)
    c, _ = fit(X, y, 0, num_bins=16, depth=3)
    assert torch.equal(c.bins, g.bins.cpu()) and torch.equal(bits(c.cuts), bits(g.cuts.cpu()))
    lc = [float(c.boost(gh=gh)) for gh in ghs]
    for p, q in zip(trees_of(g), trees_of(c)):
        assert torch.equal(p, q)
    assert torch.equal(bits(g.z.cpu()), bits(c.z)) and torch.equal(g.node.cpu(), c.node)
    assert all(abs(a - b) <= 2000 * 2.0 ** -24 + 1e-5 * abs(b) for a, b in zip(lg, lc)) and lg[-1] < lg[0]
    assert bool((g.feat[:5] >= 0).any())
    # prediction against training, on the GPU
    assert torch.equal(bits(g.predict_logits(X.to(dev))), bits(g.z))
    assert torch.equal(g.leaf_index(X.to(dev))[:, -1], g.node)
    rowptr, cols, vals = g.leaf_csr(X.to(dev))
    assert rowptr.is_cuda and cols.numel() == 2000 * 5 and int(cols.max()) < 5 * 8
    # two GPU runs are bit-identical
    g2, lg2 = gpu_run(dev, X, y, 5)
    assert lg2 == lg and torch.equal(bits(g2.z), bits(g.z))
    for p, q in zip(trees_of(g), trees_of(g2)):
        assert torch.equal(p, q)


def test_steady_boost_has_no_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    (X, y), _ = synth(2000, features=7)
    m = GBDT(GBDTConfig(num_features=7, num_bins=16, depth=3, lr=0.3), Comm(device=dev))
    m.make_cuts(X)
    m.attach(X.to(dev), y.to(dev))
    for _ in range(3):  # warm-up: first launches, scratch allocations
        m.boost()
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for _ in range(3):
            audit.step_begin()
            m.boost()
            audit.step_end()
    rep = audit.report()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep
    assert m.num_trees == 6


def test_evaluate_writes_no_model_state(dev):
    (X, y), (Xh, yh) = synth(2000, features=7)
    m, _ = gpu_run(dev, X, y, 3)
    torch.cuda.synchronize()

    def state():
        return [t.clone() for t in (m.feat, m.thr, m.leaf, m.cuts, m.z, m.node, m.gh, m.bins, m._hist, m._loss)], \
            m.num_trees

    before = state()
    r = m.evaluate([(Xh[:1000].to(dev), yh[:1000].to(dev)), (Xh[1000:2000].to(dev), yh[1000:2000].to(dev))])
    torch.cuda.synchronize()
    after = state()
    assert r["n"] == 2000 and r["logloss"] < math.log(2) and before[1] == after[1]
    for a, b in zip(before[0], after[0]):
        assert torch.equal(a, b)
    c, _ = fit(X, y, 0, num_bins=16, depth=3)
    c.load_state_dict(m.state_dict())
    rc = c.evaluate([(Xh[:2000], yh[:2000])])
    assert rc["n"] == 2000 and abs(rc["logloss"] - r["logloss"]) < 1e-6  # the same trees, the same logits


def _gbdt_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _gbdt_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_equal_one_rank(dev):
    many = run_world(_gbdt_two_ranks_gpu, world=2)
    one = _gbdt_world(0, 1, dev=dev)
    print(f"2 ranks on one card {many[0]['losses']} vs one rank {one['losses']}")
    assert len(one["losses"]) == WORLD_ROUNDS
    for r in range(2):
        for k in ("feat", "thr", "leaf", "losses"):
            assert many[r][k] == one[k], (r, k)
        assert many[r]["z"] == one["z"][many[r]["lo"]: many[r]["hi"]]
        assert many[r]["cuts"] == many[0]["cuts"]


def test_empty_inputs_launch_nothing(dev):
    F, NB = 3, 4
    e8 = torch.zeros(0, 16, dtype=torch.uint8, device=dev)
    e32 = torch.zeros(0, dtype=I32, device=dev)
    hist = torch.full((2, F, NB, 3), 5, dtype=I64, device=dev)
    for path in (0, 1, 2):
        ops.gbdt_hist(e8, e32, torch.zeros(0, 2, dtype=I32, device=dev), hist, path=path)
    acc = torch.full((1,), 5, dtype=I64, device=dev)
    ops.gbdt_grad(torch.zeros(0, device=dev), torch.zeros(0, device=dev), torch.zeros(0, 2, dtype=I32, device=dev), acc)
    assert ops.gbdt_bin(torch.zeros(0, F, device=dev), torch.zeros(F, NB - 1, device=dev)).shape == (0, 16)
    ft = torch.zeros(2, dtype=I32, device=dev)
    ops.gbdt_advance(e8, e32, ft, ft, F)
    ops.gbdt_advance(e8, e32, ft, ft, F, torch.zeros(4, device=dev), torch.zeros(0, device=dev))
    z = torch.zeros(0, device=dev)
    ops.gbdt_predict(e8, torch.zeros(1, 1, dtype=I32, device=dev), torch.zeros(1, 1, dtype=torch.uint8, device=dev),
                     torch.zeros(1, 2, device=dev), F, 1, 0.0, z, torch.zeros(0, 1, dtype=I32, device=dev))
    torch.cuda.synchronize()
    assert bool((hist == 5).all()) and int(acc) == 5
    # no tree: the base score
    z = torch.zeros(9, device=dev)
    ops.gbdt_predict(torch.zeros(9, 16, dtype=torch.uint8, device=dev), torch.zeros(0, 7, dtype=I32, device=dev),
                     torch.zeros(0, 7, dtype=torch.uint8, device=dev), torch.zeros(0, 8, device=dev), F, 3, 0.25, z)
    assert bool((z == 0.25).all())
