"""Histogram GBDT in exact fixed point (csrc/kernels/gbdt.h, minips_amd/models/gbdt.py), CPU part: the ops'
references against brute-force loops in Python integers and floats, the fixed-point gradients against the fp64
rule, prediction against the training state, ranks bit for bit, what the trees buy over a linear model, the
GBDT + LR pipeline, state, refusals and the driver."""
import json
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import GBDTSynth
from minips_amd.models.gbdt import GBDT, GBDTConfig
from minips_amd.ps.comm import Comm

CPU = torch.device("cpu")
S = 1 << 20
I32, I64 = torch.int32, torch.int64


def bits(t):
    return t.contiguous().view(I64 if t.dtype == torch.float64 else I32)


# ------------------------------------------------------------------------------ a. histogram
def hist_inputs(N, F, NB, nodes, seed=0, ldb=None, dirty=True):
    """bins uint8 [N, ldb], node int32 [N], gh int32 [N, 2]; ``dirty``: some node ids out of range (negative and
    >= nodes) and, below 256 bins, some bins >= NB."""
    g = torch.Generator().manual_seed(seed)
    ldb = ldb or (F + 15) & ~15
    bins = torch.zeros(N, ldb, dtype=torch.uint8)
    bins[:, :F] = torch.randint(0, NB, (N, F), generator=g).to(torch.uint8)
    node = torch.randint(0, nodes, (N,), generator=g).to(I32)
    if dirty:
        node[::7] = nodes
        node[3::11] = -1
        if NB < 256:
            bins[1::5, F - 1] = NB
            bins[2::9, 0] = 255
    gh = torch.stack([torch.randint(-S, S + 1, (N,), generator=g), torch.randint(1, S // 4 + 1, (N,), generator=g)],
                     1).to(I32)
    return bins, node, gh


def hist_brute(bins, node, gh, nodes, F, NB):
    h = [0] * (nodes * F * NB * 3)
    b, n, q = bins.tolist(), node.tolist(), gh.tolist()
    for i in range(len(n)):
        if not 0 <= n[i] < nodes:
            continue
        for f in range(F):
            if b[i][f] < NB:
                at = ((n[i] * F + f) * NB + b[i][f]) * 3
                h[at] += q[i][0]
                h[at + 1] += q[i][1]
                h[at + 2] += 1
    return torch.tensor(h, dtype=I64).view(nodes, F, NB, 3)


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("NB", [2, 16, 256])
@pytest.mark.parametrize("F", [1, 7])
@pytest.mark.parametrize("N", [1, 65, 1000])
def test_hist_matches_the_integer_loop(N, F, NB, level):
    nodes = 1 << level
    bins, node, gh = hist_inputs(N, F, NB, nodes, seed=N + F + NB)
    ref = hist_brute(bins, node, gh, nodes, F, NB)
    hist = torch.zeros(nodes, F, NB, 3, dtype=I64)
    ops.gbdt_hist(bins, node, gh, hist)
    assert torch.equal(hist, ref)
    ops.gbdt_hist(bins, node, gh, hist)  # it adds
    assert torch.equal(hist, 2 * ref)
    if N == 1000:
        assert int(ref[..., 2].sum()) < N * F  # the out-of-range node ids and bins were skipped


# ------------------------------------------------------------------------------ b. split
def split_brute(hist, lam, min_child, min_gain):
    """The exhaustive loop in Python floats (IEEE doubles, every operation rounded on its own)."""
    nodes, F, NB, _ = hist.shape
    h = hist.tolist()
    sc = 1.0 / S
    feat, thr, gain, child = [], [], [], []
    for n in range(nodes):
        best = None
        for f in range(F):
            tot = [sum(h[n][f][b][c] for b in range(NB)) for c in range(3)]
            G, H = tot[0] * sc, tot[1] * sc
            L = [0, 0, 0]
            for t in range(NB - 1):
                L = [L[c] + h[n][f][t][c] for c in range(3)]
                if L[2] < min_child or tot[2] - L[2] < min_child:
                    continue
                GL, HL, GR, HR = L[0] * sc, L[1] * sc, (tot[0] - L[0]) * sc, (tot[1] - L[1]) * sc
                g = (GL * GL / (HL + lam) + GR * GR / (HR + lam)) - G * G / (H + lam)
                if g > min_gain and (best is None or g > best[0]):
                    best = (g, f, t, list(L), [tot[c] - L[c] for c in range(3)])
        if best is None:
            tot0 = [sum(h[n][0][b][c] for b in range(NB)) for c in range(3)]
            best = (0.0, -1, 0, tot0, [0, 0, 0])
        feat.append(best[1])
        thr.append(best[2])
        gain.append(best[0])
        child.append([best[3], best[4]])
    return (torch.tensor(feat, dtype=I32), torch.tensor(thr, dtype=I32), torch.tensor(gain, dtype=torch.float64),
            torch.tensor(child, dtype=I64))


def run_split(hist, lam=1.0, min_child=1, min_gain=0.0):
    nodes = hist.shape[0]
    dev = hist.device
    out = (torch.full((nodes,), -7, dtype=I32, device=dev), torch.full((nodes,), -7, dtype=I32, device=dev),
           torch.full((nodes,), -7.0, dtype=torch.float64, device=dev),
           torch.full((nodes, 2, 3), -7, dtype=I64, device=dev))
    ops.gbdt_split(hist, lam, min_child, min_gain, *out)
    return out


def assert_split_equal(got, ref):
    for name, a, b in zip(("feat", "thr", "gain", "child"), got, ref):
        a = a.cpu()
        assert torch.equal(bits(a) if name == "gain" else a, bits(b) if name == "gain" else b), (name, a, b)


def split_cases():
    """name -> (hist, lambda, min_child_count, min_gain): random histograms and the tie / no-split cases."""
    cases = {}
    for N, F, NB, level in [(1000, 7, 16, 3), (300, 1, 2, 0), (1000, 3, 256, 1), (65, 7, 16, 0)]:
        nodes = 1 << level
        bins, node, gh = hist_inputs(N, F, NB, nodes, seed=5 + N + NB, dirty=False)
        cases[f"random-{N}-{F}-{NB}-{nodes}"] = (hist_brute(bins, node, gh, nodes, F, NB), 1.0, 1, 0.0)
    bins, node, gh = hist_inputs(1000, 7, 16, 8, seed=2, dirty=False)
    h = hist_brute(bins, node, gh, 8, 7, 16)
    cases["min-child-40-lambda-0.5-min-gain-0.01"] = (h, 0.5, 40, 0.01)
    # two identical features (2 and 5): the lower index wins; feature 0 is constant and never chosen
    bins, node, gh = hist_inputs(500, 6, 8, 2, seed=3, dirty=False)
    bins[:, 0] = 3
    bins[:, 5] = bins[:, 2]
    bins[:, 1] = bins[:, 2] // 4  # coarser than feature 2: never better
    bins[:, 3] = bins[:, 4] = 0
    cases["twins"] = (hist_brute(bins, node, gh, 2, 6, 8), 1.0, 1, 0.0)
    # node 0: one sample; node 1: 5 samples below min_child_count 3 on either side of every cut; node 2: empty;
    # node 3: splittable
    bins = torch.zeros(26, 16, dtype=torch.uint8)
    node = torch.tensor([0] + [1] * 5 + [3] * 20, dtype=I32)
    bins[1:6, 0] = torch.tensor([0, 0, 0, 0, 1], dtype=torch.uint8)
    bins[6:, 0] = torch.arange(20, dtype=torch.uint8) % 4
    gh = torch.stack([torch.tensor([S // 2, -S // 3] * 13), torch.full((26,), S // 4)], 1).to(I32)
    gh[6:, 0] = torch.where(bins[6:, 0] < 2, S // 2, -S // 2).to(I32)
    cases["no-split"] = (hist_brute(bins, node, gh, 4, 2, 4), 1.0, 3, 0.0)
    return cases


SPLIT_CASES = split_cases()


@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_matches_the_exhaustive_loop(name):
    hist, lam, mc, mg = SPLIT_CASES[name]
    got, ref = run_split(hist, lam, mc, mg), split_brute(hist, lam, mc, mg)
    assert_split_equal(got, ref)
    feat, thr, gain, child = got
    if name == "twins":
        assert feat.tolist() == [2, 2]
    if name == "no-split":
        assert feat.tolist() == [-1, -1, -1, 0] and thr.tolist()[:3] == [0, 0, 0] and gain.tolist()[:3] == [0, 0, 0]
        tot = hist[:, 0].sum(1)
        assert torch.equal(child[:3, 0], tot[:3]) and not bool(child[:3, 1].any())
        assert child[0, 0, 2] == 1 and child[1, 0, 2] == 5 and child[2, 0, 2] == 0
        leaf = torch.full((8,), 9.0)
        ops.gbdt_leaf(child, 1.0, 0.1, leaf)
        assert bits(leaf)[4] == 0 and bits(leaf)[5] == 0 and bits(leaf)[1] == 0 and bits(leaf)[3] == 0  # +0.0
        # leaf = -(G / S) / (H / S + lambda) * lr in Python floats, rounded to fp32 once
        c = child.tolist()
        ref = [0.0 if c[n][s][2] == 0 else -(c[n][s][0] / S) / (c[n][s][1] / S + 1.0) * 0.1
               for n in range(4) for s in range(2)]
        assert torch.equal(bits(leaf), bits(torch.tensor(ref, dtype=torch.float64).float()))
    if name.startswith("min-child"):
        ok = feat >= 0
        assert bool((child[ok][:, :, 2] >= 40).all()) and bool((gain[ok] > 0.01).all())


# ------------------------------------------------------------------------------ c. gradients
def grad64(z, labels):
    """The rule in fp64 on the same fp32 logits: (q_g, q_h) before rounding, and the per-sample loss."""
    z64 = z.double()
    zc = z64.clamp(-30, 30)
    p = 1 / (1 + torch.exp(-zc))
    y = (labels > 0.5).double()
    zl = z64.clamp(-64, 64)
    loss = zl.clamp(min=0) - zl * y + torch.log1p(torch.exp(-zl.abs()))
    return (p - y) * S, (p * (1 - p)).clamp(min=1.0 / S) * S, loss


def grad_inputs(n=100_000, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g) * 6
    z[:8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 31.0, -45.0, 80.0, -80.0])
    return z, (torch.rand(n, generator=g) < 0.5).float()


def test_fixed_point_gradients_are_within_one_unit_of_fp64():
    z, y = grad_inputs()
    gh = torch.zeros(z.numel(), 2, dtype=I32)
    acc = torch.zeros(1, dtype=I64)
    ops.gbdt_grad(z, y, gh, acc)
    qg, qh, loss = grad64(z, y)
    dg = (gh[:, 0].long() - torch.round(qg).long()).abs()
    dh = (gh[:, 1].long() - torch.round(qh).long()).abs()
    print(f"max |q - round(q64)|: g {int(dg.max())} ({float((dg > 0).float().mean()):.4f} differ), "
          f"h {int(dh.max())} ({float((dh > 0).float().mean()):.4f} differ)")
    assert int(dg.max()) <= 1 and int(dh.max()) <= 1
    assert int(gh[:, 1].min()) >= 1 and int(gh[:, 0].abs().max()) <= S and int(gh[:, 1].max()) <= S // 4
    # the loss sum: one unit of 2^-24 per sample covers the rounding, the fp32 loss itself a few ulp of <= 64
    ref = float(loss.sum())
    assert abs(int(acc) / 2.0 ** 24 - ref) <= z.numel() * (2.0 ** -24 + 64 * 2.0 ** -22)
    ops.gbdt_grad(z, y, gh, acc)  # it adds
    assert abs(int(acc) / 2.0 ** 24 - 2 * ref) <= 2 * z.numel() * (2.0 ** -24 + 64 * 2.0 ** -22)


def test_labels_in_pm1_are_the_same_as_01():
    z, y = grad_inputs(1000, seed=1)
    a, b = torch.zeros(1000, 2, dtype=I32), torch.zeros(1000, 2, dtype=I32)
    la, lb = torch.zeros(1, dtype=I64), torch.zeros(1, dtype=I64)
    ops.gbdt_grad(z, y, a, la)
    ops.gbdt_grad(z, y * 2 - 1, b, lb)
    assert torch.equal(a, b) and torch.equal(la, lb)


# ------------------------------------------------------------------------------ d. bins and cuts
def test_bins_count_the_cuts_below():
    cuts = torch.tensor([[-1.0, 0.0, 0.5, math.inf], [0.25, math.inf, math.inf, math.inf]])
    X = torch.tensor([[-2.0, 0.0], [-1.0, 0.25], [-0.5, 0.26], [0.0, math.nan], [0.6, math.inf], [math.nan, -math.inf],
                      [math.inf, 1.0], [-math.inf, 0.3]])
    b = ops.gbdt_bin(X, cuts)
    assert b.shape == (8, 16) and b.dtype == torch.uint8 and not bool(b[:, 2:].any())
    assert b[:, 0].tolist() == [0, 0, 1, 1, 3, 0, 3, 0] and b[:, 1].tolist() == [0, 0, 1, 0, 1, 0, 1, 1]
    out = torch.full((8, 3), 77, dtype=torch.uint8)
    ops.gbdt_bin(X, cuts, out=out)
    assert torch.equal(out[:, :2], b[:, :2]) and bool((out[:, 2] == 77).all())


def test_make_cuts_quantiles_deduplicated_and_padded():
    m = GBDT(GBDTConfig(num_features=3, num_bins=8), Comm(device=CPU))
    g = torch.Generator().manual_seed(0)
    X = torch.rand(1000, 3, generator=g)
    X[:, 1] = (X[:, 1] > 0.5).float()  # two values: at most two distinct quantiles
    X[::10, 2] = math.nan
    cuts = m.make_cuts(X)
    assert cuts.shape == (3, 7) and cuts.dtype == torch.float32
    q = torch.quantile(X[:, 0].double(), torch.arange(1, 8, dtype=torch.float64) / 8).float()
    assert torch.equal(cuts[0], q)
    fin = torch.isfinite(cuts[1])
    assert 1 <= int(fin.sum()) <= 2 and bool((cuts[1][~fin] == math.inf).all())
    for f in range(3):
        c = cuts[f][torch.isfinite(cuts[f])]
        assert bool((c[1:] > c[:-1]).all())
    b = m.bin(X)
    assert int(b[:, :3].max()) <= 7 and int(b[::10, 2].max()) == 0  # NaN lands in bin 0
    counts = torch.bincount(b[:, 0].long(), minlength=8)
    assert int(counts.min()) >= 100 and int(counts.max()) <= 150  # equal-frequency bins of 1000 samples


# ------------------------------------------------------------------------------ e. the model
def synth(n=4096, features=8, seed=0, held_seed=99):
    d = GBDTSynth(n, features=features, seed=seed)
    return d.next(), d.holdout(held_seed).next()


def fit(X, y, rounds, comm=None, cuts_from=None, **cfg):
    m = GBDT(GBDTConfig(**{**dict(num_features=X.shape[1], num_bins=32, depth=4, lr=0.3), **cfg}),
             comm or Comm(device=CPU))
    if cuts_from is None:
        m.make_cuts(X)
    else:
        m.set_cuts(cuts_from)
    m.attach(X, y)
    losses = [m.boost() for _ in range(rounds)]
    return m, losses


def trees_of(m):
    T = m.num_trees
    return m.feat[:T].cpu(), m.thr[:T].cpu(), bits(m.leaf[:T].cpu())


def test_predict_reproduces_the_training_logits():
    (X, y), _ = synth(1500)
    m, losses = fit(X, y, 6, depth=3, num_bins=16, base_score=-0.25)
    assert m.num_trees == 6 and torch.equal(bits(m.predict_logits(X)), bits(m.z))
    li = m.leaf_index(X)
    assert li.shape == (1500, 6) and li.dtype == I32 and torch.equal(li[:, -1], m.node)
    assert torch.equal(bits(m.predict_logits(m.bins)), bits(m.z))  # uint8 input is taken as bins
    ls = [float(l) for l in losses]
    # the first round's loss is that of the base score z = -0.25: log1p(exp(-|z|)) - z mean(y)
    assert all(b < a for a, b in zip(ls, ls[1:]))
    assert abs(ls[0] / 1500 - (math.log1p(math.exp(-0.25)) + 0.25 * float(y.mean()))) < 1e-5
    # no tree yet: the base score
    m0 = GBDT(GBDTConfig(num_features=8, base_score=0.5), Comm(device=CPU))
    m0.set_cuts(torch.full((8, 63), math.inf))
    assert bool((m0.predict_logits(X) == 0.5).all()) and m0.leaf_index(X).shape == (1500, 0)


def test_a_given_gh_replaces_the_rounds_gradients():
    (X, y), _ = synth(800)
    a, _ = fit(X, y, 0, depth=3)
    b, _ = fit(X, y, 0, depth=3)
    for _ in range(3):
        a.boost()
        b.z.copy_(a.z + 1.0)  # b's own gradients would differ
        b.boost(gh=a.gh.clone())
        b.z.copy_(a.z)
    for p, q in zip(trees_of(a), trees_of(b)):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------ f. several ranks
WORLD_N, WORLD_ROUNDS = 1536, 4


def _gbdt_world(rank, world, dev=CPU):
    torch.set_num_threads(1)
    (X, y), _ = synth(WORLD_N, seed=4)
    # the cuts of the whole data on every rank (every rank passes the same X: rank 0's cuts are everyone's)
    cuts = GBDT(GBDTConfig(num_features=8, num_bins=32), Comm(device=CPU)).make_cuts(X)
    # uneven shards: rank r takes the rows [lo, hi)
    edges = [0] + [WORLD_N * (r + 1) // world - (7 if r + 1 < world else 0) for r in range(world)]
    lo, hi = edges[rank], edges[rank + 1]
    m, losses = fit(X[lo:hi].to(dev), y[lo:hi].to(dev), WORLD_ROUNDS, comm=Comm(device=dev), cuts_from=cuts)
    f, t, l = trees_of(m)
    # make_cuts on several ranks: rank 0's cuts everywhere
    mine = GBDT(GBDTConfig(num_features=8, num_bins=32), Comm(device=dev)).make_cuts(X[lo:hi].to(dev))
    return dict(feat=f.tolist(), thr=t.tolist(), leaf=l.tolist(), losses=[float(v) for v in losses],
                z=bits(m.z.cpu()).tolist(), lo=lo, hi=hi, cuts=bits(mine.cpu()).tolist())


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_match_one_rank_bit_for_bit(world):
    many = run_world(_gbdt_world, world=world)
    one = _gbdt_world(0, 1)
    print(f"world {world}: losses {many[0]['losses']} vs one rank {one['losses']}")
    for r in range(world):
        for k in ("feat", "thr", "leaf", "losses"):
            assert many[r][k] == one[k], (r, k)
        assert many[r]["z"] == one["z"][many[r]["lo"]: many[r]["hi"]]
        assert many[r]["cuts"] == many[0]["cuts"]
    assert any(f >= 0 for f in one["feat"][0]) and one["losses"][-1] < one["losses"][0]


# ------------------------------------------------------------------------------ g. what it buys
MEASURED = (0.3161, 0.6875)  # held-out log loss: the trees, the logistic regression on the raw features
MEASURED_RATIO = MEASURED[0] / MEASURED[1]


def _raw_lr_logloss(X, y, Xh, yh):
    """A logistic regression on the raw features (with a bias), fitted by full-batch gradient descent in fp64."""
    A = torch.cat([X.double(), torch.ones(X.shape[0], 1, dtype=torch.float64)], 1)
    w = torch.zeros(A.shape[1], dtype=torch.float64)
    for _ in range(500):
        w -= 1.0 * (A.T @ (torch.sigmoid(A @ w) - y.double())) / A.shape[0]
    Ah = torch.cat([Xh.double(), torch.ones(Xh.shape[0], 1, dtype=torch.float64)], 1)
    return float(torch.nn.functional.binary_cross_entropy_with_logits(Ah @ w, yh.double()))


def test_trees_beat_the_linear_model_on_a_nonlinear_teacher():
    """GBDTSynth (a teacher of sign products and gated terms), 4096 training samples, 20 rounds of depth 4 with 32
    bins and lr 0.3, 4096 held-out samples. Measured on this reference path: the trees 0.3161, a logistic
    regression on the raw features 0.6875 (ln 2 = 0.6931). Integer sums make the CPU run bit-reproducible; the
    factor 1.1 covers torch versions (the quantiles, exp)."""
    (X, y), (Xh, yh) = synth(4096)
    m, _ = fit(X, y, 20)
    r = m.evaluate([(Xh, yh)])
    lin = _raw_lr_logloss(X, y, Xh, yh)
    print(f"held-out logloss: gbdt {r['logloss']:.4f} (auc {r['auc']:.4f}), raw-feature LR {lin:.4f}, "
          f"ln 2 {math.log(2):.4f}")
    assert r["n"] == 4096
    assert r["logloss"] < math.log(2)
    assert r["logloss"] < lin
    assert MEASURED_RATIO * 1.1 < 1
    assert r["logloss"] < lin * MEASURED_RATIO * 1.1


# ------------------------------------------------------------------------------ h. the GBDT + LR pipeline
def test_leaf_csr_feeds_the_sparse_lr():
    from minips_amd.models.lr import SparseLR, SparseLRConfig

    (X, y), _ = synth(1024)
    m, _ = fit(X, y, 5, depth=3)
    rowptr, cols, vals = m.leaf_csr(X)
    T, L = 5, 8
    assert rowptr.tolist() == list(range(0, 1024 * T + 1, T)) and bool((vals == 1).all())
    assert torch.equal(cols.view(1024, T), m.leaf_index(X).long() + torch.arange(T)[None, :] * L)
    assert int(cols.max()) < T * L
    # (the reference step w += alpha * sum over the batch: a leaf holds about 1024 / 8 samples)
    lr = SparseLR(SparseLRConfig(num_dims=T * L, alpha=0.005), Comm(device=CPU))

    def loss():
        w = lr.table.get_rows(cols).view(1024, T).sum(1).float()
        return float(torch.nn.functional.binary_cross_entropy_with_logits(w, y))

    first = loss()
    for _ in range(20):
        lr.train_step(rowptr, cols, vals, y)
    lr.drain()
    last = loss()
    print(f"LR on the leaves: log loss {first:.4f} -> {last:.4f}")
    assert abs(first - math.log(2)) < 1e-6 and last < 0.9 * first


# ------------------------------------------------------------------------------ i. state
def test_state_round_trip_and_continuation(tmp_path):
    (X, y), (Xh, _) = synth(1000)
    a, _ = fit(X, y, 3, depth=3, base_score=0.125, reg_lambda=2.0)
    sd = a.state_dict()
    assert sd["num_trees"] == 3 and sd["feat"].shape == (3, 7) and sd["config"]["depth"] == 3
    path = str(tmp_path / "trees.pt")
    a.save(path)
    # another model, other hyperparameters: they come with the state
    b = GBDT(GBDTConfig(num_features=8, num_bins=32, depth=3, lr=0.9, max_trees=16), Comm(device=CPU))
    b.load(path)
    assert b.num_trees == 3 and b.cfg.lr == 0.3 and b.cfg.reg_lambda == 2.0 and b.cfg.base_score == 0.125
    for k in ("cuts", "feat", "thr", "leaf"):
        assert torch.equal(b.state_dict()[k], sd[k]) and b.state_dict()[k].dtype == sd[k].dtype
    assert torch.equal(bits(b.predict_logits(Xh)), bits(a.predict_logits(Xh)))
    b.attach(X, y)
    assert torch.equal(bits(b.z), bits(a.z))
    la, lb = [float(a.boost()) for _ in range(2)], [float(b.boost()) for _ in range(2)]
    assert la == lb and torch.equal(bits(b.z), bits(a.z))
    for p, q in zip(trees_of(a), trees_of(b)):
        assert torch.equal(p, q)
    c = GBDT(GBDTConfig(num_features=8, num_bins=32, depth=3), Comm(device=CPU)).load_state_dict(a.state_dict())
    assert c.num_trees == 5
    with pytest.raises(ValueError, match="gbdt"):
        GBDT(GBDTConfig(num_features=8, num_bins=32, depth=4), Comm(device=CPU)).load_state_dict(sd)
    with pytest.raises(ValueError, match="gbdt"):
        GBDT(GBDTConfig(num_features=8, num_bins=32, depth=3, max_trees=2), Comm(device=CPU)).load_state_dict(sd)


# ------------------------------------------------------------------------------ j. refusals
@pytest.mark.parametrize("kw", [dict(num_bins=1), dict(num_bins=257), dict(depth=0), dict(depth=9),
                                dict(num_features=0), dict(num_features=4097), dict(reg_lambda=0.0),
                                dict(reg_lambda=-1.0), dict(min_child_count=0), dict(min_gain=-0.1), dict(lr=0.0),
                                dict(max_trees=0), dict(transport="onesided"),
                                dict(num_features=4096, num_bins=256, depth=8)],  # hist above 1 GiB
                         ids=lambda kw: "-".join(f"{a}={b}" for a, b in kw.items()))
def test_config_refusals_name_gbdt(kw):
    with pytest.raises(ValueError, match="gbdt"):
        GBDTConfig(**{**dict(num_features=8), **kw})


def test_model_refusals_name_gbdt(monkeypatch):
    import minips_amd.models.gbdt as G

    (X, y), _ = synth(64)
    m = GBDT(GBDTConfig(num_features=8, num_bins=4, depth=1, max_trees=2), Comm(device=CPU))
    with pytest.raises(ValueError, match="gbdt.*cuts"):
        m.attach(X, y)
    with pytest.raises(ValueError, match="gbdt"):
        m.bin(X)
    with pytest.raises(ValueError, match="gbdt"):
        m.set_cuts(torch.zeros(8, 4))
    m.make_cuts(X)
    with pytest.raises(ValueError, match="gbdt"):
        m.boost()  # before attach
    with pytest.raises(ValueError, match="gbdt"):
        m.attach(X, y[:-1])
    with pytest.raises(ValueError, match="gbdt"):
        m.attach(X[:, :7], y)
    m.attach(X, y)
    with pytest.raises(ValueError, match="gbdt"):
        m.boost(gh=torch.zeros(64, 2, dtype=I64))
    m.boost()
    m.boost()
    with pytest.raises(ValueError, match="gbdt.*max_trees"):
        m.boost()
    monkeypatch.setattr(G, "MAX_SAMPLES", 63)  # (2^33 - 1 samples do not fit a test)
    with pytest.raises(ValueError, match="gbdt.*samples"):
        m.attach(X, y)
    assert G.MAX_SAMPLES == 63 and (1 << 33) - 1 == 8589934591


def test_gpu_tensors_need_the_extension(monkeypatch):
    """A GPU tensor without the extension is an error, never a fall-back to the reference."""
    import minips_amd.ops as O

    def missing():
        raise RuntimeError("minips_amd._gbdtk is not built")

    monkeypatch.setattr(O, "gbdtk", missing)
    monkeypatch.setattr(O, "_gpu", lambda t: True)
    bins, node, gh = hist_inputs(8, 2, 4, 1)
    hist = torch.zeros(1, 2, 4, 3, dtype=I64)
    calls = [lambda: O.gbdt_bin(torch.zeros(8, 2), torch.zeros(2, 3)),
             lambda: O.gbdt_grad(torch.zeros(8), torch.zeros(8), gh, torch.zeros(1, dtype=I64)),
             lambda: O.gbdt_hist(bins, node, gh, hist),
             lambda: run_split(hist),
             lambda: O.gbdt_leaf(torch.zeros(1, 2, 3, dtype=I64), 1.0, 0.1, torch.zeros(2)),
             lambda: O.gbdt_advance(bins, node, torch.zeros(1, dtype=I32), torch.zeros(1, dtype=I32), 2),
             lambda: O.gbdt_predict(bins, torch.zeros(1, 1, dtype=I32), torch.zeros(1, 1, dtype=torch.uint8),
                                    torch.zeros(1, 2), 2, 1, 0.0, torch.zeros(8))]
    for call in calls:
        with pytest.raises(RuntimeError, match="_gbdtk"):
            call()


def test_cpu_ops_refuse_bad_shapes():
    bins, node, gh = hist_inputs(8, 2, 4, 1)
    with pytest.raises(RuntimeError, match="gbdt"):
        ops.gbdt_hist(bins, node, gh, torch.zeros(3, 2, 4, 3, dtype=I64))  # nodes is no power of two
    with pytest.raises(RuntimeError, match="gbdt"):
        ops.gbdt_hist(bins, node, gh, torch.zeros(1, 2, 4, 3, dtype=I32))
    with pytest.raises(RuntimeError, match="gbdt"):
        ops.gbdt_hist(bins[:, :1], node, gh, torch.zeros(1, 2, 4, 3, dtype=I64))
    with pytest.raises(RuntimeError, match="gbdt"):
        run_split(torch.zeros(1, 2, 4, 3, dtype=I64), lam=0.0)
    with pytest.raises(RuntimeError, match="gbdt"):
        ops.gbdt_advance(bins, node, torch.zeros(1, dtype=I32), torch.zeros(1, dtype=I32), 2, leaf=torch.zeros(2))
    # empty inputs are fine
    hist = torch.zeros(1, 2, 4, 3, dtype=I64)
    ops.gbdt_hist(bins[:0], node[:0], gh[:0], hist)
    assert not bool(hist.any())
    assert ops.gbdt_bin(torch.zeros(0, 2), torch.zeros(2, 3)).shape == (0, 16)
    assert ops.gbdt_advance(bins[:0], node[:0], torch.zeros(1, dtype=I32), torch.zeros(1, dtype=I32), 2).numel() == 0


# ------------------------------------------------------------------------------ k. the driver
def test_driver_flags():
    from minips_amd.train import parse

    a = parse(["--model", "gbdt", "--steps", "7", "--gbdt_depth", "4", "--gbdt_bins", "32", "--gbdt_lr", "0.3",
               "--gbdt_lambda", "2", "--gbdt_rows", "100", "--gbdt_features", "9", "--gbdt_model_out", "x.pt",
               "--eval_every", "5"])
    assert (a.model, a.gbdt_depth, a.gbdt_bins, a.gbdt_lr, a.gbdt_lambda, a.gbdt_rows, a.gbdt_features) == \
        ("gbdt", 4, 32, 0.3, 2.0, 100, 9) and a.transport == "collective"
    a = parse(["--model", "gbdt"])
    assert (a.gbdt_depth, a.gbdt_bins, a.gbdt_lr, a.gbdt_lambda, a.gbdt_features) == (6, 64, 0.1, 1.0, 8)
    assert parse(["--model", "gbdt", "--input", "x.libsvm", "--gbdt_features", "3"]).gbdt_features == 3
    for bad in (["--model", "gbdt", "--gbdt_depth", "0"], ["--model", "gbdt", "--gbdt_depth", "9"],
                ["--model", "gbdt", "--gbdt_bins", "1"], ["--model", "gbdt", "--gbdt_bins", "257"],
                ["--model", "gbdt", "--gbdt_lr", "0"], ["--model", "gbdt", "--gbdt_lambda", "0"],
                ["--model", "gbdt", "--gbdt_features", "4"], ["--model", "gbdt", "--gbdt_features", "4097"],
                ["--model", "gbdt", "--gbdt_rows", "0"], ["--model", "gbdt", "--transport", "onesided"],
                ["--model", "gbdt", "--consistency", "ssp"], ["--model", "gbdt", "--input", "x.libsvm"],
                ["--model", "gbdt", "--input", "x.libsvm", "--gbdt_features", "3", "--eval_every", "5"],
                ["--model", "gbdt", "--input", "x.libsvm", "--gbdt_features", "3", "--gbdt_rows", "10"],
                ["--model", "gbdt", "--gbdt_features", "4096", "--gbdt_bins", "256", "--gbdt_depth", "8"],
                ["--model", "gbdt", "--checkpoint_toggle", "1"],
                ["--model", "fm", "--gbdt_depth", "4"], ["--model", "lr", "--gbdt_bins", "32"],
                ["--model", "widedeep", "--gbdt_lr", "0.1"], ["--model", "ffm", "--gbdt_lambda", "1"],
                ["--model", "lr", "--gbdt_rows", "10"], ["--model", "lr", "--gbdt_features", "8"],
                ["--model", "lr", "--gbdt_model_out", "x.pt"]):
        with pytest.raises(SystemExit):
            parse(bad)


def test_driver_runs_gbdt_on_the_synthetic_shard(tmp_path, capsys):
    from minips_amd.train import main

    out_path = str(tmp_path / "model.pt")
    assert main(["--model", "gbdt", "--small", "1", "--steps", "10", "--gbdt_depth", "3", "--gbdt_bins", "16",
                 "--gbdt_lr", "0.3", "--gbdt_rows", "1000", "--eval_every", "5", "--eval_batches", "1",
                 "--gbdt_model_out", out_path]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "gbdt" and (out["gbdt_trees"], out["gbdt_depth"], out["gbdt_bins"]) == (10, 3, 16)
    assert len(out["evals"]) == 2 and out["evals"][1][2] < out["evals"][0][2] < math.log(2)
    assert out["losses"][-1][0] == 9 and out["losses"][-1][1] < math.log(2)
    m = GBDT(GBDTConfig(num_features=8, num_bins=16, depth=3), Comm(device=CPU))
    m.load(out_path)
    assert m.num_trees == 10 and abs(float(m.leaf[:10].double().sum()) - out["checksum"][0]) < 1e-5


def test_driver_runs_gbdt_on_a_libsvm_file(tmp_path, capsys):
    from minips_amd.train import main

    g = torch.Generator().manual_seed(1)
    lines = []
    for _ in range(200):
        x = torch.rand(4, generator=g) * 2 - 1
        label = "1" if (x[0] * x[1] > 0) else "-1"
        # libsvm ids are 1-based; feature 3 is absent in some rows (0.0), id 9 lies beyond --gbdt_features
        feats = [f"{j + 1}:{float(x[j]):.4f}" for j in range(4) if j != 2 or x[2] > 0] + ["9:1"]
        lines.append(label + " " + " ".join(feats))
    path = tmp_path / "d.libsvm"
    path.write_text("\n".join(lines) + "\n")
    assert main(["--model", "gbdt", "--input", str(path), "--gbdt_features", "4", "--gbdt_depth", "2", "--gbdt_bins",
                 "8", "--gbdt_lr", "0.5", "--steps", "10"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "gbdt" and out["gbdt_trees"] == 10
    assert out["losses"][-1][1] < 0.5  # x0 x1 > 0 is two levels deep: far below ln 2
