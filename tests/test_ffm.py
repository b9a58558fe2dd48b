"""Field-aware factorization machine on the sparse PS (minips_amd/models/ffm.py, ops.ffm_forward /
ops.ffm_backward), CPU side: the fp32 reference ops against fp64 autograd of the pairwise formula written with
explicit loops, against the FM ops at F = 1 and against the bounds the GPU test uses; learning against the FM
of the same parameter count; the linear limit; ranks over gloo against one rank; evaluation beside training;
the FTRL linear column; checkpoints; and every refusal."""
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import FFMSynth
from minips_amd.models.ffm import FFM, FFMConfig
from minips_amd.models.fm import FM, FMConfig
from minips_amd.ps.comm import Comm

CPU = torch.device("cpu")
U = 2.0 ** -24


# ------------------------------------------------------------------------------ a. ops against autograd
def _batch(F, k, labels_pm1=False, seed=0):
    """5 samples over 7 pulled rows (cap 9 > U): a duplicate feature within sample 0 (row 0 twice), two
    features in one field (sample 3, and sample 0's duplicate), an empty sample 2, negative values, a row (4) no
    lookup reads."""
    g = torch.Generator().manual_seed(seed)
    rowptr = torch.tensor([0, 4, 6, 6, 9, 11])
    inv = torch.tensor([0, 3, 0, 5, 1, 2, 6, 0, 2, 5, 1])
    fields = torch.tensor([0, 1, 0, 2, 1, 4, 3, 3, 0, 2, 63], dtype=torch.int32) % F
    vals = torch.randn(11, generator=g)
    vals[2] = -1.5
    labels = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])
    if labels_pm1:
        labels = labels * 2 - 1
    rows = torch.randn(9, F * k + 4, generator=g) * 0.5
    rows[:, F * k + 1:] = 0
    w0 = torch.tensor([0.3])
    return rowptr, inv, vals, fields, labels, rows, w0


def _pairwise_loss64(rowptr, inv, vals, fields, labels, rows64, w0_64, F, k, gscale):
    """The rule of csrc/kernels/ffm.h per sample, with explicit loops over the pairs of lookups i < j."""
    total = rows64.new_zeros(())
    zs = []
    for b in range(rowptr.numel() - 1):
        js = range(int(rowptr[b]), int(rowptr[b + 1]))
        z = w0_64[0].clone()
        for j in js:
            z = z + rows64[inv[j], F * k] * vals[j].double()
        for a in js:
            for c in js:
                if a < c:
                    fa, fc = int(fields[a]), int(fields[c])
                    va = rows64[inv[a], fc * k: fc * k + k]
                    vc = rows64[inv[c], fa * k: fa * k + k]
                    z = z + (va * vc).sum() * vals[a].double() * vals[c].double()
        y = 1.0 if labels[b] > 0.5 else 0.0
        total = total + (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))) * gscale
        zs.append(z)
    return total, torch.stack(zs)


@pytest.mark.parametrize("F,k", [(1, 4), (3, 4), (5, 8), (64, 8)])
@pytest.mark.parametrize("pm1", [False, True], ids=["01", "pm1"])
def test_cpu_ops_match_fp64_autograd(F, k, pm1):
    rowptr, inv, vals, fields, labels, rows, w0 = _batch(F, k, pm1)
    gscale = 1.0 / 5
    z, dz, loss, rowid = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, gscale)
    assert rowid.dtype == torch.int32 and rowid.tolist() == [0, 0, 0, 0, 1, 1, 3, 3, 3, 4, 4]
    sentinel = 7.0
    grad = torch.full((9, F * k + 4), sentinel)
    ops.ffm_backward(inv, rowid, rowptr, vals, fields, dz, rows, F, k, grad)
    rows64 = rows.double().requires_grad_(True)
    w64 = w0.double().requires_grad_(True)
    total, z64 = _pairwise_loss64(rowptr, inv, vals, fields, labels, rows64, w64, F, k, gscale)
    total.backward()
    assert float(z[2]) == float(w0[0])  # the empty sample
    torch.testing.assert_close(z.double(), z64.detach(), rtol=1e-5, atol=1e-6)
    y = (labels > 0.5).double()
    l64 = z64.detach().clamp(min=0) - z64.detach() * y + torch.log1p(torch.exp(-z64.detach().abs()))
    torch.testing.assert_close(loss.double(), l64, rtol=1e-5, atol=1e-6)
    touched = torch.zeros(9, dtype=torch.bool)
    touched[inv] = True
    FK = F * k
    torch.testing.assert_close(grad[touched][:, :FK + 1].double(), rows64.grad[touched][:, :FK + 1], rtol=1e-5,
                               atol=1e-6)
    assert bool((grad[touched][:, FK + 1:] == 0).all())
    assert bool((grad[~touched] == sentinel).all())  # rows without lookups are left untouched
    torch.testing.assert_close(dz.sum().double(), w64.grad[0], rtol=1e-5, atol=1e-7)  # the bias gradient


def test_cpu_ops_skip_out_of_range_lookups():
    """A lookup whose inv or field is out of range contributes nothing and receives nothing: the outputs equal
    those of the batch without it."""
    F, k = 3, 4
    rowptr, inv, vals, fields, labels, rows, w0 = _batch(F, k)
    keep = torch.tensor([0, 1, 2, 3, 4, 5, 6, 8, 9, 10])  # without lookup 7 (sample 3)
    rp2 = torch.tensor([0, 4, 6, 6, 8, 10])
    ref = ops.ffm_forward(rp2, inv[keep], vals[keep], fields[keep], labels, rows, F, k, w0, 0.2)
    gref = torch.zeros(9, F * k + 4)
    ops.ffm_backward(inv[keep], ref[3], rp2, vals[keep], fields[keep], ref[1], rows, F, k, gref)
    for bad_inv, bad_field in ((9, 0), (-1, 0), (0, F), (0, -1)):
        inv2, f2 = inv.clone(), fields.clone()
        if bad_inv != 0:
            inv2[7] = bad_inv
        else:
            f2[7] = bad_field
        z, dz, loss, rowid = ops.ffm_forward(rowptr, inv2, vals, f2, labels, rows, F, k, w0, 0.2)
        assert torch.equal(z, ref[0]) and torch.equal(dz, ref[1]) and torch.equal(loss, ref[2])
        g = torch.zeros(9, F * k + 4)
        ops.ffm_backward(inv2, rowid, rowptr, vals, f2, dz, rows, F, k, g)
        assert torch.equal(g, gref)


def test_cpu_ops_empty_batch_and_bad_shapes():
    rows = torch.zeros(3, 12)
    e64, ef, e32 = torch.zeros(0, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.int32)
    z, dz, loss, rowid = ops.ffm_forward(torch.zeros(1, dtype=torch.int64), e64, ef, e32, ef, rows, 2, 4)
    assert z.numel() == 0 and rowid.numel() == 0
    g = torch.full((3, 12), 2.0)
    ops.ffm_backward(e64, rowid, torch.zeros(1, dtype=torch.int64), ef, e32, dz, rows, 2, 4, g)
    assert bool((g == 2.0).all())
    for F, k in ((1, 0), (1, 6), (1, 20), (0, 4), (65, 4), (64, 12)):
        with pytest.raises(RuntimeError, match="ffm"):
            ops.ffm_forward(torch.zeros(1, dtype=torch.int64), e64, ef, e32, ef, torch.zeros(3, 1024), F, k)
    with pytest.raises(RuntimeError, match="wide"):
        ops.ffm_forward(torch.zeros(1, dtype=torch.int64), e64, ef, e32, ef, torch.zeros(3, 11), 2, 4)


# ------------------------------------------------------------------------------ b. F = 1 is the FM
def _random_batch(F, k, B, seed, nnz_choices=(0, 1, 2, 5, 9), num_rows=12):
    g = torch.Generator().manual_seed(seed)
    nnz = torch.tensor(nnz_choices)[torch.randint(0, len(nnz_choices), (B,), generator=g)]
    nnz[: len(nnz_choices)] = torch.tensor(nnz_choices)[: B]
    rowptr = torch.zeros(B + 1, dtype=torch.int64)
    rowptr[1:] = nnz.cumsum(0)
    n = int(rowptr[-1])
    inv = torch.randint(0, num_rows, (n,), generator=g)
    fields = torch.randint(0, F, (n,), generator=g).to(torch.int32)
    vals = torch.randn(n, generator=g)
    labels = (torch.rand(B, generator=g) < 0.5).float()
    rows = torch.randn(num_rows + 2, F * k + 4, generator=g) * (0.6 / math.sqrt(k))
    rows[:, F * k + 1:] = 0
    return rowptr, inv, vals, fields, labels, rows, torch.tensor([0.25])


@pytest.mark.parametrize("k", [4, 16])
def test_one_field_is_the_fm(k):
    """With F = 1 the rule is the FM's. Both fp32 ops sit within their own bounds of the exact value (below, and
    tests/test_fm_gpu.py for the FM), so they differ by at most the two bounds' sum."""
    rowptr, inv, vals, fields, labels, rows, w0 = _random_batch(1, k, 40, seed=k)
    gs = 1.0 / 40
    z, dz, loss, rowid = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, 1, k, w0, gs)
    S, z_fm, dz_fm, loss_fm, rowid_fm = ops.fm_forward(rowptr, inv, vals, labels, rows, k, w0, gs)
    assert torch.equal(rowid, rowid_fm)
    ref = _forward64(rowptr, inv, vals, fields, labels, rows, w0, 1, k, gs)
    nnz = (rowptr[1:] - rowptr[:-1]).double()
    rid = rowid.long()
    p = rows[inv, :k].double() * vals.double()[:, None]
    Sabs = torch.zeros(40, k, dtype=torch.float64).index_add_(0, rid, p.abs())
    Q = torch.zeros(40, dtype=torch.float64).index_add_(0, rid, (p * p).sum(1))
    lin = torch.zeros(40, dtype=torch.float64).index_add_(0, rid, (rows[inv, k].double() * vals.double()).abs())
    b_fm = (2 * nnz + k + 16) * U * (0.25 + lin + 0.5 * ((Sabs * Sabs).sum(1) + Q))  # test_fm_gpu.py's bound
    assert bool(((z.double() - z_fm.double()).abs() <= ref["bz"] + b_fm).all())
    g, g_fm = torch.zeros(rows.shape[0], k + 4), torch.zeros(rows.shape[0], k + 4)
    ops.ffm_backward(inv, rowid, rowptr, vals, fields, dz_fm, rows, 1, k, g)
    ops.fm_backward(inv, rowid, vals, dz_fm, S, rows, k, g_fm)
    g64, bound, touched = _backward64(rowptr, inv, vals, fields, dz_fm, rows, 1, k)
    # the FM's bound (test_fm_gpu.py): (M + 6) u sum_m |c_m| (|S| + |v x_m|)
    c = dz_fm.double()[rid] * vals.double()
    mag = torch.zeros(rows.shape[0], k, dtype=torch.float64).index_add_(
        0, inv, c.abs()[:, None] * (S.double()[rid].abs() + p.abs()))
    M = torch.zeros(rows.shape[0], dtype=torch.float64).index_add_(0, inv, torch.ones_like(c))
    b_g = bound[:, :k] + (M + 6)[:, None] * U * mag
    assert bool(((g[:, :k].double() - g_fm[:, :k].double()).abs() <= b_g).all())
    torch.testing.assert_close(g[:, k], g_fm[:, k], rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------ c. the reference meets the GPU bounds
def _padded(rowptr, inv, vals, fields, cap, F):
    B = rowptr.numel() - 1
    cnt = rowptr[1:] - rowptr[:-1]
    Mx = max(int(cnt.max()) if B else 0, 1)
    ar = torch.arange(Mx)
    inside = ar[None, :] < cnt[:, None]
    pos = torch.where(inside, rowptr[:-1, None] + ar[None, :], torch.zeros(1, dtype=torch.int64))
    n = inv.numel()
    if n == 0:
        z = torch.zeros(B, Mx, dtype=torch.int64)
        return z, z, torch.zeros(B, Mx, dtype=torch.float64), z.bool(), z
    r, f = inv[pos], fields[pos].long()
    ok = inside & (r >= 0) & (r < cap) & (f >= 0) & (f < F)
    return r * ok, f * ok, vals.double()[pos] * ok, ok, pos


def _forward64(rowptr, inv, vals, fields, labels, rows, w0, F, k, gscale, chunk=16):
    """Vectorised fp64 of the forward rule on fp32 inputs and the bounds of its fp32 evaluation:
    |z - z64| <= (P_b + nnz_b + k + 16) u A_b, A_b = |w0| + sum |w x| + sum_{i<j} sum_c |v v'| |x_i x_j|;
    dz and loss as in tests/test_fm_gpu.py."""
    B, cap, FK = rowptr.numel() - 1, rows.shape[0], F * k
    r, f, x, ok, pos = _padded(rowptr, inv, vals, fields, cap, F)
    Mx = r.shape[1]
    slots = rows[:, :FK].double().reshape(cap * F, k)
    wx = rows[:, FK].double()[r] * x
    lin, linabs = wx.sum(1), wx.abs().sum(1)
    upper = torch.triu(torch.ones(Mx, Mx, dtype=torch.bool), diagonal=1)
    pair, pairabs = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for lo in range(0, B, chunk):
        rr, ff, xx = r[lo:lo + chunk], f[lo:lo + chunk], x[lo:lo + chunk]
        A = slots[rr[:, :, None] * F + ff[:, None, :]]
        xx2 = xx[:, :, None] * xx[:, None, :] * upper
        At = A.transpose(1, 2)
        pair[lo:lo + chunk] = ((A * At).sum(-1) * xx2).sum((1, 2))
        pairabs[lo:lo + chunk] = ((A * At).abs().sum(-1) * xx2.abs()).sum((1, 2))
    z = w0.double()[0] + lin + pair
    y = (labels > 0.5).double()
    dz = (torch.sigmoid(z) - y) * gscale
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    nnz = (rowptr[1:] - rowptr[:-1]).double()
    P = nnz * (nnz - 1) / 2
    A_b = w0.double().abs()[0] + linabs + pairabs
    bz = (P + nnz + k + 16) * U * A_b
    return dict(z=z, dz=dz, loss=loss, bz=bz, bdz=gscale * (bz / 4 + 4 * U), bloss=bz + 4 * U * (z.abs() + 1))


def _backward64(rowptr, inv, vals, fields, dz, rows, F, k, chunk=16, member_ok=None):
    """Vectorised fp64 of the backward rule on fp32 inputs, its bound per element -- (N + 6) u sum |terms| with N
    the (member, partner) terms of the element, (M_u + 2) u sum |c_m| on the linear column -- and the rows that
    have lookups. ``member_ok`` [n] bool: lookups that receive nothing as members (they stay partners)."""
    B, cap, FK = rowptr.numel() - 1, rows.shape[0], F * k
    r, f, x, ok, pos = _padded(rowptr, inv, vals, fields, cap, F)
    Mx = r.shape[1]
    c = dz.double()[:, None] * x
    if member_ok is not None:
        c = c * member_ok[pos]
    slots = rows[:, :FK].double().reshape(cap * F, k)
    acc, mag = torch.zeros(cap * F, k, dtype=torch.float64), torch.zeros(cap * F, k, dtype=torch.float64)
    cntN = torch.zeros(cap * F, dtype=torch.float64)
    off = ~torch.eye(Mx, dtype=torch.bool)
    for lo in range(0, B, chunk):
        rr, ff, xx, oo = r[lo:lo + chunk], f[lo:lo + chunk], x[lo:lo + chunk], ok[lo:lo + chunk]
        pair = oo[:, :, None] & oo[:, None, :] & off
        if member_ok is not None:
            pair = pair & member_ok[pos[lo:lo + chunk]][:, :, None]
        src = (rr[:, None, :] * F + ff[:, :, None]).expand(-1, Mx, Mx)[pair]
        dst = (rr[:, :, None] * F + ff[:, None, :]).expand(-1, Mx, Mx)[pair]
        s = (c[lo:lo + chunk][:, :, None] * xx[:, None, :]).expand(-1, Mx, Mx)[pair]
        t = slots[src] * s[:, None]
        acc.index_add_(0, dst, t)
        mag.index_add_(0, dst, t.abs())
        cntN.index_add_(0, dst, torch.ones_like(s))
    g = torch.zeros(cap, FK + 4, dtype=torch.float64)
    bound = torch.zeros(cap, FK + 4, dtype=torch.float64)
    g[:, :FK] = acc.reshape(cap, FK)
    bound[:, :FK] = ((cntN + 6)[:, None] * U * mag).reshape(cap, FK)
    mo = ok if member_ok is None else ok & member_ok[pos]
    g[:, FK] = torch.zeros(cap, dtype=torch.float64).index_add_(0, r[mo], c[mo])
    M = torch.zeros(cap, dtype=torch.float64).index_add_(0, r[mo], torch.ones_like(c[mo]))
    bound[:, FK] = (M + 2) * U * torch.zeros(cap, dtype=torch.float64).index_add_(0, r[mo], c[mo].abs())
    touched = torch.zeros(cap, dtype=torch.bool)
    touched[inv[(inv >= 0) & (inv < cap)]] = True
    return g, bound, touched


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - bound).max()) if err.numel() else 0.0
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"  {name}: max err {float(err.max()) if err.numel() else 0.0:.3e}, max err / bound {ratio:.3f}")
    assert worst <= 0, f"{name}: error exceeds the bound by {worst:.3e} (err / bound {ratio:.3f})"


@pytest.mark.parametrize("F,k", [(1, 4), (5, 8), (39, 4), (26, 16)])
def test_cpu_reference_meets_the_gpu_bounds(F, k):
    rowptr, inv, vals, fields, labels, rows, w0 = _random_batch(F, k, 33, seed=F + k, nnz_choices=(0, 1, 2, 17, 40))
    gs = 1.0 / 33
    ref = _forward64(rowptr, inv, vals, fields, labels, rows, w0, F, k, gs)
    assert float(ref["z"].abs().max()) < 60
    z, dz, loss, rowid = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, gs)
    _within("z", z, ref["z"], ref["bz"])
    _within("dz", dz, ref["dz"], ref["bdz"])
    _within("loss", loss, ref["loss"], ref["bloss"])
    g64, bound, touched = _backward64(rowptr, inv, vals, fields, dz, rows, F, k)
    g = torch.full((rows.shape[0], F * k + 4), 7.0)
    ops.ffm_backward(inv, rowid, rowptr, vals, fields, dz, rows, F, k, g)
    FK = F * k
    _within("grad", g[touched][:, :FK + 1], g64[touched][:, :FK + 1], bound[touched][:, :FK + 1])
    assert bool((g[touched][:, FK + 1:] == 0).all()) and bool((g[~touched] == 7.0).all())


# ------------------------------------------------------------------------------ d. learning
def _held(data, n=8, seed=99):
    hold = data.holdout(seed)
    return [hold.next() for _ in range(n)]


def _train_ffm(std=0.01, steps=200, evals_at=(), batch=512, **cfg):
    data = FFMSynth(batch, fields=8, card=32, seed=0)
    m = FFM(FFMConfig(num_dims=data.num_dims, num_fields=8, k=4, lr=0.05, init_std=std, **cfg), Comm(device=CPU))
    held = _held(data)
    losses = []
    for i in range(steps):
        if i in evals_at:
            m.evaluate(held)
        losses.append(float(m.train_step(*data.next())))
    return m, losses, held


def _train_fm(k, steps=200):
    data = FFMSynth(512, fields=8, card=32, seed=0)  # the same labels
    m = FM(FMConfig(num_dims=data.num_dims, k=k, lr=0.05, init_std=0.01), Comm(device=CPU))
    for _ in range(steps):
        m.train_step(*data.next())
    return m


# FFM k = 4 / FM k = 32 held-out log loss measured on this reference path: 0.4595 / 0.5742
MEASURED_RATIO = 0.4595 / 0.5742


def test_ffm_beats_the_fm_of_the_same_size():
    """Held-out log loss (8 batches of 512) after 200 steps of 512 samples on labels of a field-aware teacher
    (8 fields x 32 ids, rank 4), lr 0.05, seed 0: FFM k = 4 against the FM with the same parameter count
    (k = 32) and the FM k = 8. Measured on this reference path: FFM 0.4595, FM k = 32 0.5742, FM k = 8 0.6473
    (the linear model 0.6778, ln 2 = 0.6931). CPU training is bit-reproducible, the factor 1.1 covers torch
    versions."""
    ffm, _, held = _train_ffm()
    r = ffm.evaluate(held)
    r32, r8 = _train_fm(32).evaluate(held), _train_fm(8).evaluate(held)
    print(f"held-out logloss: ffm k=4 {r['logloss']:.4f} (auc {r['auc']:.4f}), fm k=32 {r32['logloss']:.4f}, "
          f"fm k=8 {r8['logloss']:.4f}, ln 2 {math.log(2):.4f}")
    assert r["n"] == 8 * 512
    assert r["logloss"] < math.log(2)
    assert r["logloss"] < r32["logloss"]
    assert MEASURED_RATIO * 1.1 < 1
    assert r["logloss"] < r32["logloss"] * MEASURED_RATIO * 1.1
    FK = ffm.FK
    assert bool(ffm.table.shard[:, FK].any()) and not bool(ffm.table.shard[:, FK + 1:].any())


# ------------------------------------------------------------------------------ e. the linear limit
def test_zero_init_is_the_linear_model():
    """init_std 0: every factor gradient is a sum of other factors, so the factors never leave zero and the
    losses are, step for step, those of the FM at init_std 0 -- the same linear model on the same table rule."""
    steps = 12
    ffm, losses, _ = _train_ffm(std=0.0, steps=steps)
    data = FFMSynth(512, fields=8, card=32, seed=0)
    lin = FM(FMConfig(num_dims=data.num_dims, k=4, lr=0.05, init_std=0.0), Comm(device=CPU))
    ref = [float(lin.train_step(*data.next())) for _ in range(steps)]
    assert losses == ref  # bit for bit: both references sum the linear terms in lookup order
    assert not bool(ffm.table.shard[:, :ffm.FK].any()) and bool(ffm.table.shard[:, ffm.FK].any())
    assert torch.equal(ffm.table.shard[:, ffm.FK], lin.table.shard[:, 4])


# ------------------------------------------------------------------------------ f. ranks
TOTAL, NF, CARD, K = 64, 8, 16, 4
ND = NF * CARD


def _init_rows(m):
    """The same routed-space table at every world size (a table's own init is seeded per rank)."""
    g = torch.Generator().manual_seed(5)
    full = torch.randn(ND, NF * K + 4, generator=g) * 0.05
    full[:, NF * K:] = 0
    t = m.table
    t.shard[: t.rows_local].copy_(full[t.base: t.base + t.rows_local].to(t.shard.device))


def _ffm_world(rank, world, consistency="bsp", staleness=0, steps=6, dev=CPU):
    torch.set_num_threads(1)
    comm = Comm(device=dev)
    m = FFM(FFMConfig(num_dims=ND, num_fields=NF, k=K, lr=0.05, consistency=consistency, staleness=staleness), comm)
    _init_rows(m)
    data = FFMSynth(TOTAL, fields=NF, card=CARD, device=dev, seed=11)  # the same global batch on every rank
    per = TOTAL // world
    losses = []
    for _ in range(steps):
        rowptr, cols, vals, y = data.next()
        lo, hi = rank * per, (rank + 1) * per
        t = m.train_step(rowptr[lo: hi + 1] - rowptr[lo], cols[lo * NF: hi * NF], vals[lo * NF: hi * NF],
                         y[lo:hi]).clone()
        comm.all_reduce_(t)
        losses.append(float(t) / TOTAL)
    m.drain()
    return losses


def _ffm_bsp(rank, world):
    return _ffm_world(rank, world)


@pytest.mark.parametrize("world", [2, 4])
def test_ffm_ranks_match_one_rank(world):
    many = run_world(_ffm_bsp, world=world)
    one = _ffm_bsp(0, 1)
    print(f"world {world}: {many[0]} vs one rank {one}")
    for r in range(1, world):
        assert many[r] == many[0]  # the all-reduced loss is identical on every rank
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert one[-1] < one[0]


# ------------------------------------------------------------------------------ g. evaluation beside training
def test_evaluate_does_not_disturb_training():
    m0, plain, _ = _train_ffm(steps=12)
    m1, mixed, held = _train_ffm(steps=12, evals_at=(0, 3, 4, 11))
    assert plain == mixed
    assert torch.equal(m0.table.shard, m1.table.shard) and torch.equal(m0.bias.master, m1.bias.master)
    z = m1.predict_logits(*held[0][:3])
    assert z.shape == (512,) and bool(torch.isfinite(z).all())
    # 5-tuples carry the fields; the keys' own fields give the same result
    r4 = m1.evaluate(held[:2])
    r5 = m1.evaluate([b + (m1.fields_of(b[1]),) for b in held[:2]])
    assert r4 == r5 and r4["n"] == 1024


def test_fields_from_bounds_and_from_the_batch():
    data = FFMSynth(64, fields=8, card=32, seed=0)
    b = data.next()
    kw = dict(num_dims=data.num_dims, num_fields=8, k=4, lr=0.05)
    m_default = FFM(FFMConfig(**kw), Comm(device=CPU))
    m_bounds = FFM(FFMConfig(field_bounds=[32 * f for f in range(1, 8)], **kw), Comm(device=CPU))
    f = m_default.fields_of(b[1])
    assert f.dtype == torch.int32 and torch.equal(f.long(), b[1] // 32) and torch.equal(m_bounds.fields_of(b[1]), f)
    # uneven boundaries, and equal ranges that do not divide num_dims (the last field takes the rest)
    m_odd = FFM(FFMConfig(num_dims=10, num_fields=3, k=4, field_bounds=[1, 7]), Comm(device=CPU))
    assert m_odd.fields_of(torch.arange(10)).tolist() == [0, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    m_eq = FFM(FFMConfig(num_dims=10, num_fields=4, k=4), Comm(device=CPU))  # ceil(10 / 4) = 3 keys per field
    assert m_eq.fields_of(torch.arange(10)).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    l_keys = float(m_default.train_step(*b))
    l_given = float(m_bounds.train_step(*b, fields=f))
    assert l_keys == l_given and torch.equal(m_default.table.shard, m_bounds.table.shard)
    other = float(FFM(FFMConfig(**kw), Comm(device=CPU)).train_step(*b, fields=(f + 1) % 8))
    assert math.isfinite(other)


# ------------------------------------------------------------------------------ h. FTRL linear column
def test_ftrl_linear_column_l1_sparsifies():
    nnz, touched = [], None
    for l1 in (0.0, 0.5, 2.0):
        data = FFMSynth(256, fields=8, card=32, seed=3)
        m = FFM(FFMConfig(num_dims=data.num_dims, num_fields=8, k=4, lr=0.05, linear_optimizer="ftrl", linear_l1=l1),
                Comm(device=CPU))
        seen = torch.zeros(data.num_dims, dtype=torch.bool)
        for _ in range(20):
            b = data.next()
            seen[b[1]] = True
            loss = m.train_step(*b)
        assert math.isfinite(float(loss))
        assert m.table.ftrl_grad_scale == 256.0  # linear_grad_scale 0.0: batch size x world
        nnz.append(m.linear_nnz())
        touched = int(seen.sum())
    print(f"linear_nnz over l1 0 / 0.5 / 2: {nnz}, touched features {touched}")
    assert nnz[0] >= nnz[1] >= nnz[2]
    assert nnz[0] == touched and nnz[2] < nnz[0]


# ------------------------------------------------------------------------------ i. checkpoints
def test_checkpoint_round_trip_and_continuation(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    def make():
        return FFM(FFMConfig(num_dims=8 * 32, num_fields=8, k=4, lr=0.05, linear_optimizer="ftrl", linear_l1=0.5),
                   Comm(device=CPU))

    def tables(m):
        return {0: m.table, 1: m.bias}

    data = FFMSynth(128, fields=8, card=32, seed=4)
    batches = [data.next() for _ in range(6)]
    a = make()
    for b in batches[:3]:
        a.train_step(*b)
    a.drain()
    Checkpointer(a.comm, str(tmp_path / "ck_")).save(tables(a), iteration=3, blocking=True)
    c = make()
    assert Checkpointer(c.comm, str(tmp_path / "ck_")).load(tables(c)) == 3
    for ta, tc in zip(tables(a).values(), tables(c).values()):  # every checkpoint array: values and optimizer state
        arrays_a, arrays_c = ta.shard_state()[1], tc.shard_state()[1]
        assert set(arrays_a) == set(arrays_c) and arrays_a
        for name in arrays_a:
            assert torch.equal(arrays_a[name], arrays_c[name]), name
    assert bool(c.table.ftrl_zn.any()) and bool(c.table.state.any())
    la = [float(a.train_step(*b)) for b in batches[3:]]
    lc = [float(c.train_step(*b)) for b in batches[3:]]
    assert la == lc and torch.equal(a.table.shard, c.table.shard)


# ------------------------------------------------------------------------------ j. refusals
@pytest.mark.parametrize("kw", [dict(k=0), dict(k=6), dict(k=20), dict(k=-4), dict(num_fields=0),
                                dict(num_fields=65), dict(num_fields=64, k=12), dict(field_bounds=[5]),
                                dict(num_fields=3, field_bounds=[7, 7]), dict(num_fields=3, field_bounds=[9, 2]),
                                dict(transport="onesided"), dict(storage="map"), dict(storage="hash"),
                                dict(value_dtype=torch.bfloat16), dict(value_dtype=torch.float64),
                                dict(pull_dtype=torch.bfloat16), dict(linear_optimizer="sgd")],
                         ids=lambda kw: "-".join(f"{a}={b}" for a, b in kw.items()))
def test_config_refusals_name_ffm(kw):
    with pytest.raises(ValueError, match="ffm"):
        FFMConfig(**{**dict(num_dims=100, num_fields=8), **kw})


def test_gpu_tensors_need_the_extension(monkeypatch):
    """A GPU tensor without the extension is an error, never a fall-back to the reference."""
    import minips_amd.ops as O

    def missing():
        raise RuntimeError("minips_amd._ffmk is not built")

    monkeypatch.setattr(O, "ffmk", missing)
    monkeypatch.setattr(O, "_gpu", lambda t: True)
    rowptr, inv, vals, fields, labels, rows, w0 = _batch(3, 4)
    with pytest.raises(RuntimeError, match="_ffmk"):
        O.ffm_forward(rowptr, inv, vals, fields, labels, rows, 3, 4, w0)
    with pytest.raises(RuntimeError, match="_ffmk"):
        O.ffm_backward(inv, torch.zeros(11, dtype=torch.int32), rowptr, vals, fields, torch.zeros(5), rows, 3, 4,
                       torch.zeros(9, 16), csr=(inv.int(), inv.int()))


def test_driver_flags():
    from minips_amd.train import parse

    a = parse(["--model", "ffm", "--eval_every", "5", "--wide_optimizer", "ftrl", "--ftrl_l1", "1.0", "--ffm_k", "8",
               "--fm_fields", "6", "--fm_card", "10"])
    assert a.model == "ffm" and a.ffm_k == 8 and a.transport == "collective" and a.ffm_bounds is None
    assert parse(["--model", "ffm", "--consistency", "ssp"]).transport == "collective"
    a = parse(["--model", "ffm", "--input", "x.libsvm", "--ffm_fields", "3", "--ffm_field_bounds", "10,20"])
    assert a.ffm_bounds == [10, 20]
    for bad in (["--model", "ffm", "--ffm_k", "6"], ["--model", "ffm", "--ffm_k", "20"],
                ["--model", "ffm", "--transport", "onesided"], ["--model", "ffm", "--kStorageType", "Map"],
                ["--model", "ffm", "--value_dtype", "float64"], ["--model", "ffm", "--fm_fields", "65"],
                ["--model", "ffm", "--fm_fields", "64", "--ffm_k", "12"],
                ["--model", "ffm", "--input", "x.libsvm"],  # no --ffm_fields
                ["--model", "ffm", "--input", "x.libsvm", "--ffm_fields", "3", "--ffm_field_bounds", "10"],
                ["--model", "ffm", "--input", "x.libsvm", "--ffm_fields", "3", "--ffm_field_bounds", "20,10"],
                ["--model", "ffm", "--input", "x.libsvm", "--ffm_fields", "3", "--ffm_field_bounds", "a,b"],
                ["--model", "ffm", "--ffm_field_bounds", "1,2,3,4,5,6,7"],  # the synthetic stream has its own fields
                ["--model", "ffm", "--input", "x.libsvm", "--ffm_fields", "3", "--eval_every", "5"],
                ["--model", "fm", "--ffm_fields", "3"], ["--model", "lr", "--ffm_field_bounds", "1,2"]):
        with pytest.raises(SystemExit):
            parse(bad)


def test_driver_runs_ffm_with_ftrl_and_eval(capsys):
    import json

    from minips_amd.train import main

    assert main(["--model", "ffm", "--small", "1", "--steps", "12", "--eval_every", "10", "--wide_optimizer", "ftrl",
                 "--ftrl_l1", "0.5", "--ffm_k", "4"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "ffm" and "linear_nnz" in out and len(out["evals"]) == 2
    assert out["ffm_fields"] == 8 and out["ffm_k"] == 4
    assert main(["--model", "ffm", "--small", "1", "--steps", "2", "--fm_fields", "5", "--ffm_k", "8"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "linear_nnz" not in out and "evals" not in out and out["ffm_fields"] == 5 and out["ffm_k"] == 8


def test_driver_runs_ffm_on_a_libsvm_file(tmp_path, capsys):
    import json

    from minips_amd.train import main

    g = torch.Generator().manual_seed(1)
    lines = []
    for _ in range(96):
        keys = sorted({int(v) for v in torch.randint(1, 31, (5,), generator=g)})  # libsvm ids are 1-based: keys 0..29
        lines.append(("1" if torch.rand(1, generator=g) < 0.5 else "-1") + " " + " ".join(f"{c}:1" for c in keys))
    path = tmp_path / "d.libsvm"
    path.write_text("\n".join(lines) + "\n")
    assert main(["--model", "ffm", "--input", str(path), "--ffm_fields", "3", "--ffm_field_bounds", "10,20",
                 "--batch_size", "32", "--steps", "4", "--num_dims", "30"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "ffm" and out["ffm_fields"] == 3 and all(math.isfinite(v) for _, v in out["losses"])


