"""The factorization-machine kernels (csrc/kernels/fm.hip through ops.fm_forward / ops.fm_backward) on the GPU
against fp64 references with derived bounds, u = 2^-24 (csrc/kernels/fm.h states the rule):
  forward   |S - S64|   <= (nnz_b + 2) u sum_j |v x|                      per (sample, factor)
            |z - z64|   <= (2 nnz_b + k + 16) u A,  A = |w0| + sum |w x| + (sum_f (sum_j |v x|)^2 + Q) / 2
            |dz - dz64| <= gscale (bound_z / 4 + 4 u)                      (sigmoid' <= 1/4)
            |loss - loss64| <= bound_z + 4 u (|z| + 1)                     (|dloss/dz| <= 1; max, product, log1p, sum)
  backward  alone, on inputs produced by the fp32 CPU reference forward, so only its own summation is judged:
            |g - g64| <= (M_u + 6) u sum_m |c_m| (|S| + |v x_m|), M_u the row's member count; pad columns
            exactly 0; rows without lookups keep a sentinel.
Shapes: the smallest that reach every path -- every lane shape (k 4 / 8 / 16 / 32 / 60), one sample, three, more
than one block (257), per-sample nnz from {0, 1, 63, 64, 65, 130} (around the 64-lookup chunk of the forward),
duplicates within a sample, cap > U, a strided rows view (ld > W), a misaligned one (the one-lane-per-element
fallback), and member counts on both sides of every backward switch (32 | 33, 2048 | 2049) plus one batch whose
5003 lookups all read one row. Then the model: GPU against CPU, no host sync in a steady step, two ranks on
one card."""
import math

import pytest
import torch

from test_fm import K as WORLD_K, _fm_world
from test_multirank_gpu import run_world

from minips_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NNZ = (0, 1, 63, 64, 65, 130)


def _case(k, B, seed, cap_extra=5, num_rows=None, nnz_choices=NNZ):
    """A CSR batch on the CPU: per-sample nnz drawn from ``nnz_choices`` (every choice present when B allows),
    lookups drawn from few rows so that samples hold duplicates, cap > U."""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(nnz_choices), (B,), generator=g)
    first = {1: [5], 3: [0, 3, 5]}.get(B, list(range(len(nnz_choices))))  # one sample: 130 lookups; three: 0, 64, 130
    pick[: len(first)] = torch.tensor(first)
    nnz = torch.tensor(nnz_choices)[pick]
    rowptr = torch.zeros(B + 1, dtype=torch.int64)
    rowptr[1:] = nnz.cumsum(0)
    n = int(rowptr[-1])
    num_rows = num_rows or max(3, n // 4)
    inv = torch.randint(0, num_rows, (n,), generator=g)
    if n:
        inv[torch.randint(0, n, (1,), generator=g)] = num_rows - 1  # memrow[n-1] + 1 == num_rows
    vals = torch.randn(n, generator=g)
    labels = (torch.rand(B, generator=g) < 0.5).float() * 2 - 1  # {-1, 1}
    # (factors of std 0.6 / sqrt(k): |z| stays far below 87, where exp(-|z|) and with it dz would leave fp32's
    # normal range -- the bounds above are relative ones, they hold for results that do not underflow)
    rows = torch.randn(num_rows + cap_extra, k + 4, generator=g) * (0.6 / math.sqrt(k))
    rows[:, k] *= math.sqrt(k) / 2  # the linear weights keep std 0.3
    rows[:, k + 1:] = 0
    w0 = torch.tensor([0.25])
    return rowptr, inv, vals, labels, rows, w0


def _layout(rows, how, dev):
    """rows on the GPU as a contiguous matrix, a strided view (ld = W + 4) or a misaligned one (base + 4 bytes)."""
    cap, W = rows.shape
    if how == "contig":
        return rows.to(dev)
    if how == "strided":
        buf = torch.full((cap, W + 4), float("nan"), device=dev)
        buf[:, :W] = rows.to(dev)
        return buf[:, :W]
    flat = torch.full((cap * W + 1,), float("nan"), device=dev)
    v = flat[1:].view(cap, W)
    v.copy_(rows.to(dev))
    assert v.data_ptr() % 16 == 4
    return v


def _forward64(rowptr, inv, vals, labels, rows, w0, k, gscale):
    B = rowptr.numel() - 1
    rowid = torch.repeat_interleave(torch.arange(B), rowptr[1:] - rowptr[:-1])
    x = vals.double()
    p = rows[inv, :k].double() * x[:, None]
    S = torch.zeros(B, k, dtype=torch.float64).index_add_(0, rowid, p)
    Sabs = torch.zeros(B, k, dtype=torch.float64).index_add_(0, rowid, p.abs())
    Q = torch.zeros(B, dtype=torch.float64).index_add_(0, rowid, (p * p).sum(1))
    wx = rows[inv, k].double() * x
    lin = torch.zeros(B, dtype=torch.float64).index_add_(0, rowid, wx)
    linabs = torch.zeros(B, dtype=torch.float64).index_add_(0, rowid, wx.abs())
    z = w0.double()[0] + lin + 0.5 * ((S * S).sum(1) - Q)
    y = (labels > 0.5).double()
    dz = (torch.sigmoid(z) - y) * gscale
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    nnz = (rowptr[1:] - rowptr[:-1]).double()
    A = w0.double().abs()[0] + linabs + 0.5 * ((Sabs * Sabs).sum(1) + Q)
    bS = (nnz + 2)[:, None] * U * Sabs
    bz = (2 * nnz + k + 16) * U * A
    return dict(S=S, z=z, dz=dz, loss=loss, rowid=rowid, bS=bS, bz=bz, bdz=gscale * (bz / 4 + 4 * U),
                bloss=bz + 4 * U * (z.abs() + 1))


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - bound).max()) if err.numel() else 0.0
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"  {name}: max err {float(err.max()) if err.numel() else 0.0:.3e}, max err / bound {ratio:.3f}")
    assert worst <= 0, f"{name}: error exceeds the bound by {worst:.3e} (err / bound {ratio:.3f})"


def _csr(inv):
    order = torch.sort(inv, stable=True).indices
    return order.to(torch.int32), inv[order].to(torch.int32)


def _backward64(inv, rowid, vals, dz, S, rows, k):
    """fp64 of the backward rule on fp32 inputs, and its bound per element."""
    cap = rows.shape[0]
    b, x = rowid.long(), vals.double()
    c = dz.double()[b] * x
    vx = rows[inv, :k].double() * x[:, None]
    g = torch.zeros(cap, k + 4, dtype=torch.float64)
    g[:, :k].index_add_(0, inv, c[:, None] * (S.double()[b] - vx))
    g[:, k].index_add_(0, inv, c)
    mag = torch.zeros(cap, k + 4, dtype=torch.float64)
    mag[:, :k].index_add_(0, inv, c.abs()[:, None] * (S.double()[b].abs() + vx.abs()))
    mag[:, k].index_add_(0, inv, c.abs())
    M = torch.zeros(cap, dtype=torch.float64).index_add_(0, inv, torch.ones_like(x))
    return g, (M + 6)[:, None] * U * mag, M > 0


def _check_backward(case, k, dev, how="contig", blocks=(0, 3)):
    rowptr, inv, vals, labels, rows, w0 = case
    gscale = 1.0 / max(labels.numel(), 1)
    S, z, dz, loss, rowid = ops.fm_forward(rowptr, inv, vals, labels, rows, k, w0, gscale)  # the fp32 CPU reference
    assert float(z.abs().max()) < 60  # no underflow anywhere (see _case)
    g64, bound, touched = _backward64(inv, rowid, vals, dz, S, rows, k)
    members, memrow = _csr(inv)
    rows_d = _layout(rows, how, dev)
    args = [t.to(dev) for t in (inv, rowid, vals, dz, S)]
    outs = []
    for bl in blocks + (blocks[0],):
        grad = torch.full((rows.shape[0], k + 4), 7.0, device=dev)
        ops.fm_backward(*args, rows_d, k, grad, csr=(members.to(dev), memrow.to(dev)), blocks=bl)
        outs.append(grad)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])  # every grid size and every launch: the same bits
    g = outs[0].cpu()
    _within("grad", g[touched][:, :k + 1], g64[touched][:, :k + 1], bound[touched][:, :k + 1])
    assert bool((g[touched][:, k + 1:] == 0).all())  # the pad columns
    assert bool((g[~touched] == 7.0).all())  # rows without lookups keep the sentinel
    return outs[0], args, rows_d


CASES = [(k, B, "contig") for k in (4, 8, 16, 32, 60) for B in (1, 3, 257)] + \
        [(k, 257, how) for k in (4, 16, 60) for how in ("strided", "misaligned")]


@pytest.mark.parametrize("k,B,how", CASES)
def test_forward_and_backward_against_fp64(k, B, how, dev):
    case = _case(k, B, seed=100 * k + B)
    rowptr, inv, vals, labels, rows, w0 = case
    gscale = 1.0 / B
    ref = _forward64(rowptr, inv, vals, labels, rows, w0, k, gscale)
    assert float(ref["z"].abs().max()) < 60  # no underflow anywhere (see _case)
    rows_d = _layout(rows, how, dev)
    a = [t.to(dev) for t in (rowptr, inv, vals, labels)]
    outs = [ops.fm_forward(*a, rows_d, k, w0.to(dev), gscale, blocks=bl) for bl in (0, 1, 7, 0)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(x, y)  # every grid size and every launch: the same bits
    S, z, dz, loss, rowid = outs[0]
    print(f"k {k} B {B} {how}: n {inv.numel()}")
    assert rowid.dtype == torch.int32 and torch.equal(rowid.cpu().long(), ref["rowid"])
    _within("S", S, ref["S"], ref["bS"])
    _within("z", z, ref["z"], ref["bz"])
    _within("dz", dz, ref["dz"], ref["bdz"])
    _within("loss", loss, ref["loss"], ref["bloss"])
    empty = (rowptr[1:] == rowptr[:-1])
    assert bool((z.cpu()[empty] == 0.25).all())  # an empty sample: z = w0
    _check_backward(case, k, dev, how)


def test_forward_without_bias_and_csr_built_on_the_device(dev):
    k = 8
    case = _case(k, 9, seed=5)
    rowptr, inv, vals, labels, rows, _ = case
    ref = _forward64(rowptr, inv, vals, labels, rows, torch.zeros(1), k, 0.5)
    a = [t.to(dev) for t in (rowptr, inv, vals, labels, rows)]
    S, z, dz, loss, rowid = ops.fm_forward(*a, k, None, 0.5)
    _within("z", z, ref["z"], ref["bz"])
    # the plan's CSR kernel instead of the host sort: any member order within a row is inside the bound
    S_c, z_c, dz_c, _, rowid_c = ops.fm_forward(rowptr, inv, vals, labels, rows, k, None, 0.5)
    g64, bound, touched = _backward64(inv, rowid_c, vals, dz_c, S_c, rows, k)
    grad = torch.full((rows.shape[0], k + 4), 7.0, device=dev)
    ops.fm_backward(a[1], rowid_c.to(dev), a[2], dz_c.to(dev), S_c.to(dev), a[4], k, grad)
    g = grad.cpu()
    _within("grad", g[touched][:, :k + 1], g64[touched][:, :k + 1], bound[touched][:, :k + 1])
    assert bool((g[~touched] == 7.0).all())


def _members_case(k, counts, B, seed):
    """Row u has counts[u] member lookups, scattered over B samples."""
    g = torch.Generator().manual_seed(seed)
    inv = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    n = inv.numel()
    inv = inv[torch.randperm(n, generator=g)]
    cuts = torch.sort(torch.randint(0, n + 1, (B - 1,), generator=g)).values
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([n])])
    vals = torch.randn(n, generator=g)
    labels = (torch.rand(B, generator=g) < 0.5).float()
    rows = torch.randn(len(counts) + 3, k + 4, generator=g) * 0.05
    rows[:, k + 1:] = 0
    return rowptr, inv, vals, labels, rows, torch.tensor([0.1])


@pytest.mark.parametrize("k,how", [(4, "contig"), (16, "contig"), (60, "contig"), (16, "misaligned")])
def test_backward_member_count_switches(k, how, dev):
    """Both sides of the lane-group | wave switch (32 | 33) and of the wave | workgroup switch (2048 | 2049);
    two heavy rows side by side (one chunk holds the end of one and the start of the next), a heavy row that
    starts on a chunk boundary (row 0) and light rows between them."""
    counts = [3072, 1, 32, 33, 2, 2048, 2049, 2500, 31, 64, 5, 2047, 4097, 1]
    _check_backward(_members_case(k, counts, 257, seed=k), k, dev, how, blocks=(0, 2))


@pytest.mark.parametrize("how", ["contig", "misaligned"])
@pytest.mark.parametrize("counts", [[2049], [1, 2049]])
def test_backward_heavy_row_at_the_edges_of_memrow(counts, how, dev):
    """The smallest heavy row as the only row (every chunk is its own, the first has no member before it) and as
    the last row after a light one (it ends at n: the last chunk has no member after it)."""
    _check_backward(_members_case(4, counts, 40, seed=len(counts)), 4, dev, how, blocks=(0, 2))


@pytest.mark.parametrize("k", [8, 32])
def test_backward_every_lookup_on_one_row(k, dev):
    _check_backward(_members_case(k, [5003], 40, seed=3), k, dev)
    _check_backward(_members_case(k, [2048], 40, seed=4), k, dev)  # n <= the wave limit: no workgroup launch


def test_empty_inputs_launch_nothing(dev):
    k = 8
    rows = torch.zeros(4, k + 4, device=dev)
    e64, ef = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, device=dev)
    S, z, dz, loss, rowid = ops.fm_forward(torch.zeros(1, dtype=torch.int64, device=dev), e64, ef, ef, rows, k)
    assert S.shape == (0, k) and rowid.numel() == 0
    # B == 2, n == 0: both samples are empty
    S, z, dz, loss, rowid = ops.fm_forward(torch.zeros(3, dtype=torch.int64, device=dev), e64, ef,
                                           torch.tensor([1.0, 0.0], device=dev), rows, k,
                                           torch.tensor([0.5], device=dev))
    assert z.tolist() == [0.5, 0.5] and bool((S == 0).all())
    grad = torch.full((4, k + 4), 7.0, device=dev)
    e32 = torch.zeros(0, dtype=torch.int32, device=dev)
    ops.fm_backward(e64, e32, ef, dz, S, rows, k, grad, csr=(e32, e32))
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())


# ------------------------------------------------------------------------------ the model
def _models(dev, **cfg):
    from minips_amd.models.fm import FM, FMConfig
    from minips_amd.ps.comm import Comm

    c = FMConfig(num_dims=8 * 32, k=8, lr=0.05, **cfg)
    cpu, gpu = FM(c, Comm(device=torch.device("cpu"))), FM(c, Comm(device=dev))
    gpu.table.shard.copy_(cpu.table.shard.to(dev))
    return cpu, gpu


@pytest.mark.parametrize("linear", ["adagrad", "ftrl"])
def test_model_gpu_matches_cpu(linear, dev):
    from minips_amd.data.synthetic import FMSynth

    cpu, gpu = _models(dev, linear_optimizer=linear, linear_l1=0.5 if linear == "ftrl" else 0.0)
    data = FMSynth(256, fields=8, card=32, seed=3)
    for step in range(5):
        b = data.next()
        lc = float(cpu.train_step(*b)) / 256
        lg = float(gpu.train_step(*(t.to(dev) for t in b))) / 256
        print(f"step {step}: cpu {lc:.6f} gpu {lg:.6f}")
        assert abs(lg - lc) <= 3e-3 * max(1.0, abs(lc))
    held = [data.holdout(7).next() for _ in range(2)]
    rc, rg = cpu.evaluate(held), gpu.evaluate([tuple(t.to(dev) for t in b) for b in held])
    assert rc["n"] == rg["n"] == 512 and abs(rc["logloss"] - rg["logloss"]) <= 3e-3
    if linear == "ftrl":
        assert 0 < gpu.linear_nnz() <= 8 * 32


def test_steady_step_has_no_host_sync(dev):
    from minips_amd.data.synthetic import FMSynth
    from minips_amd.utils.syncaudit import SyncAudit

    _, gpu = _models(dev)
    data = FMSynth(256, fields=8, card=32, device=dev, seed=3)
    batches = [data.next() for _ in range(6)]
    for b in batches[:3]:  # warm-up: first plans, scratch allocations
        gpu.train_step(*b)
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for b in batches[3:]:
            audit.step_begin()
            gpu.train_step(*b)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep


def test_evaluate_writes_no_training_state(dev):
    """evaluate() between two steps changes no table value, optimizer state, gradient buffer or clock. (The
    CPU test compares whole runs bit for bit; on the GPU two runs of a step agree to rounding only, whatever
    lies between them: the planner's lookup CSR orders a row's members through atomic cursors, and the
    backward -- bitwise reproducible for a given CSR, above -- sums in that order.)"""
    from minips_amd.data.synthetic import FMSynth

    _, gpu = _models(dev)
    data = FMSynth(256, fields=8, card=32, device=dev, seed=3)
    for _ in range(3):
        gpu.train_step(*data.next())
    gpu.drain()
    torch.cuda.synchronize()

    def state():
        t, b = gpu.table, gpu.bias
        return [x.clone() for x in (t.shard, t.state, t.state2, b.master, b.m, b.params, b.grad, b.step_dev)], \
            (b.step, len(t._pending), b._pending)

    before = state()
    held = data.holdout(9)
    r = gpu.evaluate([held.next() for _ in range(2)])
    gpu.drain()
    torch.cuda.synchronize()
    after = state()
    assert r["n"] == 512 and before[1] == after[1]
    for x, y in zip(before[0], after[0]):
        assert torch.equal(x, y)
    assert math.isfinite(float(gpu.train_step(*data.next())))


def _fm_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _fm_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_match_one_rank(dev):
    many = run_world(_fm_two_ranks_gpu, world=2)
    one = _fm_world(0, 1, dev=dev)  # (the device's sample stream: a CPU run would draw other batches)
    print(f"2 ranks on one card {many[0]} vs one rank {one} (k {WORLD_K})")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert all(math.isfinite(v) for v in many[0])
