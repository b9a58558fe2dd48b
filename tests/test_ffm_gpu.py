"""The field-aware factorization-machine kernels (csrc/kernels/ffm.hip through ops.ffm_forward /
ops.ffm_backward) on the GPU against vectorised fp64 references with derived bounds, u = 2^-24
(csrc/kernels/ffm.h states the rule; the references and bounds are tests/test_ffm.py's, which also shows that the
fp32 CPU reference meets them):
  forward   |z - z64| <= (P_b + nnz_b + k + 16) u A_b, P_b the pair count, A_b = |w0| + sum |w x| + sum_{i<j}
            sum_c |v v'| |x_i x_j|; dz and loss with the bounds of tests/test_fm_gpu.py built on that
  backward  alone, on dz from the fp32 CPU forward: |g - g64| <= (N + 6) u sum |terms|, N the (member, partner)
            terms of the element; the linear column (M_u + 2) u sum |c_m|; pad columns exactly 0; rows without
            lookups keep a sentinel.
Shapes: every lane shape -- (F, k) = (1, 4), (2, 4), (5, 8), (39, 4), (64, 8), (26, 16): 2, 4, 16, 64 lanes and 2
or 3 column chunks per lane -- one sample, three, more than one block (257), per-sample nnz from {0, 1, 2, 63, 64,
65, 130}, lookups drawn from few rows and few fields (duplicates, shared fields), cap > U, a strided rows view
(ld = W + 4), a misaligned one (the one-float-per-lane form), member counts on both sides of every backward
switch (8 | 9, 64 | 65), one batch whose 5003 lookups of short samples all read one row, and an out-of-range
inv, field, member and sample index. Bits identical at blocks = 1, 7, the default, and across two runs. Then the
model: GPU against CPU, no host sync in a steady step, evaluate() writes nothing, two ranks on one card."""
import math

import pytest
import torch

from test_ffm import K as WORLD_K, _backward64, _ffm_world, _forward64, _within
from test_multirank_gpu import run_world

from minips_amd import ops

pytestmark = pytest.mark.gpu

NNZ = (0, 1, 2, 63, 64, 65, 130)
SHAPES = [(1, 4), (2, 4), (5, 8), (39, 4), (64, 8), (26, 16)]


def _case(F, k, B, seed, cap_extra=5, num_rows=None, nnz_choices=NNZ):
    """A CSR batch on the CPU: per-sample nnz drawn from ``nnz_choices`` (every choice present when B allows),
    lookups drawn from few rows so that samples hold duplicates, fields drawn at random so that lookups of a
    sample share fields, cap > U."""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(nnz_choices), (B,), generator=g)
    first = {1: [6], 3: [0, 4, 6]}.get(B, list(range(len(nnz_choices))))  # one sample: 130 lookups; three: 0, 64, 130
    pick[: len(first)] = torch.tensor(first)
    nnz = torch.tensor(nnz_choices)[pick]
    rowptr = torch.zeros(B + 1, dtype=torch.int64)
    rowptr[1:] = nnz.cumsum(0)
    n = int(rowptr[-1])
    num_rows = num_rows or max(3, n // 4)
    inv = torch.randint(0, num_rows, (n,), generator=g)
    inv[torch.randint(0, n, (1,), generator=g)] = num_rows - 1  # memrow[n-1] + 1 == num_rows
    fields = torch.randint(0, F, (n,), generator=g).to(torch.int32)
    vals = torch.randn(n, generator=g)
    labels = (torch.rand(B, generator=g) < 0.5).float() * 2 - 1  # {-1, 1}
    # (factors of std 0.25 / k^(1/4): the 8385 pairs of a 130-lookup sample sum to a z of std about 6, far
    # below 87, where exp(-|z|) and with it dz would leave fp32's normal range -- the bounds are relative ones)
    rows = torch.randn(num_rows + cap_extra, F * k + 4, generator=g) * (0.25 / k ** 0.25)
    rows[:, F * k] = torch.randn(num_rows + cap_extra, generator=g) * 0.1
    rows[:, F * k + 1:] = 0
    return rowptr, inv, vals, fields, labels, rows, torch.tensor([0.25])


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


def _csr(inv):
    order = torch.sort(inv, stable=True).indices
    return order.to(torch.int32), inv[order].to(torch.int32)


def _check_backward(case, F, k, dev, how="contig", blocks=(0, 1, 7), csr=None, member_ok=None, rowid=None):
    """The backward alone, on dz of the fp32 CPU reference forward; returns the GPU gradient."""
    rowptr, inv, vals, fields, labels, rows, w0 = case
    gscale = 1.0 / max(labels.numel(), 1)
    z, dz, loss, rid = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, gscale)
    assert float(z.abs().max()) < 60  # no underflow anywhere (see _case)
    rowid = rid if rowid is None else rowid
    g64, bound, touched = _backward64(rowptr, inv, vals, fields, dz, rows, F, k, member_ok=member_ok)
    members, memrow = csr if csr is not None else _csr(inv)
    rows_d = _layout(rows, how, dev)
    a = [t.to(dev) for t in (inv, rowid, rowptr, vals, fields, dz)]
    outs = []
    for bl in blocks + (blocks[0],):
        grad = torch.full((rows.shape[0], F * k + 4), 7.0, device=dev)
        ops.ffm_backward(*a, rows_d, F, k, grad, csr=(members.to(dev), memrow.to(dev)), blocks=bl)
        outs.append(grad)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])  # every grid size and every launch: the same bits
    g, FK = outs[0].cpu(), F * k
    _within("grad", g[touched][:, :FK + 1], g64[touched][:, :FK + 1], bound[touched][:, :FK + 1])
    assert bool((g[touched][:, FK + 1:] == 0).all())  # the pad columns
    assert bool((g[~touched] == 7.0).all())  # rows without lookups keep the sentinel
    return g


CASES = [(F, k, B, "contig") for F, k in SHAPES for B in (1, 3, 257)] + \
        [(F, k, 257, how) for F, k in ((2, 4), (39, 4), (64, 8)) for how in ("strided", "misaligned")]


@pytest.mark.parametrize("F,k,B,how", CASES)
def test_forward_and_backward_against_fp64(F, k, B, how, dev):
    case = _case(F, k, B, seed=1000 * F + 10 * k + B)
    rowptr, inv, vals, fields, labels, rows, w0 = case
    gscale = 1.0 / B
    ref = _forward64(rowptr, inv, vals, fields, labels, rows, w0, F, k, gscale)
    assert float(ref["z"].abs().max()) < 60  # no underflow anywhere (see _case)
    rows_d = _layout(rows, how, dev)
    a = [t.to(dev) for t in (rowptr, inv, vals, fields, labels)]
    outs = [ops.ffm_forward(*a, rows_d, F, k, w0.to(dev), gscale, blocks=bl) for bl in (0, 1, 7, 0)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(x, y)  # every grid size and every launch: the same bits
    z, dz, loss, rowid = outs[0]
    print(f"F {F} k {k} B {B} {how}: n {inv.numel()}")
    want = torch.repeat_interleave(torch.arange(B), rowptr[1:] - rowptr[:-1])
    assert rowid.dtype == torch.int32 and torch.equal(rowid.cpu().long(), want)
    _within("z", z, ref["z"], ref["bz"])
    _within("dz", dz, ref["dz"], ref["bdz"])
    _within("loss", loss, ref["loss"], ref["bloss"])
    empty = (rowptr[1:] == rowptr[:-1])
    assert bool((z.cpu()[empty] == 0.25).all())  # an empty sample: z = w0
    _check_backward(case, F, k, dev, how)


def test_forward_without_bias_and_csr_built_on_the_device(dev):
    F, k = 5, 8
    case = _case(F, k, 9, seed=5)
    rowptr, inv, vals, fields, labels, rows, _ = case
    ref = _forward64(rowptr, inv, vals, fields, labels, rows, torch.zeros(1), F, k, 0.5)
    a = [t.to(dev) for t in (rowptr, inv, vals, fields, labels, rows)]
    z, dz, loss, rowid = ops.ffm_forward(*a, F, k, None, 0.5)
    _within("z", z, ref["z"], ref["bz"])
    # the plan's CSR kernel instead of the host sort: any member order within a row is inside the bound
    z_c, dz_c, _, rowid_c = ops.ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, None, 0.5)
    g64, bound, touched = _backward64(rowptr, inv, vals, fields, dz_c, rows, F, k)
    grad = torch.full((rows.shape[0], F * k + 4), 7.0, device=dev)
    ops.ffm_backward(a[1], rowid_c.to(dev), a[0], a[2], a[3], dz_c.to(dev), a[5], F, k, grad)
    g, FK = grad.cpu(), F * k
    _within("grad", g[touched][:, :FK + 1], g64[touched][:, :FK + 1], bound[touched][:, :FK + 1])
    assert bool((g[~touched] == 7.0).all())


def _members_case(F, k, counts, B, seed):
    """Row u has counts[u] member lookups, scattered over B short samples."""
    g = torch.Generator().manual_seed(seed)
    inv = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    n = inv.numel()
    inv = inv[torch.randperm(n, generator=g)]
    cuts = torch.sort(torch.randint(0, n + 1, (B - 1,), generator=g)).values
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([n])])
    fields = torch.randint(0, F, (n,), generator=g).to(torch.int32)
    vals = torch.randn(n, generator=g)
    labels = (torch.rand(B, generator=g) < 0.5).float()
    rows = torch.randn(len(counts) + 3, F * k + 4, generator=g) * 0.05
    rows[:, F * k + 1:] = 0
    return rowptr, inv, vals, fields, labels, rows, torch.tensor([0.1])


@pytest.mark.parametrize("F,k,how", [(1, 4, "contig"), (5, 8, "contig"), (39, 4, "contig"), (64, 8, "contig"),
                                     (5, 8, "misaligned")])
def test_backward_member_count_switches(F, k, how, dev):
    """Both sides of the lane-group | wave switch (8 | 9) and of the wave | workgroup switch (64 | 65); two
    heavy rows side by side (one chunk holds the end of one and the start of the next), a heavy row that starts
    on a chunk boundary (row 0) and light rows between them."""
    counts = [768, 1, 8, 9, 2, 64, 65, 700, 7, 33, 5, 63, 1025, 66, 1]
    _check_backward(_members_case(F, k, counts, 600, seed=F + k), F, k, dev, how, blocks=(0, 2))


@pytest.mark.parametrize("counts", [[65], [1, 65]])
def test_backward_heavy_row_at_the_edges_of_memrow(counts, dev):
    """The smallest heavy row as the only row (every chunk is its own, the first has no member before it) and as
    the last row after a light one (it ends at n: the last chunk has no member after it)."""
    _check_backward(_members_case(2, 4, counts, 20, seed=len(counts)), 2, 4, dev, blocks=(0, 2))


@pytest.mark.parametrize("F,k", [(2, 4), (26, 16)])
def test_backward_every_lookup_on_one_row(F, k, dev):
    _check_backward(_members_case(F, k, [5003], 1200, seed=3), F, k, dev)
    _check_backward(_members_case(F, k, [64], 20, seed=4), F, k, dev)  # n <= the wave limit: no workgroup launch


def test_out_of_range_indices_are_skipped(dev):
    """An inv beyond cap and a negative one, a field beyond F and a negative one: those lookups contribute
    nothing and receive nothing, in both kernels. A member index beyond n and a sample index beyond B: that
    member receives nothing (it stays a partner)."""
    F, k = 5, 8
    case = _case(F, k, 12, seed=9, nnz_choices=(0, 3, 7, 20))
    rowptr, inv, vals, fields, labels, rows, w0 = case
    n, cap = inv.numel(), rows.shape[0]
    inv[2], inv[11], fields[5], fields[17] = cap + 3, -1, F, -2
    ref = _forward64(rowptr, inv, vals, fields, labels, rows, w0, F, k, 1.0 / 12)
    a = [t.to(dev) for t in (rowptr, inv, vals, fields, labels, rows)]
    z, dz, loss, rowid = ops.ffm_forward(*a, F, k, w0.to(dev), 1.0 / 12)
    _within("z", z, ref["z"], ref["bz"])
    _check_backward(case, F, k, dev)
    # a bad member index and a bad sample index, each on a lookup of a row that has other members
    members, memrow = _csr(inv)
    ok = torch.ones(n, dtype=torch.bool)
    bad_m, bad_b = 30, 40
    jm, jb = int(members[bad_m]), int(members[bad_b])
    assert 0 <= int(memrow[bad_m]) < cap and 0 <= int(memrow[bad_b]) < cap and jm != jb
    members[bad_m] = n + 5
    ok[jm] = ok[jb] = False
    rid = torch.repeat_interleave(torch.arange(12), rowptr[1:] - rowptr[:-1]).to(torch.int32)
    rid[jb] = 12
    _check_backward(case, F, k, dev, csr=(members, memrow), member_ok=ok, rowid=rid)


def test_empty_inputs_launch_nothing(dev):
    F, k = 2, 4
    rows = torch.zeros(4, F * k + 4, device=dev)
    e64, ef = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, device=dev)
    e32 = torch.zeros(0, dtype=torch.int32, device=dev)
    z, dz, loss, rowid = ops.ffm_forward(torch.zeros(1, dtype=torch.int64, device=dev), e64, ef, e32, ef, rows, F, k)
    assert z.numel() == 0 and rowid.numel() == 0
    # B == 2, n == 0: both samples are empty
    rp = torch.zeros(3, dtype=torch.int64, device=dev)
    z, dz, loss, rowid = ops.ffm_forward(rp, e64, ef, e32, torch.tensor([1.0, 0.0], device=dev), rows, F, k,
                                         torch.tensor([0.5], device=dev))
    assert z.tolist() == [0.5, 0.5]
    grad = torch.full((4, F * k + 4), 7.0, device=dev)
    ops.ffm_backward(e64, e32, rp, ef, e32, dz, rows, F, k, grad, csr=(e32, e32))
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())


# ------------------------------------------------------------------------------ the model
def _models(dev, **cfg):
    from minips_amd.models.ffm import FFM, FFMConfig
    from minips_amd.ps.comm import Comm

    c = FFMConfig(num_dims=8 * 32, num_fields=8, k=4, lr=0.05, **cfg)
    cpu, gpu = FFM(c, Comm(device=torch.device("cpu"))), FFM(c, Comm(device=dev))
    gpu.table.shard.copy_(cpu.table.shard.to(dev))
    return cpu, gpu


@pytest.mark.parametrize("linear", ["adagrad", "ftrl"])
def test_model_gpu_matches_cpu(linear, dev):
    from minips_amd.data.synthetic import FFMSynth

    cpu, gpu = _models(dev, linear_optimizer=linear, linear_l1=0.5 if linear == "ftrl" else 0.0)
    data = FFMSynth(256, fields=8, card=32, seed=3)
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
    from minips_amd.data.synthetic import FFMSynth
    from minips_amd.utils.syncaudit import SyncAudit

    _, gpu = _models(dev)
    data = FFMSynth(256, fields=8, card=32, device=dev, seed=3)
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
    """evaluate() between two steps changes no table value, optimizer state, gradient buffer or clock (the CPU
    test compares whole runs bit for bit; on the GPU two runs of a step agree to rounding only: the planner's
    lookup CSR orders a row's members through atomic cursors)."""
    from minips_amd.data.synthetic import FFMSynth

    _, gpu = _models(dev)
    data = FFMSynth(256, fields=8, card=32, device=dev, seed=3)
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


def _ffm_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _ffm_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_match_one_rank(dev):
    many = run_world(_ffm_two_ranks_gpu, world=2)
    one = _ffm_world(0, 1, dev=dev)  # (the device's sample stream: a CPU run would draw other batches)
    print(f"2 ranks on one card {many[0]} vs one rank {one} (k {WORLD_K})")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert all(math.isfinite(v) for v in many[0])
