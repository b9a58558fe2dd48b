"""FTRL-Proximal on the GPU: the gfx950 kernel (csrc/kernels/ftrl.hip) against ops.sparse_ftrl's CPU
reference at the rows-per-wave boundaries of each lane mapping, the stride loop, the scalar path, the
device-count prefix, the row check, SparseTable(optimizer="ftrl") and SparseLR against their CPU twins,
and the host-sync audit of the steady-state LR step."""
import pytest
import torch

from _ftrl_util import ATOL, HYPERS, RTOL, check_zero_pattern, decided, distinct_keys, eighths, oracle_rows

from minips_amd import ops

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
ROWS, BASE = 400, 1000
COUNTS = {1: (1, 63, 64, 65, 257), 4: (1, 63, 64, 65, 257)}  # rows-per-wave boundaries; wider rows: below
WIDE_COUNTS = (3, 4, 5, 67)


def _inputs(W, n, seed, applies=3):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(ROWS, W, generator=g)
    zn = torch.cat([torch.randn(ROWS, W, generator=g), torch.rand(ROWS, W, generator=g) * 4], 1)
    zn[::5, W:] = 0
    steps = [(distinct_keys(n, ROWS, BASE, g), torch.randn(n, W, generator=g)) for _ in range(applies)]
    return w, zn, steps


def _run(w, zn, steps, hp, dev=None, **kw):
    w, zn = w.clone().to(dev or "cpu"), zn.clone().to(dev or "cpu")
    for keys, grads in steps:
        ops.sparse_ftrl(w, zn, keys.to(w.device), BASE, grads.to(w.device), **hp, **kw)
    return w.cpu(), zn.cpu()


def _bit_diff(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())


@pytest.mark.parametrize("hp", HYPERS, ids=lambda h: f"l1_{h['l1']}-l2_{h['l2']}")
@pytest.mark.parametrize("W", [1, 4, 20, 33, 64, 128])
def test_kernel_matches_cpu_reference(W, hp, dev):
    """Three successive applies from random (w, z, n >= 0) at base != 0. The kernel keeps g * g a separate
    multiply and uses the IEEE division and the correctly rounded square root; the CPU reference takes its
    square roots through fp64 for the same rounding. On the card no element of any case here differs from
    the reference (profiles/ftrl/kernels.txt), so beside the tolerance the comparison is torch.equal."""
    for n in COUNTS.get(W, WIDE_COUNTS):
        w, zn, steps = _inputs(W, n, 100 * W + n)
        cw, czn = _run(w, zn, steps, hp)
        gw, gzn = _run(w, zn, steps, hp, dev)
        diff = _bit_diff(gw, cw) + _bit_diff(gzn, czn)
        print(f"W {W} n {n} {hp}: {diff} of {gw.numel() + gzn.numel()} elements differ bitwise from the CPU reference")
        torch.testing.assert_close(gw, cw, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(gzn, czn, rtol=RTOL, atol=ATOL)
        w64, zn64 = w.double(), zn.double()
        touched = torch.zeros(ROWS, dtype=torch.bool)
        for keys, grads in steps:
            oracle_rows(w64, zn64, keys, BASE, grads.double(), **hp)
            touched[keys - BASE] = True
        check_zero_pattern(gw[touched], zn64[touched][:, :W], hp["l1"], f"W {W} n {n}")
        # the invariant on the GPU's own state: a touched row's w is the closed form of its stored (z, n)
        f = ops.ftrl_weights(gzn[:, :W], gzn[:, W:], hp["alpha"], hp["beta"], hp["l1"], hp["l2"])
        assert torch.equal(gw[touched], f[touched])
        assert torch.equal(gw[~touched], w[~touched]) and torch.equal(gzn[~touched], zn[~touched])
        assert torch.equal(gw, cw) and torch.equal(gzn, czn)


@pytest.mark.parametrize("W,n", [(1, 257), (4, 257), (64, 67), (33, 67)])
def test_stride_loop_and_determinism(W, n, dev):
    hp = HYPERS[3]
    w, zn, steps = _inputs(W, n, 7 * W + n)
    ref = _run(w, zn, steps, hp, dev)
    again = _run(w, zn, steps, hp, dev)
    assert torch.equal(ref[0], again[0]) and torch.equal(ref[1], again[1])
    for blocks in (1, 2):
        got = _run(w, zn, steps, hp, dev, blocks=blocks)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), blocks


@pytest.mark.parametrize("W", [1, 4, 64])
def test_unaligned_views_take_the_scalar_path(W, dev):
    """grads 4 bytes past a 16-byte boundary, a table of odd leading dimension and a state 4 bytes past
    alignment: no vector access is possible, and the result is the aligned one."""
    hp, n = HYPERS[3], 67
    w, zn, steps = _inputs(W, n, 31 + W, applies=2)
    ref = _run(w, zn, steps, hp)
    wide = torch.zeros(ROWS, W + 1 + W % 2, device=dev)  # W + 1 (W even) or W + 2 (W == 1): odd, > W
    assert wide.stride(0) % 2 == 1
    tv = wide[:, :W]
    tv.copy_(w)
    zbuf = torch.zeros(ROWS * 2 * W + 1, device=dev)
    zv = zbuf[1:].view(ROWS, 2 * W)
    zv.copy_(zn)
    for keys, grads in steps:
        gbuf = torch.zeros(n * W + 1, device=dev)
        gv = gbuf[1:].view(n, W)
        gv.copy_(grads)
        assert gv.data_ptr() % 16 == 4 and zv.data_ptr() % 8 == 4
        ops.sparse_ftrl(tv, zv, keys.to(dev), BASE, gv, **hp)
    assert torch.equal(tv.cpu(), ref[0]) and torch.equal(zv.cpu(), ref[1])
    assert not bool(wide[:, W:].any()) and float(zbuf[0]) == 0.0


@pytest.mark.parametrize("W", [1, 4, 33])
def test_device_count_bounds_the_prefix(W, dev):
    hp, n, m = HYPERS[1], 130, 71
    w, zn, steps = _inputs(W, n, 17 + W, applies=1)
    keys, grads = steps[0]
    n_dev = torch.tensor([m], dtype=I64, device=dev)
    gw, gzn = _run(w, zn, steps, hp, dev, n_dev=n_dev)
    cw, czn = _run(w, zn, [(keys[:m], grads[:m])], hp)
    assert torch.equal(gw, cw) and torch.equal(gzn, czn)
    rest = keys[m:] - BASE  # valid rows past the count: bit for bit as they were
    assert torch.equal(gw[rest], w[rest]) and torch.equal(gzn[rest], zn[rest])


@pytest.mark.parametrize("W", [1, 4, 33])
def test_rows_outside_the_shard_are_skipped_and_counted(W, dev):
    """The table and the state are views [lo:hi] of larger allocations, so the two stray keys (two rows
    below and two rows above the view) point at memory this test owns."""
    hp, lo, hi, n = HYPERS[3], 8, 72, 40
    g = torch.Generator().manual_seed(5 + W)
    big_w, big_zn = torch.randn(80, W, generator=g), torch.rand(80, 2 * W, generator=g)
    keys = distinct_keys(n, hi - lo, BASE, g)
    grads = torch.randn(n, W, generator=g)
    bad = keys.clone()
    bad[5], bad[29] = BASE - 2, BASE + (hi - lo) + 1
    keep = torch.ones(n, dtype=torch.bool)
    keep[[5, 29]] = False
    cw, czn = big_w.clone(), big_zn.clone()
    ops.sparse_ftrl(cw[lo:hi], czn[lo:hi], keys[keep], BASE, grads[keep], **hp)
    gw, gzn = big_w.to(dev), big_zn.to(dev)
    oor = torch.zeros(1, dtype=I64, device=dev)
    ops.sparse_ftrl(gw[lo:hi], gzn[lo:hi], bad.to(dev), BASE, grads.to(dev), **hp, oor=oor)
    assert int(oor) == 2
    assert torch.equal(gw.cpu(), cw) and torch.equal(gzn.cpu(), czn)
    for a, b in ((gw.cpu(), big_w), (gzn.cpu(), big_zn)):
        assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:])


# ------------------------------------------------------------------------------ table and model
T_RTOL, T_ATOL = 1e-4, 1e-5  # the multi-step owner-apply tolerance of tests/test_kernels_gpu.py
T_ROWS = 5000


def _tables(W, dev):
    from minips_amd.ps.comm import Comm
    from minips_amd.ps.tables import SparseTable

    mk = lambda d: SparseTable(Comm(device=d), T_ROWS, W, optimizer="ftrl", lr=0.1, ftrl_beta=1.0, l1=0.5,  # noqa: E731
                               l2=0.01, init_std=0.0, pull_dtype=F32, push_dtype=F32)
    return mk(torch.device("cpu")), mk(dev)


def _clocks(tables, W, first, count):
    for c in range(first, first + count):
        g = torch.Generator().manual_seed(50 + c)
        keys, vals = torch.randint(0, T_ROWS, (512,), generator=g), eighths((512, W), g)
        for t in tables:
            t.add_keys(keys.to(t.comm.device), vals.to(t.comm.device))
            t.clock()
    for t in tables:
        t.drain()


@pytest.mark.parametrize("W", [1, 16])
def test_table_matches_its_cpu_twin_and_checkpoints(W, dev, tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    cpu, gpu = _tables(W, dev)
    _clocks((cpu, gpu), W, 0, 5)
    print(f"W {W}: {_bit_diff(gpu.shard.cpu(), cpu.shard) + _bit_diff(gpu.ftrl_zn.cpu(), cpu.ftrl_zn)} elements "
          f"differ bitwise from the CPU table after 5 clocks")
    torch.testing.assert_close(gpu.shard.cpu(), cpu.shard, rtol=T_RTOL, atol=T_ATOL)
    torch.testing.assert_close(gpu.ftrl_zn.cpu(), cpu.ftrl_zn, rtol=T_RTOL, atol=T_ATOL)
    near = int((~decided(cpu.ftrl_zn[:, :W].double(), 0.5)).sum())
    assert abs(gpu.nnz() - cpu.nnz()) <= near and 0 < gpu.nnz() < T_ROWS * W
    # checkpoint round trip on the GPU table, then both continue alike
    Checkpointer(gpu.comm, str(tmp_path / "ck_")).save({0: gpu}, iteration=5, blocking=True)
    fresh = _tables(W, dev)[1]
    assert Checkpointer(fresh.comm, str(tmp_path / "ck_")).load({0: fresh}) == 5
    assert torch.equal(fresh.shard, gpu.shard) and torch.equal(fresh.ftrl_zn, gpu.ftrl_zn)
    _clocks((gpu, fresh), W, 5, 2)
    assert torch.equal(fresh.shard, gpu.shard) and torch.equal(fresh.ftrl_zn, gpu.ftrl_zn)


def _lr_models(dev, l1=0.25):
    from minips_amd.models.lr import SparseLR, SparseLRConfig
    from minips_amd.ps.comm import Comm

    cfg = SparseLRConfig(num_dims=4000, optimizer="ftrl", ftrl_alpha=0.1, l1=l1)
    return SparseLR(cfg, Comm(device=torch.device("cpu"))), SparseLR(cfg, Comm(device=dev))


def test_sparse_lr_ftrl_tracks_the_cpu_run(dev):
    from minips_amd.data.synthetic import SparseLRSynth

    cpu, gpu = _lr_models(dev)
    data = SparseLRSynth(256, num_dims=4000, nnz=16, seed=7)
    for _ in range(10):
        batch = data.next()
        cpu.train_step(*batch)
        gpu.train_step(*(t.to(dev) for t in batch))
    torch.testing.assert_close(gpu.table.shard.cpu(), cpu.table.shard, rtol=T_RTOL, atol=T_ATOL)
    torch.testing.assert_close(gpu.table.ftrl_zn.cpu(), cpu.table.ftrl_zn, rtol=T_RTOL, atol=T_ATOL)
    near = int((~decided(cpu.table.ftrl_zn[:, :1].double(), 0.25)).sum())
    print(f"nnz cpu {cpu.nnz()} gpu {gpu.nnz()}, {near} coordinates near the threshold")
    assert abs(gpu.nnz() - cpu.nnz()) <= near and 0 < gpu.nnz() < 4000


def test_ftrl_lr_step_has_no_host_sync(dev):
    from minips_amd.data.synthetic import SparseLRSynth
    from minips_amd.utils.syncaudit import SyncAudit

    gpu = _lr_models(dev)[1]
    data = SparseLRSynth(256, num_dims=4000, nnz=16, device=dev, seed=3)
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
    assert 0 < gpu.nnz() <= 4000
