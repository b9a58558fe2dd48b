"""FTRL-Proximal on sparse tables, CPU side: ops.sparse_ftrl's fp32 reference against an independent fp64
oracle, its exact properties (closed form, exact zeros, w == f(z, n), untouched rows, prefix and row check),
SparseTable(optimizer="ftrl") at one and several gloo ranks, checkpoints (round trip, continuation,
2 -> 3 ranks), the refusals, SparseLR's FTRL mode and the driver flags."""
import functools
import json

import pytest
import torch

from _ftrl_util import ATOL, HYPERS, RTOL, check_zero_pattern, distinct_keys, eighths, oracle_rows
from test_ps_gloo import run_world

from minips_amd import ops

F32 = torch.float32


def _state(rows, W, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, W, generator=g)
    zn = torch.cat([torch.randn(rows, W, generator=g), torch.rand(rows, W, generator=g) * 4], 1)
    return w, zn, g


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("hp", HYPERS)
@pytest.mark.parametrize("W", [1, 4, 33])
def test_reference_matches_fp64_oracle(W, hp):
    rows, n, base = 600, 257, 1000
    w, zn, gen = _state(rows, W, 3 + W)
    zn[::7, W:] = 0  # fresh coordinates (n == 0) among used ones
    keys = distinct_keys(n, rows, base, gen)
    grads = torch.randn(n, W, generator=gen)
    w64, zn64 = w.double(), zn.double()
    oracle_rows(w64, zn64, keys, base, grads.double(), **hp)
    ops.sparse_ftrl(w, zn, keys, base, grads, **hp)
    err = max(float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max()) for a, b in ((w, w64), (zn, zn64)))
    print(f"W {W} {hp}: worst error / bound {err:.3g}")
    torch.testing.assert_close(w.double(), w64, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(zn.double(), zn64, rtol=RTOL, atol=ATOL)


def test_closed_form_from_zero_state():
    gen = torch.Generator().manual_seed(1)
    rows, W, alpha = 300, 4, 0.1
    w, zn = torch.zeros(rows, W), torch.zeros(rows, 2 * W)
    keys = distinct_keys(rows, rows, 0, gen)
    grads = torch.randn(rows, W, generator=gen)
    grads[grads == 0] = 1.0
    ops.sparse_ftrl(w, zn, keys, 0, grads, alpha, beta=0.0, l1=0.0, l2=0.0)
    g = torch.empty_like(grads)
    g[keys] = grads
    assert torch.equal(zn[:, W:], g * g)
    expect = -torch.tensor(alpha, dtype=F32) * torch.sign(g)
    ulp = torch.tensor(alpha, dtype=F32) * 2.0 ** -23
    assert float((w - expect).abs().max()) <= float(ulp)


def test_large_l1_gives_exact_zeros():
    w, zn, gen = _state(200, 4, 5)
    keys = distinct_keys(150, 200, 0, gen)
    for _ in range(3):
        ops.sparse_ftrl(w, zn, keys, 0, torch.randn(150, 4, generator=gen), 0.1, l1=1e4)
    assert float(zn[keys, :4].abs().max()) < 1e4
    assert torch.equal(w[keys], torch.zeros(150, 4)) and not bool((torch.signbit(w[keys])).any())


def test_zero_pattern_at_moderate_l1():
    rows, W, l1 = 4000, 4, 0.5
    w, zn, gen = _state(rows, W, 9)
    keys = distinct_keys(rows, rows, 0, gen)
    grads = torch.randn(rows, W, generator=gen)
    w64, zn64 = w.double(), zn.double()
    oracle_rows(w64, zn64, keys, 0, grads.double(), alpha=0.1, beta=1.0, l1=l1, l2=0.0)
    ops.sparse_ftrl(w, zn, keys, 0, grads, 0.1, l1=l1)
    check_zero_pattern(w, zn64[:, :W], l1, "cpu reference")
    assert 0.1 < float((w == 0).float().mean()) < 0.9  # the threshold really cuts through these inputs


@pytest.mark.parametrize("hp", HYPERS)
def test_weights_are_the_closed_form_of_the_state_and_untouched_rows_stay(hp):
    rows, W = 500, 4
    w, zn, gen = _state(rows, W, 11)
    w0, zn0 = w.clone(), zn.clone()
    touched = torch.zeros(rows, dtype=torch.bool)
    for _ in range(4):
        keys = distinct_keys(100, rows - 50, 20, gen)  # rows [0, 20) and the last 30 are never named
        touched[keys - 20] = True
        ops.sparse_ftrl(w, zn, keys, 20, torch.randn(100, W, generator=gen), **hp)
    f = ops.ftrl_weights(zn[:, :W], zn[:, W:], hp["alpha"], hp["beta"], hp["l1"], hp["l2"])
    assert torch.equal(w[touched], f[touched])
    assert touched.sum() < rows and torch.equal(w[~touched], w0[~touched]) and torch.equal(zn[~touched], zn0[~touched])


def test_prefix_and_row_check():
    rows, W = 64, 4
    w, zn, gen = _state(rows, W, 13)
    keys = distinct_keys(40, rows, 100, gen)
    grads = torch.randn(40, W, generator=gen)
    a, b = (w.clone(), zn.clone()), (w.clone(), zn.clone())
    ops.sparse_ftrl(*a, keys, 100, grads, 0.1, l1=0.2, n_dev=torch.tensor([25]))
    ops.sparse_ftrl(*b, keys[:25], 100, grads[:25], 0.1, l1=0.2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][keys[25:] - 100], w[keys[25:] - 100])
    # keys below and above the owned range are skipped and counted
    bad = keys.clone()
    bad[3], bad[17] = 100 - 2, 100 + rows + 1
    oor = torch.zeros(1, dtype=torch.int64)
    c = (w.clone(), zn.clone())
    ops.sparse_ftrl(*c, bad, 100, grads, 0.1, l1=0.2, oor=oor)
    keep = torch.ones(40, dtype=torch.bool)
    keep[[3, 17]] = False
    d = (w.clone(), zn.clone())
    ops.sparse_ftrl(*d, keys[keep], 100, grads[keep], 0.1, l1=0.2)
    assert int(oor) == 2 and torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


def test_bad_hyperparameters_raise():
    w, zn, _ = _state(8, 1, 1)
    k, g = torch.arange(4), torch.ones(4, 1)
    for kw in (dict(alpha=0.0), dict(alpha=0.1, beta=-1.0), dict(alpha=0.1, l1=-1.0), dict(alpha=0.1, l2=-1.0)):
        with pytest.raises(RuntimeError):
            ops.sparse_ftrl(w, zn, k, 0, g, **kw)


# ------------------------------------------------------------------------------ the table
ROWS, K = 1000, 5
HP = dict(lr=0.1, ftrl_beta=1.0, l1=0.5, l2=0.01)


def _batch(clock, rank, n=96, W=4):
    g = torch.Generator().manual_seed(1000 * clock + rank)
    return torch.randint(0, ROWS, (n,), generator=g), eighths((n, W), g)


def _table(comm, W=4, **kw):
    from minips_amd.ps.tables import SparseTable

    return SparseTable(comm, ROWS, W, optimizer="ftrl", init_std=0.0, pull_dtype=F32, push_dtype=F32, **HP, **kw)


def _cpu_comm():
    from minips_amd.ps.comm import Comm

    return Comm(device=torch.device("cpu"))


def _one_rank(world, clocks=K, W=4, first=0, table=None):
    """One rank fed the concatenated batches of ``world`` ranks."""
    t = table or _table(_cpu_comm(), W)
    for c in range(first, first + clocks):
        ks, vs = zip(*[_batch(c, r, W=W) for r in range(world)])
        t.add_keys(torch.cat(ks), torch.cat(vs))
        t.clock()
    t.drain()
    return t


@pytest.mark.parametrize("W", [1, 4])
def test_table_one_rank_equals_a_hand_replay(W):
    t = _one_rank(1, W=W, table=_table(_cpu_comm(), W, route="range"))
    w, zn = torch.zeros(ROWS, W), torch.zeros(ROWS, 2 * W)
    for c in range(K):
        keys, vals = _batch(c, 0, W=W)
        uniq, inv = torch.unique(keys, return_inverse=True)
        g = torch.zeros(uniq.numel(), W).index_add_(0, inv, vals)
        ops.sparse_ftrl(w, zn, uniq, 0, g, 0.1, 1.0, 0.5, 0.01)
    assert t.state is None and t.state2 is None
    assert torch.equal(t.shard, w) and torch.equal(t.ftrl_zn, zn)
    assert t.nnz() == int(torch.count_nonzero(w)) and 0 < t.nnz() < w.numel()


def _ranks_fn(rank, world, consistency="bsp", staleness=0):
    t = _table(_cpu_comm(), consistency=consistency, staleness=staleness)
    for c in range(K):
        t.add_keys(*_batch(c, rank))
        t.clock()
    t.drain()
    return t.base, t.shard[: t.rows_local].clone(), t.ftrl_zn[: t.rows_local].clone(), t.nnz()


def _assert_ranks_equal_one(out, world):
    one = _one_rank(world)
    parts = [out[r] for r in range(world)]
    assert [p[0] for p in parts] == sorted(p[0] for p in parts) and parts[0][0] == 0
    assert torch.equal(torch.cat([p[1] for p in parts]), one.shard)
    assert torch.equal(torch.cat([p[2] for p in parts]), one.ftrl_zn)
    assert {p[3] for p in parts} == {one.nnz()}


@pytest.mark.parametrize("world", [2, 4])
def test_several_bsp_ranks_equal_one_rank(world):
    _assert_ranks_equal_one(run_world(_ranks_fn, world), world)


def test_ssp_ranks_equal_one_rank_after_drain():
    _assert_ranks_equal_one(run_world(functools.partial(_ranks_fn, consistency="ssp", staleness=1), 2), 2)


# ------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_and_continuation(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    comm = _cpu_comm()
    a = _one_rank(1, clocks=3)
    Checkpointer(comm, str(tmp_path / "ck_")).save({0: a}, iteration=3, blocking=True)
    b = _table(comm)
    assert Checkpointer(comm, str(tmp_path / "ck_")).load({0: b}) == 3
    assert torch.equal(a.shard, b.shard) and torch.equal(a.ftrl_zn, b.ftrl_zn) and bool(b.ftrl_zn.any())
    _one_rank(1, clocks=2, first=3, table=a)
    _one_rank(1, clocks=2, first=3, table=b)
    whole = _one_rank(1, clocks=5)
    for t in (a, b):
        assert torch.equal(t.shard, whole.shard) and torch.equal(t.ftrl_zn, whole.ftrl_zn)


def _save_fn(rank, world, prefix):
    from minips_amd.ps.checkpoint import Checkpointer

    t = _table(_cpu_comm())
    for c in range(3):
        t.add_keys(*_batch(c, rank))
        t.clock()
    Checkpointer(t.comm, prefix).save({0: t}, iteration=3, blocking=True)
    return True


def _load_fn(rank, world, prefix):
    from minips_amd.ps.checkpoint import Checkpointer

    t = _table(_cpu_comm())
    it = Checkpointer(t.comm, prefix).load({0: t})
    return it, t.shard[: t.rows_local].clone(), t.ftrl_zn[: t.rows_local].clone()


def test_checkpoint_reshards_two_to_three_ranks(tmp_path):
    prefix = str(tmp_path / "ck_")
    run_world(functools.partial(_save_fn, prefix=prefix), 2)
    out = run_world(functools.partial(_load_fn, prefix=prefix), 3)
    one = _one_rank(2, clocks=3)
    assert [out[r][0] for r in range(3)] == [3, 3, 3]
    assert torch.equal(torch.cat([out[r][1] for r in range(3)]), one.shard)
    assert torch.equal(torch.cat([out[r][2] for r in range(3)]), one.ftrl_zn) and bool(one.ftrl_zn.any())


# ------------------------------------------------------------------------------ refusals
def test_table_refusals():
    from minips_amd.models.lr import SparseLRConfig
    from minips_amd.ps.tables import HashSparseTable, SparseTable

    comm = _cpu_comm()
    with pytest.raises(ValueError, match="ftrl"):
        SparseTable(comm, 100, 16, optimizer="ftrl", value_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="ftrl"):
        SparseTable(comm, 100, 16, optimizer="ftrl", value_dtype=torch.float64)
    with pytest.raises(ValueError, match="ftrl"):
        SparseTable(comm, 100, 16, optimizer="ftrl", split=8)
    with pytest.raises(ValueError, match="ftrl"):
        HashSparseTable(comm, 1, optimizer="ftrl")
    with pytest.raises(ValueError, match="ftrl"):
        SparseLRConfig(storage="map", optimizer="ftrl")
    with pytest.raises(ValueError, match="ftrl"):
        SparseLRConfig(value_dtype=torch.float64, optimizer="ftrl")


# ------------------------------------------------------------------------------ SparseLR
def _lr_run(steps=40, **cfg):
    from minips_amd.data.synthetic import SparseLRSynth
    from minips_amd.models.lr import SparseLR, SparseLRConfig

    m = SparseLR(SparseLRConfig(num_dims=4000, alpha=0.05, **cfg), _cpu_comm())
    data = SparseLRSynth(256, num_dims=4000, nnz=16, seed=7)
    accs = [float(m.train_step(*data.next())) / 256 for _ in range(steps)]
    m.drain()
    return m, accs


def test_sparse_lr_ftrl_learns_and_l1_sparsifies():
    """l1 = 0.25 is one step's typical summed gradient of a feature here (a feature occurs about once per
    256 x 16 batch over 4000 dims, x ~ U(0, 1), |p - y| ~ 0.5): an informative feature crosses it in a step
    or two, an uninformative one (a seventh of the teacher's weights are 0) random-walks around it. Measured
    on the CPU, last-10-step accuracy after 40 steps: add 0.7887, ftrl l1=0 0.7918, l1=0.25 0.7910 (nnz 3775
    of 4000); a four times larger l1 = 1.0 delays the weights enough to trail add (0.7660, nnz 3095)."""
    _, add = _lr_run()
    m0, dense = _lr_run(optimizer="ftrl", l1=0.0)
    m1, sparse = _lr_run(optimizer="ftrl", l1=0.25)
    tail = lambda a: sum(a[-10:]) / 10  # noqa: E731
    print(f"accuracy add {tail(add):.4f} ftrl {tail(dense):.4f} ftrl+l1 {tail(sparse):.4f}; "
          f"nnz l1=0 {m0.nnz()} l1=1 {m1.nnz()}")
    assert tail(sparse) >= tail(add)
    assert m1.nnz() < m0.nnz()
    assert m1.table.state is None and m1.table.ftrl_zn.shape == (4000, 2)


def test_sparse_lr_add_mode_is_unchanged_by_the_new_fields():
    from minips_amd.data.synthetic import SparseLRSynth
    from minips_amd.ps.tables import SparseTable

    m, accs = _lr_run(steps=8)
    assert m.cfg.optimizer == "add" and m.table.optimizer == "add" and m.table.ftrl_zn is None
    # the step as it was before the option existed: plain add of alpha * x * (y - p)
    t = SparseTable(_cpu_comm(), 4000, 1, optimizer="add", pull_dtype=F32, init_std=0.0)
    data, ref = SparseLRSynth(256, num_dims=4000, nnz=16, seed=7), []
    for _ in range(8):
        rowptr, cols, vals, y = data.next()
        rows, plan = t.get(cols)
        delta, correct = torch.zeros(max(plan.cap, 1)), torch.zeros(1)
        ops.lr_sparse_step(rowptr, plan.inv, vals, y, rows.view(-1)[: plan.cap], 0.05, delta[: plan.cap], correct)
        t.add(plan, delta.view(-1, 1))
        t.clock()
        ref.append(float(correct) / 256)
    assert accs == ref and torch.equal(m.table.shard, t.shard)


# ------------------------------------------------------------------------------ the driver
def _drive(capsys, monkeypatch, *argv):
    from minips_amd import train

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert train.main(list(argv)) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize("argv", [("--model", "widedeep"), ("--model", "lr", "--kStorageType", "map"),
                                  ("--model", "lr", "--value_dtype", "float64"),
                                  ("--model", "lr", "--ftrl_alpha", "0"), ("--model", "lr", "--ftrl_alpha", "-1"),
                                  ("--model", "lr", "--ftrl_beta", "-1"), ("--model", "lr", "--ftrl_l1", "-0.5"),
                                  ("--model", "lr", "--ftrl_l2", "-0.5")])
def test_train_refuses_bad_ftrl_flags(argv, capsys):
    from minips_amd import train

    with pytest.raises(SystemExit) as e:
        train.parse(["--sparse_optimizer", "ftrl", *argv])
    assert e.value.code == 2
    assert "ftrl" in capsys.readouterr().err


# the keys of the final JSON line of `--small 1 --model lr --steps 5`, recorded from a run of the commit
# before the option existed
PARENT_KEYS = json.loads('["checksum", "generation", "losses", "model", "start", "steady_ms_per_iter", "steps", '
                         '"total_ms", "world"]')


def test_train_ftrl_reports_nnz_and_the_default_adds_no_key(capsys, monkeypatch):
    base = ("--small", "1", "--model", "lr", "--steps", "5")
    plain = _drive(capsys, monkeypatch, *base)
    assert sorted(plain) == PARENT_KEYS
    out = _drive(capsys, monkeypatch, *base, "--sparse_optimizer", "ftrl", "--ftrl_l1", "0.5")
    assert sorted(out) == sorted(PARENT_KEYS + ["nnz", "sparse_optimizer"])
    assert out["sparse_optimizer"] == "ftrl" and 0 <= out["nnz"] < 5000
    dense = _drive(capsys, monkeypatch, *base, "--sparse_optimizer", "ftrl")
    assert out["nnz"] < dense["nnz"] <= 5000
