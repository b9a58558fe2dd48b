"""Wide & Deep's recipe on split rows, CPU side: ops.sparse_adagrad_ftrl (row-wise Adagrad on the deep
columns, FTRL-Proximal on the wide ones) against a hand composition of the two existing references, its exact
properties (pad columns, untouched rows, prefix, row check), SparseTable(wide_optimizer="ftrl") at one and
several gloo ranks, checkpoints (round trip, continuation, 2 -> 3 ranks), the refusals, the W&D model's
sparsity / loss trade and the driver flags."""
import functools
import json

import pytest
import torch

from _ftrl_util import distinct_keys, eighths
from test_ps_gloo import run_world

from minips_amd import ops

F32, BF16 = torch.float32, torch.bfloat16
LR, EPS = 0.02, 1e-8


def _state(rows, W, D1, seed):
    g = torch.Generator().manual_seed(seed)
    Wf = W - D1
    w = torch.randn(rows, W, generator=g)
    st = torch.rand(rows, generator=g)
    zn = torch.cat([torch.randn(rows, Wf, generator=g), torch.rand(rows, Wf, generator=g) * 4], 1)
    zn[::5, Wf:] = 0  # fresh coordinates (n == 0) among used ones
    return w, st, zn, g


def _compose(w, st, zn, D1, keys, base, grads, scale, alpha, beta, l1, l2):
    """The rule by hand: the two existing ops, each on a copy of its columns."""
    W = grads.shape[1]
    ops.sparse_rowwise_adagrad(w, st, keys, base, grads[:, :D1].contiguous(), LR, EPS)  # columns [0, D1) only
    wide = w[:, D1:W].clone()
    ops.sparse_ftrl(wide, zn, keys, base, grads[:, D1:] * torch.tensor(scale, dtype=F32), alpha, beta, l1, l2)
    w[:, D1:W] = wide


# ------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("scale", [1.0, 512.0])
@pytest.mark.parametrize("W,D1", [(36, 32), (20, 16), (7, 5)])
def test_op_equals_the_composition_of_the_two_references(W, D1, scale):
    rows, n, base = 300, 130, 1000
    w, st, zn, gen = _state(rows, W, D1, 3 + W)
    a, b = (w.clone(), st.clone(), zn.clone()), (w.clone(), st.clone(), zn.clone())
    hp = dict(alpha=0.1, beta=1.0, l1=0.5, l2=0.01)
    for _ in range(3):
        keys = distinct_keys(n, rows, base, gen)
        grads = torch.randn(n, W, generator=gen) / scale
        ops.sparse_adagrad_ftrl(*a, D1, keys, base, grads, LR, EPS, grad_scale=scale, **hp)
        _compose(*b, D1, keys, base, grads, scale, **hp)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], w) and not torch.equal(a[1], st) and not torch.equal(a[2], zn)


@pytest.mark.parametrize("l1", [0.0, 0.5])
def test_pad_columns_stay_exactly_zero_and_untouched_rows_stay(l1):
    rows, W, D1 = 200, 36, 32
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(rows, W, generator=gen)
    w[:, D1:] = 0
    st, zn = torch.zeros(rows), torch.zeros(rows, 2 * (W - D1))
    w0 = w.clone()
    touched = torch.zeros(rows, dtype=torch.bool)
    for _ in range(3):
        keys = distinct_keys(60, rows - 50, 20, gen)  # rows [0, 20) and the last 30 are never named
        touched[keys - 20] = True
        grads = torch.randn(60, W, generator=gen)
        grads[:, D1 + 1:] = 0  # the 3 pad columns of a W&D row
        ops.sparse_adagrad_ftrl(w, st, zn, D1, keys, 20, grads, LR, EPS, 0.1, l1=l1, grad_scale=4.0)
    for t in (w[:, D1 + 1:], zn[:, 1:4], zn[:, 5:]):
        assert not bool(t.any()) and not bool(torch.signbit(t).any())
    assert bool(zn[touched][:, 0].any()) and bool((zn[touched][:, 4] > 0).all()) and bool((st[touched] > 0).all())
    assert touched.sum() < rows and torch.equal(w[~touched], w0[~touched])
    assert not bool(st[~touched].any()) and not bool(zn[~touched].any())


def test_prefix_and_row_check():
    rows, W, D1 = 64, 20, 16
    w, st, zn, gen = _state(rows, W, D1, 13)
    keys = distinct_keys(40, rows, 100, gen)
    grads = torch.randn(40, W, generator=gen)
    run = lambda s, k, g, **kw: ops.sparse_adagrad_ftrl(*s, D1, k, 100, g, LR, EPS, 0.1, l1=0.2, **kw)  # noqa: E731
    new = lambda: (w.clone(), st.clone(), zn.clone())  # noqa: E731
    a, b = new(), new()
    run(a, keys, grads, n_dev=torch.tensor([25]))
    run(b, keys[:25], grads[:25])
    rest = keys[25:] - 100
    for x, y, orig in zip(a, b, (w, st, zn)):
        assert torch.equal(x, y) and torch.equal(x[rest], orig[rest])
    # keys below and above the owned range are skipped whole and counted
    bad = keys.clone()
    bad[3], bad[17] = 100 - 2, 100 + rows + 1
    keep = torch.ones(40, dtype=torch.bool)
    keep[[3, 17]] = False
    oor = torch.zeros(1, dtype=torch.int64)
    c, d = new(), new()
    run(c, bad, grads, oor=oor)
    run(d, keys[keep], grads[keep])
    assert int(oor) == 2
    for x, y in zip(c, d):
        assert torch.equal(x, y)


def test_bad_arguments_raise():
    w, st, zn, _ = _state(8, 6, 4, 1)
    k, g = torch.arange(4), torch.ones(4, 6)
    ok = dict(alpha=0.1, beta=1.0, l1=0.0, l2=0.0, grad_scale=1.0)
    for kw in (dict(alpha=0.0), dict(beta=-1.0), dict(l1=-1.0), dict(l2=-1.0), dict(grad_scale=0.0),
               dict(grad_scale=float("inf")), dict(grad_scale=float("nan"))):
        with pytest.raises(RuntimeError):
            ops.sparse_adagrad_ftrl(w, st, zn, 4, k, 0, g, LR, EPS, **{**ok, **kw})
    for split in (0, 6):
        with pytest.raises(RuntimeError):
            ops.sparse_adagrad_ftrl(w, st, zn, split, k, 0, g, LR, EPS, **ok)


# ------------------------------------------------------------------------------ the table
ROWS, K, W, D1 = 1000, 5, 36, 32
HP = dict(lr=LR, wide_lr=0.1, ftrl_beta=1.0, l1=0.5, l2=0.01, ftrl_grad_scale=2.0)


def _batch(clock, rank, n=96):
    g = torch.Generator().manual_seed(1000 * clock + rank)
    vals = eighths((n, W), g)
    vals[:, D1 + 1:] = 0  # pad columns carry no gradient
    return torch.randint(0, ROWS, (n,), generator=g), vals


def _cpu_comm():
    from minips_amd.ps.comm import Comm

    return Comm(device=torch.device("cpu"))


def _table(comm, push_dtype=F32, **kw):
    from minips_amd.ps.tables import SparseTable

    return SparseTable(comm, ROWS, W, optimizer="rowwise_adagrad", split=D1, wide_optimizer="ftrl", init_std=0.0,
                       pull_dtype=F32, push_dtype=push_dtype, **HP, **kw)


def _one_rank(world, clocks=K, first=0, table=None):
    """One rank fed the concatenated batches of ``world`` ranks."""
    t = table or _table(_cpu_comm())
    for c in range(first, first + clocks):
        ks, vs = zip(*[_batch(c, r) for r in range(world)])
        t.add_keys(torch.cat(ks), torch.cat(vs))
        t.clock()
    t.drain()
    return t


def _parts(t):
    return t.shard, t.state, t.ftrl_zn


def _owned(t):
    """A rank's owned rows as numpy arrays: they cross the result queue by value (a tensor travels as a
    file descriptor its rank must stay alive to serve)."""
    return tuple(x[: t.rows_local].numpy().copy() for x in _parts(t))


def _cat(out, i, world):
    return torch.cat([torch.from_numpy(out[r][i]) for r in range(world)])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_parts(a), _parts(b)))


def test_default_table_is_unchanged():
    from minips_amd.ps.tables import SparseTable

    t = SparseTable(_cpu_comm(), ROWS, W, optimizer="rowwise_adagrad", split=D1)
    assert t.wide_optimizer is None and t.ftrl_zn is None and t.state2 is not None and t.state2.shape == (ROWS,)
    assert sorted(t.shard_state()[1]) == ["params", "state", "state2"]


def test_table_one_rank_equals_a_hand_replay():
    t = _one_rank(1, table=_table(_cpu_comm(), route="range"))
    w, st, zn = torch.zeros(ROWS, W), torch.zeros(ROWS), torch.zeros(ROWS, 2 * (W - D1))
    for c in range(K):
        keys, vals = _batch(c, 0)
        uniq, inv = torch.unique(keys, return_inverse=True)
        g = torch.zeros(uniq.numel(), W).index_add_(0, inv, vals)
        ops.sparse_adagrad_ftrl(w, st, zn, D1, uniq, 0, g, LR, EPS, 0.1, 1.0, 0.5, 0.01, grad_scale=2.0)
    assert t.state2 is None and t.ftrl_zn.shape == (ROWS, 8)
    assert torch.equal(t.shard, w) and torch.equal(t.state, st) and torch.equal(t.ftrl_zn, zn)
    assert sorted(t.shard_state()[1]) == ["ftrl_zn", "params", "state"]
    touched = int((st > 0).sum())
    assert t.wide_nnz() == int(torch.count_nonzero(w[:, D1:])) and 0 < t.wide_nnz() < touched
    assert not bool(w[:, D1 + 1:].any())


def _ranks_fn(rank, world, consistency="bsp", staleness=0):
    # rows cross the ranks in bf16, the GPU default: eighths up to a few times 4 are exact in it
    t = _table(_cpu_comm(), push_dtype=BF16, consistency=consistency, staleness=staleness)
    assert not t._owner_fused_ok()
    for c in range(K):
        t.add_keys(*_batch(c, rank))
        t.clock()
    t.drain()
    return (t.base, *_owned(t), t.wide_nnz())


def _assert_ranks_equal_one(out, world):
    one = _one_rank(world)
    parts = [out[r] for r in range(world)]
    assert [p[0] for p in parts] == sorted(p[0] for p in parts) and parts[0][0] == 0
    for i, ref in enumerate(_parts(one), start=1):
        assert torch.equal(_cat(out, i, world), ref), i
    assert {p[4] for p in parts} == {one.wide_nnz()} and one.wide_nnz() > 0


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
    assert _same(a, b) and bool(b.ftrl_zn.any()) and bool(b.state.any())
    _one_rank(1, clocks=2, first=3, table=a)
    _one_rank(1, clocks=2, first=3, table=b)
    whole = _one_rank(1, clocks=5)
    assert _same(a, whole) and _same(b, whole)


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
    return (it, *_owned(t))


def test_checkpoint_reshards_two_to_three_ranks(tmp_path):
    prefix = str(tmp_path / "ck_")
    run_world(functools.partial(_save_fn, prefix=prefix), 2)
    out = run_world(functools.partial(_load_fn, prefix=prefix), 3)
    one = _one_rank(2, clocks=3)
    assert [out[r][0] for r in range(3)] == [3, 3, 3]
    for i, ref in enumerate(_parts(one), start=1):
        assert torch.equal(_cat(out, i, 3), ref), i
    assert bool(one.ftrl_zn.any())


# ------------------------------------------------------------------------------ refusals
def test_table_refusals():
    from minips_amd.engine import create_table
    from minips_amd.ps.onesided import AsyncSparseTable
    from minips_amd.ps.tables import HashSparseTable, SparseTable

    comm = _cpu_comm()
    ok = dict(optimizer="rowwise_adagrad", split=32, wide_optimizer="ftrl")
    bad = [{**ok, "split": None}, {**ok, "split": 36}, {**ok, "optimizer": "sgd"}, {**ok, "optimizer": "add"},
           {**ok, "value_dtype": BF16, "split": 16}, {**ok, "wide_optimizer": "adam"}, {**ok, "wide_lr": 0.0},
           {**ok, "wide_lr": float("nan")}, {**ok, "ftrl_beta": -1.0}, {**ok, "l1": -0.5}, {**ok, "l2": -0.5},
           {**ok, "ftrl_grad_scale": 0.0}, {**ok, "ftrl_grad_scale": float("inf")}]
    for kw in bad:
        width = 32 if kw.get("value_dtype") == BF16 else 36
        with pytest.raises(ValueError, match="wide_optimizer"):
            SparseTable(comm, 100, width, **kw)
    with pytest.raises(ValueError, match="wide_optimizer"):
        SparseTable(comm, 100, 36, optimizer="add", value_dtype=torch.float64, wide_optimizer="ftrl", split=32)
    with pytest.raises(ValueError, match="wide_optimizer"):
        HashSparseTable(comm, 36, optimizer="rowwise_adagrad", wide_optimizer="ftrl")
    with pytest.raises(ValueError, match="wide_optimizer"):
        AsyncSparseTable(comm, 100, 36, split=32, wide_optimizer="ftrl")
    with pytest.raises(ValueError, match="wide_optimizer"):
        create_table(comm, "sparse", num_rows=100, width=36, model="ssp", staleness=1, transport="onesided",
                     optimizer="rowwise_adagrad", split=32, wide_optimizer="ftrl")
    with pytest.raises(ValueError, match="ftrl"):  # as it was: one rule for every column has no split
        SparseTable(comm, 100, 36, optimizer="ftrl", split=32)


def test_config_refusals():
    from minips_amd.models.widedeep import WideDeepConfig

    assert WideDeepConfig().wide_optimizer == "adagrad"
    for kw in (dict(consistency="ssp", staleness=1), dict(consistency="asp"), dict(transport="onesided")):
        with pytest.raises(ValueError, match="wide_optimizer"):
            WideDeepConfig(wide_optimizer="ftrl", **kw)
    with pytest.raises(ValueError, match="wide_optimizer"):
        WideDeepConfig(wide_optimizer="sgd")
    assert WideDeepConfig(wide_optimizer="ftrl", consistency="ssp", staleness=1,
                          transport="collective").transport == "collective"


# ------------------------------------------------------------------------------ the model
SMOKE_CARDS = [1000, 50, 20000, 7, 300, 20, 5, 60, 90, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24,
               25, 26]  # __graft_entry__.smoke()'s


def _wd_run(steps=60, B=512, **cfg):
    from minips_amd.data.synthetic import CriteoSynth
    from minips_amd.models.widedeep import WideDeep, WideDeepConfig

    torch.manual_seed(0)
    m = WideDeep(WideDeepConfig(cards=SMOKE_CARDS, **cfg), _cpu_comm())
    data = CriteoSynth(B, cards=SMOKE_CARDS, device="cpu", seed=0)
    losses = [float(m.train_step(*data.next())) / B for _ in range(steps)]
    m.drain()
    return m, sum(losses[-10:]) / 10


@pytest.fixture(scope="module")
def wd_runs():
    ftrl = dict(wide_optimizer="ftrl", wide_alpha=0.1, wide_beta=1.0, wide_grad_scale=512.0)
    return {"default": _wd_run(), **{l1: _wd_run(wide_l1=l1, **ftrl) for l1 in (0.0, 0.5, 1.0, 2.0)}}


def test_widedeep_l1_sparsifies_the_wide_column_at_the_default_loss(wd_runs):
    """smoke()'s cards, B = 512, 60 steps, alpha 0.1, beta 1, gradient scale B. Measured on the CPU with this
    code: last-10-step mean loss 0.4500 at l1 = 0.5 against the default's 0.4465 (1.008 x), non-zero wide
    weights among the 9243 touched rows 9243 / 4054 / 1761 / 934 at l1 = 0 / 0.5 / 1 / 2. The 2 % bound is
    test_widedeep_gpu_matches_cpu's loss tolerance."""
    default, base_loss = wd_runs["default"]
    assert default.emb.state2 is not None and default.emb.ftrl_zn is None
    nnz = {}
    for l1 in (0.0, 0.5, 1.0, 2.0):
        m, loss = wd_runs[l1]
        D = m.cfg.emb_dim
        nnz[l1] = m.wide_nnz()
        touched = int((m.emb.state > 0).sum())
        print(f"l1 {l1}: last-10 loss {loss:.4f} (default {base_loss:.4f}, ratio {loss / base_loss:.4f}), "
              f"wide_nnz {nnz[l1]} of {touched} touched rows")
        assert m.emb.state2 is None and m.emb.ftrl_zn.shape == (m.emb.shard.shape[0], 8)
        assert nnz[l1] == int(torch.count_nonzero(m.emb.shard[:, D])) and nnz[l1] > 0
        assert not bool(m.emb.shard[:, D + 1:].any()) and not bool(m.emb.ftrl_zn[:, [1, 2, 3, 5, 6, 7]].any())
    assert nnz[0.0] == int((wd_runs[0.0][0].emb.state > 0).sum())
    assert nnz[0.0] > nnz[0.5] > nnz[1.0] > nnz[2.0]
    assert wd_runs[0.5][1] <= 1.02 * base_loss


def test_widedeep_evaluate_reads_the_ftrl_column(wd_runs):
    from minips_amd.data.synthetic import CriteoSynth

    m = wd_runs[0.5][0]
    data = CriteoSynth(512, cards=SMOKE_CARDS, device="cpu", seed=77)
    shard = m.emb.shard.clone()
    res = m.evaluate([data.next() for _ in range(2)])
    assert 0.5 < res["auc"] <= 1.0 and torch.equal(m.emb.shard, shard)


# ------------------------------------------------------------------------------ the driver
def _drive(capsys, monkeypatch, *argv):
    from minips_amd import train

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert train.main(list(argv)) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize("argv,flag", [
    (("--model", "lr"), "wide_optimizer"), (("--model", "dlrm"), "wide_optimizer"),
    (("--model", "mlp"), "wide_optimizer"), (("--ftrl_alpha", "0"), "ftrl_alpha"),
    (("--ftrl_beta", "-1"), "ftrl_beta"), (("--ftrl_l1", "-0.5"), "ftrl_l1"), (("--ftrl_l2", "-0.5"), "ftrl_l2"),
    (("--ftrl_grad_scale", "-1"), "ftrl_grad_scale"), (("--ftrl_grad_scale", "inf"), "ftrl_grad_scale"),
    (("--consistency", "ssp", "--staleness", "1"), "transport"), (("--consistency", "asp"), "transport"),
    (("--consistency", "ssp", "--staleness", "1", "--transport", "onesided"), "transport")])
def test_train_refuses_bad_wide_flags(argv, flag, capsys):
    from minips_amd import train

    with pytest.raises(SystemExit) as e:
        train.parse(["--wide_optimizer", "ftrl", *argv])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--wide_optimizer" in err and flag in err


def test_train_accepts_the_good_combinations():
    from minips_amd import train

    a = train.parse(["--wide_optimizer", "ftrl", "--consistency", "ssp", "--staleness", "1", "--transport",
                     "collective"])
    assert a.transport == "collective" and a.ftrl_grad_scale == 0.0
    assert train.parse([]).wide_optimizer == "adagrad"
    with pytest.raises(SystemExit):  # as it was
        train.parse(["--sparse_optimizer", "ftrl", "--model", "widedeep"])


# the keys of the final JSON line of `--small 1 --model widedeep --steps 5`, recorded from a run of the commit
# before the option existed
PARENT_KEYS = json.loads('["checksum", "generation", "losses", "model", "start", "steady_ms_per_iter", "steps", '
                         '"total_ms", "world"]')


def test_train_ftrl_reports_wide_nnz_and_the_default_adds_no_key(capsys, monkeypatch):
    base = ("--small", "1", "--model", "widedeep", "--steps", "5")
    plain = _drive(capsys, monkeypatch, *base)
    assert sorted(plain) == PARENT_KEYS
    dense = _drive(capsys, monkeypatch, *base, "--wide_optimizer", "ftrl")
    out = _drive(capsys, monkeypatch, *base, "--wide_optimizer", "ftrl", "--ftrl_l1", "1.0")
    assert sorted(out) == sorted(PARENT_KEYS + ["wide_nnz", "wide_optimizer"])
    assert out["wide_optimizer"] == "ftrl" and 0 <= out["wide_nnz"] < dense["wide_nnz"]
