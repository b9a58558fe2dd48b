"""Global-norm gradient clipping and the lr schedule of DenseTable on the CPU reference path
(minips_amd/ops grad_sumsq / adam_clip_apply, ps/tables.py clip_norm / LRSchedule): the rule against
torch.nn.utils.clip_grad_norm_, the skip of a non-finite clock, the schedule's values and its resume
after a restore, two gloo ranks (flat and bucketed) against one rank, and the driver flags."""
import json
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.ps.comm import Comm
from minips_amd.ps.tables import DenseTable, LRSchedule

CPU = torch.device("cpu")
N = 1000
BETAS, EPS, WD, LR = (0.9, 0.95), 1e-8, 0.01, 1e-2


def _table(comm=None, **kw):
    t = DenseTable(comm or Comm(device=CPU), N, optimizer="adam", lr=LR, betas=BETAS, eps=EPS, weight_decay=WD,
                   pull_dtype=torch.float32, **kw)
    t.load_full(torch.linspace(-1, 1, N))
    return t


def _grads(steps, seed=3, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, generator=g) * scale * (1 + i) for i in range(steps)]


def _state(t):
    return [x.clone() for x in (t.master, t.m, t.v, t.params)]


def test_grad_sumsq_cpu():
    g = torch.randn(4100, generator=torch.Generator().manual_seed(0))
    part = torch.full((8,), 7.0, dtype=torch.float64)
    ops.grad_sumsq(g, part)
    assert float(part.sum()) == float(g.double().square().sum()) and int((part[1:] != 0).sum()) == 0
    # an element of 1e30 squares to 1e60: finite in fp64
    g[5] = 1e30
    ops.grad_sumsq(g, part, 3)
    assert math.isfinite(float(part[:3].sum())) and float(part[:3].sum()) == float(g.double().square().sum())
    # split-K planes are folded in the Adam kernel's order: groups of four, then one by one
    planes = torch.randn(6, 8, generator=torch.Generator().manual_seed(1))
    x = g.clone()
    x[16:24] = ((x[16:24] + ((planes[0] + planes[1]) + (planes[2] + planes[3]))) + planes[4]) + planes[5]
    ops.grad_sumsq(g, part, slabs=[(planes.reshape(-1), 6, 8, 16)])
    assert float(part.sum()) == float(x.double().square().sum())


def test_fold_slabs_models(monkeypatch):
    """ops._fold_slabs is the one CPU model of the kernels' two plane-fold orders: plane by plane against a
    plain loop, grouped against the written-out expression, and the CPU branches of slab_pack (plane by
    plane) and adam_apply (grouped) route through it."""
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(64, generator=gen)
    planes = torch.randn(6, 16, generator=gen)
    slabs = [(planes.reshape(-1), 6, 16, 32)]
    loop = g.clone()
    for z in range(6):
        for e in range(16):
            loop[32 + e] = loop[32 + e] + planes[z, e]
    assert torch.equal(ops._fold_slabs(g, slabs, group4=False), loop)
    grouped = g.clone()
    grouped[32:48] = ((g[32:48] + ((planes[0] + planes[1]) + (planes[2] + planes[3]))) + planes[4]) + planes[5]
    assert torch.equal(ops._fold_slabs(g, slabs), grouped)
    assert not torch.equal(grouped, loop)  # the two orders differ on this input
    assert ops._fold_slabs(g, ()) is g
    calls = []
    fold = ops._fold_slabs

    def spy(g_, slabs_, group4=True):
        calls.append(group4)
        return fold(g_, slabs_, group4)

    monkeypatch.setattr(ops, "_fold_slabs", spy)
    src, out = g.clone(), torch.empty(64)
    ops.slab_pack(src, out, slabs)
    assert calls == [False] and torch.equal(out, loop) and int((src != 0).sum()) == 0
    m, w = torch.zeros(64), torch.zeros(64)
    ops.adam_apply(w, m, torch.zeros(64), g, 1e-3, beta1=0.0, slabs=slabs)
    assert calls == [False, True] and torch.equal(m, grouped)  # beta1 = 0: m = 0 * m + 1 * g, exact


def test_clip_scale_rule():
    assert ops.clip_scale(4.0, 10.0) == (2.0, 1.0, False)  # below the threshold: exactly 1
    norm, scale, skip = ops.clip_scale(1e60, 1.0)
    assert norm == 1e30 and not skip and scale == float(torch.tensor(1.0 / (1e30 + 1e-6), dtype=torch.float32))
    assert ops.clip_scale(float("inf"), 1.0)[1:] == (0.0, True) and ops.clip_scale(float("nan"), 1.0)[2]


def test_clipped_table_matches_clip_grad_norm():
    """6 clocks, clipped at some and not at others, against clip_grad_norm_ + the table's Adam formula."""
    t = _table(clip_norm=40.0)
    w = torch.linspace(-1, 1, N).clone().requires_grad_(True)
    m, v = torch.zeros(N), torch.zeros(N)
    clipped = 0
    for step, g in enumerate(_grads(6), 1):
        t.add(g)
        t.clock()
        w.grad = g.clone()
        norm = float(torch.nn.utils.clip_grad_norm_([w], 40.0))
        clipped += norm > 40.0
        with torch.no_grad():
            m = BETAS[0] * m + (1 - BETAS[0]) * w.grad
            v = BETAS[1] * v + (1 - BETAS[1]) * w.grad * w.grad
            mh, vh = m / (1 - BETAS[0] ** step), v / (1 - BETAS[1] ** step)
            w -= LR * (mh / (vh.sqrt() + EPS) + WD * w)
        st = t.clip_stats()
        assert st["norm"] == pytest.approx(norm, rel=1e-6)
        torch.testing.assert_close(t.full_master(), w.detach(), rtol=1e-5, atol=1e-6)
    assert 0 < clipped < 6, "the gradients were meant to cross the threshold"
    assert t.clip_stats()["clipped"] == clipped and t.clip_stats()["skipped"] == 0
    assert int((t.grad != 0).sum()) == 0


def test_huge_clip_norm_is_bit_identical_to_no_clipping():
    a, b = _table(), _table(clip_norm=1e30)
    for g in _grads(4):
        for t in (a, b):
            t.add(g)
            t.clock()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert b.clip_stats()["clipped"] == 0 and b.clip_stats()["scale"] == 1.0


def test_non_finite_clock_is_skipped():
    t, ref = _table(clip_norm=1.0), _table(clip_norm=1.0)
    g0, g1 = _grads(2)
    for x in (t, ref):
        x.add(g0)
        x.clock()
    before = _state(t)
    bad = g1.clone()
    bad[17] = float("inf")
    t.add(bad)
    t.clock()
    for x, y in zip(_state(t), before):
        assert torch.equal(x, y)  # master, m, v and the parameters bit for bit
    assert int((t.grad != 0).sum()) == 0 and not bool(torch.isnan(t.grad).any())
    st = t.clip_stats()
    assert st["skipped"] == 1 and st["clipped"] == 1 and st["scale"] == 0.0 and math.isinf(st["norm"])
    assert t.step == 2  # the step counter counts clocks, applied or not
    # the next finite clock applies normally: the reference table takes the same clock as its step 3
    ref.step = 2
    for x in (t, ref):
        x.add(g1)
        x.clock()
    for x, y in zip(_state(t), _state(ref)):
        assert torch.equal(x, y)
    assert t.clip_stats()["skipped"] == 1 and t.clip_stats()["clipped"] == 2


def test_clip_norm_needs_fp32_adam():
    for kw in (dict(optimizer="sgd"), dict(optimizer="add", value_dtype=torch.float64), dict(optimizer="adagrad")):
        with pytest.raises(ValueError):
            DenseTable(Comm(device=CPU), 64, clip_norm=1.0, **kw)
    with pytest.raises(ValueError):
        DenseTable(Comm(device=CPU), 64, clip_norm=0.0)
    with pytest.raises(RuntimeError):
        DenseTable(Comm(device=CPU), 64).clip_stats()


def test_schedule_values():
    s = LRSchedule(warmup=10, decay_steps=110, min_ratio=0.1)
    assert s.lr(1, 2.0) == 2.0 * 1 / 10
    assert s.lr(10, 2.0) == 2.0
    assert s.lr(60, 2.0) == pytest.approx(2.0 * (0.1 + 0.9 * 0.5), rel=1e-12)  # the middle of the half cosine
    assert s.lr(35, 2.0) == pytest.approx(2.0 * (0.1 + 0.9 * 0.5 * (1 + math.cos(math.pi * 0.25))), rel=1e-12)
    assert s.lr(110, 2.0) == pytest.approx(0.2, rel=1e-12) and s.lr(5000, 2.0) == s.lr(110, 2.0)
    assert all(s.lr(k, 1.0) >= s.lr(k + 1, 1.0) for k in range(10, 120))
    assert LRSchedule(warmup=4).lr(100, 3.0) == 3.0  # no decay
    for bad in (dict(warmup=-1), dict(warmup=5, decay_steps=5), dict(min_ratio=1.5)):
        with pytest.raises(ValueError):
            LRSchedule(**bad)


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_schedule_drives_the_optimizer_and_resumes(optimizer):
    """A scheduled table equals a constant-lr table whose lr is set by hand each step; a table restored at
    step k (finish_restore) continues the schedule from k."""
    sched = LRSchedule(warmup=3, decay_steps=8, min_ratio=0.2)
    def mk(**kw):
        return DenseTable(Comm(device=CPU), N, optimizer=optimizer, lr=LR, pull_dtype=torch.float32, **kw)

    a, b = mk(lr_schedule=sched), mk()
    grads = _grads(6)
    for step, g in enumerate(grads, 1):
        assert a.lr_at(step) == sched.lr(step, LR)
        b.lr = sched.lr(step, LR)
        for t in (a, b):
            t.add(g)
            t.clock()
    assert torch.equal(a.master, b.master)
    c = mk(lr_schedule=sched)
    for g in grads[:4]:
        c.add(g)
        c.clock()
    r = mk(lr_schedule=sched)
    for n, dst in r.restore_dst().items():
        dst.copy_(getattr(c, n).view(-1, 1))
    r.finish_restore(4)
    for g in grads[4:]:
        r.add(g)
        r.clock()
    assert r.step == 6 and torch.equal(r.master, a.master)


# ------------------------------------------------------------------------------ two gloo ranks
def _world_fn(rank, world, bucketed):
    comm = Comm(device=CPU)
    kw = dict(buckets=[0, 256, 640]) if bucketed else {}
    t = _table(comm, clip_norm=25.0, **kw)
    assert (t.buckets is not None) == bucketed
    comm.trace = []
    norms = []
    for g in _grads(4, seed=10 + rank):
        if bucketed:  # written in place, the last bucket issued from the "backward"
            t.grad[:N] += g
            t.bucket_ready(len(t.buckets) - 1)
        else:
            t.add(g)
        t.clock()
        norms.append(t.clip_stats()["norm"])
    trace = [op for op, _, _ in comm.trace]
    st = t.clip_stats()
    return t.full_master().tolist(), norms, trace, st["clipped"]  # (pickled by value)


def _flat2(rank, world):
    return _world_fn(rank, world, False)


def _bucketed2(rank, world):
    return _world_fn(rank, world, True)


@pytest.fixture(scope="module")
def one_rank_on_summed_gradient():
    t = _table(clip_norm=25.0)
    norms = []
    for g0, g1 in zip(_grads(4, seed=10), _grads(4, seed=11)):
        t.add(g0 + g1)
        t.clock()
        norms.append(t.clip_stats()["norm"])
    return t.full_master(), norms, t.clip_stats()["clipped"]


@pytest.mark.parametrize("fn", [_flat2, _bucketed2], ids=["flat", "bucketed"])
def test_two_ranks_match_one_rank(fn, one_rank_on_summed_gradient):
    ref_w, ref_norms, ref_clipped = one_rank_on_summed_gradient
    out = run_world(fn)
    (w0, n0, tr0, c0), (w1, n1, tr1, c1) = out[0], out[1]
    assert n0 == n1  # the norm: the same bits on both ranks
    assert n0 == pytest.approx(ref_norms, rel=1e-6)
    assert c0 == c1 == ref_clipped and 0 < ref_clipped
    for w in (w0, w1):
        torch.testing.assert_close(torch.tensor(w), ref_w, rtol=1e-5, atol=1e-6)
    assert tr0 == tr1
    # per clock: the reduce-scatters, then exactly one all-reduce, then the all-gathers
    clocks, cur = [], []
    for op in tr0:
        if op == "reduce_scatter" and "all_gather" in cur:
            clocks.append(cur)
            cur = []
        cur.append(op)
    clocks.append(cur)
    assert len(clocks) == 4
    for c in clocks:
        nb = c.count("reduce_scatter")
        assert c == ["reduce_scatter"] * nb + ["all_reduce"] + ["all_gather"] * nb, c


def _no_clip_trace(rank, world):
    comm = Comm(device=CPU)
    t = _table(comm)
    comm.trace = []
    t.add(_grads(1)[0])
    t.clock()
    return [op for op, _, _ in comm.trace]


def test_without_clip_norm_no_all_reduce():
    out = run_world(_no_clip_trace)
    assert out[0] == out[1] == ["reduce_scatter", "all_gather"]


# ------------------------------------------------------------------------------ the driver
def _drive(capsys, monkeypatch, *argv):
    """minips_amd.train in this process, on the CPU whatever the machine has."""
    from minips_amd import train

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert train.main(list(argv)) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    return json.loads(lines[-1]), lines


def test_train_flags(capsys, tmp_path, monkeypatch):
    from minips_amd.utils import metrics

    monkeypatch.setenv("MINIPS_METRICS_DIR", str(tmp_path))
    monkeypatch.setattr(metrics, "_LOGGER", None)
    out, lines = _drive(capsys, monkeypatch, "--model", "gpt2", "--small", "1", "--steps", "10", "--clip_norm", "0.5",
                        "--lr_warmup", "20", "--metrics_dir", str(tmp_path))
    line = next(l for l in lines if l.startswith("Current iteration=10"))
    assert "grad_norm=" in line and "clip_scale=" in line and "lr=0.00015" in line, line  # 3e-4 * 10 / 20
    assert out["clipped_steps"] == 10 and out["skipped_steps"] == 0
    metrics.get_logger().close()
    rec = [json.loads(l) for l in open(tmp_path / "rank0.jsonl")]
    rec = [r for r in rec if "grad_norm" in r]
    assert len(rec) == 1 and rec[0]["clip_scale"] < 1.0 and rec[0]["lr"] == pytest.approx(1.5e-4)


@pytest.mark.parametrize("argv", [("--model", "widedeep", "--clip_norm", "1"), ("--model", "dlrm", "--lr_warmup", "5"),
                                  ("--model", "gpt2", "--clip_norm", "-1"),
                                  ("--model", "mlp", "--lr_warmup", "5", "--lr_decay_steps", "5")])
def test_train_refuses_bad_flags(argv, capsys):
    from minips_amd import train

    with pytest.raises(SystemExit) as e:
        train.parse(list(argv))
    assert e.value.code == 2
    assert "--clip_norm" in capsys.readouterr().err


def test_train_defaults_add_no_keys(capsys, monkeypatch):
    out, lines = _drive(capsys, monkeypatch, "--model", "mlp", "--small", "1", "--steps", "10")
    assert not any("grad_norm" in l or "lr=" in l for l in lines)
    assert "clipped_steps" not in out and "skipped_steps" not in out
