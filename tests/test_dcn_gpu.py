"""The Deep & Cross kernels (csrc/kernels/dcn.hip through ops.wd_cross_forward / wd_cross_backward / wd_cross_fold)
on the GPU; csrc/kernels/dcn.h states the rule, tests/test_dcn.py the references and the bounds (u = 2^-24,
K = (L + 2)(d + 8), M_T the abs companion of T in fp64):
  forward    |p - p64| <= (d + 2) u sum |x||w|, |wide_out - (wide_in + c64)| <= K u M_c + u |wide_out|; the same bits
             at blocks = 1, 7 and the default
  backward   on the same X, p, k, dwide, Pc and dX as the fp32 CPU reference: dX torch.equal, without perm, through a
             random permutation, and with one out-of-range entry whose row keeps a sentinel
  batch sums part and Gc have the same bits at blocks = 1, 3 and the default; Gc within (K + B) u M of fp64
Shapes (F, D, n_dense, L): (1, 8, 0, 1) one lane; (2, 8, 3, 2) d = 19, a tail piece and dense columns; (26, 32, 13, 3)
d = 845, two pieces per lane, also on an X view 2 bytes off and on one with ldx % 8 != 0 (the scalar form);
(9, 64, 1, 4); (3, 12, 5, 2) the scalar form by D. B in {1, 3, CHUNK + 1, 2 CHUNK + 1}: one wave, one chunk, a chunk
of one sample behind a full one, three chunks. NaN in every X column >= d and in Pc's pad. Then the model: GPU
against CPU, two same-seed runs bit for bit, evaluate() writes no training state, two ranks on one card."""
import math

import pytest
import torch

from test_dcn import BF, check_dx_from_zero, check_forward, check_gc, make_case
from test_multirank_gpu import run_world

from minips_amd import _native, ops
from minips_amd.data.synthetic import CriteoSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu

CH = ops.CROSS_CHUNK
LAYOUTS = [(1, 8, 0, 1, "pad"), (2, 8, 3, 2, "pad"), (26, 32, 13, 3, "pad"), (9, 64, 1, 4, "pad"),
           (3, 12, 5, 2, "pad"), (26, 32, 13, 3, "off2"), (26, 32, 13, 3, "ld4")]
BATCHES = [1, 3, CH + 1, 2 * CH + 1]
_CASES = {}


def _case(B, F, D, nd, L, how):
    """The fp64 references are computed once per shape and shared, unchanged, by the tests."""
    key = (B, F, D, nd, L, how)
    if key not in _CASES:
        d = F * D + nd
        _CASES[key] = make_case(B, F, D, nd, L, seed=B + F + D, ldx=(d + 7) // 8 * 8 + (4 if how == "ld4" else 8))
    return _CASES[key]


def _x_on(c, how, dev):
    X = c["X"]
    if how != "off2":
        return X.to(dev)
    flat = torch.zeros(X.numel() + 8, dtype=BF, device=dev)  # the same matrix, its base 2 bytes off
    v = flat[1: 1 + X.numel()].view(X.shape)
    v.copy_(X)
    assert v.data_ptr() % 16 == 2
    return v


def _params():
    for lay in LAYOUTS:
        for B in BATCHES:
            yield pytest.param(B, *lay, id=f"B{B}-F{lay[0]}-D{lay[1]}-n{lay[2]}-L{lay[3]}-{lay[4]}")


def test_the_chunk_constant_is_the_bindings():
    assert _native.dcnk().CHUNK == CH and _native.dcnk().MAX_D == ops.CROSS_MAX_D


@pytest.mark.parametrize("B,F,D,nd,L,how", _params())
def test_forward(B, F, D, nd, L, how, dev):
    c = _case(B, F, D, nd, L, how)
    X, Pc = _x_on(c, how, dev), c["Pc"].to(dev)
    outs = []
    for bl in (0, 1, 7):
        wide = c["wide"].clone().to(dev)
        p, k = ops.wd_cross_forward(X, c["d"], Pc, L, wide, blocks=bl)
        outs.append((wide, p, k))
    check_forward(c, outs[0][0], outs[0][1])
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    # k against fp64: k_j = <b_0 + ... + b_{j-1}, w_j>, a length-d dot product of bf16 values
    W, bb = c["Pc"][0::2, : c["d"]].double(), c["Pc"][1::2, : c["d"]].double()
    Bj = torch.cat([torch.zeros(1, c["d"], dtype=torch.float64), torch.cumsum(bb, 0)])
    err = (outs[0][2].double().cpu() - (Bj * W).sum(1)).abs()
    assert bool((err <= (c["d"] + L + 2) * 2.0 ** -24 * (Bj.abs() * W.abs()).sum(1)).all())


@pytest.mark.parametrize("B,F,D,nd,L,how", _params())
def test_backward_equals_the_cpu_reference(B, F, D, nd, L, how, dev):
    c = _case(B, F, D, nd, L, how)
    d, n = c["d"], B * F
    X, Pc, dz = c["X"], c["Pc"], c["dz"]
    Xd, Pcd, dzd = _x_on(c, how, dev), Pc.to(dev), dz.to(dev)
    p, k = ops.wd_cross_forward(X, d, Pc, L, c["wide"].clone())  # the same p and k for both
    pd, kd = p.to(dev), k.to(dev)
    g = torch.Generator().manual_seed(B + F)
    dX0 = torch.randn(n, D, generator=g).to(BF)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    bad = perm.clone()
    lost = int(torch.randint(0, n, (1,), generator=g))
    bad[lost] = n if B % 2 else -1  # outside [0, n): row perm[lost] is addressed by nobody
    shape = ops.wd_cross_part_shape(B, d, L)
    for name, pm in (("natural", None), ("perm", perm), ("perm with a hole", bad)):
        for bl in (0, 3):
            want, got = dX0.clone(), dX0.clone()
            if pm is bad:
                want[int(perm[lost])] = got[int(perm[lost])] = 7.0  # the sentinel
            got = got.to(dev)
            ops.wd_cross_backward(X, d, p, k, dz, Pc, L, want, F, D, torch.empty(shape), perm=pm)
            ops.wd_cross_backward(Xd, d, pd, kd, dzd, Pcd, L, got, F, D, torch.empty(shape, device=dev),
                                  perm=None if pm is None else pm.to(dev), blocks=bl)
            assert torch.equal(got.cpu(), want), f"{name}, blocks {bl}"
            assert not torch.equal(want, dX0)
            if pm is bad:
                assert bool((got[int(perm[lost])] == 7.0).all())
    dXn = dX0.clone().view(B, F * D).to(dev)  # the lookup-order layout [B, F*D]
    want = dX0.clone()
    ops.wd_cross_backward(X, d, p, k, dz, Pc, L, want, F, D, torch.empty(shape))
    ops.wd_cross_backward(Xd, d, pd, kd, dzd, Pcd, L, dXn, F, D, torch.empty(shape, device=dev))
    assert torch.equal(dXn.cpu().view(n, D), want)


@pytest.mark.parametrize("B,F,D,nd,L,how", _params())
def test_batch_sums(B, F, D, nd, L, how, dev):
    c = _case(B, F, D, nd, L, how)
    d = c["d"]
    X, Pc, dz = _x_on(c, how, dev), c["Pc"].to(dev), c["dz"].to(dev)
    p, k = ops.wd_cross_forward(X, d, Pc, L, c["wide"].clone().to(dev))
    outs = []
    for bl in (0, 1, 3):
        dX = torch.zeros(B, F * D, dtype=BF, device=dev)
        part = torch.full(ops.wd_cross_part_shape(B, d, L), float("nan"), device=dev)
        ops.wd_cross_backward(X, d, p, k, dz, Pc, L, dX, F, D, part, blocks=bl)
        Gc = torch.zeros(2 * L + 1, c["dp"], device=dev)
        ops.wd_cross_fold(part, Pc, d, L, Gc)
        rows = (L + 1) * c["dp"]
        live = torch.cat([part[:, :rows].reshape(-1), part[:, rows: rows + L + 1].reshape(-1)])
        outs.append((live, Gc, dX))
    assert bool(torch.isfinite(outs[0][0]).all())  # every live slot of part was written (it started as NaN)
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    check_dx_from_zero(c, outs[0][2])
    check_gc(c, outs[0][1])
    assert bool((outs[0][1][:, d:] == 0).all())  # the pad columns get no gradient
    G2 = torch.full_like(outs[0][1], 0.5)  # the fold adds
    part = torch.empty(ops.wd_cross_part_shape(B, d, L), device=dev)
    ops.wd_cross_backward(X, d, p, k, dz, Pc, L, torch.zeros(B, F * D, dtype=BF, device=dev), F, D, part)
    ops.wd_cross_fold(part, Pc, d, L, G2)
    assert torch.equal(G2[:, :d], 0.5 + outs[0][1][:, :d])


def test_empty_batch_launches_nothing(dev):
    X = torch.zeros(0, 40, dtype=BF, device=dev)
    Pc = torch.zeros(5, 40, dtype=BF, device=dev)
    k0 = torch.full((3,), 7.0, device=dev)
    p, k = ops.wd_cross_forward(X, 35, Pc, 2, torch.zeros(0, device=dev), k=k0)
    part = torch.zeros(ops.wd_cross_part_shape(0, 35, 2), device=dev)
    ops.wd_cross_backward(X, 35, p, k, torch.zeros(0, device=dev), Pc, 2, torch.zeros(0, 32, dtype=BF, device=dev), 4,
                          8, part)
    Gc = torch.full((5, 40), 3.0, device=dev)
    ops.wd_cross_fold(part, Pc, 35, 2, Gc)
    torch.cuda.synchronize()
    assert p.shape == (0, 3) and part.shape[0] == 0 and bool((k == 7).all()) and bool((Gc == 3).all())


# ------------------------------------------------------------------------------ the model
CARDS = [100, 50, 3000, 7, 300, 20, 5, 60, 90, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26]


def _init_rows(m):
    g = torch.Generator().manual_seed(9)
    r = torch.randn(m.emb.rows_local, m.cfg.row_width, generator=g) * 0.01
    r[:, m.cfg.emb_dim:] = 0
    return r.to(m.emb.shard.device)


def _run(device, steps=12):
    torch.manual_seed(0)
    m = WideDeep(WideDeepConfig(cards=CARDS, transport="collective", cross_layers=3),
                 Comm(device=torch.device(device)))
    m.emb.shard.copy_(_init_rows(m))
    data = CriteoSynth(512, cards=CARDS, device="cpu", seed=3)
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        losses.append(float(m.train_step(dense.to(device), keys.to(device), y.to(device)).item()) / 512)
    m.drain()
    return losses, m


def test_model_gpu_matches_cpu(dev):
    """test_widedeep_gpu.py's cards, steps and bounds, with three cross layers."""
    l_cpu, m_cpu = _run("cpu")
    l_gpu, m_gpu = _run(dev)
    print(f"cpu {l_cpu}\ngpu {l_gpu}")
    assert l_gpu[-1] < l_gpu[0]
    for a, b in zip(l_gpu, l_cpu):
        assert abs(a - b) < 2e-2 * max(1.0, abs(b)), (l_gpu, l_cpu)
    diff = (m_gpu.dense.master.cpu() - m_cpu.dense.master).abs()
    assert float(diff.max()) <= 1e-3 * 12 * 1.5
    assert float((diff > 2e-3).float().mean()) < 1e-2
    o, shape = m_gpu.layout["cross"]
    init = WideDeep(WideDeepConfig(cards=CARDS, transport="collective", cross_layers=3),
                    Comm(device=torch.device("cpu"))).dense.master
    moved = (m_gpu.dense.master.cpu()[o: o + math.prod(shape)] != init[o: o + math.prod(shape)]).view(shape)
    assert bool(moved[:, : m_gpu.k_in[0]].all()), "a cross parameter was not trained on the GPU"


def _feeder_run(dev, steps=6, B=4096):
    from minips_amd.models.feeder import LookaheadFeeder

    comm = Comm(device=torch.device(dev))
    m = WideDeep(WideDeepConfig(cards=CARDS, cross_layers=3), comm)
    feeder = LookaheadFeeder(m, CriteoSynth(B, cards=CARDS, device=dev, seed=11), comm)
    losses = [feeder.step().clone() for _ in range(steps)]
    m.drain()
    torch.cuda.synchronize()
    return m, feeder, (torch.stack(losses).cpu(), m.dense.full_master().cpu(), m.emb.shard.cpu().clone(),
                       m.emb.state.cpu().clone())


def test_one_rank_bit_identical(dev):
    """Two same-seed runs through the look-ahead feeder end bit-identical (loss, dense master, shard, Adagrad
    state): the kernels add no run-dependent order, and the side-stream Adam waits for the cross fold -- a point
    taken before it lets the Adam clear the gradient buffer under the fold and rewrite the values the cross
    backward reads."""
    a, b = _feeder_run(dev)[2], _feeder_run(dev)[2]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_evaluate_writes_no_training_state(dev):
    m, feeder, _ = _feeder_run(dev, steps=3, B=512)

    def state():
        e, d, b = m.emb, m.dense, m._bufs[512]
        ts = [e.shard, e.state, d.master, d.m, d.v, d.grad, d.step_dev, b["dX"], b["p"], b["k"], b["part"], b["wide"],
              b["dwide"], b["X"]]
        if e.state2 is not None:
            ts.append(e.state2)
        return [t.clone() for t in ts], (d.step, len(e._pending), d._pending)

    before = state()
    held = CriteoSynth(512, cards=CARDS, device=dev, seed=5)
    r = m.evaluate(held.next() for _ in range(2))
    m.drain()
    torch.cuda.synchronize()
    after = state()
    assert r["n"] == 1024 and r["logloss"] > 0 and before[1] == after[1]
    for x, y in zip(before[0], after[0]):
        assert torch.equal(x, y)
    assert m._ebufs[512]["p"].shape == (512, 4) and "part" not in m._ebufs[512]
    assert math.isfinite(float(feeder.step()))
    m.drain()


WD_TOTAL = 256


def _dcn_world(rank, world, steps=6):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    comm = Comm(device=dev)
    per = WD_TOTAL // world
    cfg = WideDeepConfig(cards=CARDS, transport="collective", max_batch=per, cross_layers=3)
    m = WideDeep(cfg, comm)
    g = torch.Generator().manual_seed(5)
    full = torch.randn(m.num_rows, cfg.row_width, generator=g) * 0.01
    full[:, cfg.emb_dim:] = 0
    m.emb.shard.copy_(full[m.emb.base: m.emb.base + m.emb.rows_local].to(dev))
    torch.cuda.synchronize()
    comm.barrier()
    data = CriteoSynth(WD_TOTAL, cards=CARDS, device=dev, seed=11)  # the same global batch on every rank
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        sl = slice(rank * per, (rank + 1) * per)
        t = m.train_step(dense[sl], keys[sl], y[sl]).clone()
        comm.all_reduce_(t)
        losses.append(float(t) / WD_TOTAL)
    m.drain()
    torch.cuda.synchronize()
    return losses


def test_two_ranks_on_one_card_match_one_rank():
    many = run_world(_dcn_world, world=2)
    one = run_world(_dcn_world, world=1)[0]
    print(f"2 ranks on one card {many[0]} vs one rank {one}")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert all(math.isfinite(v) for v in many[0])
