"""The DeepFM interaction-term kernels (csrc/kernels/deepfm.hip through ops.wd_fm_forward / ops.wd_fm_backward)
on the GPU, u = 2^-24 (csrc/kernels/deepfm.h states the rule):
  forward   against fp64 of the same bf16 inputs, per (sample, column) and per sample:
            |S - S64| <= (F + 2) u sum_f |v_fc|
            |wide_out - (wide_in + fm64)| <= (2F + D + 16) u 0.5 sum_c ((sum_f |v_fc|)^2 + q_c) + u |wide_out|
            and the same bits at blocks = 1, 7 and the default
  backward  on the same S, dwide, X and dX as the fp32 CPU reference: torch.equal, without perm and through a
            random permutation; with an out-of-range perm entry the unaddressed dX row keeps a sentinel
Shapes: the smallest that reach every path -- (F, D) = (1, 8), (70, 8), (2, 16), (26, 32), (9, 64): every lane
shape of the vector form, with fields below, equal to and above one pass of the lane groups; (3, 12), (5, 20): one
lane per column; D = 32 on an X view whose base is 2 bytes off and on one with ldx % 8 != 0 (the same fallback);
B in {1, 3, 257} (one wave, one block, more than one block); ldx > F*D with NaN in every column >= F*D. Then the
model: GPU against CPU, two same-seed runs bit for bit, evaluate() writes no training state, two ranks on one card."""
import math

import pytest
import torch

from test_multirank_gpu import run_world

from minips_amd import ops
from minips_amd.data.synthetic import CriteoSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16
SHAPES = [(1, 8, "pad"), (70, 8, "pad"), (2, 16, "pad"), (26, 32, "pad"), (9, 64, "pad"), (3, 12, "pad"),
          (5, 20, "pad"), (26, 32, "off2"), (26, 32, "ld4")]


def _case(B, F, D, how, seed):
    """(X on the CPU as a [B, ldx] matrix with NaN beyond F*D, wide_in, dwide)."""
    g = torch.Generator().manual_seed(seed)
    ldx = (F * D + 7) // 8 * 8 + 8 if how != "ld4" else F * D + 4
    X = torch.full((B, ldx), float("nan"), dtype=BF)
    X[:, : F * D] = (torch.randn(B, F * D, generator=g) * 0.5).to(BF)
    return X, torch.randn(B, generator=g), torch.randn(B, generator=g)


def _on_gpu(X, how, dev):
    """X on the GPU: a whole 16-byte aligned matrix, or a view whose base is 2 bytes off."""
    B, ldx = X.shape
    if how != "off2":
        Xd = X.to(dev)
        assert Xd.data_ptr() % 16 == 0 and (ldx % 8 == 0) == (how != "ld4")
        return Xd
    flat = torch.full((B * ldx + 1,), float("nan"), dtype=BF, device=dev)
    v = flat[1:].view(B, ldx)
    v.copy_(X.to(dev))
    assert v.data_ptr() % 16 == 2
    return v


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"  {name}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{name}: err / bound {ratio:.3f}"


@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("F,D,how", SHAPES)
def test_forward_and_backward(F, D, how, B, dev):
    X, wide_in, dz = _case(B, F, D, how, seed=1000 * F + 10 * D + B)
    Xd = _on_gpu(X, how, dev)
    v = X[:, : F * D].double().view(B, F, D)
    S64, Sabs, q = v.sum(1), v.abs().sum(1), (v * v).sum(1)
    fm64 = 0.5 * (S64 * S64 - q).sum(1)
    outs = []
    for bl in (0, 1, 7, 0):
        wide = wide_in.to(dev)
        S = torch.full((B, D), float("nan"), device=dev)
        assert ops.wd_fm_forward(Xd, F, D, wide, S, blocks=bl) is S
        outs.append((S, wide))
    torch.cuda.synchronize()
    for S, wide in outs[1:]:
        assert torch.equal(S, outs[0][0]) and torch.equal(wide, outs[0][1])  # every grid size: the same bits
    S, wide = outs[0]
    print(f"F {F} D {D} {how} B {B}")
    _within("S", S, S64, (F + 2) * U * Sabs)
    _within("wide", wide, wide_in.double() + fm64,
            (2 * F + D + 16) * U * 0.5 * (Sabs * Sabs + q).sum(1) + U * wide.double().cpu().abs())
    if F == 1:
        assert torch.equal(wide.cpu(), wide_in)  # no pair, fm == 0.0 exactly
    assert ops.wd_fm_forward(Xd, F, D, wide_in.to(dev)).shape == (B, D)  # S allocated when not given

    # backward: the same S, dwide, X, dX on both sides
    Sc = ops.wd_fm_forward(X, F, D, wide_in.clone())  # the fp32 CPU reference's S
    n = B * F
    g = torch.Generator().manual_seed(7)
    dX0 = torch.randn(n, D, generator=g).to(BF)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    bad = perm.clone()
    lost = int(torch.randint(0, n, (1,), generator=g))
    bad[lost] = n if B % 2 else -1  # outside [0, n): row perm[lost] is addressed by nobody
    for name, p in (("natural", None), ("perm", perm), ("perm with a hole", bad)):
        for bl in (0, 3):
            want, got = dX0.clone(), dX0.clone()
            if p is bad:
                want[int(perm[lost])] = got[int(perm[lost])] = 7.0  # the sentinel
            got = got.to(dev)
            ops.wd_fm_backward(X, Sc, dz, want, F, D, perm=p)
            ops.wd_fm_backward(Xd, Sc.to(dev), dz.to(dev), got, F, D, perm=None if p is None else p.to(dev),
                               blocks=bl)
            assert torch.equal(got.cpu(), want), f"{name}, blocks {bl}"
            assert F == 1 or not torch.equal(want, dX0)
            if p is bad:
                assert bool((got[int(perm[lost])] == 7.0).all())
    dXn = dX0.clone().view(B, F * D).to(dev)  # the lookup-order layout [B, F*D]
    want = dX0.clone()
    ops.wd_fm_backward(X, Sc, dz, want, F, D)
    ops.wd_fm_backward(Xd, Sc.to(dev), dz.to(dev), dXn, F, D)
    assert torch.equal(dXn.cpu().view(n, D), want)


def test_empty_batch_launches_nothing(dev):
    X = torch.zeros(0, 40, dtype=BF, device=dev)
    S = ops.wd_fm_forward(X, 4, 8, torch.zeros(0, device=dev))
    ops.wd_fm_backward(X, S, torch.zeros(0, device=dev), torch.zeros(0, 32, dtype=BF, device=dev), 4, 8)
    torch.cuda.synchronize()
    assert S.shape == (0, 8)


# ------------------------------------------------------------------------------ the model
CARDS = [100, 50, 3000, 7, 300, 20, 5, 60, 90, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26]


def _init_rows(m):
    g = torch.Generator().manual_seed(9)
    r = torch.randn(m.emb.rows_local, m.cfg.row_width, generator=g) * 0.01
    r[:, m.cfg.emb_dim:] = 0
    return r.to(m.emb.shard.device)


def _run(device, steps=12):
    torch.manual_seed(0)
    m = WideDeep(WideDeepConfig(cards=CARDS, transport="collective", fm_term=True), Comm(device=torch.device(device)))
    m.emb.shard.copy_(_init_rows(m))
    data = CriteoSynth(512, cards=CARDS, device="cpu", seed=3)
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        losses.append(float(m.train_step(dense.to(device), keys.to(device), y.to(device)).item()) / 512)
    m.drain()
    return losses, m


def test_model_gpu_matches_cpu(dev):
    """test_widedeep_gpu.py's cards, steps and bounds, with the term on."""
    l_cpu, m_cpu = _run("cpu")
    l_gpu, m_gpu = _run(dev)
    print(f"cpu {l_cpu}\ngpu {l_gpu}")
    assert l_gpu[-1] < l_gpu[0]
    for a, b in zip(l_gpu, l_cpu):
        assert abs(a - b) < 2e-2 * max(1.0, abs(b)), (l_gpu, l_cpu)
    diff = (m_gpu.dense.master.cpu() - m_cpu.dense.master).abs()
    assert float(diff.max()) <= 1e-3 * 12 * 1.5
    assert float((diff > 2e-3).float().mean()) < 1e-2
    assert "S" in m_gpu._bufs[512]


def _feeder_run(dev, steps=6, B=4096):
    from minips_amd.models.feeder import LookaheadFeeder

    comm = Comm(device=torch.device(dev))
    m = WideDeep(WideDeepConfig(cards=CARDS, fm_term=True), comm)
    feeder = LookaheadFeeder(m, CriteoSynth(B, cards=CARDS, device=dev, seed=11), comm)
    losses = [feeder.step().clone() for _ in range(steps)]
    m.drain()
    torch.cuda.synchronize()
    return m, feeder, (torch.stack(losses).cpu(), m.dense.full_master().cpu(), m.emb.shard.cpu().clone(),
                       m.emb.state.cpu().clone())


def test_one_rank_bit_identical(dev):
    """Two same-seed runs through the look-ahead feeder end bit-identical (loss, dense master, shard, Adagrad
    state), as test_widedeep_bsp_one_rank_bit_identical asserts for Wide&Deep: the two kernels add no
    run-dependent order."""
    a, b = _feeder_run(dev)[2], _feeder_run(dev)[2]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_evaluate_writes_no_training_state(dev):
    m, feeder, _ = _feeder_run(dev, steps=3, B=512)

    def state():
        e, d, b = m.emb, m.dense, m._bufs[512]
        ts = [e.shard, e.state, d.master, d.m, d.v, d.grad, d.step_dev, b["dX"], b["S"], b["wide"], b["dwide"], b["X"]]
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
    assert m._ebufs[512]["S"].shape == (512, 32)
    assert math.isfinite(float(feeder.step()))
    m.drain()


WD_TOTAL = 256


def _dfm_world(rank, world, steps=6):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    comm = Comm(device=dev)
    per = WD_TOTAL // world
    cfg = WideDeepConfig(cards=CARDS, transport="collective", max_batch=per, fm_term=True)
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
    many = run_world(_dfm_world, world=2)
    one = run_world(_dfm_world, world=1)[0]
    print(f"2 ranks on one card {many[0]} vs one rank {one}")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert all(math.isfinite(v) for v in many[0])
