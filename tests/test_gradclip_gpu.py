"""Global-norm gradient clipping on the GPU (csrc/kernels/gradclip.hip through minips_amd._optk):
grad_sumsq against the CPU fold summed in fp64, adam_clip_apply bit for bit against adam_apply at the
scale it derived, the two plane-fold orders bit for bit against their CPU models, the skip of a non-finite
clock, and the clipped DenseTable / GPT-2 / graphed MLP
against their CPU or eager twins."""
import math

import pytest
import torch

from test_gpt2 import TINY
from test_ps_gloo import run_world

from minips_amd import ops

pytestmark = pytest.mark.gpu

F64 = torch.float64
BIG = 3 * 2 ** 18 + 64


def _regions(n, seed=0):
    """(planes [nsplit * plane], nsplit, plane, offset): regions at the start, in the middle (two) and at
    the end of a gradient of n elements, nsplit 1 / 3 / 5 / 8 (n = 4: one region of 5 planes)."""
    g = torch.Generator().manual_seed(100 + seed)
    if n < 64:
        return [(torch.randn(5 * n, generator=g), 5, n, 0)]
    mid = (n // 2) // 4 * 4
    spec = [(1, 8, 0), (3, 12, mid - 12), (5, 16, mid), (8, 8, n - 8)]
    return [(torch.randn(ns * p, generator=g), ns, p, o) for ns, p, o in spec]


def _to(slabs, dev):
    return [(s.to(dev), ns, p, o) for s, ns, p, o in slabs]


@pytest.fixture(scope="module")
def gradients():
    """n -> (g, slabs, fp64 sum of squares of g, of g + slabs in the kernel's fold order), on the CPU."""
    out = {}
    for n in (4, 1020, 4100, BIG):
        g = torch.randn(n, generator=torch.Generator().manual_seed(n))
        slabs = _regions(n)
        out[n] = (g, slabs, float(g.double().square().sum()),
                  float(ops._fold_slabs(g, slabs).double().square().sum()))
    return out


@pytest.mark.parametrize("with_slabs", [False, True], ids=["plain", "slabs"])
@pytest.mark.parametrize("L", [1, 3, 64])
@pytest.mark.parametrize("n", [4, 1020, 4100, BIG])
def test_grad_sumsq(n, L, with_slabs, gradients, dev):
    g, slabs, ref_plain, ref_slabs = gradients[n]
    ref = ref_slabs if with_slabs else ref_plain
    gd, sd = g.to(dev), _to(slabs, dev) if with_slabs else ()
    part = torch.full((L + 1,), -1.0, dtype=F64, device=dev)
    ops.grad_sumsq(gd, part, L, sd)
    again = torch.full((L + 1,), -1.0, dtype=F64, device=dev)
    ops.grad_sumsq(gd, again, L, sd)
    assert torch.equal(part, again)  # no atomics: a function of the data and L
    assert float(part[L]) == -1.0  # L partial sums, no more
    assert bool((part[:L] >= 0).all())
    if L * 256 > n // 4:  # workgroups without elements wrote zero
        assert int((part[-(-(n // 4) // 256): L] != 0).sum()) == 0
    got = float(part[:L].sum())
    # every term is an exact fp64 square and non-negative: any summation order is within n * 2^-53
    tol = max(n * 2.0 ** -53, 1e-9)
    print(f"grad_sumsq n={n} L={L} slabs={with_slabs}: rel err {abs(got - ref) / ref:.3e} (bound {tol:.1e})")
    assert abs(got - ref) <= tol * ref
    assert torch.equal(gd.cpu(), g)  # a read pass


def _check_fold_orders(g, slabs, dev, must_differ):
    """Both plane-fold orders of the dense clock, bit for bit against their CPU models (ops._fold_slabs):
    slab_pack ships the planes added one by one, an Adam consumes them in groups of four."""
    n = g.numel()
    seq, grouped = ops._fold_slabs(g, slabs, group4=False), ops._fold_slabs(g, slabs)
    differ = int((seq != grouped).sum())
    print(f"fold orders n={n} nsplit={[s[1] for s in slabs]}: {differ} elements differ")
    if must_differ:  # (not vacuous: this input tells the two orders apart)
        assert differ > 0
    ref_out, ref_src = torch.empty(n), g.clone()
    ops.slab_pack(ref_src, ref_out, slabs)
    assert torch.equal(ref_out, seq)
    src, out = g.to(dev), torch.empty(n, device=dev)
    ops.slab_pack(src, out, _to(slabs, dev))
    assert torch.equal(out.cpu(), ref_out) and int((src != 0).sum()) == 0
    # beta1 = 0 and m = 0: m = 0 * m + 1 * (g * 1) is the folded gradient itself, exactly
    w, m, v = (torch.zeros(n, device=dev) for _ in range(3))
    ops.adam_apply(w, m, v, g.to(dev), 1e-3, beta1=0.0, grad_scale=1.0, slabs=_to(slabs, dev))
    assert torch.equal(m.cpu(), grouped)


@pytest.mark.parametrize("nsplit", [3, 4, 5, 8, 16])
def test_slab_fold_orders_are_pinned(nsplit, dev):
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(64, generator=gen)
    slabs = [(torch.randn(nsplit * 16, generator=gen), nsplit, 16, 32)]
    _check_fold_orders(g, slabs, dev, must_differ=nsplit >= 5)


def test_slab_fold_orders_are_pinned_across_workgroups(gradients, dev):
    """The same at n = 4100 (several workgroups), regions of 1 / 3 / 5 / 8 planes at the start, in the
    middle and at the end."""
    g, slabs, _, _ = gradients[4100]
    _check_fold_orders(g, slabs, dev, must_differ=True)


def test_grad_sumsq_large_elements_stay_finite(dev):
    g = torch.randn(4100, generator=torch.Generator().manual_seed(5))
    g[::7] = 1e30
    part = torch.zeros(8, dtype=F64, device=dev)
    ops.grad_sumsq(g.to(dev), part)
    got, ref = float(part.sum()), float(g.double().square().sum())
    assert math.isfinite(got) and abs(got - ref) <= 1e-9 * ref
    # ... and a clock of such a gradient is clipped, not skipped
    w, m, v = (torch.zeros(4100, device=dev) for _ in range(3))
    stats = torch.zeros(4, dtype=F64, device=dev)
    ops.adam_clip_apply(w, m, v, g.to(dev), 1e-2, part, 1.0, stats)
    norm, scale, clipped, skipped = stats.tolist()
    assert (clipped, skipped) == (1.0, 0.0) and norm == pytest.approx(math.sqrt(ref), rel=1e-9)
    assert scale == pytest.approx(1.0 / math.sqrt(ref), rel=1e-6) and bool(torch.isfinite(w).all())


def _adam_state(n, dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    w, m, v, gr = (torch.randn(n, generator=g) for _ in range(4))
    return [t.to(dev) for t in (w, m, v.abs())], gr


HYPER = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01)


@pytest.mark.parametrize("step_dev", [False, True], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("with_slabs", [False, True], ids=["plain", "slabs"])
@pytest.mark.parametrize("max_norm", [1e9, 0.5], ids=["below", "above"])
def test_adam_clip_apply_is_adam_apply_at_its_scale(max_norm, with_slabs, step_dev, dev):
    """Bit-identical to adam_apply(grad_scale = the scale the kernel derived): w, m, v, the bf16 copy and
    the cleared gradient; the scale is 1 below the threshold and the rule's value (1e-6 relative) above."""
    n = 4100
    st_a, gr = _adam_state(n, dev)
    st_b = [t.clone() for t in st_a]
    slabs = _regions(n, seed=1) if with_slabs else ()
    ga, gb = gr.to(dev), gr.to(dev)
    wa, wb = (torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(2))
    sd = torch.tensor([3], dtype=torch.int32, device=dev) if step_dev else None
    part = torch.zeros(16, dtype=F64, device=dev)
    stats = torch.zeros(4, dtype=F64, device=dev)
    ops.grad_sumsq(ga, part, slabs=_to(slabs, dev))
    ops.adam_clip_apply(*st_a, ga, 1e-2, part, max_norm, stats, step=1 if step_dev else 3, w_bf16=wa, step_dev=sd,
                        zero_g=True, slabs=_to(slabs, dev), **HYPER)
    norm, scale, clipped, skipped = stats.tolist()
    total = float(ops._fold_slabs(gr, slabs).double().square().sum())
    ref_norm, ref_scale, _ = ops.clip_scale(total, max_norm)
    assert norm == pytest.approx(ref_norm, rel=1e-9) and skipped == 0.0
    if max_norm > ref_norm:
        assert scale == 1.0 and clipped == 0.0
    else:
        assert clipped == 1.0 and scale < 1.0 and abs(scale - ref_scale) <= 1e-6 * ref_scale
        assert scale == float(torch.tensor(scale, dtype=torch.float32))  # an fp32 value
    ops.adam_apply(*st_b, gb, 1e-2, step=1 if step_dev else 3, grad_scale=scale, w_bf16=wb, step_dev=sd, zero_g=True,
                   slabs=_to(slabs, dev), **HYPER)
    for name, a, b in zip(("w", "m", "v", "w_bf16", "g"), st_a + [wa, ga], st_b + [wb, gb]):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    assert int((ga != 0).sum()) == 0


@pytest.mark.parametrize("where", ["nan_in_g", "inf_in_slab"])
@pytest.mark.parametrize("zero_g", [True, False])
def test_non_finite_gradient_skips_the_clock(where, zero_g, dev):
    n = 4100
    st, gr = _adam_state(n, dev)
    before = [t.clone() for t in st]
    slabs = _regions(n, seed=2)
    if where == "nan_in_g":
        gr[n - 3] = float("nan")
    else:
        slabs[2][0][7] = float("inf")
    g = gr.to(dev)
    wb = torch.full((n,), 3.0, dtype=torch.bfloat16, device=dev)
    part = torch.zeros(16, dtype=F64, device=dev)
    stats = torch.tensor([0.0, 0.0, 5.0, 2.0], dtype=F64, device=dev)
    ops.grad_sumsq(g, part, slabs=_to(slabs, dev))
    assert not math.isfinite(float(part.sum()))
    ops.adam_clip_apply(*st, g, 1e-2, part, 1.0, stats, step=3, w_bf16=wb, zero_g=zero_g, slabs=_to(slabs, dev),
                        **HYPER)
    for a, b in zip(st, before):
        assert torch.equal(a, b)
    assert bool((wb == 3.0).all())
    norm, scale, clipped, skipped = stats.tolist()
    assert not math.isfinite(norm) and (scale, clipped, skipped) == (0.0, 5.0, 3.0)
    if zero_g:  # cleared all the same: the NaN must not survive into the next accumulation
        assert int((g != 0).sum()) == 0 and not bool(torch.isnan(g).any())
    else:
        assert torch.equal(torch.nan_to_num(g.cpu(), nan=7.0), torch.nan_to_num(gr, nan=7.0))


def test_write_stats_off_and_one_scale_for_every_launch(dev):
    """Two launches over different slices of one buffer (two buckets of a clock) with the same partial sums
    derive the same scale; a launch with write_stats off leaves stats alone."""
    n, cut = 4100, 2048
    st, gr = _adam_state(n, dev)
    ref = [t.clone() for t in st]
    g, g2 = gr.to(dev), gr.to(dev)
    part = torch.zeros(24, dtype=F64, device=dev)
    ops.grad_sumsq(g[:cut], part[:8], 8)
    ops.grad_sumsq(g[cut:], part[8:], 16)
    s0, s1 = (torch.full((4,), -2.0, dtype=F64, device=dev) for _ in range(2))
    quiet = s0.clone()
    ops.adam_clip_apply(*(t[:cut] for t in st), g[:cut], 1e-2, part, 0.25, s0, step=2, **HYPER)
    ops.adam_clip_apply(*(t[cut:] for t in st), g[cut:], 1e-2, part, 0.25, s1, step=2, **HYPER)
    assert s0[:2].tolist() == s1[:2].tolist() and 0.0 < float(s0[1]) < 1.0
    ops.adam_clip_apply(*(t.clone() for t in st), g.clone(), 1e-2, part, 0.25, quiet, step=2, write_stats=False,
                        **HYPER)
    assert quiet.tolist() == [-2.0] * 4
    # the two slices together are one Adam over the whole buffer at that scale
    ops.adam_apply(*ref, g2, 1e-2, step=2, grad_scale=float(s0[1]), **HYPER)
    for a, b in zip(st, ref):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ table and models
def test_clipped_table_gpu_matches_cpu(dev):
    from minips_amd.ps.comm import Comm
    from minips_amd.ps.tables import DenseTable

    n = 5000
    res = {}
    for d in (torch.device("cpu"), dev):
        t = DenseTable(Comm(device=d), n, optimizer="adam", lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01,
                       clip_norm=60.0)
        t.load_full(torch.linspace(-1, 1, n))
        g = torch.Generator().manual_seed(3)
        norms = []
        for i in range(5):
            t.add((torch.randn(n, generator=g) * (0.4 + 0.2 * i)).to(d))
            t.clock()
            norms.append(t.clip_stats()["norm"])
        res[d.type] = (t.full_master().cpu(), norms, t.clip_stats(), int((t.grad != 0).sum()))
    (wc, nc, sc, zc), (wg, ng, sg, zg) = res["cpu"], res["cuda"]
    assert ng == pytest.approx(nc, rel=1e-9) and zc == zg == 0
    assert sg["clipped"] == sc["clipped"] and 0 < sc["clipped"] < 5 and sg["skipped"] == 0
    torch.testing.assert_close(wg, wc, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("overlap_w1", [False, True], ids=["flat", "overlap_w1"])
def test_gpt2_clipped_gpu_matches_cpu(overlap_w1, dev):
    """GPT-2 (tiny) with every clock clipped: the GPU training (one Adam, or per-layer buckets on the clock
    stream) against the CPU reference ops, at test_gpt2_layer_buckets_world1_match_gpu's tolerances."""
    from minips_amd.models.gpt2 import GPT2, GPT2Config
    from minips_amd.ps.comm import Comm

    res = {}
    for d in ("cpu", dev):
        m = GPT2(GPT2Config(lr=1e-3, overlap_w1=overlap_w1, clip_norm=0.05, **TINY), Comm(device=torch.device(d)))
        if d != "cpu":
            assert (m.table.buckets is not None) == overlap_w1 and m.table.pipe.async_ == overlap_w1
        g = torch.Generator().manual_seed(2)
        tokens = torch.randint(0, 500, (2, 64), generator=g).to(d)
        targets = torch.roll(tokens, -1, 1)
        losses = [float(m.train_step(tokens, targets)) / tokens.numel() for _ in range(5)]
        m.drain()
        res[d == "cpu"] = (losses, m.table.full_master().cpu(), m.table.clip_stats())
    (l0, p0, s0), (l1, p1, s1) = res[True], res[False]
    print("gpt2 clipped: cpu", l0, s0, "gpu", l1, s1, "max |dp|", float((p0 - p1).abs().max()))
    assert s0["clipped"] == s1["clipped"] == 5 and s1["skipped"] == 0
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-3 * abs(a) + 1e-4, (l0, l1)
    assert float((p0 - p1).abs().max()) < 5 * 2e-3, float((p0 - p1).abs().max())


def _gpt2_clip_world(rank, world):
    """GPT-2 (tiny), bucketed and clipped, on `world` ranks of one card: each rank a slice of one batch."""
    from minips_amd.models.gpt2 import GPT2, GPT2Config
    from minips_amd.ps.comm import Comm

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    comm = Comm(device=dev)
    m = GPT2(GPT2Config(lr=1e-3, bucketed=True, clip_norm=0.05, **TINY), comm)
    assert m.table.buckets is not None and m.table.pipe.async_
    comm.trace = []
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 500, (4, 64), generator=g)
    targets = torch.roll(tokens, -1, 1)
    per = 4 // world
    sl = slice(rank * per, (rank + 1) * per)
    norms = []
    for _ in range(4):
        m.train_step(tokens[sl].to(dev), targets[sl].to(dev))
        norms.append(m.table.clip_stats()["norm"])
    m.drain()
    trace = [op for op, _, _ in comm.trace]
    out = (m.table.full_master().cpu().numpy(), norms, m.table.clip_stats(), trace)  # (pickled by value)
    torch.cuda.synchronize()
    return out


def test_gpt2_clipped_two_ranks_match_one(dev):
    one = run_world(_gpt2_clip_world, world=1)[0]
    two = run_world(_gpt2_clip_world, world=2)
    (p0, n0, s0, t0), (p1, n1, s1, t1) = two[0], two[1]
    assert n0 == n1 and t0 == t1  # the norm bit for bit, the same collective sequence
    assert t0.count("all_reduce") == 4 and s0["clipped"] == s1["clipped"] == one[2]["clipped"] == 4
    assert n0 == pytest.approx(one[1], rel=2e-2), (n0, one[1])  # (bf16 GEMMs on half the batch each)
    assert (p0 == p1).all()
    # test_gpt2_bucketed_clocks_gpu_streams' bound: Adam lr 1e-3 per step
    assert float(abs(p0 - one[0]).max()) < 4 * 2e-3, float(abs(p0 - one[0]).max())


def test_graphed_mlp_with_clipping_matches_eager(dev):
    from minips_amd.data.synthetic import MnistSynth
    from minips_amd.models.mlp import MLP, MLPConfig
    from minips_amd.ps.comm import Comm
    from minips_amd.utils.graph import GraphedStep

    data = MnistSynth(1024, device=dev, seed=4)
    batches = [data.next() for _ in range(10)]
    cfg = dict(clip_norm=0.05)
    eager = MLP(MLPConfig(**cfg), Comm(device=dev))
    graphed = MLP(MLPConfig(**cfg), Comm(device=dev))
    for _ in range(3):  # GraphedStep's 3 warm-up steps are real steps on the example batch
        eager.train_step(*batches[0])
    step = GraphedStep(lambda x, y: graphed.train_step(x, y)[0], batches[0], tables=[graphed.table])
    assert graphed.table.clip_stats()["clipped"] == 3  # the capture itself ran nothing
    le, lg = [], []
    for x, y in batches[1:]:
        le.append(float(eager.train_step(x, y)[0].item()))
        lg.append(float(step(x, y).item()))
    torch.cuda.synchronize()
    se, sg = eager.table.clip_stats(), graphed.table.clip_stats()
    assert sg["clipped"] == se["clipped"] == 3 + 9 and sg["skipped"] == 0  # the counters survive the replays
    assert sg["norm"] == pytest.approx(se["norm"], rel=1e-3) and sg["scale"] < 1.0
    assert graphed.table.step == eager.table.step
    assert lg == pytest.approx(le, rel=1e-3, abs=1e-3), (le, lg)
    torch.testing.assert_close(graphed.table.master, eager.table.master, rtol=1e-3, atol=1e-4)


def test_schedule_refuses_a_graph_capture(dev, monkeypatch):
    from minips_amd.ps.comm import Comm
    from minips_amd.ps.tables import DenseTable, LRSchedule

    t = DenseTable(Comm(device=dev), 256, lr_schedule=LRSchedule(warmup=4))
    t.add(torch.ones(256, device=dev))
    t.clock()  # eager: fine
    assert t.lr_at(2) == 1e-3 * 2 / 4
    # what a clock inside torch.cuda.graph() sees (nothing is captured here)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="lr_schedule"):
        t.lr_at(2)
