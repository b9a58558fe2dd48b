"""The ALS kernels (csrc/kernels/als.hip) on the GPU against fp64, and the model on the GPU against the CPU.

The judge is derived, not fitted. With u = 2^-24, A64 and b64 formed in fp64 from the same inputs and x the kernel's
result, the fp64 residual obeys

  ||b64 - A64 x||_2 <= u [ (n + 2) (trace(sum_j |a_j| y_j y_j^T) ||x||_2 + sum_j |c_j| ||y_j||_2)
                           + k (3k + 1) ||A64||_2 ||x||_2  +  2 sqrt(k) ||A64||_2 ||x||_2 ]

The first term is the rounding of forming A and b (n products and sums an entry, in any order: the MFMA's internal
order and the chunk fold are covered; a PSD matrix's 2-norm is at most its trace). The second is Higham's backward
error of a Cholesky solve, |dA| <= gamma_{3k+1} |R^T||R| with || |R^T||R| ||_2 <= k ||A||_2. The third is the two
roundings of adding gram0 and reg to the summed Gram matrix (each at most u |A_ij|, ||.||_F <= sqrt(k) ||.||_2). A
dropped member, a wrong triangle or a missing reg leaves a residual of the order of ||A|| ||x||: 1 / (k^2 u) times the
bound. delta is judged as x_out - x_old, bit for bit; als_gram entry by entry: |G - G64| <= (R + 2) u (|Y|^T |Y|)."""
import math

import pytest
import torch

from test_als import _als_world, _attach, _init_rows, case as _case, run, systems64
from test_multirank_gpu import run_world
from test_w2v_gpu import _layout

from minips_amd import ops
from minips_amd.data.synthetic import MFSynth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WORST = [0.0]  # the largest residual / bound of this run (printed by every case)


def _run(cs, dev, how="contig", **kw):
    return run(cs, dev, rows=_layout(cs["rows"], how, dev), **kw)


def _judge(cs, x_out, delta, gram0=None):
    k, slot, x_old = cs["k"], cs["slot"], cs["x_old"]
    sys64 = systems64(cs["rowptr"], cs["inv"], cs["a"], cs["c"], cs["rows"], cs["reg"], gram0)
    for e, (A, b, n) in enumerate(sys64):
        s = int(slot[e])
        if n == 0:  # the skip rule
            assert torch.equal(x_out[s], x_old[s]) and not delta[s].any(), e
            continue
        assert torch.equal(delta[s], x_out[s] - x_old[s]), e
        x = x_out[s].double()
        lo, hi = int(cs["rowptr"][e]), int(cs["rowptr"][e + 1])
        j = torch.arange(lo, hi)
        j = j[(cs["inv"][j] >= 0) & (cs["inv"][j] < cs["rows"].shape[0])]
        Y = cs["rows"][cs["inv"][j]].double()
        tr = float((cs["a"][j].double().abs() * (Y * Y).sum(1)).sum())
        cy = float((cs["c"][j].double().abs() * Y.norm(dim=1)).sum())
        nA, nx = float(torch.linalg.matrix_norm(A, 2)), float(x.norm())
        bound = U * ((n + 2) * (tr * nx + cy) + k * (3 * k + 1) * nA * nx + 2 * math.sqrt(k) * nA * nx)
        res = float((b - A @ x).norm())
        WORST[0] = max(WORST[0], res / bound)
        assert res <= bound, (e, n, res, bound)
    untouched = torch.ones(x_old.shape[0], dtype=torch.bool)
    untouched[slot] = False
    assert bool((x_out[untouched] == 7.0).all()) and bool((delta[untouched] == 7.0).all())
    print(f"largest residual / bound so far: {WORST[0]:.4f}")


EDGES = [0, 1, 3, 4, 63, 64, 65]   # the skip rule, the MFMA tail, the stage boundary


@pytest.mark.parametrize("k", [4, 16, 20, 64, 128])
@pytest.mark.parametrize("counts,with_gram", [(EDGES, False), ([3], True), ([4, 0, 65, 1, 64], True)])
def test_solve_against_fp64(k, counts, with_gram, dev):
    cs = _case(k, counts, seed=k + len(counts))
    Y = torch.randn(40, k, generator=torch.Generator().manual_seed(1)) * k ** -0.25
    gram0 = (Y.t() @ Y).contiguous() if with_gram else None
    x_out, delta, bad = _run(cs, dev, gram0=gram0)
    assert bad == 0
    _judge(cs, x_out, delta, gram0)


@pytest.mark.parametrize("k", [20, 128])
@pytest.mark.parametrize("counts", [[64], [65], [130], [130, 3, 5], [3, 5, 130]])
def test_chunked_entities_fold_in_order_and_repeat_bit_for_bit(k, counts, dev):
    """chunk = 64: one, two and three partials, a heavy entity first and last; forced grid sizes give the same bits."""
    cs = _case(k, counts, seed=7 * k + len(counts))
    x_out, delta, bad = _run(cs, dev, chunk=64)
    assert bad == 0
    _judge(cs, x_out, delta)
    for blocks in (1, 7):
        again = _run(cs, dev, chunk=64, blocks=blocks)
        assert torch.equal(again[0], x_out) and torch.equal(again[1], delta)


@pytest.mark.parametrize("k,how", [(20, "strided"), (20, "odd_ld"), (20, "misaligned"), (128, "strided"),
                                   (128, "misaligned")])
def test_row_layouts(k, how, dev):
    """ld = k + 4 keeps the float4 loads; ld = k + 1 and a base off by 4 bytes take the scalar staging loads."""
    cs = _case(k, [65, 3, 0, 64], seed=k)
    x_out, delta, bad = _run(cs, dev, how=how)
    assert bad == 0
    _judge(cs, x_out, delta)
    same = _run(cs, dev)
    assert torch.equal(same[0], x_out)  # only the loads differ


def test_a_negative_pivot_is_skipped_and_counted(dev):
    cs = _case(16, [5, 6], seed=2)
    cs["a"][:5], cs["reg"][0] = -1.0, 0.0   # entity 0's first pivot is -sum y^2 < 0
    cs["inv"][1] = 0
    x_out, delta, bad = _run(cs, dev)
    s = int(cs["slot"][0])
    assert bad == 1 and torch.equal(x_out[s], cs["x_old"][s]) and not delta[s].any()
    assert delta[int(cs["slot"][1])].any()


@pytest.mark.parametrize("R", [1, 65, 300])
@pytest.mark.parametrize("k,how", [(4, "contig"), (20, "odd_ld"), (128, "contig")])
def test_gram_against_fp64(R, k, how, dev):
    Y = torch.randn(R, k, generator=torch.Generator().manual_seed(R + k))
    G = ops.als_gram(_layout(Y, how, dev)).cpu().double()
    err = (G - Y.double().t() @ Y.double()).abs()
    bound = (R + 2) * U * (Y.double().abs().t() @ Y.double().abs())
    assert G.shape == (k, k) and torch.equal(G, G.t()) and bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(ops.als_gram(torch.empty(0, k, device=dev)).cpu(), torch.zeros(k, k))


# ------------------------------------------------------------------------------ the model
def _models(dev, implicit=False):
    from minips_amd.models.als import ALS, ALSConfig
    from minips_amd.ps.comm import Comm

    synth = MFSynth(users=96, items=40, k_teacher=3, per_user=12, noise=0.1, seed=4)
    if implicit:
        synth.vals = synth.vals.abs()
    cfg = ALSConfig(users=96, items=40, k=20, reg=0.05, implicit=implicit, alpha=4.0, batch_entities=32, chunk=16)
    out = []
    for d in (torch.device("cpu"), dev):
        m = _attach(ALS(cfg, Comm(device=d)), synth)
        _init_rows(m)
        out.append(m)
    return synth, out[0], out[1]


@pytest.mark.parametrize("implicit", [False, True])
def test_model_gpu_matches_cpu(implicit, dev):
    """chunk = 16 < 40 users an item at most: the item half runs the multi-chunk fold."""
    synth, cpu, gpu = _models(dev, implicit)
    hold = synth.holdout(0)
    for sweep in range(2):
        cpu.sweep(), gpu.sweep()
        rc, rg = cpu.rmse(*hold), gpu.rmse(*hold)
        print(f"sweep {sweep}: cpu {rc:.6f} gpu {rg:.6f}")
        assert abs(rg - rc) <= 3e-3 * max(1.0, abs(rc))
    cpu.drain(), gpu.drain()
    assert gpu.bad_total == 0 == cpu.bad_total


def test_steady_clock_has_no_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    _, _, gpu = _models(dev)
    gpu.sweep()  # warm-up: first plans, scratch allocations
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for side in ("users", "items", "users"):
            audit.step_begin()
            gpu.half_sweep(side)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep


def _als_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _als_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_match_one_rank(dev):
    many = run_world(_als_two_ranks_gpu, world=2)
    one = _als_world(0, 1, dev=dev)
    print(f"2 ranks on one card {many[0]} vs one rank {one}")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
