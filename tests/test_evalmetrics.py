"""Held-out evaluation metrics: ops.binary_hist / ops.eval_head (csrc/kernels/evalmetrics.hip, module
minips_amd._evalk) and utils.evalmetrics.BinaryEvaluator.

CPU part: the AUC formula against brute-force pair counts (exact, as fractions), the slack bound,
the edge cases of the per-sample rule with hand-written bins, and the exactness of updates and of
the cross-rank reduce. GPU part: the kernels against the CPU op, bit for bit on every count.
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _util import free_ports

from minips_amd import ops
from minips_amd.utils.evalmetrics import BinaryEvaluator

F32, I64 = torch.float32, torch.int64
INF, NAN = float("inf"), float("nan")


def _nudge(x, toward):
    return float(np.nextafter(np.float32(x), np.float32(toward)))


# (logit, expected bin as a function of NB; None: counted in n_nan) -- written by hand from the rule
# bin = min(NB-1, floor((clamp(z, -16, 16) + 16) * NB/32)):
#   16 - 1ulp = 16 - 2^-20; + 16 = 32 - 2^-20, a tie between 32 - 2^-19 and 32 -> even -> 32 -> NB -> NB-1
#   -16 + 1ulp: + 16 = 2^-20 exactly; * NB/32 <= 2^-12 -> bin 0
EDGES = [(INF, lambda nb: nb - 1), (-INF, lambda nb: 0), (16.0, lambda nb: nb - 1), (-16.0, lambda nb: 0),
         (_nudge(16.0, INF), lambda nb: nb - 1), (_nudge(16.0, 0.0), lambda nb: nb - 1),
         (_nudge(-16.0, -INF), lambda nb: 0), (_nudge(-16.0, 0.0), lambda nb: 0),
         (-0.0, lambda nb: nb // 2), (0.0, lambda nb: nb // 2), (NAN, None), (-NAN, None),
         (1e30, lambda nb: nb - 1), (-1e30, lambda nb: 0), (100.0, lambda nb: nb - 1), (-64.5, lambda nb: 0)]


def _py_bin(z, nb):
    """The bin of one fp32 logit with numpy scalars (independent of the torch implementation)."""
    zc = np.float32(min(max(np.float32(z), np.float32(-16.0)), np.float32(16.0)))
    t = np.float32(zc + np.float32(16.0)) * np.float32(nb // 32)
    return min(nb - 1, int(math.floor(float(t))))


def _pair_auc(scores, labels):
    """O(n^2) Mann-Whitney AUC as a Fraction; ties count 1/2."""
    pos = [s for s, y in zip(scores, labels) if y]
    neg = [s for s, y in zip(scores, labels) if not y]
    twice = sum(2 if p > q else (1 if p == q else 0) for p in pos for q in neg)
    return Fraction(twice, 2 * len(pos) * len(neg))


def _loss_tol(l):
    """Allowed |logloss - fp64 reference| for per-sample fp64 losses ``l``: the fixed-point quantisation (half a
    unit of 2^-24 per sample) + 8 fp32 ulps of the largest per-sample loss (expf / log1pf and the two adds)."""
    lmax = float(l.max())
    ulp = 2.0 ** (math.floor(math.log2(lmax)) - 23) if lmax > 0 else 2.0 ** -149
    return 2.0 ** -25 + 8 * ulp


def _acc(nb, device="cpu"):
    return torch.zeros(2 * nb + 2, dtype=I64, device=device)


# ---- CPU -----------------------------------------------------------------------------------------
def test_auc_is_the_exact_pair_count_and_the_slack_bound_holds():
    nb, n = 64, 257  # 0.5-wide bins: many ties
    g = torch.Generator().manual_seed(5)
    z = torch.randn(n, generator=g) * 3
    z[10:40] = z[40:70]  # forced duplicates
    z[70:110] = (torch.arange(40) - 20) * 0.5  # on bin edges
    z[110:115] = torch.tensor([16.0, -16.0, 20.0, -20.0, 0.0])
    y = (torch.rand(n, generator=g) < 0.4).float()
    ev = BinaryEvaluator("cpu", bins=nb)
    ev.update_logits(z, y)
    r = ev.result()
    labels = [v > 0.5 for v in y.tolist()]
    bins = [_py_bin(v, nb) for v in z.tolist()]
    want = _pair_auc(bins, labels)
    assert r["auc_exact"] == want
    assert r["auc"] == float(want) == want.numerator / want.denominator
    assert (r["n"], r["n_pos"], r["n_nan"]) == (n, sum(labels), 0)
    raw = _pair_auc(z.tolist(), labels)
    assert 0 < r["auc_slack"] < 0.1
    assert abs(want - raw) <= Fraction(r["auc_slack"]) + Fraction(1, 10**12)  # (the float of the exact slack)
    # log loss against fp64 (fixed-point quantisation 2^-25 per sample + fp32 rounding of the terms)
    zl = z.double().clamp(-64, 64)
    l = zl.clamp_min(0) - zl * y.double() + torch.log1p(torch.exp(-zl.abs()))
    assert abs(r["logloss"] - float(l.mean())) <= _loss_tol(l)


@pytest.mark.parametrize("nb", [32, 4096, 8192])
def test_edge_logits_land_in_the_bins_the_rule_says(nb):
    for z, want in EDGES:
        for label in (1.0, 0.0, -1.0):  # an LR-style -1 label is a negative
            acc = _acc(nb)
            ops.binary_hist(torch.tensor([z], dtype=F32), torch.tensor([label]), acc)
            a = acc.tolist()
            if want is None:
                assert a[2 * nb + 1] == 1 and sum(a[:2 * nb]) == 0 and a[2 * nb] == 0, (z, a[2 * nb:])
                continue
            side = nb if label > 0.5 else 0
            assert a[side + want(nb)] == 1 and sum(a[:2 * nb]) == 1 and a[2 * nb + 1] == 0, (z, label)
            assert _py_bin(z, nb) == want(nb)


def test_one_class_and_empty_inputs_have_no_auc():
    for labels in ([1.0] * 5, [0.0] * 5, []):
        ev = BinaryEvaluator("cpu", bins=32)
        ev.update_logits(torch.linspace(-1, 1, len(labels)), torch.tensor(labels))
        r = ev.result()
        assert r["auc"] is None and r["auc_slack"] is None and r["n"] == len(labels)
        assert (r["logloss"] is None) == (not labels)
    with pytest.raises(ValueError):
        BinaryEvaluator("cpu", bins=48)
    with pytest.raises(RuntimeError, match="acc"):
        ops.binary_hist(torch.zeros(1), torch.zeros(1), torch.zeros(2 * 48 + 2, dtype=I64))


def _data(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g) * 3
    z[::17] = NAN
    return z, (torch.rand(n, generator=g) < 0.3).float()


def test_two_updates_equal_one_update_on_the_concatenation():
    z, y = _data(1000)
    one, two = BinaryEvaluator("cpu", 256), BinaryEvaluator("cpu", 256)
    one.update_logits(z, y)
    two.update_logits(z[:333], y[:333])
    two.update_logits(z[333:], y[333:])
    assert torch.equal(one.acc, two.acc)
    two.reset()
    assert int(two.acc.abs().sum()) == 0


BIG = {5: (1 << 31) + 7, 300: (1 << 40) + 1, 2 * 256: (1 << 50) + 3, 2 * 256 + 1: (1 << 33) + 9}  # acc word -> count


def _reduce_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from minips_amd.ps.comm import Comm

        z, y = _data(1000)
        ev = BinaryEvaluator("cpu", 256)
        for i, v in BIG.items():  # counts above 2^31 / 2^32: an inexact transport (fp32, int32) would show
            ev.acc[i] = v + rank
        lo, hi = (0, 400) if rank == 0 else (400, 1000)
        ev.update_logits(z[lo:hi], y[lo:hi])
        ev.reduce(Comm(device=torch.device("cpu")))
        q.put((rank, ev.acc.tolist()))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "ERROR " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_reduce_over_two_gloo_ranks_is_exact():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_ports(1)[0]
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(2):
            r, v = q.get(timeout=120)
            out[r] = v
            if isinstance(v, str):
                break
    finally:
        for p in procs:
            p.join(timeout=30 if len(out) == 2 else 1)
            if p.is_alive():
                p.kill()
    assert not any(isinstance(v, str) for v in out.values()), out
    z, y = _data(1000)
    ref = BinaryEvaluator("cpu", 256)
    for i, v in BIG.items():
        ref.acc[i] = 2 * v + 1
    ref.update_logits(z, y)
    assert out[0] == out[1] == ref.acc.tolist()


# ---- GPU -----------------------------------------------------------------------------------------
def _edge_logits(n, g):
    z = torch.randn(n, generator=g) * 3
    e = torch.tensor([v for v, _ in EDGES], dtype=F32)
    k = min(n, len(e))
    z[:k] = e[:k]
    return z


def _check_hist(z, y, nb, dev):
    """GPU binary_hist == CPU op on every count; the loss within the derived bound of an fp64 reference."""
    ref, acc = _acc(nb), _acc(nb, dev)
    ops.binary_hist(z, y, ref)
    ops.binary_hist(z.to(dev), y.to(dev), acc)
    a = acc.cpu()
    assert torch.equal(a[:2 * nb], ref[:2 * nb])
    assert int(a[2 * nb + 1]) == int(ref[2 * nb + 1]) == int(torch.isnan(z).sum())
    ok = ~torch.isnan(z)
    n = int(ok.sum())
    if n:
        zl = z[ok].double().clamp(-64, 64)
        l = zl.clamp_min(0) - zl * (y[ok] > 0.5).double() + torch.log1p(torch.exp(-zl.abs()))
        tol = _loss_tol(l)
        got = int(a[2 * nb]) / 2 ** 24 / n
        print(f"binary_hist n={z.numel()} NB={nb}: logloss {got:.9f} ref {float(l.mean()):.9f} tol {tol:.3e}")
        assert abs(got - float(l.mean())) <= tol
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [32, 4096, 8192])
def test_binary_hist_is_bit_exact(nb, dev):
    g = torch.Generator().manual_seed(nb)
    for n in (1, 63, 64, 65, 4097):
        z = _edge_logits(n, g)
        y = (torch.rand(n, generator=g) < 0.4).float()
        y[::5] = -1.0
        _check_hist(z, y, nb, dev)
    # every sample in one bin (the hottest possible bin), and a grid of more than one workgroup per CU
    z = torch.full((4097,), 1.25)
    a = _check_hist(z, torch.ones(4097), nb, dev)
    assert int(a[nb + _py_bin(1.25, nb)]) == 4097
    z = torch.randn(200_000, generator=g) * 3
    _check_hist(z, (torch.rand(200_000, generator=g) < 0.25).float(), nb, dev)


@pytest.mark.gpu
def test_binary_hist_accumulates_across_calls(dev):
    g = torch.Generator().manual_seed(1)
    z, y = torch.randn(5000, generator=g) * 4, (torch.rand(5000, generator=g) < 0.5).float()
    one, two = _acc(4096, dev), _acc(4096, dev)
    ops.binary_hist(z.to(dev), y.to(dev), one)
    ops.binary_hist(z[:1234].to(dev), y[:1234].to(dev), two)
    ops.binary_hist(z[1234:].to(dev), y[1234:].to(dev), two)
    ops.binary_hist(z[:0].to(dev), y[:0].to(dev), two)  # n = 0: nothing launched
    assert torch.equal(one, two)


@pytest.mark.gpu
@pytest.mark.parametrize("Hd", [8, 64, 256, 1000])
def test_eval_head_matches_the_reference_and_the_standalone_path(Hd, dev):
    g = torch.Generator().manual_seed(Hd)
    nb = 4096
    for B in (1, 65, 1000):
        for padded in (False, True):
            for with_wide in (True, False):
                Hs = torch.randn(B, Hd + (24 if padded else 0), generator=g).to(torch.bfloat16)
                H = Hs[:, :Hd]  # ld > Hd: a padded view
                w = (torch.randn(Hd, generator=g) / Hd ** 0.5).to(torch.bfloat16)
                b0 = torch.tensor([0.25], dtype=torch.bfloat16)
                wide = torch.randn(B, generator=g) if with_wide else None
                y = (torch.rand(B, generator=g) < 0.4).float()
                zr, racc = torch.empty(B), _acc(nb)
                ops.eval_head(H, w, b0, wide, y, racc, zr)  # fp32 CPU reference of the same bf16 inputs
                acc, zo = _acc(nb, dev), torch.empty(B, device=dev)
                ops.eval_head(Hs.to(dev)[:, :Hd], w.to(dev), b0.to(dev), None if wide is None else wide.to(dev),
                              y.to(dev), acc, zo)
                torch.testing.assert_close(zo.cpu(), zr, rtol=2e-2, atol=1e-4)
                # the fused and the standalone path apply one rule: the same acc, bit for bit
                alone = _acc(nb, dev)
                ops.binary_hist(zo, y.to(dev), alone)
                assert torch.equal(acc, alone), (B, Hd, padded, with_wide)
                assert int(acc[:2 * nb].sum()) == B
                # without logits_out: the same acc again
                again = _acc(nb, dev)
                ops.eval_head(Hs.to(dev)[:, :Hd], w.to(dev), b0.to(dev), None if wide is None else wide.to(dev),
                              y.to(dev), again)
                assert torch.equal(acc, again)
