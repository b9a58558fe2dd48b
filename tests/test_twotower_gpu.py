"""The in-batch sampled softmax kernels (csrc/kernels/ibs.hip) on the GPU against fp64, and the model against the CPU's.

The judge is derived, not fitted. The fp64 reference (test_twotower.rule64) evaluates the rule on the same fp32
inputs. With E = 2^-23 and the tree's (n + 16) E rule for an fp32 reduction of n terms:
  mag_pq = sum_i |a_pi b_qi| / tau + |logq_q|,   delta_pq = (d + 16) E mag_pq      (a logit: d products, 1 / tau, logq)
  |lse_p - lse64_p|   <= Delta_p = max_{q live} delta_pq + (P + 16) E     (the logits' shift, then a sum of <= P exps)
  |loss_p - loss64_p| <= Delta_p + delta_pp
The gradient sweeps recompute s_pq (within delta_pq) and read the forward's lse (within Delta_p), so pi_pq =
exp(s_pq - lse_p) carries the relative slack rho_p = expm1(Delta_p + max_q delta_pq); with Gm = (pi64 + I) gscale / tau
on the live entries (|pi - [p == q]| <= pi + 1)
  |dA - dA64| <= (rho Gm) |B| + (P + 16) E ((1 + rho) Gm) |B|       (the slack, then a sum of <= P fp32 terms)
and dB likewise with |A| and the transpose. A unique row sums its M member rows in member order: its bound is the sum
of its members' bounds plus (M + 16) E sum_m |member row 64|. The kernels' sums are plain fp32 chains (MFMA over d and
over the streamed pairs, the online softmax, the member walk, the chunk fold), so no term needs another form.
The inputs make the bound mean something: rows ~ N(0, 0.5 / sqrt(d)), so the logits have a standard deviation of 2 at
tau = 0.25; a dropped tile, a wrong mask or a swapped index moves lse by the order of 1, thousands of bounds --
asserted for one seeded mistake of the reference, un-masking the accidental hits."""
import functools
import math

import pytest
import torch

from test_twotower import rule64
from test_w2v_gpu import _csr

from minips_amd import _native, ops
from minips_amd.models.twotower import TwoTower, TwoTowerConfig
from minips_amd.ps.comm import Comm
from minips_amd.utils.syncaudit import SyncAudit

pytestmark = pytest.mark.gpu

E23 = 2.0 ** -23
TAU = 0.25
WORST = [0.0]  # the largest error / bound of this run (printed by every case)


def _inputs(P, d, hot=0):
    # users from 40 ids; items from 5 ids at P = 130 (many accidental hits, rows of ~26 members), else from 50; the
    # first ``hot`` pairs share one item; P = 65 carries two invalid pairs (inv -1 and cap)
    g = torch.Generator().manual_seed(1000 * P + d)
    nu, ni = 40, 5 if P == 130 else 50
    u, it = torch.randint(0, nu, (P,), generator=g), nu + torch.randint(0, ni, (P,), generator=g)
    if hot:
        it[:hot] = nu
    cap = nu + ni + 1  # (the last row has no lookup)
    inv = torch.stack([u, it], 1).reshape(-1)
    if P == 65:
        inv[2 * 7], inv[2 * 40 + 1] = -1, cap
    rows = torch.randn(cap, d, generator=g) * math.sqrt(0.5 / math.sqrt(d))
    logq = (torch.randn(P, generator=g) * 0.5 - 3.0) if (P + d // 4) % 2 == 0 else None
    return inv, rows, logq


@functools.lru_cache(maxsize=None)  # the inputs and their fp64 reference with its bounds, computed once a case
def _case(P, d, hot=0):
    inv, rows, logq = _inputs(P, d, hot)
    gscale, cap = 1.0 / P, rows.shape[0]
    r64 = rows.double()
    loss, lse, s, live = rule64(inv, r64, d, TAU, logq)
    iv = inv.view(P, 2)
    ok = (inv >= 0) & (inv < cap)
    valid = ok.view(P, 2).all(1)
    A = r64[iv[:, 0].clamp(0, cap - 1)] * valid[:, None]
    B = r64[iv[:, 1].clamp(0, cap - 1)] * valid[:, None]
    mag = A.abs() @ B.abs().t() / TAU + (0 if logq is None else logq.double().abs()[None, :])
    delta = (d + 16) * E23 * mag * live
    Delta = delta.max(1).values + (P + 16) * E23
    rho = torch.expm1(Delta + delta.max(1).values)
    pi = torch.exp(s.masked_fill(~live, -math.inf) - lse[:, None]) * valid[:, None]
    eye = torch.eye(P, dtype=torch.float64)
    G = (pi - eye * live) * gscale / TAU
    Gm = (pi + eye) * live * gscale / TAU
    sl, acc = rho[:, None] * Gm, (P + 16) * E23 * (1 + rho)[:, None] * Gm
    dA, dB = G @ B, G.t() @ A
    bA, bB = sl @ B.abs() + acc @ B.abs(), sl.t() @ A.abs() + acc.t() @ A.abs()
    lookups = torch.stack([dA, dB], 1).reshape(2 * P, d)      # row j: lookup j's gradient (zero for an invalid pair)
    lbound = torch.stack([bA, bB], 1).reshape(2 * P, d)
    M = torch.zeros(cap, dtype=torch.float64).index_add_(0, inv[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    grad = torch.zeros(cap, d, dtype=torch.float64).index_add_(0, inv[ok], lookups[ok])
    gb = torch.zeros(cap, d, dtype=torch.float64).index_add_(0, inv[ok], lbound[ok]) + \
        ((M + 16) * E23)[:, None] * torch.zeros(cap, d, dtype=torch.float64).index_add_(0, inv[ok], lookups[ok].abs())
    return dict(inv=inv, rows=rows, logq=logq, gscale=gscale, loss=loss, lse=lse, valid=valid, lse_b=Delta,
                loss_b=Delta + delta.diagonal(), grad=grad, grad_b=gb, touched=M > 0, M=M,
                lse_unmasked=rule64(inv, r64, d, TAU, logq, unmask_hits=True)[1])


def _place(rows, how, dev):
    # contiguous, ld = d + 4 (float4 loads still), or ld = d + 1 with the base off by 4 bytes (scalar staging); NaN pads
    cap, d = rows.shape
    if how == "contig":
        return rows.to(dev)
    ld = d + (4 if how == "pad4" else 1)
    flat = torch.full((cap * ld + 1,), float("nan"), device=dev)
    v = flat[(0 if how == "pad4" else 1):][: cap * ld].view(cap, ld)[:, :d]
    v.copy_(rows.to(dev))
    assert how == "pad4" or v.data_ptr() % 16 == 4
    return v


def _run(ref, dev, how="contig", blocks=0):
    d = ref["rows"].shape[1]
    inv, rows = ref["inv"].to(dev), _place(ref["rows"], how, dev)
    logq = None if ref["logq"] is None else ref["logq"].to(dev)
    loss, lse = ops.ibs_forward(inv, rows, d, TAU, logq, blocks=blocks)
    grad = torch.full((rows.shape[0], d), 7.0, device=dev)
    csr = tuple(t.to(dev) for t in _csr(ref["inv"], rows.shape[0]))  # members in lookup order (the device's: any)
    ops.ibs_backward(inv, rows, d, TAU, lse, grad, logq, ref["gscale"], csr=csr, blocks=blocks)
    return loss.cpu(), lse.cpu(), grad.cpu()


def _judge(ref, loss, lse, grad, what):
    worst = 0.0
    for name, got, want, bound in (("lse", lse, ref["lse"], ref["lse_b"]), ("loss", loss, ref["loss"], ref["loss_b"]),
                                   ("grad", grad[ref["touched"]], ref["grad"][ref["touched"]],
                                    ref["grad_b"][ref["touched"]])):
        ratio = float(((got.double() - want).abs() / bound.clamp(min=1e-300)).max()) if want.numel() else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: {name} misses its bound by {ratio:.3g}"
    assert bool((loss[~ref["valid"]] == 0).all()) and bool((lse[~ref["valid"]] == 0).all())
    assert bool((grad[~ref["touched"]] == 7.0).all()), "rows without lookups stay untouched"
    WORST[0] = max(WORST[0], worst)
    print(f"{what}: largest error / bound {worst:.4f} (run so far {WORST[0]:.4f})")


@pytest.mark.parametrize("d", [8, 20, 64, 128])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130, 200])
def test_kernels_within_the_derived_bound(P, d, dev):
    ref = _case(P, d)
    how = {8: "contig", 20: "pad4", 64: "odd", 128: "contig"}[d]
    _judge(ref, *_run(ref, dev, how), f"P {P} d {d} {how} logq {ref['logq'] is not None}")
    if P == 130:  # the mistake the bound must catch: the accidental hits counted as negatives
        miss = float(((ref["lse_unmasked"] - ref["lse"]).abs() / ref["lse_b"]).max())
        assert miss > 1000, miss
    assert int((~ref["valid"]).sum()) == (2 if P == 65 else 0)


def test_a_hot_item_takes_the_chunk_rule(dev):
    limit = _native.ibsk().WAVE_MAX
    P = int(1.1 * limit)
    ref = _case(P, 8, hot=limit + 8)
    assert float(ref["M"].max()) > limit
    _judge(ref, *_run(ref, dev), f"P {P} d 8, one item of {int(ref['M'].max())} members")


def test_same_bits_for_every_grid_and_run(dev):
    ref = _case(200, 20)
    base = _run(ref, dev, "pad4")
    for blocks in (1, 7, 0):
        for a, b in zip(base, _run(ref, dev, "pad4", blocks)):
            assert torch.equal(a, b), blocks


def _models(dev):
    ms = [TwoTower(TwoTowerConfig(users=40, items=12, dim=20, tau=TAU, lr=0.1, seed=4), Comm(device=dv))
          for dv in (torch.device("cpu"), dev)]
    ms[1].table.shard.copy_(ms[0].table.shard.to(dev))
    for m in ms:
        m.set_item_counts(torch.arange(1, 13))
    return ms


def _pairs(seed, dev, P=130):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 40, (P,), generator=g).to(dev), torch.randint(0, 12, (P,), generator=g).to(dev)


def test_model_matches_the_cpu_and_does_not_sync(dev):
    cpu, gpu = _models(dev)
    for s in range(3):
        a, b = float(cpu.train_step(*_pairs(s, "cpu"))) / 130, float(gpu.train_step(*_pairs(s, dev))) / 130
        print(f"step {s}: cpu {a:.6f} gpu {b:.6f}")
        assert abs(a - b) <= 3e-3 * max(1.0, abs(a))
    torch.cuda.synchronize()
    batches = [_pairs(10 + s, dev) for s in range(3)]
    with SyncAudit() as audit:
        for b in batches:
            audit.step_begin()
            gpu.train_step(*b)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep
    before = gpu.table.shard.clone()
    assert 0 < gpu.evaluate(batches) < 10 and torch.equal(gpu.table.shard, before)
