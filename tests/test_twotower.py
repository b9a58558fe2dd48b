"""Two-tower retrieval on the CPU: the references ops.ibs_* against fp64 autograd of the rule with explicit masks,
reproducible training and checkpoints, learning of PairSynth's teacher against the untrained and the popularity-only
baselines, two ranks over gloo against one rank, and every refusal and driver flag."""
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import PairSynth
from minips_amd.models.twotower import TwoTower, TwoTowerConfig
from minips_amd.ps.comm import Comm
from minips_amd.train import parse

CPU = torch.device("cpu")


def rule64(inv, rows, d, tau, logq, unmask_hits=False):
    """(loss, lse, s, live) of the rule in csrc/kernels/ibs.h on the dtype of ``rows`` (fp64 in the tests)."""
    P, cap = inv.numel() // 2, rows.shape[0]
    u, it = inv.view(P, 2)[:, 0], inv.view(P, 2)[:, 1]
    valid = (u >= 0) & (u < cap) & (it >= 0) & (it < cap)
    A, B = rows[u.clamp(0, cap - 1)][:, :d], rows[it.clamp(0, cap - 1)][:, :d]
    s = A @ B.t() / tau - (0 if logq is None else logq.to(rows.dtype)[None, :])
    eye = torch.eye(P, dtype=torch.bool, device=inv.device)
    live = valid[:, None] & valid[None, :] & (eye | (it[:, None] != it[None, :]) | unmask_hits)
    lse = torch.logsumexp(s.masked_fill(~live, -math.inf), 1)
    lse = torch.where(valid, lse, torch.zeros_like(lse))
    loss = torch.where(valid, lse - s.diagonal(), torch.zeros_like(lse))
    return loss, lse, s, live


def _case(P, d, cap_u=7, cap_i=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    inv = torch.stack([torch.randint(0, cap_u, (P,), generator=g),
                       cap_u + torch.randint(0, cap_i, (P,), generator=g)], 1).reshape(-1)
    inv[3] = -1  # pair 1's item: the pair is invalid, its user lookup contributes nothing
    rows = torch.randn(cap_u + cap_i + 1, d + 4, generator=g) * 0.5  # (one row without lookups, padded ld)
    return inv, rows, torch.randn(P, generator=g) * 0.3 - 2.0


@pytest.mark.parametrize("d,logq", [(8, True), (20, False)])
def test_cpu_ops_match_fp64_autograd(d, logq):
    inv, rows, lq = _case(23, d)[:2] + (_case(23, d)[2] if logq else None,)
    tau, gscale = 0.25, 1.0 / 23
    loss, lse = ops.ibs_forward(inv, rows, d, tau, lq)
    grad = torch.full((rows.shape[0], d), 7.0)
    ops.ibs_backward(inv, rows, d, tau, lse, grad, lq, gscale)
    r64 = rows.double().requires_grad_()
    loss64, lse64, s, live = rule64(inv, r64, d, tau, lq)
    (loss64.sum() * gscale).backward()
    assert int((live.sum(1) < live.diagonal().sum()).sum()) > 0  # there are accidental hits
    assert (loss - loss64).abs().max() <= 1e-5 * loss64.abs().max() and float(loss[1]) == 0 == float(lse[1])
    assert (lse - lse64.detach()).abs().max() <= 1e-5 * lse64.abs().max()
    touched = torch.zeros(rows.shape[0], dtype=torch.bool)
    touched[inv[inv >= 0]] = True
    g64 = r64.grad[:, :d]
    assert (grad[touched] - g64[touched]).abs().max() <= 1e-5 * g64.abs().max()
    assert bool((grad[~touched] == 7.0).all()) and int((~touched).sum()) >= 1


def _model(seed=3, dev=CPU, **kw):
    kw = dict(dict(users=40, items=24, dim=8, tau=0.25, lr=0.1, seed=seed), **kw)
    return TwoTower(TwoTowerConfig(**kw), Comm(device=dev))


def test_training_is_reproducible_and_checkpoints_are_bit_exact(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    synth = PairSynth(40, 24, 3, batch=50, seed=1, zipf=1.0)
    batches = [synth.next() for _ in range(6)]

    def run(m, bs):
        m.set_item_counts(synth.item_counts())
        return [float(m.train_step(*b)) for b in bs]

    a, b = _model(), _model()
    assert run(a, batches[:3]) == run(b, batches[:3]) and torch.equal(a.table.shard, b.table.shard)
    a.drain()
    Checkpointer(a.comm, str(tmp_path / "ck_")).save({0: a.table}, iteration=3, blocking=True)
    c = _model(seed=11)
    assert Checkpointer(c.comm, str(tmp_path / "ck_")).load({0: c.table}) == 3
    assert torch.equal(a.table.shard, c.table.shard)
    assert run(a, batches[3:]) == run(c, batches[3:]) and torch.equal(a.table.shard, c.table.shard)
    before = a.table.shard.clone()
    assert 0 < a.evaluate(batches[:2]) < 10 and torch.equal(a.table.shard, before)
    assert float(a.train_step(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))) == 0.0  # P = 0


def test_it_learns_the_teacher():
    P, items = 64, 48
    synth = PairSynth(96, items, 3, batch=P, seed=5, zipf=1.0, scale=3.0)
    m = TwoTower(TwoTowerConfig(users=96, items=items, dim=16, tau=0.25, lr=0.1, seed=2), Comm(device=CPU))
    counts = synth.item_counts()
    m.set_item_counts(counts)
    for _ in range(300):
        m.train_step(*synth.next())
    hold = synth.holdout(1)
    held = [hold.next() for _ in range(8)]
    got = m.evaluate(held)
    pop = 0.0
    for u, i in held:  # the popularity-only model: logits = log count_i, the same live rule and loss
        inv = torch.stack([torch.zeros_like(i), 1 + i], 1).reshape(-1)
        rows = torch.cat([torch.ones(1, 8), torch.log(counts.double() + 1).float()[:, None].expand(items, 8) / 8])
        pop += float(ops.ibs_forward(inv, rows.contiguous(), 8, 1.0)[0].mean()) / len(held)
    print(f"held-out in-batch loss: trained {got:.4f}, popularity only {pop:.4f}, untrained ln P {math.log(P):.4f}")
    assert got < math.log(P) and got < pop


def _tt_world(rank, world, steps=4, RU=30, RI=20, RD=12, RP=48):
    torch.set_num_threads(1)
    comm = Comm(device=CPU)
    m = TwoTower(TwoTowerConfig(users=RU, items=RI, dim=RD, tau=0.25, lr=0.1, seed=9), comm)
    t, g = m.table, torch.Generator().manual_seed(5)
    full = torch.zeros(RU + RI, RD)  # the same routed-space table at every world size
    full[t._route_keys(torch.arange(RU + RI))] = torch.randn(RU + RI, RD, generator=g) * 0.3
    t.shard[: t.rows_local].copy_(full[t.base: t.base + t.rows_local])
    m.set_item_counts(torch.randint(1, 50, (RI,), generator=g))
    u, i = torch.randint(0, RU, (RP,), generator=g), torch.randint(0, RI, (RP,), generator=g)
    losses = [float(m.train_step(u, i)) / RP for _ in range(steps)]  # every rank is fed the same pairs
    losses.append(m.evaluate([(u, i)]))
    m.drain()
    return losses


def test_two_ranks_fed_the_same_pairs_match_one_rank():
    many, one = run_world(_tt_world, world=2), _tt_world(0, 1)
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert one[-1] < one[0]


@pytest.mark.parametrize("kw", [dict(dim=6), dict(dim=4), dict(dim=132), dict(tau=0.0), dict(tau=-1.0),
                                dict(tau=float("nan")), dict(transport="onesided"), dict(storage="hash"),
                                dict(storage="map"), dict(value_dtype=torch.bfloat16), dict(pull_dtype=torch.bfloat16),
                                dict(users=0), dict(init_std=-1.0)])
def test_config_refusals_name_twotower(kw):
    with pytest.raises(ValueError, match="twotower"):
        TwoTowerConfig(**kw)


@pytest.mark.parametrize("bad", ["twotower --tt_dim 6", "twotower --tt_dim 132", "twotower --tt_tau 0",
                                 "twotower --tt_users 0", "twotower --transport onesided", "fm --tt_dim 16",
                                 "twotower --kStorageType Map", "twotower --value_dtype bfloat16", "lr --tt_items 8",
                                 "twotower --input x.libsvm", "w2v --tt_tau 0.1", "als --tt_users 8",
                                 "widedeep --tt_no_bias_correction"])
def test_driver_refusals(bad):
    with pytest.raises(SystemExit):
        parse(["--model"] + bad.split())

