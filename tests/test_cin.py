"""xDeepFM's Compressed Interaction Network on the CPU (csrc/kernels/cin.h states the rule; ops.wd_cin_* carry its fp32
references; WideDeepConfig(cin_layers=...) runs it).
References against fp64 autograd of the direct triple sum, written with explicit loops over (i, j). Bounds: u = 2^-8;
along any path from an input to an output lie at most R = 3 T + 1 roundings to bf16 (z and X^k per layer going up, a
stored dX^k per layer coming down, dX^T), each of relative size u on a term bounded by the "abs companion" M -- the same
fp64 computation on absolute values: within 1.1 R u M, plus the fp32 sums' K 2^-23 M over the longest chain's K terms,
plus the output's own bf16 rounding where it has one. Then the model: default untouched, layout, checkpoints, two gloo
ranks, quality, refusals."""
import json
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops, train
from minips_amd.data.synthetic import CriteoSynth, FMSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

BF, U = torch.bfloat16, 2.0 ** -8
CARDS = [50, 7, 300, 20, 5, 60, 90, 10, 11, 12]
HID = (64, 32, 16)


def direct64(x0, Ws, w_out):
    """The CIN term from the definition: x0 [B, m, D], Ws[k] [H_k, H_{k-1}, m], w_out [sum H]."""
    out, xp, o = 0, x0, 0
    for W in Ws:
        xk = torch.zeros(x0.shape[0], W.shape[0], x0.shape[2], dtype=x0.dtype)
        for i in range(xp.shape[1]):
            for j in range(x0.shape[1]):
                xk = xk + W[:, i, j][None, :, None] * (xp[:, i] * x0[:, j])[:, None, :]
        out = out + (xk.sum(2) * w_out[o: o + W.shape[0]]).sum(1)
        xp, o = xk, o + W.shape[0]
    return out


@pytest.mark.parametrize("layers", [(16,), (16, 32)], ids=str)
def test_references_against_fp64(layers):
    B, m, D, T = 5, 3, 8, len(layers)
    g = torch.Generator().manual_seed(len(layers))
    X = torch.full((B, m * D + 5), float("nan"), dtype=BF)
    X[:, : m * D] = torch.randn(B, m * D, generator=g).to(BF)
    n = ops.wd_cin_layout(m, layers)[1]
    Pc = torch.zeros(n, dtype=BF)
    Ws, w_out = ops.wd_cin_views(Pc, m, layers)
    for W in Ws:
        W[:, :, :m] = ((torch.rand(W.shape[0], W.shape[1], m, generator=g) * 2 - 1) / math.sqrt(W.shape[1] * m)).to(BF)
    w_out.copy_((torch.randn(sum(layers), generator=g) * 0.5).to(BF))
    wide0, dz = torch.randn(B, generator=g), torch.randn(B, generator=g)
    ref = {}
    for tag, f in (("", lambda t: t), ("M_", torch.abs)):
        x0 = f(X[:, : m * D].double().view(B, m, D)).requires_grad_(True)
        W64 = [f(W[:, :, :m].double()).requires_grad_(True) for W in Ws]
        wo = f(w_out.double()).requires_grad_(True)
        out = direct64(x0, W64, wo)
        (out * f(dz.double())).sum().backward()
        ref.update({tag + "c": out.detach(), tag + "gx": x0.grad, tag + "dW": [w.grad for w in W64],
                    tag + "dwo": wo.grad})
    bufs = ops.wd_cin_buffers(B, m, D, layers, "cpu")
    wide = wide0.clone()
    ops.wd_cin_forward(X, m, D, Pc, layers, wide, bufs)
    dX, Gc = torch.zeros(B * m, D, dtype=BF), torch.zeros(n)
    ops.wd_cin_backward(X, m, D, Pc, layers, dz, dX, bufs, Gc)
    tol = 1.1 * (3 * T + 1) * U + (max(layers) * 8 * T + B * D + 64) * 2.0 ** -23
    assert bool(((wide.double() - wide0.double() - ref["c"]).abs() <= tol * ref["M_c"] + 2.0 ** -23 * wide.abs()).all())
    gx = dX.double().view(B, m, D)
    assert bool(((gx - ref["gx"]).abs() <= tol * ref["M_gx"] + U * ref["gx"].abs()).all())
    Gs, g_out = ops.wd_cin_views(Gc, m, layers)
    for G, dW, M in zip(Gs, ref["dW"], ref["M_dW"]):
        assert bool(((G[:, :, :m].double() - dW).abs() <= tol * M).all()) and float(dW.abs().max()) > 0
        assert bool((G[:, :, m:] == 0).all())  # the pad columns get a zero gradient
    assert bool(((g_out.double() - ref["dwo"]).abs() <= tol * ref["M_dwo"]).all())


def _model(cin_layers, cards=CARDS, seed=0, **kw):
    return WideDeep(WideDeepConfig(cards=cards, hidden=HID, seed=seed, emb_dim=8, row_width=12, cin_layers=cin_layers,
                                   **kw), Comm(device=torch.device("cpu")))


def test_default_is_unchanged_and_the_layers_move_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a CIN op ran without cin_layers")

    for name in [n for n in dir(ops) if n.startswith("wd_cin_")]:
        monkeypatch.setattr(ops, name, boom)
    assert WideDeepConfig(cards=CARDS).cin_layers == ()
    m = _model(())
    data = CriteoSynth(64, cards=CARDS, seed=3)
    for _ in range(5):
        assert math.isfinite(float(m.train_step(*data.next())))
    m.evaluate(data.holdout(9).next() for _ in range(2))
    m.drain()
    assert all("cin" not in b for b in m._bufs.values())
    monkeypatch.undo()
    want = {"W1": (0, (64, 128)), "W2": (8192, (32, 64)), "b2": (10240, (32,)), "W3": (10304, (16, 32)),
            "b3": (10816, (16,)), "w4": (10880, (24,))}  # the parent's layout, 64-aligned
    assert m.layout == want and m.n_params == 10904
    layers = (16, 32)
    on, both = _model(layers), _model(layers, cross_layers=2, fm_term=True)
    n_cin = ops.wd_cin_layout(10, layers)[1]
    assert list(on.layout) == ["W1", "cin", "W2", "b2", "W3", "b3", "w4"] and on.layout["cin"] == (64 * 128, (n_cin,))
    assert list(both.layout)[:3] == ["W1", "cross", "cin"] and on.n_params == m.n_params + n_cin
    m0, mc = _model(()).dense.full_master(), _model((), cross_layers=2).dense.full_master()
    for model, base, ref in ((on, _model(()), m0), (both, _model((), cross_layers=2), mc)):
        full = model.dense.full_master()
        for name, (o, shape) in base.layout.items():  # every existing parameter keeps its initial value
            o2, k = model.layout[name][0], math.prod(shape)
            assert torch.equal(ref[o: o + k], full[o2: o2 + k]), name
    init = both.dense.full_master().clone()
    for _ in range(20):  # every term on: the CIN behind the DeepFM term and the cross layers, one Adam point
        assert math.isfinite(float(both.train_step(*data.next())))
    both.drain()
    assert not torch.equal(both.view(both.dense.full_master(), "cin"), both.view(init, "cin"))
    for full in (init, both.dense.full_master()):
        Ws, w_out = ops.wd_cin_views(both.view(full, "cin"), 10, layers)
        assert all(bool((W[:, :, 10:] == 0).all()) and float(W[:, :, :10].std()) > 0 for W in Ws)
        assert float(w_out.abs().max()) <= 1 / math.sqrt(48) + 0.03


def test_checkpoints(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    data = CriteoSynth(64, cards=CARDS, seed=3)
    batches = [data.next() for _ in range(3)]
    prefix = str(tmp_path / "ck") + "/"
    a = _model((16, 16), fm_term=True, wide_optimizer="ftrl", wide_l1=0.5, wide_grad_scale=64.0)
    for b in batches[:2]:
        a.train_step(*b)
    a.drain()
    Checkpointer(a.comm, prefix).save({0: a.emb, 1: a.dense}, iteration=2, blocking=True)
    b_ = _model((16, 16), seed=1, fm_term=True, wide_optimizer="ftrl", wide_l1=0.5, wide_grad_scale=64.0)
    assert Checkpointer(b_.comm, prefix).load({0: b_.emb, 1: b_.dense}) == 2
    for ta, tb in ((a.emb, b_.emb), (a.dense, b_.dense)):  # every array of both tables, optimizer state included
        sa, sb = ta.shard_state()[1], tb.shard_state()[1]
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(b_.train_step(*batches[2]), a.train_step(*batches[2]))
    o = _model((16, 32), seed=1)  # another cin_layers is another n_params: refused
    with pytest.raises(ValueError, match="does not match"):
        Checkpointer(Comm(device=torch.device("cpu")), prefix).load({0: o.emb, 1: o.dense})


def _cin_run(rank, world, steps=4):
    torch.set_num_threads(1)
    m = _model((16, 16))
    g = torch.Generator().manual_seed(5)
    full = torch.randn(m.num_rows, m.cfg.row_width, generator=g) * 0.1
    full[:, m.cfg.emb_dim:] = 0
    m.emb.shard.copy_(full[m.emb.base: m.emb.base + m.emb.rows_local])
    total = 128
    data = CriteoSynth(total, cards=CARDS, device="cpu", seed=11)
    per, losses = total // world, []
    for _ in range(steps):
        dense, keys, y = data.next()
        sl = slice(rank * per, (rank + 1) * per)
        t = m.train_step(dense[sl], keys[sl], y[sl]).clone()
        m.comm.all_reduce_(t)
        losses.append(float(t) / total)
    return losses


def test_two_ranks_match_one_rank():
    many, one = run_world(_cin_run, world=2), _cin_run(0, 1)
    assert many[0] == many[1]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)


def _fm_teacher_logloss(cin_layers, seed=0, steps=100):
    F, card, B = 8, 32, 512
    data = FMSynth(B, fields=F, card=card, seed=seed)
    m = _model(cin_layers, cards=[card] * F, seed=seed)

    def batch(gen):
        _, cols, _, y = gen.next()
        return torch.zeros(B, m.cfg.n_dense), cols.view(B, F), y

    for _ in range(steps):
        m.train_step(*batch(data))
    return m.evaluate(batch(data.holdout(777 + seed)) for _ in range(8))["logloss"]


def test_what_the_layers_buy():  # the DeepFM / DCN tests' FM-teacher setup at emb_dim 8; reported, not ranked
    wd, cin = _fm_teacher_logloss(()), _fm_teacher_logloss((16, 16))
    print(f"held-out log loss: Wide&Deep {wd:.4f}, with cin_layers=(16, 16) {cin:.4f} ({cin / wd:.3f} x)")
    assert cin < math.log(2)


def test_refusals_and_the_driver(capsys, monkeypatch):
    for bad in ((8,), (24,), (144,), (16, 16, 16, 16), 16, (16.0,), (True,)):
        with pytest.raises(ValueError, match="cin_layers"):
            WideDeepConfig(cards=CARDS, cin_layers=bad)
    for kw in (dict(transport="onesided"), dict(consistency="ssp", staleness=1),
               dict(consistency="asp", dense_transport="onesided", transport="collective"),
               dict(emb_dim=12, row_width=16), dict(emb_dim=128, row_width=132), dict(cards=[5] * 65)):
        with pytest.raises(ValueError, match="cin_layers"):
            WideDeepConfig(**{"cards": CARDS, "cin_layers": (16,), **kw})
    WideDeepConfig(cards=[5] * 65, emb_dim=128, row_width=132)  # without the layers nothing is refused
    assert WideDeepConfig(cards=CARDS, cin_layers=[16, 128, 32], fm_term=True, cross_layers=2, consistency="ssp",
                          staleness=1, transport="collective", wide_optimizer="ftrl").cin_layers == (16, 128, 32)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert train.main(["--model", "xdeepfm", "--cin_layers", "16,16", "--small", "1", "--steps", "4", "--eval_every",
                       "2", "--wide_optimizer", "ftrl", "--ftrl_l1", "0.5"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["cin_layers"] == [16, 16] and out["model"] == "xdeepfm" and "wide_nnz" in out
    assert [e[0] for e in out["evals"]] == [2, 4] and all(math.isfinite(l) for _, l in out["losses"])
    assert train.parse(["--model", "xdeepfm"]).cin_layers == [64, 64]
    for argv in (("--model", "xdeepfm", "--consistency", "ssp"), ("--model", "xdeepfm", "--transport", "onesided"),
                 ("--model", "xdeepfm", "--cin_layers", "24"), ("--model", "xdeepfm", "--cin_layers", "16,x"),
                 ("--model", "widedeep", "--cin_layers", "16"), ("--model", "dcn", "--cin_layers", "16")):
        with pytest.raises(SystemExit) as e:
            train.parse(list(argv))
        assert e.value.code == 2 and ("xdeepfm" in capsys.readouterr().err)
