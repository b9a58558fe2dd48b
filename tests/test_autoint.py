"""AutoInt's interacting layers on the CPU (csrc/kernels/attnint.h states the rule; ops.wd_attn_* carry its fp32
references; WideDeepConfig(attn_layers=...) runs it).
The reference against fp64 autograd of the plain formula. Bound, norm-wise: along any path from an input to an output
lie at most R = 5 T + 1 roundings to bf16 (Q / K, P, V and the stored E^l per layer going up; dS, dQ / dK / dV and the
stored dE per layer coming down share the count; dE^T), each of relative size u = 2^-8 on terms whose absolute sum is at
most ||.||_1-bounded by m A max|ref| for the sums met here; the scores are kept small (e_s <= 0.05) so the softmax
amplifies a rounding by at most exp(0.1): |got - ref| <= 1.2 R u max|ref| element-wise. Then the model: default
untouched, layout, initial values, training, quality, refusals."""
import math

import pytest
import torch

from minips_amd import ops, train
from minips_amd.data.synthetic import CriteoSynth, FMSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

BF, U = torch.bfloat16, 2.0 ** -8
CARDS = [50, 7, 300, 20, 5, 60, 90, 10, 11, 12]
HID = (64, 32, 16)


def plain64(E, Ws, w_out, H, d, masks):
    """The AutoInt term from the definition, fp64: E [B, m, D], Ws[l] [Din_l, 4 A], w_out [m A]. The ReLU is taken
    with the given masks (where the path under test stored E^l > 0): a value that rounds across zero is itself within
    the bound of zero, but its gradient is not continuous there."""
    B, m, A = E.shape[0], E.shape[1], H * d
    for W, mask in zip(Ws, masks):
        Y = E @ W
        Q, K, V = (Y[..., i * A:(i + 1) * A].view(B, m, H, d).transpose(1, 2) for i in range(3))
        O = torch.softmax(Q @ K.transpose(-1, -2), -1) @ V
        E = (O.transpose(1, 2).reshape(B, m, A) + Y[..., 3 * A:]) * mask
    return E.reshape(B, -1) @ w_out


def test_reference_against_fp64_autograd():
    B, m, D, cfg = ops.ATTN_CHUNK + 5, 5, 8, (2, 2, 16)
    T, H, d = cfg
    g = torch.Generator().manual_seed(0)
    n = ops.wd_attn_layout(m, D, cfg)[1]
    Pc = torch.zeros(n, dtype=BF)
    Ws, w_out = ops.wd_attn_views(Pc, m, D, cfg)
    for W in Ws:
        W.copy_(torch.randn(W.shape, generator=g) / W.shape[0] ** 0.5)
        W[:, :2 * H * d] *= 0.4  # small scores: e_s <= 0.05
    w_out.copy_(torch.randn(w_out.shape, generator=g))
    X = torch.randn(B, m * D + 3, generator=g).to(BF)
    dz, wide0 = torch.randn(B, generator=g), torch.randn(B, generator=g)
    x64 = X[:, :m * D].double().view(B, m, D).requires_grad_()
    W64 = [W.double().requires_grad_() for W in Ws]
    wo64 = w_out.double().requires_grad_()
    bufs, wide = ops.wd_attn_buffers(B, m, D, cfg, "cpu"), wide0.clone()
    ops.wd_attn_forward(X, m, D, Pc, cfg, wide, bufs)
    ref = plain64(x64, W64, wo64, H, d, [(bufs["EK"][:, l] > 0).double() for l in range(T)])
    ref.backward(dz.double())
    dX, Gc = torch.zeros(B * m, D, dtype=BF), torch.zeros(n)
    ops.wd_attn_backward(X, m, D, Pc, cfg, dz, dX, bufs, Gc)
    tol = 1.2 * (5 * T + 1) * U
    pairs = [("wide", wide.double() - wide0.double(), ref.detach()), ("dX", dX.double().view(B, m, D), x64.grad),
             ("dw_out", ops.wd_attn_views(Gc, m, D, cfg)[1].double(), wo64.grad)]
    pairs += [(f"dW{l + 1}", G.double(), w.grad)
              for l, (G, w) in enumerate(zip(ops.wd_attn_views(Gc, m, D, cfg)[0], W64))]
    for name, got, want in pairs:
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name}: max error {err:.3e}, bound {tol * scale:.3e}")
        assert scale > 0 and err <= tol * scale, name


def _model(attn_layers, cards=CARDS, seed=0, **kw):
    return WideDeep(WideDeepConfig(cards=cards, hidden=HID, seed=seed, emb_dim=8, row_width=12,
                                   attn_layers=attn_layers, attn_heads=2, attn_dim=16, **kw),
                    Comm(device=torch.device("cpu")))


def test_default_is_unchanged_and_the_layers_move_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an AutoInt op ran without attn_layers")

    for name in [n for n in dir(ops) if n.startswith("wd_attn_")]:
        monkeypatch.setattr(ops, name, boom)
    assert WideDeepConfig(cards=CARDS).attn_layers == 0
    m = _model(0)
    data = CriteoSynth(64, cards=CARDS, seed=3)
    for _ in range(5):
        assert math.isfinite(float(m.train_step(*data.next())))
    m.evaluate(data.holdout(9).next() for _ in range(2))
    m.drain()
    assert all("attn" not in b for b in m._bufs.values())
    monkeypatch.undo()
    want = {"W1": (0, (64, 128)), "W2": (8192, (32, 64)), "b2": (10240, (32,)), "W3": (10304, (16, 32)),
            "b3": (10816, (16,)), "w4": (10880, (24,))}  # the parent's layout, 64-aligned
    assert m.layout == want and m.n_params == 10904
    on, both = _model(2), _model(2, cross_layers=2, fm_term=True, cin_layers=(16, 16))
    n_attn = ops.wd_attn_layout(10, 8, (2, 2, 16))[1]
    assert list(on.layout) == ["W1", "attn", "W2", "b2", "W3", "b3", "w4"]
    assert on.layout["attn"] == (64 * 128, (n_attn,))
    assert list(both.layout)[:4] == ["W1", "cross", "cin", "attn"] and on.n_params == m.n_params + n_attn
    base = _model(0, cross_layers=2, fm_term=True, cin_layers=(16, 16))
    for model, ref in ((on, _model(0)), (both, base)):
        full, old = model.dense.full_master(), ref.dense.full_master()
        for name, (o, shape) in ref.layout.items():  # every existing parameter keeps its initial value
            o2, k = model.layout[name][0], math.prod(shape)
            assert torch.equal(old[o: o + k], full[o2: o2 + k]), name
    init = both.dense.full_master().clone()
    for _ in range(20):  # every term on: AutoInt behind the DeepFM term, the cross layers and the CIN
        assert math.isfinite(float(both.train_step(*data.next())))
    both.drain()
    assert not torch.equal(both.view(both.dense.full_master(), "attn"), both.view(init, "attn"))


def _fm_teacher_logloss(attn_layers, seed=0, steps=100):
    F, card, B = 8, 32, 512
    data = FMSynth(B, fields=F, card=card, seed=seed)
    m = _model(attn_layers, cards=[card] * F, seed=seed)

    def batch(gen):
        _, cols, _, y = gen.next()
        return torch.zeros(B, m.cfg.n_dense), cols.view(B, F), y

    for _ in range(steps):
        m.train_step(*batch(data))
    return m.evaluate(batch(data.holdout(777 + seed)) for _ in range(8))["logloss"]


def test_what_the_layers_buy():  # the DeepFM / DCN / CIN tests' FM-teacher setup at emb_dim 8; reported, not ranked
    wd, att = _fm_teacher_logloss(0), _fm_teacher_logloss(2)
    print(f"held-out log loss: Wide&Deep {wd:.4f}, with attn_layers=2 (2 heads of 16) {att:.4f}")
    assert att < math.log(2)


@pytest.mark.parametrize("kw", [dict(attn_layers=4), dict(attn_layers=1, attn_dim=8),
                                dict(attn_layers=1, attn_heads=3), dict(attn_layers=1, attn_heads=0),
                                dict(attn_layers=1, emb_dim=12, row_width=16),
                                dict(attn_layers=1, cards=[5] * 33), dict(attn_layers=1, transport="onesided"),
                                dict(attn_layers=1, consistency="ssp", staleness=1, transport="auto")])
def test_refusals(kw):
    with pytest.raises(ValueError, match="attn_layers"):
        WideDeepConfig(**{"cards": CARDS, **kw})


@pytest.mark.parametrize("argv", ["widedeep --attn_layers 2", "xdeepfm --attn_dim 16", "autoint --consistency ssp",
                                  "autoint --attn_dim 8", "autoint --transport onesided", "autoint --attn_layers 4"])
def test_the_driver_refuses(argv, capsys):
    with pytest.raises(SystemExit):
        train.parse(["--model"] + argv.split())
    assert "attn_" in capsys.readouterr().err


def test_the_driver_accepts():
    a = train.parse(["--model", "autoint", "--wide_optimizer", "ftrl", "--eval_every", "5"])
    assert (a.attn_layers, a.attn_heads, a.attn_dim, a.transport) == (3, 2, 32, "collective")
