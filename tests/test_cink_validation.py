"""Argument validation of the _cink binding (csrc/bindings/cin_py.cpp), test_kmk_validation.py's harness: a mutation
of a tiny valid argument set raises RuntimeError naming the argument and launches nothing; CPU tensors are refused."""
import types

import pytest
import torch

from test_w2vk_validation import F32, I32, _bytes, _names, _t, _tensors, pinned, short, strided, value, wider

from minips_amd import _native, ops

BF = torch.bfloat16
B, F, D, LAYERS = 3, 3, 8, [16, 32]
HS, MP = sum(LAYERS), 8


def _common(d):
    g = torch.Generator().manual_seed(0)
    return dict(X=torch.randn(B, F * D + 8, generator=g).to(BF).to(d),
                XK=torch.randn(B, HS, D, generator=g).to(BF).to(d),
                dXK=torch.randn(B, HS, D, generator=g).to(BF).to(d), W=_t(d, (32, 16, MP), BF, 0.1),
                w_out=_t(d, (HS,), BF, 0.5), dwide=_t(d, (B,), F32, 1.0))


def _bf(shape):
    return value(lambda dv: _t(dv, shape, BF))


_STACK = (pinned, strided, short, _bf((B, HS, D + 8)), value(lambda dv: _t(dv, (B, HS, D), F32)))
_X = (pinned, _bf((B, F * D - 8)), value(lambda dv: _t(dv, (B, F * D + 8), F32)), _bf((B * F * D,)))
_WOUT = (pinned, short, value(lambda dv: _t(dv, (HS,), F32)))
_DWIDE = (wider, pinned, strided, short)
_BLOCKS = (value(-1), value(65536))
_SHAPE = dict(F=(value(0), value(65)), D=(value(4), value(12), value(16)),
              layers=(value([]), value([16, 24]), value([16, 32, 16, 16]), value([16, 256])), k=(value(0), value(3)))


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _forward(d):
    c = _common(d)
    a = dict(X=c["X"], F=F, D=D, W=c["W"], layers=LAYERS, k=2, XK=c["XK"], blocks=0)
    per = dict(X=_X, W=(pinned, short, _bf((32, 16, MP + 8)), value(lambda dv: _t(dv, (32, 16, MP), F32))), XK=_STACK,
               blocks=_BLOCKS, **_SHAPE)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _output(d):
    c = _common(d)
    a = dict(XK=c["XK"], w_out=c["w_out"], wide=_t(d, (B,), F32, 9.0), p=_t(d, (B, HS), F32, 9.0), blocks=0)
    per = dict(XK=(pinned, strided, _bf((B, HS, 12)), value(lambda dv: _t(dv, (B, HS, D), F32))), w_out=_WOUT,
               wide=_DWIDE, p=(wider, pinned, strided, short), blocks=_BLOCKS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _backward(d):
    c = _common(d)
    a = dict(X=c["X"], F=F, D=D, W=c["W"], layers=LAYERS, k=2, XK=c["XK"], dXK=c["dXK"], w_out=c["w_out"],
             dwide=c["dwide"], g0=_t(d, (B, F, D), F32, 9.0), perm=torch.arange(B * F, dtype=I32, device=d),
             dX=_t(d, (B * F, D), BF, 1.0), blocks=0)
    per = dict(X=_X, W=(pinned, short), XK=_STACK, dXK=_STACK, w_out=_WOUT, dwide=_DWIDE,
               g0=(wider, pinned, strided, short), perm=(wider, pinned, short),
               dX=(pinned, strided, short, value(lambda dv: _t(dv, (B * F, D), F32))), blocks=_BLOCKS, **_SHAPE)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _wgrad(d):
    c = _common(d)
    a = dict(X=c["X"], F=F, D=D, layers=LAYERS, k=2, XK=c["XK"], dXK=c["dXK"], w_out=c["w_out"], dwide=c["dwide"],
             part=_t(d, (1, 32, 16 * MP), F32, 9.0))
    per = dict(X=_X, XK=_STACK, dXK=_STACK, w_out=_WOUT, dwide=_DWIDE,
               part=(wider, pinned, value(lambda dv: _t(dv, (1, 32, 16 * MP + 8), F32))), **_SHAPE)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _wout(d):
    a = dict(dwide=_t(d, (B,), F32, 1.0), p=_t(d, (B, HS), F32, 2.0), part=_t(d, (1, HS), F32, 9.0))
    per = dict(dwide=_DWIDE, p=(wider, pinned, strided, value(lambda dv: _t(dv, (B, 8), F32))),
               part=(wider, pinned, value(lambda dv: _t(dv, (2, HS), F32))))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _fold(d):
    a = dict(part=_t(d, (2, 40), F32, 1.0), G=_t(d, (40,), F32, 9.0))
    per = dict(part=(wider, pinned, strided, value(lambda dv: _t(dv, (65, 40), F32))), G=(wider, pinned, short))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


TABLE = dict(wd_cin_layer_forward=_forward, wd_cin_output=_output, wd_cin_layer_backward=_backward,
             wd_cin_layer_wgrad=_wgrad, wd_cin_wout_partial=_wout, wd_cin_fold=_fold)


_CASES = [pytest.param(n, i, id=f"{n}-{m[0]}-{i}") for n in sorted(TABLE)
          for i, m in enumerate(TABLE[n](torch.device("cpu"))[1])]


def test_every_exported_op_is_in_the_table():
    K_ = _native.cink()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE), sorted(exported ^ set(TABLE))
    assert all(n.startswith("wd_cin_") for n in exported) and _native.cink_available()
    assert (K_.MAX_T, K_.MAX_H, K_.MAX_F, K_.MAX_D, K_.CHUNK, K_.MAX_CHUNKS) == (
        ops.CIN_MAX_T, ops.CIN_MAX_H, ops.CIN_MAX_F, ops.CIN_MAX_D, ops.CIN_CHUNK, ops.CIN_MAX_CHUNKS)
    for other in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
                  _native.fmk(), _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak(),
                  _native.w2vk(), _native.alsk(), _native.gmmk(), _native.gmmfk(), _native.ibsk(), _native.kmk()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    for name in sorted(TABLE):
        getattr(_native.cink(), name)(*TABLE[name](dev)[0].values())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _CASES)
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.cink(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.cink(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
