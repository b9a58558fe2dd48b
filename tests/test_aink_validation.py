"""Argument validation of the _aink binding (csrc/bindings/attn_py.cpp), test_cink_validation.py's harness: a mutation
of a tiny valid argument set raises RuntimeError naming the argument and launches nothing; CPU tensors are refused."""
import types

import pytest
import torch

from test_w2vk_validation import F32, I32, _bytes, _names, _t, _tensors, pinned, short, strided, value, wider

from minips_amd import _native, ops

BF = torch.bfloat16
B, F, D, T, H, HD = 3, 3, 8, 2, 1, 16
A = H * HD


def _common(d):
    g = torch.Generator().manual_seed(0)
    return dict(X=torch.randn(B, F * D + 8, generator=g).to(BF).to(d),
                EK=torch.randn(B, T, F, A, generator=g).to(BF).to(d),
                dEK=torch.randn(B, T, F, A, generator=g).to(BF).to(d), W=_t(d, (A, 4 * A), BF, 0.1),
                w_out=_t(d, (F * A,), BF, 0.5), dwide=_t(d, (B,), F32, 1.0))


def _bf(shape):
    return value(lambda dv: _t(dv, shape, BF))


_STACK = (pinned, strided, short, _bf((B, T, F, A + 8)), value(lambda dv: _t(dv, (B, T, F, A), F32)))
_X = (pinned, _bf((B, F * D - 8)), value(lambda dv: _t(dv, (B, F * D + 8), F32)), _bf((B * F * D,)))
_W = (pinned, short, _bf((A, 4 * A + 8)), value(lambda dv: _t(dv, (A, 4 * A), F32)))
_WOUT = (pinned, short, value(lambda dv: _t(dv, (F * A,), F32)))
_DWIDE = (wider, pinned, strided, short)
_BLOCKS = (value(-1), value(65536))
_SHAPE = dict(F=(value(0), value(33)), D=(value(4), value(12), value(72)), T=(value(0), value(4)),
              H=(value(0), value(5)), d=(value(8), value(64)), l=(value(0), value(3)))


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _forward(d):
    c = _common(d)
    a = dict(X=c["X"], F=F, D=D, W=c["W"], T=T, H=H, d=HD, l=2, EK=c["EK"], blocks=0)
    per = dict(X=_X, W=_W, EK=_STACK, blocks=_BLOCKS, **_SHAPE)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _output(d):
    c = _common(d)
    a = dict(EK=c["EK"], d=HD, w_out=c["w_out"], wide=_t(d, (B,), F32, 9.0), blocks=0)
    per = dict(EK=(pinned, strided, _bf((B, T, F, A + 8)), value(lambda dv: _t(dv, (B, T, F, A), F32))),
               d=(value(8), value(64)), w_out=_WOUT, wide=_DWIDE, blocks=_BLOCKS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _backward(d):
    c = _common(d)
    a = dict(X=c["X"], F=F, D=D, W=c["W"], T=T, H=H, d=HD, l=2, EK=c["EK"], dEK=c["dEK"], w_out=c["w_out"],
             dwide=c["dwide"], perm=torch.arange(B * F, dtype=I32, device=d), dX=_t(d, (B * F, D), BF, 1.0),
             part=_t(d, (1, A, 4 * A), F32, 9.0), blocks=0)
    per = dict(X=_X, W=_W, EK=_STACK, dEK=_STACK, w_out=_WOUT, dwide=_DWIDE, perm=(wider, pinned, short),
               dX=(pinned, strided, short, value(lambda dv: _t(dv, (B * F, D), F32))),
               part=(wider, pinned, value(lambda dv: _t(dv, (2, A, 4 * A), F32))), blocks=_BLOCKS, **_SHAPE)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _wout(d):
    c = _common(d)
    a = dict(EK=c["EK"], d=HD, dwide=c["dwide"], part=_t(d, (1, F * A), F32, 9.0))
    per = dict(EK=(pinned, strided, value(lambda dv: _t(dv, (B, T, F, A), F32))), d=(value(8), value(64)),
               dwide=_DWIDE, part=(wider, pinned, value(lambda dv: _t(dv, (2, F * A), F32))))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _fold(d):
    a = dict(part=_t(d, (2, 40), F32, 1.0), G=_t(d, (40,), F32, 9.0))
    per = dict(part=(wider, pinned, strided, value(lambda dv: _t(dv, (513, 40), F32))), G=(wider, pinned, short))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


TABLE = dict(wd_attn_layer_forward=_forward, wd_attn_output=_output, wd_attn_layer_backward=_backward,
             wd_attn_wout_partial=_wout, wd_attn_fold=_fold)


_CASES = [pytest.param(n, i, id=f"{n}-{m[0]}-{i}") for n in sorted(TABLE)
          for i, m in enumerate(TABLE[n](torch.device("cpu"))[1])]


def test_every_exported_op_is_in_the_table():
    K_ = _native.aink()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE), sorted(exported ^ set(TABLE))
    assert all(n.startswith("wd_attn_") for n in exported) and _native.aink_available()
    assert (K_.MAX_T, K_.MAX_F, K_.MAX_D, K_.MAX_A, K_.CHUNK, K_.MAX_CHUNKS) == (
        ops.ATTN_MAX_T, ops.ATTN_MAX_F, ops.ATTN_MAX_D, ops.ATTN_MAX_A, ops.ATTN_CHUNK, ops.ATTN_MAX_CHUNKS)
    for other in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
                  _native.fmk(), _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak(),
                  _native.w2vk(), _native.alsk(), _native.gmmk(), _native.gmmfk(), _native.ibsk(), _native.kmk(),
                  _native.cink()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    for name in sorted(TABLE):
        getattr(_native.aink(), name)(*TABLE[name](dev)[0].values())
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
        getattr(_native.aink(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.aink(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
