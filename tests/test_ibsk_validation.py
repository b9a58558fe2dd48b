"""Argument validation of the _ibsk binding (csrc/bindings/ibs_py.cpp), test_gmmk_validation.py's harness: a mutation
of a tiny valid argument set raises RuntimeError naming the argument and launches nothing; CPU tensors are refused."""
import types

import pytest
import torch

from test_w2vk_validation import (F32, I32, _bytes, _names, _t, _tensors, column, narrower, no_unit_stride, pinned,
                                  short, strided, value, wider)

from minips_amd import _native, ops

P, D, CAP = 5, 8, 6


def _inputs(d):
    g = torch.Generator().manual_seed(0)
    inv = torch.stack([torch.randint(0, 3, (P,), generator=g), 3 + torch.randint(0, 3, (P,), generator=g)], 1)
    rows, logq = torch.randn(CAP, D, generator=g) * 0.5, torch.randn(P, generator=g) - 2
    return inv.reshape(-1).to(d), rows.to(d), logq.to(d)


_SCALARS = dict(d=(value(6), value(4), value(132)), tau=(value(0.0), value(-1.0), value(float("nan"))),
                blocks=(value(-1), value(65536)))
_F32 = (wider, pinned, strided, short, column)  # (wider: fp32 -> fp64, int32 -> int64)


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _forward(d):
    inv, rows, logq = _inputs(d)
    a = dict(inv=inv, rows=rows, d=D, tau=0.25, logq=logq, lse=_t(d, (P,), F32, 9.0), loss=_t(d, (P,), F32, 9.0),
             blocks=0)
    per = dict(inv=(narrower, pinned, strided, short, column), rows=(wider, pinned, no_unit_stride,
                                                                      value(lambda dv: _t(dv, (CAP, D - 4), F32))),
               logq=_F32, lse=_F32, loss=_F32, **_SCALARS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _backward(d):
    inv, rows, logq = _inputs(d)
    loss, lse = ops.ibs_forward(inv.cpu(), rows.cpu(), D, 0.25, logq.cpu())
    order = torch.sort(inv.cpu(), stable=True)
    a = dict(members=order.indices.to(I32).to(d), memrow=order.values.to(I32).to(d), inv=inv, rows=rows, d=D, tau=0.25,
             logq=logq, lse=lse.to(d), gscale=1.0 / P, grad_rows=_t(d, (CAP, D), F32, 9.0), blocks=0)
    per = dict(members=_F32, memrow=_F32, inv=(narrower, pinned, strided, short, column),
               rows=(wider, pinned, no_unit_stride, value(lambda dv: _t(dv, (CAP, D - 4), F32))), logq=_F32, lse=_F32,
               gscale=(value(float("nan")), value(float("inf"))),
               grad_rows=(wider, pinned, strided, short, value(lambda dv: _t(dv, (CAP, D + 4), F32))), **_SCALARS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


TABLE = dict(ibs_forward=_forward, ibs_backward=_backward)


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](torch.device("cpu"))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_exported_op_is_in_the_table():
    K_ = _native.ibsk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"ibs_forward", "ibs_backward"}, sorted(exported ^ set(TABLE))
    assert (K_.MIN_D, K_.MAX_D, K_.TILE) == (ops.IBS_MIN_D, ops.IBS_MAX_D, ops.IBS_TILE) == (8, 128, 64)
    assert K_.WAVE_MAX >= 2 * K_.CHUNK and _native.ibsk_available()
    for other in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
                  _native.fmk(), _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak(),
                  _native.w2vk(), _native.alsk(), _native.gmmk(), _native.gmmfk()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    for name in sorted(TABLE):
        getattr(_native.ibsk(), name)(*TABLE[name](dev)[0].values())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ibsk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ibsk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
