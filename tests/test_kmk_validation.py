"""Argument validation of the _kmk binding (csrc/bindings/kmeans_py.cpp), test_ibsk_validation.py's harness: a mutation
of a tiny valid argument set raises RuntimeError naming the argument and launches nothing; CPU tensors are refused."""
import types

import pytest
import torch

from test_w2vk_validation import (F32, I32, _bytes, _names, _t, _tensors, column, no_unit_stride, pinned, short,
                                  strided, value, wider)

from minips_amd import _native, ops

N, K, D = 5, 3, 4


def _inputs(d):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, D, generator=g).to(d), (3 * torch.randn(K, D, generator=g)).to(d)


_VEC = (wider, pinned, strided, short, column)  # (wider: fp32 -> fp64, int32 -> int64)
_X = (wider, pinned, no_unit_stride, value(lambda dv: _t(dv, (N, D - 1), F32)))
_BLOCKS = (value(-1), value(65536))


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _nearest(d):
    X, C = _inputs(d)
    a = dict(X=X, C=C, assign=_t(d, (N,), I32, 9), dist=_t(d, (N,), F32, 9.0),
             sse=torch.full((1,), 9.0, dtype=torch.float64, device=d), bad=_t(d, (1,), I32), blocks=0)
    per = dict(X=_X, C=(wider, pinned, strided, value(lambda dv: _t(dv, (ops.KM_MAX_K + 1, D), F32)),
                        value(lambda dv: _t(dv, (K, ops.KM_MAX_D + 1), F32)), value(lambda dv: _t(dv, (0, D), F32))),
               assign=_VEC, dist=_VEC, sse=(pinned, value(lambda dv: _t(dv, (1,), F32)),
                                            value(lambda dv: _t(dv, (2,), torch.float64))),
               bad=(wider, pinned, value(lambda dv: _t(dv, (2,), I32))), blocks=_BLOCKS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _sums(d):
    X, _ = _inputs(d)
    a = dict(X=X, assign=torch.tensor([0, 2, 2, -1, 7], dtype=I32, device=d), sums=_t(d, (K, D), F32, 9.0),
             counts=_t(d, (K,), I32, 9), blocks=0)
    per = dict(X=_X, assign=_VEC, sums=(wider, pinned, strided, value(lambda dv: _t(dv, (ops.KM_MAX_K + 1, D), F32)),
                                        value(lambda dv: _t(dv, (K, D + 1), F32))),
               counts=_VEC, blocks=_BLOCKS)
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


TABLE = dict(km_nearest=_nearest, km_sums=_sums)


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](torch.device("cpu"))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_exported_op_is_in_the_table():
    K_ = _native.kmk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"km_nearest", "km_sums"}, sorted(exported ^ set(TABLE))
    assert (K_.MAX_K, K_.MAX_D, K_.CHUNK, K_.WAVE_MAX) == (ops.KM_MAX_K, ops.KM_MAX_D, ops.KM_CHUNK, ops.KM_WAVE_MAX)
    assert (K_.TILE, K_.STRIP) == (64, 64) and K_.WAVE_MAX >= 2 * K_.ROW_CHUNK and _native.kmk_available()
    for other in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
                  _native.fmk(), _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak(),
                  _native.w2vk(), _native.alsk(), _native.gmmk(), _native.gmmfk(), _native.ibsk()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    for name in sorted(TABLE):
        getattr(_native.kmk(), name)(*TABLE[name](dev)[0].values())
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
        getattr(_native.kmk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.kmk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
