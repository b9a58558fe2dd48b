"""Argument validation of the _gmmk binding (csrc/bindings/gmm_py.cpp), the harness of test_alsk_validation.py: every
mutation of a tiny valid argument set raises RuntimeError naming the mutated argument and launches nothing (and is
harmless even if its check were missing); the valid set is accepted; the valid set on CPU tensors is refused."""
import types

import pytest
import torch

from test_w2vk_validation import (F32, F64, I32, _bytes, _names, _t, _tensors, column, flat, no_unit_stride, pinned,
                                  short, strided, value, wider)

from minips_amd import _native, ops

K, D, N = 3, 5, 7
DP = 16


def _inputs(d):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, D, generator=g)
    mu = torch.randn(K, D, generator=g)
    s = torch.cat([mu, 1.0 + mu * mu, torch.ones(K, 1)], 1) / K
    return X.to(d), torch.zeros(D, device=d), s.contiguous().to(d)


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _prepare(d):
    a = dict(s=_inputs(d)[2], var_floor=1e-4, coef=_t(d, (K, 2 * DP), F32, 9.0), cst=_t(d, (K,), F32, 9.0))
    per = dict(s=(wider, pinned, strided, flat, value(lambda dv: _t(dv, (K, 2 * D), F32)),      # an even width
                  value(lambda dv: _t(dv, (129, 2 * D + 1), F32))),                             # K > 128
               var_floor=(value(0.0), value(float("nan")), value(float("inf"))),
               coef=(wider, pinned, strided, flat, short, value(lambda dv: _t(dv, (K, 2 * D), F32))),  # unpadded
               cst=(wider, pinned, strided, short, column))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


def _estep(d):
    X, shift, s = _inputs(d)
    coef, cst = ops.gmm_prepare(s.cpu(), 1e-4)
    a = dict(X=X, shift=shift, coef=coef.to(d), cst=cst.to(d), S=_t(d, (K, 2 * D + 1), F32, 9.0),
             ll=_t(d, (1,), F64, 9.0), assign=_t(d, (N,), I32, 9), logp=_t(d, (N,), F32, 9.0), bad=_t(d, (1,), I32),
             blocks=0)
    f32 = (wider, pinned, strided, short)
    per = dict(X=(wider, pinned, flat, no_unit_stride, value(lambda dv: _t(dv, (N, D - 1), F32))),
               shift=f32 + (column,), coef=(wider, pinned, strided, flat, short), cst=f32 + (column,),
               S=(wider, pinned, strided, flat, short, value(lambda dv: _t(dv, (K, 2 * D), F32))),
               ll=(pinned, value(lambda dv: _t(dv, (1,), F32)), value(lambda dv: _t(dv, (2,), F64))),
               assign=(wider, pinned, strided, short, column), logp=f32 + (column,),
               bad=(wider, pinned, value(lambda dv: _t(dv, (2,), I32))), blocks=(value(-1), value(65536)))
    return a, [(arg, mut) for arg, ms in per.items() for mut in ms]


TABLE = dict(gmm_prepare=_prepare, gmm_estep=_estep)


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](torch.device("cpu"))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_exported_op_is_in_the_table():
    K_ = _native.gmmk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"gmm_prepare", "gmm_estep"}, sorted(exported ^ set(TABLE))
    assert (K_.MAX_K, K_.MAX_D, K_.MAX_KD, K_.CHUNK) == (ops.GMM_MAX_K, ops.GMM_MAX_D, ops.GMM_MAX_KD, ops.GMM_CHUNK) \
        == (128, 128, 8192, 2048)
    assert K_.TILE == 64 and K_.CHUNK % K_.TILE == 0 and _native.gmmk_available()
    for other in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
                  _native.fmk(), _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak(),
                  _native.w2vk(), _native.alsk()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.gmmk()
    args = {name: TABLE[name](dev)[0] for name in TABLE}
    for name in sorted(TABLE):
        getattr(K_, name)(*args[name].values())
    torch.cuda.synchronize()
    p = TABLE["gmm_prepare"](torch.device("cpu"))[0]
    coef, cst = ops.gmm_prepare(p["s"], p["var_floor"])
    g = args["gmm_prepare"]
    assert (g["coef"].cpu() - coef).abs().max() < 1e-5 and (g["cst"].cpu() - cst).abs().max() < 1e-5
    a = TABLE["gmm_estep"](torch.device("cpu"))[0]
    S, ll, assign, logp = ops.gmm_estep(a["X"], a["shift"], a["coef"], a["cst"], want_assign=True, want_logp=True)
    g = args["gmm_estep"]
    assert (g["S"].cpu() - S).abs().max() < 1e-4 and abs(float(g["ll"]) - float(ll)) < 1e-4
    assert torch.equal(g["assign"].cpu(), assign) and (g["logp"].cpu() - logp).abs().max() < 1e-4
    assert int(g["bad"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.gmmk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.gmmk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
