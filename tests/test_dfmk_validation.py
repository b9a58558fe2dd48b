"""Argument validation of the _dfmk binding (csrc/bindings/deepfm_py.cpp, tensor_access.h), the harness of
test_fmk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
GPU part: every mutation raises RuntimeError naming the mutated argument and launches nothing (no tensor
argument changes); the valid set is accepted. Every mutation is harmless even if its check were missing: the
mutated argument is backed by memory the kernel may touch at the extent it would address, or is a scalar the
launcher refuses as well, and the backward skips any perm entry outside its range. CPU part: the valid set on
pageable CPU tensors raises RuntimeError naming a tensor argument (the device check comes before any launch, on
every machine)."""
import re
import types

import pytest
import torch

from minips_amd import _native

BF, F32, F64, I32, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
B, F, D, LDX = 3, 2, 8, 24


def wider(t):  # same element count, a larger element type
    return t.to({BF: F32, F32: F64, I32: I64}[t.dtype])


def strided(t):  # the same shape, every other row of a twice-as-large buffer
    return torch.zeros((2 * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)[::2]


def pinned(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)


def value(v):  # replaces the argument (v may be a callable taking the device)
    return lambda old, dev=None: v


def _t(dev, shape, dtype, fill=0):
    return torch.full(shape, fill, dtype=dtype, device=dev)


def short(t):  # one element (row) fewer
    return t[:-1]


def column(t):  # a [n, 1] matrix, not a vector
    return t.reshape(-1, 1)


TABLE = {}


def entry(name):
    def reg(fn):
        TABLE[name] = fn
        return fn
    return reg


def _x(d):
    x = _t(d, (B, LDX), BF, 0.5)
    x[:, F * D:] = float("nan")  # never read
    return x


X_MUTS = [("X", wider), ("X", pinned),
          ("X", value(lambda dv: _t(dv, (B, 2 * LDX), BF)[:, ::2])),  # no unit column stride
          ("X", value(lambda dv: _t(dv, (B, F * D - 1), BF))),  # narrower than F * D
          ("X", value(lambda dv: _t(dv, (B * LDX,), BF))),  # flat
          ("F", value(0)), ("F", value(-1)), ("F", value(4)),  # 4 * 8 columns > ld
          ("D", value(0)), ("D", value(65)), ("D", value(-8)),
          ("blocks", value(-1)), ("blocks", value(65536))]


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("wd_fm_forward")
def _(d):
    a = dict(X=_x(d), F=F, D=D, wide=_t(d, (B,), F32, 0.25), S=_t(d, (B, D), F32, -1), blocks=0)
    muts = X_MUTS + [("wide", wider), ("wide", pinned), ("wide", strided), ("wide", short), ("wide", column),
                     ("S", wider), ("S", pinned), ("S", strided), ("S", short),
                     ("S", value(lambda dv: _t(dv, (B, D + 8), F32))),  # the wrong width
                     ("S", value(lambda dv: _t(dv, (B * D,), F32)))]  # flat
    return a, muts


@entry("wd_fm_backward")
def _(d):
    a = dict(X=_x(d), S=_t(d, (B, D), F32, 1.0), dwide=_t(d, (B,), F32, 0.5),
             perm=torch.arange(B * F - 1, -1, -1, dtype=I32, device=d), dX=_t(d, (B * F, D), BF, 1.0), F=F, D=D,
             blocks=0)
    muts = X_MUTS + [("S", wider), ("S", pinned), ("S", strided), ("S", short),
                     ("S", value(lambda dv: _t(dv, (B, D + 8), F32))), ("S", value(lambda dv: _t(dv, (B * D,), F32))),
                     ("dwide", wider), ("dwide", pinned), ("dwide", strided), ("dwide", short), ("dwide", column),
                     ("perm", wider), ("perm", pinned), ("perm", strided), ("perm", short), ("perm", column),
                     ("dX", wider), ("dX", pinned), ("dX", strided), ("dX", short),
                     ("dX", value(lambda dv: _t(dv, (B * F, D + 8), BF))),  # the wrong width
                     ("dX", value(lambda dv: _t(dv, (B * F * D,), BF)))]  # flat
    return a, muts


# ---- the harness ----------------------------------------------------------------------------------
def _tensors(args):
    return [v for v in args.values() if torch.is_tensor(v)]


def _bytes(t):
    return t.contiguous().view(-1).view(U8) if t.numel() else t.reshape(0)


def _names(arg):
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(arg) + r"(?![A-Za-z0-9_])")


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](torch.device("cpu"))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_exported_op_is_in_the_table():
    K_ = _native.dfmk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert ops == set(TABLE) == {"wd_fm_forward", "wd_fm_backward"}, sorted(ops ^ set(TABLE))
    assert K_.MAX_D == 64


def test_the_other_modules_export_none_of_them():
    assert set(TABLE) <= set(dir(_native.dfmk()))
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
               _native.fmk()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    fa, _ = TABLE["wd_fm_forward"](dev)
    _native.dfmk().wd_fm_forward(*fa.values())
    ba, _ = TABLE["wd_fm_backward"](dev)
    _native.dfmk().wd_fm_backward(*ba.values())
    ba2, _ = TABLE["wd_fm_backward"](dev)
    ba2["perm"] = None
    ba2["dX"] = ba2["dX"].view(B, F * D)  # the lookup-order layout
    _native.dfmk().wd_fm_backward(*ba2.values())
    torch.cuda.synchronize()
    # forward: v = 0.5, two fields: S = 1, q = 0.5 per column; fm = 0.5 * 8 * (1 - 0.5) = 2
    assert bool((fa["S"] == 1.0).all()) and bool((fa["wide"] == 2.25).all())
    assert bool(torch.isnan(fa["X"][:, F * D:].float()).all())
    # backward: 1 + 0.5 * (1 - 0.5), exact in bf16
    assert bool((ba["dX"] == 1.25).all()) and bool((ba2["dX"] == 1.25).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.dfmk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.dfmk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
