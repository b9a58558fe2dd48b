"""Argument validation of the _optk bindings (csrc/bindings/optim_py.cpp, tensor_access.h), in the
style of test_evalk_validation.py: one table entry per exported op -- a tiny valid argument set and
mutations of it. GPU part: every mutation raises RuntimeError naming the mutated argument and launches
nothing (no tensor argument changes); the valid set is accepted. Every mutation is harmless even if
its check were missing: the mutated argument is backed by memory the kernel may touch at the extent
it would address (a wider dtype at the same element count, a narrow view of the full-size buffer, a
strided view of a twice-as-large buffer, a pinned host copy, a misaligned view of a larger buffer, or
a count the launcher refuses as well). CPU part: the valid set on pageable CPU tensors raises
RuntimeError naming a tensor argument (the device check comes before any launch, on every machine).
"""
import re
import types

import pytest
import torch

from minips_amd import _native

BF, F32, F64, I32, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
N = 64


# ---- mutations ------------------------------------------------------------------------------------
def wider(t):  # same element count, a larger element type
    return t.to({BF: F32, F32: F64, I32: I64}[t.dtype]) if t.dtype != F64 else t.view(I64)


def short(t):  # four elements less (still a multiple of 4): a narrow view of the full-size buffer
    return t[:-4] if t.numel() > 4 else t[:-1]


def strided(t):  # the same count, every other element of a twice-as-large buffer
    return torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]


def shifted(t):  # the same count, 4 (fp32) / 2 (bf16) bytes past an aligned address inside a larger buffer
    return torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)[1: 1 + t.numel()]


def pinned(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)


def value(v):  # replaces the argument (v may be a callable taking the device)
    return lambda old, dev=None: v


def _t(dev, shape, dtype, fill=0):
    return torch.full(shape, fill, dtype=dtype, device=dev)


TABLE = {}


def entry(name):
    def reg(fn):
        TABLE[name] = fn
        return fn
    return reg


def _slabs(d, nsplit=3, plane=8, off=16):
    return [(_t(d, (nsplit * plane,), F32, 0.5), nsplit, plane, off)]


def _bad_slabs():
    return [("slabs", value(lambda dv: _slabs(dv, plane=8, off=N - 4))),  # the region ends past the gradient
            ("slabs", value(lambda dv: _slabs(dv, plane=6, off=16))),  # plane: no multiple of 4
            ("slabs", value(lambda dv: _slabs(dv, off=18))),  # offset: no multiple of 4
            ("slabs", value(lambda dv: _slabs(dv, nsplit=0))),
            ("slabs", value(lambda dv: [(_t(dv, (16,), F32), 3, 8, 16)])),  # planes shorter than nsplit * plane
            ("slabs", value(lambda dv: [(_t(dv, (24,), F64), 3, 8, 16)])),
            ("slabs", value(lambda dv: [(torch.zeros(24, pin_memory=True), 3, 8, 16)])),
            ("slabs", value(lambda dv: [(_t(dv, (32,), F32)[1:25], 3, 8, 16)])),  # misaligned planes
            ("slabs", value(lambda dv: _slabs(dv) * 5))]  # more than 4 regions


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("grad_sumsq")
def _(d):
    a = dict(g=_t(d, (N,), F32, 0.5), slabs=_slabs(d), part=_t(d, (4,), F64, 3), L=4)
    return a, [("g", wider), ("g", pinned), ("g", strided), ("g", shifted),
               ("g", value(lambda dv: _t(dv, (N - 2,), F32))),  # no multiple of 4
               ("part", wider), ("part", pinned), ("part", strided), ("part", value(lambda dv: _t(dv, (3,), F64))),
               ("part", value(lambda dv: _t(dv, (4,), F32))),
               ("L", value(0)), ("L", value(1025))] + _bad_slabs()


@entry("adam_clip_apply")
def _(d):
    a = dict(w=_t(d, (N,), F32, 1), m=_t(d, (N,), F32), v=_t(d, (N,), F32), g=_t(d, (N,), F32, 0.5), slabs=_slabs(d),
             lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, step_dev=_t(d, (1,), I32, 1),
             w_bf16=_t(d, (N,), BF), zero_g=True, part=_t(d, (4,), F64, 1), np=4, max_norm=1.0,
             stats=_t(d, (4,), F64), write_stats=True)
    muts = []
    for n in ("w", "m", "v", "g"):
        muts += [(n, wider), (n, short), (n, pinned), (n, strided), (n, shifted)]
    muts += [("w", value(lambda dv: _t(dv, (N - 2,), F32))),
             ("step_dev", wider), ("step_dev", pinned), ("step_dev", value(lambda dv: _t(dv, (0,), I32))),
             ("w_bf16", wider), ("w_bf16", short), ("w_bf16", pinned), ("w_bf16", strided), ("w_bf16", shifted),
             ("part", wider), ("part", pinned), ("part", strided), ("part", value(lambda dv: _t(dv, (3,), F64))),
             ("np", value(0)), ("np", value(4097)), ("max_norm", value(0.0)), ("max_norm", value(float("nan"))),
             ("stats", wider), ("stats", pinned), ("stats", strided), ("stats", value(lambda dv: _t(dv, (3,), F64))),
             ("stats", value(lambda dv: _t(dv, (4,), F32)))]
    return a, muts + _bad_slabs()


# ---- the harness ----------------------------------------------------------------------------------
def _tensors(args):
    out = []
    for v in args.values():
        if torch.is_tensor(v):
            out.append(v)
        elif isinstance(v, list):
            out += [e[0] for e in v]
    return out


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
    K = _native.optk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K) if not n.startswith("_") and callable(getattr(K, n))}
    assert ops == set(TABLE) == {"grad_sumsq", "adam_clip_apply"}, sorted(ops ^ set(TABLE))


def test_the_other_modules_export_none_of_them():
    for K in (_native.kernels(), _native.evalk()):
        assert not set(TABLE) & set(dir(K))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_valid_arguments_are_accepted(name, dev):
    args, _ = TABLE[name](dev)
    getattr(_native.optk(), name)(*args.values())
    torch.cuda.synchronize()
    # g = 0.5 everywhere plus three planes of 0.5 on 8 elements: 56 * 0.25 + 8 * 4
    if name == "grad_sumsq":
        assert float(args["part"].sum()) == 56 * 0.25 + 8 * 4.0
    else:  # part sums to 4: norm 2, clipped to max_norm 1
        norm, scale, clipped, skipped = args["stats"].tolist()
        assert (norm, clipped, skipped) == (2.0, 1.0, 0.0) and scale == pytest.approx(0.5, rel=1e-6)
        assert int((args["g"] != 0).sum()) == 0 and bool((args["w"] != 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.optk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.optk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
