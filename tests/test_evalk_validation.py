"""Argument validation of the _evalk bindings (csrc/bindings/eval_py.cpp, tensor_access.h), in the
style of test_bindings_validation.py: one table entry per exported op -- a tiny valid argument set
and mutations of it. GPU part: every mutation raises RuntimeError naming the mutated argument and
launches nothing (no tensor argument changes); the valid set is accepted. Every mutation is harmless
even if its check were missing: the mutated argument is backed by memory the kernel may touch at
the extent it would address (a wider dtype at the same element count, a narrow view of the
full-size buffer, a transposed same-size buffer, a pinned host copy, a shape that only shrinks
what is addressed, or a bin count the launcher refuses as well). CPU part (no GPU): the valid set
on pageable CPU tensors raises RuntimeError naming a tensor argument (the device check).
"""
import re
import types

import pytest
import torch

from minips_amd import _native

BF, F32, F64, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.uint8
NB = 32


# ---- mutations ------------------------------------------------------------------------------------
def wider(t):  # same element count, a larger (or reinterpreted) element type
    if t.dtype == I64:
        return t.view(F64)
    return t.to({BF: F32, F32: F64}[t.dtype])


def short(t):  # one element (row) less: a narrow view of the full-size buffer
    return t[:-1]


def transposed(t):  # same shape, a non-contiguous view of a same-size buffer
    assert t.dim() == 2 and min(t.shape) > 1
    return torch.zeros(t.shape[1], t.shape[0], dtype=t.dtype, device=t.device).t()


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


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("binary_hist")
def _(d):
    a = dict(logits=_t(d, (8,), F32, 0.5), labels=_t(d, (8,), F32, 1), acc=_t(d, (2 * NB + 2,), I64, 3))
    return a, [("logits", wider), ("logits", pinned), ("logits", short), ("labels", wider), ("labels", short),
               ("labels", pinned), ("acc", wider), ("acc", short), ("acc", pinned),
               ("acc", value(lambda dv: torch.zeros(2 * 48 + 2, dtype=I64, device=dv))),  # NB = 48: no power of two
               ("acc", value(lambda dv: torch.zeros(2 * 16 + 2, dtype=I64, device=dv))),  # NB = 16: too few
               ("acc", value(lambda dv: torch.zeros(2 * NB + 3, dtype=I64, device=dv)))]


@entry("eval_head_hist")
def _(d):
    a = dict(H=_t(d, (8, 16), BF, 1), w=_t(d, (16,), BF, 0.5), b0=_t(d, (1,), BF), wide=_t(d, (8,), F32, 0.25),
             labels=_t(d, (8,), F32, 1), acc=_t(d, (2 * NB + 2,), I64, 3), logits_out=_t(d, (8,), F32, 3))
    return a, [("H", wider), ("H", short), ("H", transposed), ("H", pinned),
               ("H", value(lambda dv: torch.ones(8, 12, dtype=BF, device=dv))),  # Hd = 12: no multiple of 8
               ("H", value(lambda dv: torch.ones(8, 20, dtype=BF, device=dv)[:, :16])),  # ld = 20: no multiple of 8
               ("H", value(lambda dv: torch.ones(8, 32, dtype=BF, device=dv)[:, 4:20])),  # rows 8-byte aligned only
               ("w", wider), ("w", short), ("w", pinned), ("b0", wider), ("b0", pinned), ("wide", wider),
               ("wide", short), ("wide", pinned), ("labels", wider), ("labels", short), ("labels", pinned),
               ("acc", wider), ("acc", short), ("acc", pinned),
               ("acc", value(lambda dv: torch.zeros(2 * 48 + 2, dtype=I64, device=dv))),
               ("logits_out", wider), ("logits_out", short), ("logits_out", pinned)]


# ---- the harness ----------------------------------------------------------------------------------
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
    K = _native.evalk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K) if not n.startswith("_") and callable(getattr(K, n))}
    assert ops == set(TABLE), sorted(ops ^ set(TABLE))


def test_the_kernel_module_exports_none_of_them():
    K = _native.kernels()
    assert not set(TABLE) & set(dir(K))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_valid_arguments_are_accepted(name, dev):
    args, _ = TABLE[name](dev)
    acc0 = args["acc"].clone()
    getattr(_native.evalk(), name)(*args.values())
    torch.cuda.synchronize()
    n = args["labels"].numel()
    assert int((args["acc"] - acc0)[:2 * NB].sum()) == n  # every sample was counted once


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in args.values()]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.evalk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(args.values(), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    if torch.cuda.is_available():
        pytest.skip("the pageable-memory device check is exercised where no GPU can be reached")
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.evalk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
