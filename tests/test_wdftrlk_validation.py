"""Argument validation of the _wdftrlk binding (csrc/bindings/wideftrl_py.cpp, tensor_access.h), the harness of
test_ftrlk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
GPU part: every mutation raises RuntimeError naming the mutated argument and launches nothing (no tensor
argument changes); the valid set is accepted. Every mutation is harmless even if its check were missing:
the mutated argument is backed by memory the kernel may touch at the extent it would address (a wider
dtype at the same element count, a strided view of a twice-as-large buffer, a pinned host copy, a shape
the launcher's row check keeps inside the buffers, or a scalar the launcher refuses as well). CPU part: the
valid set on pageable CPU tensors raises RuntimeError naming a tensor argument (the device check comes
before any launch, on every machine)."""
import re
import types

import pytest
import torch

from minips_amd import _native

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
ROWS, W, D1, N = 16, 8, 4, 8
WF = W - D1


def wider(t):  # same element count, a larger element type
    return t.to({F32: F64, I32: I64}[t.dtype]) if t.dtype in (F32, I32) else t.double()


def narrower(t):  # int64 -> int32 inside a buffer of the int64 size
    return torch.zeros(2 * t.numel(), dtype=I32, device=t.device)[: t.numel()].reshape(t.shape)


def strided(t):  # the same shape, every other row of a twice-as-large buffer
    return torch.zeros((2 * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)[::2]


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
@entry("sparse_adagrad_ftrl")
def _(d):
    a = dict(table=_t(d, (ROWS, W), F32, 1), state=_t(d, (ROWS,), F32), zn=_t(d, (ROWS, 2 * WF), F32), D1=D1,
             keys=torch.arange(2, 2 + N, device=d), base=0, grads=_t(d, (N, W), F32, 0.5), lr=0.1, eps=0.0,
             alpha=0.1, beta=1.0, l1=0.0, l2=0.0, grad_scale=1.0, n_dev=_t(d, (1,), I64, N), oor=_t(d, (1,), I64),
             blocks=0)
    muts = [("table", wider), ("table", pinned),
            ("table", value(lambda dv: _t(dv, (ROWS, 2 * W), F32)[:, ::2])),  # no unit column stride
            ("table", value(lambda dv: _t(dv, (ROWS, W - 1), F32))),  # narrower than the gradient rows
            ("state", wider), ("state", pinned), ("state", strided),
            ("state", value(lambda dv: _t(dv, (ROWS,), F32)[:-1])),  # a row short of the table
            ("state", value(lambda dv: _t(dv, (ROWS, 1), F32))),  # a column, not a vector
            ("zn", wider), ("zn", pinned), ("zn", strided),
            ("zn", value(lambda dv: _t(dv, (ROWS, 2 * WF), F32)[:-1])),  # a row short of the table
            ("zn", value(lambda dv: _t(dv, (ROWS, 2 * WF), F32)[:, :WF])),  # z without n
            ("zn", value(lambda dv: _t(dv, (ROWS, 2 * W), F32))),  # sparse_ftrl's whole-row state
            ("zn", value(lambda dv: _t(dv, (ROWS * 2 * WF,), F32))),  # flat
            ("D1", value(0)), ("D1", value(-4)), ("D1", value(W)), ("D1", value(W + 4)),
            ("keys", narrower), ("keys", pinned), ("keys", strided),
            ("grads", wider), ("grads", pinned), ("grads", strided),
            ("grads", value(lambda dv: _t(dv, (N, W), F32)[:-1])),  # fewer rows than keys
            ("grads", value(lambda dv: _t(dv, (N * W,), F32))),  # flat: no width
            ("alpha", value(0.0)), ("alpha", value(-0.1)), ("alpha", value(float("nan"))),
            ("beta", value(-1.0)), ("beta", value(float("nan"))), ("l1", value(-0.5)), ("l1", value(float("nan"))),
            ("l2", value(-0.5)), ("l2", value(float("nan"))),
            ("grad_scale", value(0.0)), ("grad_scale", value(-2.0)), ("grad_scale", value(float("inf"))),
            ("grad_scale", value(float("nan"))),
            ("n_dev", narrower), ("n_dev", pinned), ("n_dev", value(lambda dv: _t(dv, (0,), I64))),
            ("oor", narrower), ("oor", pinned), ("oor", value(lambda dv: _t(dv, (0,), I64))),
            ("blocks", value(-1)), ("blocks", value(65536))]
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
    K = _native.wdftrlk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K) if not n.startswith("_") and callable(getattr(K, n))}
    assert ops == set(TABLE) == {"sparse_adagrad_ftrl"}, sorted(ops ^ set(TABLE))


def test_the_other_modules_export_none_of_them():
    for K in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk()):
        assert not set(TABLE) & set(dir(K))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_valid_arguments_are_accepted(name, dev):
    args, _ = TABLE[name](dev)
    getattr(_native.wdftrlk(), name)(*args.values())
    torch.cuda.synchronize()
    touched = torch.zeros(ROWS, dtype=torch.bool)
    touched[2: 2 + N] = True
    w, st, zn = args["table"].cpu(), args["state"].cpu(), args["zn"].cpu()
    # deep: g = 0.5 on D1 columns, state 0 -> 0.25, w = 1 - 0.1 / (0.5 + 0) * 0.5
    assert torch.equal(st[touched], torch.full((N,), 0.25)) and not bool(st[~touched].any())
    torch.testing.assert_close(w[touched][:, :D1], torch.full((N, D1), 0.9), rtol=1e-6, atol=0)
    # wide: z = n = 0, w = 1, g = 0.5, l1 = l2 = 0: n' = 0.25, sigma = 0.25 / (0.1 * 0.5) = 5, z' = 0.5 - 5 * 1,
    # w' = 4.5 / ((1 + 0.5) / 0.1)
    assert torch.equal(zn[touched][:, WF:], torch.full((N, WF), 0.25)) and not bool(zn[~touched].any())
    torch.testing.assert_close(zn[touched][:, :WF], torch.full((N, WF), -4.5), rtol=1e-6, atol=0)
    torch.testing.assert_close(w[touched][:, D1:], torch.full((N, WF), 0.3), rtol=1e-6, atol=0)
    assert bool((w[~touched] == 1).all()) and int(args["oor"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.wdftrlk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.wdftrlk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
