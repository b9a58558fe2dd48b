"""Argument validation of the _ffmk binding (csrc/bindings/ffm_py.cpp, tensor_access.h), the harness of
test_fmk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
GPU part: every mutation raises RuntimeError naming the mutated argument and launches nothing (no tensor
argument changes); the valid set is accepted. Every mutation is harmless even if its check were missing: the
mutated argument is backed by memory the kernel may touch at the extent it would address, or is a scalar the
launcher refuses as well, and the kernels skip any index outside its range. CPU part: the valid set on pageable
CPU tensors raises RuntimeError naming a tensor argument (the device check comes before any launch, on every
machine)."""
import re
import types

import pytest
import torch

from minips_amd import _native

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
B, N, CAP, NF, K = 3, 6, 5, 2, 4
FK = NF * K
W = FK + 4


def wider(t):  # same element count, a larger element type
    return t.to({F32: F64, I32: I64}[t.dtype])


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


def _rows(d):
    r = _t(d, (CAP, W), F32, 0.5)
    r[:, FK:] = 0.25
    return r


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("ffm_forward")
def _(d):
    a = dict(rowptr=torch.tensor([0, 2, 2, N], device=d), inv=torch.tensor([0, 1, 1, 2, 3, 1], device=d),
             vals=_t(d, (N,), F32, 1.0), fields=torch.tensor([0, 1, 0, 1, 0, 1], dtype=I32, device=d),
             labels=torch.tensor([1.0, 0.0, 0.0], device=d), rows=_rows(d), F=NF, k=K, w0=_t(d, (1,), F32, 0.5),
             gscale=1.0, z=_t(d, (B,), F32, -1), dz=_t(d, (B,), F32, -1), loss=_t(d, (B,), F32, -1),
             rowid=_t(d, (N,), I32, -1), blocks=0)
    muts = [("rowptr", narrower), ("rowptr", pinned), ("rowptr", strided),
            ("rowptr", value(lambda dv: _t(dv, (B + 1, 1), I64))),
            ("inv", narrower), ("inv", pinned), ("inv", strided), ("inv", column),
            ("vals", wider), ("vals", pinned), ("vals", strided), ("vals", short), ("vals", column),
            ("fields", wider), ("fields", pinned), ("fields", strided), ("fields", short), ("fields", column),
            ("labels", wider), ("labels", pinned), ("labels", strided), ("labels", short), ("labels", column),
            ("rows", wider), ("rows", pinned),
            ("rows", value(lambda dv: _t(dv, (CAP, 2 * W), F32)[:, ::2])),  # no unit column stride
            ("rows", value(lambda dv: _t(dv, (CAP, W - 1), F32))),  # narrower than F k + 4
            ("rows", value(lambda dv: _t(dv, (CAP * W,), F32))),  # flat
            ("F", value(0)), ("F", value(-1)), ("F", value(65)),
            ("k", value(0)), ("k", value(6)), ("k", value(20)), ("k", value(-4)),
            ("w0", wider), ("w0", pinned), ("w0", value(lambda dv: _t(dv, (0,), F32))),
            ("gscale", value(float("nan"))), ("gscale", value(float("inf"))),
            ("z", wider), ("z", pinned), ("z", strided), ("z", short), ("z", column),
            ("dz", wider), ("dz", pinned), ("dz", strided), ("dz", short), ("dz", column),
            ("loss", wider), ("loss", pinned), ("loss", strided), ("loss", short), ("loss", column),
            ("rowid", wider), ("rowid", pinned), ("rowid", strided), ("rowid", short), ("rowid", column),
            ("blocks", value(-1)), ("blocks", value(65536))]
    return a, muts


@entry("ffm_backward")
def _(d):
    # the lookups of ffm_forward's set grouped by row: row 0 <- {0}, 1 <- {1, 2, 5}, 2 <- {3}, 3 <- {4}
    a = dict(members=torch.tensor([0, 1, 2, 5, 3, 4], dtype=I32, device=d),
             memrow=torch.tensor([0, 1, 1, 1, 2, 3], dtype=I32, device=d),
             rowid=torch.tensor([0, 0, 2, 2, 2, 2], dtype=I32, device=d),
             rowptr=torch.tensor([0, 2, 2, N], device=d), inv=torch.tensor([0, 1, 1, 2, 3, 1], device=d),
             vals=_t(d, (N,), F32, 1.0), fields=torch.tensor([0, 1, 0, 1, 0, 1], dtype=I32, device=d),
             dz=_t(d, (B,), F32, 0.5), rows=_rows(d), F=NF, k=K, grad_rows=_t(d, (CAP, W), F32, 9.0), blocks=0)
    muts = [("members", wider), ("members", pinned), ("members", strided), ("members", column),
            ("memrow", wider), ("memrow", pinned), ("memrow", strided), ("memrow", short), ("memrow", column),
            ("rowid", wider), ("rowid", pinned), ("rowid", strided), ("rowid", short), ("rowid", column),
            ("rowptr", narrower), ("rowptr", pinned), ("rowptr", strided), ("rowptr", short),
            ("rowptr", value(lambda dv: _t(dv, (B + 1, 1), I64))),
            ("inv", narrower), ("inv", pinned), ("inv", strided), ("inv", short), ("inv", column),
            ("vals", wider), ("vals", pinned), ("vals", strided), ("vals", short), ("vals", column),
            ("fields", wider), ("fields", pinned), ("fields", strided), ("fields", short), ("fields", column),
            ("dz", wider), ("dz", pinned), ("dz", strided), ("dz", column),
            ("rows", wider), ("rows", pinned),
            ("rows", value(lambda dv: _t(dv, (CAP, 2 * W), F32)[:, ::2])),
            ("rows", value(lambda dv: _t(dv, (CAP, W - 1), F32))),
            ("rows", value(lambda dv: _t(dv, (CAP * W,), F32))),
            ("F", value(0)), ("F", value(-1)), ("F", value(65)),
            ("k", value(0)), ("k", value(6)), ("k", value(20)), ("k", value(-4)),
            ("grad_rows", wider), ("grad_rows", pinned), ("grad_rows", strided), ("grad_rows", short),
            ("grad_rows", value(lambda dv: _t(dv, (CAP, W + 4), F32))),  # the wrong width
            ("grad_rows", value(lambda dv: _t(dv, (CAP * W,), F32))),  # flat
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
    K_ = _native.ffmk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert ops == set(TABLE) == {"ffm_forward", "ffm_backward"}, sorted(ops ^ set(TABLE))
    # the member counts at which the backward switches paths, and the limits of the rule (csrc/kernels/ffm.h)
    assert (K_.GROUP_MAX, K_.WAVE_MAX, K_.CHUNK) == (8, 64, 32) and K_.WAVE_MAX >= 2 * K_.CHUNK
    from minips_amd import ops as O

    assert (K_.MAX_F, K_.MAX_K, K_.MAX_FK) == (O.FFM_MAX_F, O.FFM_MAX_K, O.FFM_MAX_FK) == (64, 16, 512)


def test_the_other_modules_export_none_of_them():
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(), _native.fmk(),
               _native.dfmk(), _native.dcnk()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    fa, _ = TABLE["ffm_forward"](dev)
    _native.ffmk().ffm_forward(*fa.values())
    ba, _ = TABLE["ffm_backward"](dev)
    _native.ffmk().ffm_backward(*ba.values())
    torch.cuda.synchronize()
    # forward: v = 0.5 in every slot, w = 0.25, x = 1; sample 0 has 2 lookups, sample 1 none, sample 2 four;
    # w0 = 0.5: every pair adds K / 4, z = w0 + nnz / 4 + pairs K / 4
    nnz, pairs = torch.tensor([2.0, 0.0, 4.0]), torch.tensor([1.0, 0.0, 6.0])
    z = 0.5 + nnz / 4 + pairs * K / 4
    assert torch.equal(fa["z"].cpu(), z) and fa["rowid"].tolist() == [0, 0, 2, 2, 2, 2]
    y = torch.tensor([1.0, 0.0, 0.0])
    torch.testing.assert_close(fa["dz"].cpu(), torch.sigmoid(z) - y, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(fa["loss"].cpu(), z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs())),
                               rtol=1e-6, atol=1e-7)
    # backward: c = 0.5 per member; a partner adds c x v = 0.25 to every column of the slot of its field.
    # lookups (sample, field): 0 (0, 0), 1 (0, 1) | 2 (2, 0), 3 (2, 1), 4 (2, 0), 5 (2, 1)
    # row 0 <- {0}: partner 1 (field 1); row 1 <- {1, 2, 5}: partners 0 (f 0) | 3, 4, 5 (f 1, 0, 1) | 2, 3, 4
    # (f 0, 1, 0); row 2 <- {3}: partners 2, 4, 5 (f 0, 0, 1); row 3 <- {4}: partners 2, 3, 5 (f 0, 1, 1)
    g = ba["grad_rows"].cpu()
    slot0 = torch.tensor([0.0, 4.0, 2.0, 1.0]) * 0.25
    slot1 = torch.tensor([1.0, 3.0, 1.0, 2.0]) * 0.25
    M = torch.tensor([1.0, 3.0, 1.0, 1.0])
    assert torch.equal(g[:4, :K], slot0[:, None].expand(4, K)) and torch.equal(g[:4, K:FK], slot1[:, None].expand(4, K))
    assert torch.equal(g[:4, FK], 0.5 * M)
    assert bool((g[:4, FK + 1:] == 0).all()) and bool((g[4] == 9.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ffmk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ffmk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
