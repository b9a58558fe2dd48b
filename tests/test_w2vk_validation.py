"""Argument validation of the _w2vk binding (csrc/bindings/sgns_py.cpp, tensor_access.h), the harness of
test_ldak_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
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

from minips_amd import _native, ops

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
P, N, D, CAP, V = 3, 2, 8, 5, 4
K2 = N + 2


def wider(t):  # same element count, a larger element type
    return t.to({F32: F64, I32: I64}[t.dtype])


def narrower(t):  # int64 -> int32 inside a buffer of the larger size
    small = {I64: I32}[t.dtype]
    return torch.zeros(2 * t.numel(), dtype=small, device=t.device)[: t.numel()].reshape(t.shape)


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


def flat(t):
    return t.reshape(-1)


def no_unit_stride(t):  # the same shape, every other column of a twice-as-wide buffer
    return torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=t.device)[:, ::2]


TABLE = {}


def entry(name):
    def reg(fn):
        TABLE[name] = fn
        return fn
    return reg


COUNTS = [5, 0, 2, 9]


def _sampler(d):
    thr, alias, T, _ = ops.sgns_alias(torch.tensor(COUNTS))
    return thr.to(d), alias.to(d), T


def _pairs(d):
    """Three pairs over five pulled rows: inv [P (N + 2)] (pair 1's second negative repeats its context: masked),
    rows [CAP, D]."""
    inv = torch.tensor([0, 1, 2, 3, 4, 3, 1, 3, 0, 2, 1, 4], dtype=I64, device=d)
    g = torch.Generator().manual_seed(0)
    rows = (torch.randn(CAP, D, generator=g) * 0.5).to(d)
    return inv, rows


BLOCKS_MUTS = [("blocks", value(-1)), ("blocks", value(65536))]
N_MUTS = [("N", value(0)), ("N", value(65)), ("N", value(3))]  # (3: the other shapes say N = 2)
ROWS_MUTS = [("rows", wider), ("rows", pinned), ("rows", flat), ("rows", no_unit_stride),
             ("rows", value(lambda dv: _t(dv, (CAP, D - 4), F32)))]  # narrower than h


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("sgns_lookups")
def _(d):
    thr, alias, T = _sampler(d)
    a = dict(centres=torch.tensor([0, 3, 2], dtype=I64, device=d),
             contexts=torch.tensor([2, 0, 3], dtype=I64, device=d), thr=thr, alias=alias, T=T, seed=11, epoch=2,
             pair_base=40, N=N, negatives=torch.tensor([[0, 2], [3, 3], [2, 0]], dtype=I32, device=d),
             keys=_t(d, (P, K2), I64, 9))
    muts = N_MUTS + [
        ("centres", narrower), ("centres", pinned), ("centres", strided), ("centres", short), ("centres", column),
        ("contexts", narrower), ("contexts", pinned), ("contexts", strided), ("contexts", short), ("contexts", column),
        ("thr", narrower), ("thr", pinned), ("thr", strided), ("thr", short), ("thr", column),
        ("thr", value(lambda dv: _t(dv, (0,), I64))),
        ("alias", wider), ("alias", pinned), ("alias", strided), ("alias", short), ("alias", column),
        ("T", value(0)), ("T", value(1 << 59)), ("epoch", value(-1)), ("pair_base", value(-1)),
        ("pair_base", value(1 << 56)),
        ("negatives", wider), ("negatives", pinned), ("negatives", strided), ("negatives", short), ("negatives", flat),
        ("keys", narrower), ("keys", pinned), ("keys", strided), ("keys", short), ("keys", flat)]
    return a, muts


@entry("sgns_forward")
def _(d):
    inv, rows = _pairs(d)
    a = dict(inv=inv, rows=rows, N=N, gscale=1.0 / P, e=_t(d, (P, N + 1), F32, 9.0), loss=_t(d, (P,), F32, 9.0),
             h=_t(d, (P, D), F32, 9.0), blocks=0)
    muts = N_MUTS + BLOCKS_MUTS + ROWS_MUTS + [
        ("inv", narrower), ("inv", pinned), ("inv", strided), ("inv", short), ("inv", column),
        ("gscale", value(float("nan"))), ("gscale", value(float("inf"))),
        ("e", wider), ("e", pinned), ("e", strided), ("e", short), ("e", flat),
        ("loss", wider), ("loss", pinned), ("loss", strided), ("loss", short), ("loss", column),
        ("h", wider), ("h", pinned), ("h", strided), ("h", short), ("h", flat),
        ("h", value(lambda dv: _t(dv, (P, 6), F32))),     # d % 4 != 0
        ("h", value(lambda dv: _t(dv, (P, 516), F32)))]   # d > 512
    return a, muts


@entry("sgns_backward")
def _(d):
    inv, rows = _pairs(d)
    e, _, h = ops.sgns_forward(inv.cpu(), rows.cpu(), N, 1.0 / P)
    order = torch.sort(inv.cpu(), stable=True).indices
    a = dict(members=order.to(I32).to(d), memrow=inv.cpu()[order].to(I32).to(d), inv=inv, e=e.to(d), h=h.to(d),
             rows=rows, N=N, grad_rows=_t(d, (CAP + 1, D), F32, 9.0), blocks=0)
    muts = N_MUTS + BLOCKS_MUTS + ROWS_MUTS + [
        ("members", wider), ("members", pinned), ("members", strided), ("members", short), ("members", column),
        ("memrow", wider), ("memrow", pinned), ("memrow", strided), ("memrow", short), ("memrow", column),
        ("inv", narrower), ("inv", pinned), ("inv", strided), ("inv", short), ("inv", column),
        ("e", wider), ("e", pinned), ("e", strided), ("e", short), ("e", flat),
        ("h", wider), ("h", pinned), ("h", strided), ("h", short), ("h", flat),
        ("grad_rows", wider), ("grad_rows", pinned), ("grad_rows", strided), ("grad_rows", flat),
        ("grad_rows", no_unit_stride), ("grad_rows", value(lambda dv: _t(dv, (CAP, D + 4), F32))),
        ("grad_rows", value(lambda dv: _t(dv, (CAP - 1, D), F32)))]
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
    K_ = _native.w2vk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"sgns_lookups", "sgns_forward", "sgns_backward"}, sorted(exported ^ set(TABLE))
    # the limits of the rule and the thresholds of the backward's paths (csrc/kernels/sgns.h)
    assert (K_.MIN_DIM, K_.MAX_DIM, K_.MAX_NEG) == (ops.SGNS_MIN_DIM, ops.SGNS_MAX_DIM, ops.SGNS_MAX_NEG) == \
        (4, 512, 64)
    assert (K_.GROUP_MAX, K_.WAVE_MAX, K_.CHUNK) == (32, 512, 256) and K_.WAVE_MAX >= 2 * K_.CHUNK
    assert _native.w2vk_available()


def test_the_other_modules_export_none_of_them():
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(), _native.fmk(),
               _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk(), _native.ldak()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.w2vk()
    args = {name: TABLE[name](dev)[0] for name in TABLE}
    for name in sorted(TABLE):
        getattr(K_, name)(*args[name].values())
    torch.cuda.synchronize()
    cpu = {name: TABLE[name](torch.device("cpu"))[0] for name in TABLE}
    a = cpu["sgns_lookups"]
    want = ops.sgns_lookups(a["centres"], a["contexts"], a["thr"], a["alias"], a["T"], a["seed"], a["epoch"],
                            a["pair_base"], N, negatives=a["negatives"])
    assert torch.equal(args["sgns_lookups"]["keys"].cpu(), want)
    a = cpu["sgns_forward"]
    e, loss, h = ops.sgns_forward(a["inv"], a["rows"], N, a["gscale"])
    g = args["sgns_forward"]
    for got, ref in ((g["e"], e), (g["loss"], loss), (g["h"], h)):
        assert (got.cpu() - ref).abs().max() < 1e-5
    assert float(g["e"][1, 2]) == 0.0  # the masked negative
    a = cpu["sgns_backward"]
    grad = torch.full((CAP + 1, D), 9.0)
    ops.sgns_backward(a["inv"], a["e"], a["h"], a["rows"], N, grad)
    got = args["sgns_backward"]["grad_rows"].cpu()
    assert (got - grad).abs().max() < 1e-5 and bool((got[CAP] == 9.0).all())  # the row past cap keeps its fill


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.w2vk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.w2vk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
