"""Argument validation of the _alsk binding (csrc/bindings/als_py.cpp), the harness of test_w2vk_validation.py: a tiny
valid argument set per exported op and mutations of it. Every mutation raises RuntimeError naming the mutated argument
and launches nothing, and is harmless even if its check were missing (the kernels skip any index out of range); the
valid set is accepted; the valid set on CPU tensors is refused."""
import types

import pytest
import torch

from test_w2vk_validation import (F32, I32, I64, _bytes, _names, _t, _tensors, column, flat, narrower, no_unit_stride,
                                  pinned, short, strided, value, wider)

from minips_amd import _native, ops

K, CAP, M = 8, 5, 4
ROWPTR = [0, 3, 3, 7]


def _rows(d):
    return (torch.randn(CAP, K, generator=torch.Generator().manual_seed(0)) * 0.5).to(d)


ROWS_MUTS = [("rows", wider), ("rows", pinned), ("rows", flat), ("rows", no_unit_stride),
             ("rows", value(lambda dv: _t(dv, (CAP, K - 4), F32)))]  # narrower than k


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _solve(d):
    g = torch.Generator().manual_seed(1)
    rowptr = torch.tensor(ROWPTR, dtype=I64)
    desc, multi, nmd = ops.als_chunks(rowptr, 2)   # entities 0 and 2 have two chunks each
    a = dict(rowptr=rowptr.to(d), inv=torch.tensor([0, 1, 4, 2, 2, 3, 0], dtype=I64, device=d),
             a=(torch.rand(7, generator=g) + 0.5).to(d), c=torch.randn(7, generator=g).to(d), rows=_rows(d),
             reg=torch.tensor([0.3, 0.1, 0.4], device=d), slot=torch.tensor([2, 0, 1], dtype=I64, device=d),
             x_old=torch.randn(M, K, generator=g).to(d), x_out=_t(d, (M, K), F32, 9.0), delta=_t(d, (M, K), F32, 9.0),
             desc=desc.to(d), multi=multi.to(d), n_multi_desc=nmd, gram0=(0.1 * torch.eye(K)).to(d),
             bad=_t(d, (1,), I32), blocks=0)
    f32, i64 = (wider, pinned, strided, short), (narrower, pinned, strided, short)
    per = dict(rowptr=i64 + (column,), inv=i64 + (column,), a=f32, c=f32, reg=f32, slot=i64, x_old=f32, delta=f32,
               x_out=(wider, pinned, strided, flat, value(lambda dv: _t(dv, (M, 6), F32)),
                      value(lambda dv: _t(dv, (M, 132), F32))),
               desc=(wider, pinned, flat), multi=(wider, pinned, flat), n_multi_desc=(value(-1), value(1), value(99)),
               gram0=f32, bad=(wider, pinned, value(lambda dv: _t(dv, (2,), I32))), blocks=(value(-1), value(65536)))
    muts = ROWS_MUTS + [(arg, mut) for arg, ms in per.items() for mut in ms]
    return a, muts


def _gram(d):
    a = dict(rows=_rows(d), out=_t(d, (K, K), F32, 9.0))
    muts = ROWS_MUTS + [("out", wider), ("out", pinned), ("out", strided), ("out", flat),
                        ("out", value(lambda dv: _t(dv, (K, K + 4), F32))),
                        ("out", value(lambda dv: _t(dv, (6, 6), F32)))]
    return a, muts


TABLE = dict(als_solve=_solve, als_gram=_gram)


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](torch.device("cpu"))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_exported_op_is_in_the_table():
    K_ = _native.alsk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"als_solve", "als_gram"}, sorted(exported ^ set(TABLE))
    assert (K_.MIN_K, K_.MAX_K, K_.MAX_CHUNK) == (ops.ALS_MIN_K, ops.ALS_MAX_K, ops.ALS_MAX_CHUNK) == (4, 128, 1 << 20)
    assert (K_.STAGE, K_.GRAM_STRIP) == (64, 256) and _native.alsk_available()
    for other in (_native.kernels(), _native.fmk(), _native.ldak(), _native.w2vk()):
        assert not set(TABLE) & set(dir(other))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.alsk()
    args = {name: TABLE[name](dev)[0] for name in TABLE}
    for name in sorted(TABLE):
        getattr(K_, name)(*args[name].values())
    torch.cuda.synchronize()
    a = TABLE["als_solve"](torch.device("cpu"))[0]
    x_out, delta = torch.full((M, K), 9.0), torch.full((M, K), 9.0)
    ops.als_solve(a["rowptr"], a["inv"], a["a"], a["c"], a["rows"], a["reg"], a["slot"], a["x_old"], x_out, delta,
                  None, gram0=a["gram0"])
    g = args["als_solve"]
    assert (g["x_out"].cpu() - x_out).abs().max() < 1e-4 and (g["delta"].cpu() - delta).abs().max() < 1e-4
    assert bool((g["x_out"][3] == 9.0).all()) and int(g["bad"]) == 0   # the row of no slot keeps its fill
    assert torch.equal(g["x_out"][0].cpu(), a["x_old"][0])               # entity 1 has no lookup
    assert (args["als_gram"]["out"].cpu() - ops.als_gram(a["rows"])).abs().max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.alsk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.alsk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
