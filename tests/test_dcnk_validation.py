"""Argument validation of the _dcnk binding (csrc/bindings/dcn_py.cpp, tensor_access.h), the harness of
test_dfmk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
GPU part: every mutation raises RuntimeError naming the mutated argument and launches nothing (no tensor
argument changes); the valid set is accepted and gives hand-computable values. Every mutation is harmless even if
its check were missing: the mutated argument is backed by memory the kernel may touch at the extent it would
address, or is a scalar the launcher refuses as well, and the backward skips any perm entry outside its range.
CPU part: the valid set on pageable CPU tensors raises RuntimeError naming a tensor argument (the device check comes
before any launch, on every machine)."""
import re
import types

import pytest
import torch

from minips_amd import _native

BF, F32, F64, I32, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
B, F, D, ND, L, LDX = 3, 2, 8, 3, 2, 32
DD = F * D + ND  # d = 19, dp = 24
DP = 24
PCOLS = (L + 1) * DP + 8


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
    x[:, DD:] = float("nan")  # never read
    return x


def _pc(d):
    """w_0 = 0.25, b_0 = 1, w_1 = 0.5, b_1 = 0, w_c = 0.125; NaN in the pad."""
    pc = _t(d, (2 * L + 1, DP), BF, float("nan"))
    for r, v in enumerate((0.25, 1.0, 0.5, 0.0, 0.125)):
        pc[r, :DD] = v
    return pc


X_MUTS = [("X", wider), ("X", pinned),
          ("X", value(lambda dv: _t(dv, (B, 2 * LDX), BF)[:, ::2])),  # no unit column stride
          ("X", value(lambda dv: _t(dv, (B, DD - 1), BF))),  # narrower than d
          ("X", value(lambda dv: _t(dv, (B * LDX,), BF))),  # flat
          ("d", value(0)), ("d", value(-1)), ("d", value(2049)), ("d", value(LDX + 1)),
          ("L", value(0)), ("L", value(5)), ("L", value(-1)),
          ("Pc", wider), ("Pc", pinned), ("Pc", strided), ("Pc", short),
          ("Pc", value(lambda dv: _t(dv, (2 * L + 1, DP + 8), BF))),  # the wrong width
          ("Pc", value(lambda dv: _t(dv, ((2 * L + 1) * DP,), BF)))]  # flat
PK_MUTS = [("p", wider), ("p", pinned), ("p", strided), ("p", short),
           ("p", value(lambda dv: _t(dv, (B, L + 2), F32))), ("p", value(lambda dv: _t(dv, (B * (L + 1),), F32))),
           ("k", wider), ("k", pinned), ("k", strided), ("k", short), ("k", column)]
BLOCK_MUTS = [("blocks", value(-1)), ("blocks", value(65536))]


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("wd_cross_forward")
def _(d):
    a = dict(X=_x(d), d=DD, Pc=_pc(d), L=L, wide=_t(d, (B,), F32, 0.25), p=_t(d, (B, L + 1), F32, -1),
             k=_t(d, (L + 1,), F32, -1), blocks=0)
    muts = X_MUTS + PK_MUTS + BLOCK_MUTS + [("wide", wider), ("wide", pinned), ("wide", strided), ("wide", short),
                                            ("wide", column)]
    return a, muts


# the forward's values of the valid set (exact in fp32): p = 19 * 0.5 * (0.25, 0.5, 0.125), k = (0, 19 * 0.5, 19 / 8)
P_VALID = (2.375, 4.75, 1.1875)
K_VALID = (0.0, 9.5, 2.375)


@entry("wd_cross_backward")
def _(d):
    p = torch.tensor([P_VALID] * B, dtype=F32, device=d)
    a = dict(X=_x(d), d=DD, p=p, k=torch.tensor(K_VALID, dtype=F32, device=d), dwide=_t(d, (B,), F32, 0.5), Pc=_pc(d),
             L=L, perm=torch.arange(B * F - 1, -1, -1, dtype=I32, device=d), dX=_t(d, (B * F, D), BF, 1.0), F=F, D=D,
             part=_t(d, (1, PCOLS), F32, -1), blocks=0)
    muts = X_MUTS + PK_MUTS + BLOCK_MUTS + [
        ("dwide", wider), ("dwide", pinned), ("dwide", strided), ("dwide", short), ("dwide", column),
        ("perm", wider), ("perm", pinned), ("perm", strided), ("perm", short), ("perm", column),
        ("dX", wider), ("dX", pinned), ("dX", strided), ("dX", short),
        ("dX", value(lambda dv: _t(dv, (B * F, D + 8), BF))),  # the wrong width
        ("dX", value(lambda dv: _t(dv, (B * F * D,), BF))),  # flat
        ("F", value(0)), ("F", value(-1)), ("F", value(3)),  # 3 * 8 columns > d
        ("D", value(0)), ("D", value(65)), ("D", value(-8)),
        ("part", wider), ("part", pinned),
        ("part", value(lambda dv: _t(dv, (1, PCOLS - 8), F32))), ("part", value(lambda dv: _t(dv, (2, PCOLS), F32))),
        ("part", value(lambda dv: _t(dv, (PCOLS,), F32)))]
    return a, muts


@entry("wd_cross_fold")
def _(d):
    part = _t(d, (2, PCOLS), F32, 1.0)
    a = dict(part=part, nchunks=2, Pc=_pc(d), d=DD, L=L, Gc=_t(d, (2 * L + 1, DP), F32, 0.5))
    muts = [("part", wider), ("part", pinned), ("part", strided), ("part", short),
            ("part", value(lambda dv: _t(dv, (2, PCOLS + 8), F32))),
            ("part", value(lambda dv: _t(dv, (2 * PCOLS,), F32))),
            ("nchunks", value(1)), ("nchunks", value(3)), ("nchunks", value(-1)),
            ("Pc", wider), ("Pc", pinned), ("Pc", strided), ("Pc", short),
            ("Pc", value(lambda dv: _t(dv, (2 * L + 1, DP + 8), BF))),
            ("d", value(0)), ("d", value(2049)), ("d", value(DD + 8)), ("L", value(0)), ("L", value(5)),
            ("Gc", wider), ("Gc", pinned), ("Gc", strided), ("Gc", short),
            ("Gc", value(lambda dv: _t(dv, (2 * L + 1, DP + 8), F32))),
            ("Gc", value(lambda dv: _t(dv, ((2 * L + 1) * DP,), F32)))]
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
    K_ = _native.dcnk()  # a missing build is an error here, not a skip: build() makes it
    ops = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert ops == set(TABLE) == {"wd_cross_forward", "wd_cross_backward", "wd_cross_fold"}, sorted(ops ^ set(TABLE))
    assert (K_.MAX_D, K_.MAX_L, K_.CHUNK, K_.TRAILER) == (2048, 4, 32, 8)


def test_the_other_modules_export_none_of_them():
    assert set(TABLE) <= set(dir(_native.dcnk()))
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(),
               _native.fmk(), _native.dfmk()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.dcnk()
    fa, _ = TABLE["wd_cross_forward"](dev)
    K_.wd_cross_forward(*fa.values())
    ba, _ = TABLE["wd_cross_backward"](dev)
    K_.wd_cross_backward(*ba.values())
    ba2, _ = TABLE["wd_cross_backward"](dev)
    ba2["perm"] = None
    ba2["dX"] = ba2["dX"].view(B, F * D)  # the lookup-order layout
    K_.wd_cross_backward(*ba2.values())
    ga, _ = TABLE["wd_cross_fold"](dev)
    K_.wd_cross_fold(*ga.values())
    torch.cuda.synchronize()
    # forward: x = 0.5 in 19 columns. s_0 = 2.375, a_1 = 3.375; s_1 = 3.375 * 4.75 + 9.5 = 25.53125, a_2 = 28.90625;
    # c = 28.90625 * 1.1875 + 2.375 = 36.701171875 (every step exact in fp32)
    assert bool((fa["p"] == torch.tensor(P_VALID, device=dev)).all())
    assert bool((fa["k"] == torch.tensor(K_VALID, device=dev)).all())
    assert bool((fa["wide"] == 0.25 + 36.701171875).all())
    assert bool(torch.isnan(fa["X"][:, DD:].float()).all())
    # backward, dz = 0.5: r = 0.59375 = ds_1; r = 0.59375 + 0.59375 * 4.75 = 3.4140625 = ds_0; m = (3.4140625,
    # 0.59375 * 3.375, 0.5 * 28.90625); g = m_0 / 4 + m_1 / 2 + m_2 / 8 = 3.662109375; dX = bf16(1 + g) = 4.65625
    assert bool((ba["dX"] == 4.65625).all()) and bool((ba2["dX"] == 4.65625).all())
    # the chunk's sums: T_j = 3 m_j 0.5 in the 19 columns, zeros in the pad; Sd = 3 (ds_0, ds_1, dz)
    m = (3.4140625, 2.00390625, 14.453125)
    T = ba["part"][0, : 3 * DP].view(3, DP)
    for j in range(3):
        assert bool((T[j, :DD] == 1.5 * m[j]).all()) and bool((T[j, DD:] == 0).all())
    assert ba["part"][0, 3 * DP: 3 * DP + 3].tolist() == [3 * 3.4140625, 3 * 0.59375, 1.5]
    # fold of two chunks of ones (T = 2, Sd = 2): dw_0 = 2, dw_1 = 2 + 1 * 2, dw_c = 2 + 1 * 2;
    # db_1 = 2 * 0.125, db_0 = 0.25 + 2 * 0.5; added to 0.5; the pad keeps 0.5
    G = ga["Gc"]
    for r, v in enumerate((2.5, 1.75, 4.5, 0.75, 4.5)):
        assert bool((G[r, :DD] == v).all()) and bool((G[r, DD:] == 0.5).all()), r


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.dcnk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.dcnk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
