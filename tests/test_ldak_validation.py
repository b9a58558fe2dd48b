"""Argument validation of the _ldak binding (csrc/bindings/lda_py.cpp, tensor_access.h), the harness of
test_gbdtk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
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

F32, F64, I16, I32, I64, U8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8
B, N, K, W, CAP = 2, 5, 3, 4, 3


def wider(t):  # same element count, a larger element type
    return t.to({F32: F64, I16: I32, I32: I64}[t.dtype])


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


def _docs(d):
    """Two documents (3 and 2 tokens) over three pulled rows."""
    return dict(rowptr=torch.tensor([0, 3, 5], dtype=I64, device=d), inv=torch.tensor([0, 1, 0, 2, 1], dtype=I64,
                                                                                     device=d),
                rows=torch.tensor([[2.0, 0.0, 1.0, 0.0], [0.0, 3.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0]], device=d),
                nk=torch.tensor([3, 4, 2], dtype=I64, device=d))


def _z(d):
    return torch.tensor([0, 1, 2, 1, 1], dtype=I16, device=d)


DOC_MUTS = [("rowptr", narrower), ("rowptr", pinned), ("rowptr", strided), ("rowptr", column),
            ("rowptr", value(lambda dv: _t(dv, (0,), I64))),
            ("inv", narrower), ("inv", pinned), ("inv", strided), ("inv", column),
            ("rows", wider), ("rows", pinned), ("rows", flat), ("rows", no_unit_stride),
            ("rows", value(lambda dv: _t(dv, (CAP, K - 1), F32))),  # narrower than K
            ("nk", narrower), ("nk", pinned), ("nk", strided), ("nk", column),
            ("nk", value(lambda dv: _t(dv, (1,), I64))), ("nk", value(lambda dv: _t(dv, (1025,), I64)))]
PRIOR_MUTS = [("alpha", value(0.0)), ("alpha", value(-1.0)), ("alpha", value(64.5)), ("alpha", value(float("nan"))),
              ("beta", value(0.0)), ("beta", value(65.0)), ("beta", value(float("nan"))),
              ("Vbeta", value(0.0)), ("Vbeta", value(float("inf"))), ("Vbeta", value(float("nan")))]
BLOCKS_MUTS = [("blocks", value(-1)), ("blocks", value(65536))]


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("lda_sample")
def _(d):
    t = _docs(d)
    a = dict(rowptr=t["rowptr"], gid=torch.tensor([7, 1 << 40], dtype=I64, device=d), inv=t["inv"], z_old=_z(d),
             rows=t["rows"], nk=t["nk"], alpha=0.1, beta=0.01, Vbeta=0.05, seed=11, it=2, z_new=_t(d, (N,), I16, 9),
             dk=_t(d, (K,), I64), blocks=0)
    muts = DOC_MUTS + PRIOR_MUTS + BLOCKS_MUTS + [
        ("gid", narrower), ("gid", pinned), ("gid", strided), ("gid", short), ("gid", column),
        ("z_old", wider), ("z_old", pinned), ("z_old", strided), ("z_old", short), ("z_old", column),
        ("z_old", value(None)),  # a sweep without topics
        ("it", value(0)),        # the initialisation with topics
        ("it", value(-1)),
        ("z_new", wider), ("z_new", pinned), ("z_new", strided), ("z_new", short), ("z_new", column),
        ("dk", narrower), ("dk", pinned), ("dk", strided), ("dk", short), ("dk", column)]
    return a, muts


@entry("lda_delta")
def _(d):
    # the lookup CSR of inv = (0, 1, 0, 2, 1): row 0 <- tokens 0, 2; row 1 <- 1, 4; row 2 <- 3
    a = dict(members=torch.tensor([0, 2, 1, 4, 3], dtype=I32, device=d),
             memrow=torch.tensor([0, 0, 1, 1, 2], dtype=I32, device=d), z_old=_z(d),
             z_new=torch.tensor([1, 1, 0, 2, 0], dtype=I16, device=d), K=K, delta=_t(d, (CAP + 1, W), F32, 9.0),
             blocks=0)
    muts = BLOCKS_MUTS + [
        ("members", wider), ("members", pinned), ("members", strided), ("members", short), ("members", column),
        ("memrow", wider), ("memrow", pinned), ("memrow", strided), ("memrow", short),
        ("z_old", wider), ("z_old", pinned), ("z_old", strided), ("z_old", short),
        ("z_new", wider), ("z_new", pinned), ("z_new", strided), ("z_new", column),
        ("K", value(1)), ("K", value(1025)),
        ("K", value(5)),  # delta is align4(3) = 4 wide, not align4(5)
        ("delta", wider), ("delta", pinned), ("delta", strided), ("delta", flat), ("delta", no_unit_stride)]
    return a, muts


@entry("lda_loglik")
def _(d):
    t = _docs(d)
    a = dict(rowptr=t["rowptr"], inv=t["inv"], z=_z(d), rows=t["rows"], nk=t["nk"], alpha=0.1, beta=0.01, Vbeta=0.05,
             acc=_t(d, (2,), I64), blocks=0)
    muts = DOC_MUTS + PRIOR_MUTS + BLOCKS_MUTS + [
        ("z", wider), ("z", pinned), ("z", strided), ("z", short), ("z", column),
        ("acc", narrower), ("acc", pinned), ("acc", strided), ("acc", short), ("acc", column),
        ("acc", value(lambda dv: _t(dv, (3,), I64)))]
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
    K_ = _native.ldak()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"lda_sample", "lda_delta", "lda_loglik"}, sorted(exported ^ set(TABLE))
    from minips_amd import ops as O

    # the limits of the rule and the thresholds of lda_delta's paths (csrc/kernels/lda.h)
    assert (K_.MIN_K, K_.MAX_K, K_.MAX_DOC_LEN) == (O.LDA_MIN_K, O.LDA_MAX_K, O.LDA_MAX_DOC_LEN) == (2, 1024, 4096)
    assert (K_.WAVE_MAX, K_.CHUNK) == (2048, 1024) and K_.WAVE_MAX >= 2 * K_.CHUNK
    assert _native.ldak_available()


def test_the_other_modules_export_none_of_them():
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(), _native.fmk(),
               _native.dfmk(), _native.dcnk(), _native.ffmk(), _native.gbdtk()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.ldak()
    args = {name: TABLE[name](dev)[0] for name in TABLE}
    for name in sorted(TABLE):
        getattr(K_, name)(*args[name].values())
    torch.cuda.synchronize()
    s = args["lda_sample"]
    zn = s["z_new"].tolist()
    assert all(0 <= v < K for v in zn)
    want = [0] * K
    for o, v in zip(_z("cpu").tolist(), zn):
        want[o] -= 1
        want[v] += 1
    assert s["dk"].tolist() == want
    # delta: row 0 <- tokens 0 (0 -> 1), 2 (2 -> 0); row 1 <- 1 (1 -> 1), 4 (1 -> 0); row 2 <- 3 (1 -> 2); the pad
    # column is written as 0, the row without members keeps its fill
    assert args["lda_delta"]["delta"].tolist() == [[0.0, 1.0, -1.0, 0.0], [1.0, -1.0, 0.0, 0.0],
                                                   [0.0, -1.0, 1.0, 0.0], [9.0] * 4]
    a = args["lda_loglik"]["acc"].tolist()
    assert a[1] == N and 0 < a[0] < N * 10 * (1 << 24)


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ldak(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.ldak(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
