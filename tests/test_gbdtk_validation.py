"""Argument validation of the _gbdtk binding (csrc/bindings/gbdt_py.cpp, tensor_access.h), the harness of
test_ffmk_validation.py: one table entry per exported op -- a tiny valid argument set and mutations of it.
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
N, NF, NB, NODES, DEPTH, T = 6, 3, 4, 2, 2, 2
LDB = 16


def wider(t):  # same element count, a larger element type
    return t.to({F32: F64, I32: I64, U8: I32}[t.dtype])


def narrower(t):  # int64 -> int32 / fp64 -> fp32 inside a buffer of the larger size
    small = {I64: I32, F64: F32}[t.dtype]
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


def _bins(d):
    b = _t(d, (N, LDB), U8)
    b[:, :NF] = torch.tensor([[0, 1, 2], [1, 2, 3], [2, 3, 0], [3, 0, 1], [0, 0, 0], [3, 3, 3]], dtype=U8)
    return b


def _node(d):
    return torch.tensor([0, 1, 0, 1, 1, 0], dtype=I32, device=d)


def _gh(d):
    return torch.tensor([[4, 1], [-4, 2], [8, 3], [-8, 4], [2, 5], [-2, 6]], dtype=I32, device=d)


BINS_MUTS = [("bins", wider), ("bins", pinned), ("bins", short), ("bins", flat), ("bins", no_unit_stride),
             ("bins", value(lambda dv: _t(dv, (N, NF - 1), U8)))]  # narrower than F
BLOCKS_MUTS = [("blocks", value(-1)), ("blocks", value(65536))]


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
@entry("gbdt_bin")
def _(d):
    a = dict(X=torch.tensor([[-1.0, 0.0, 1.0]] * N, device=d),
             cuts=torch.tensor([[-0.5, 0.5, float("inf")]] * NF, device=d), bins=_t(d, (N, LDB), U8, 9), blocks=0)
    muts = [("X", wider), ("X", pinned), ("X", flat), ("X", no_unit_stride),
            ("X", value(lambda dv: _t(dv, (N, NF + 1), F32))),  # another feature count than cuts
            ("cuts", wider), ("cuts", pinned), ("cuts", strided), ("cuts", flat),
            ("cuts", value(lambda dv: _t(dv, (NF, 0), F32))), ("cuts", value(lambda dv: _t(dv, (NF, 256), F32))),
            ("cuts", value(lambda dv: _t(dv, (4097, 3), F32)))] + BINS_MUTS + BLOCKS_MUTS
    return a, muts


@entry("gbdt_grad")
def _(d):
    a = dict(z=torch.tensor([0.0, 1.0, -1.0, 40.0, -40.0, 0.5], device=d),
             labels=torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0], device=d), gh=_t(d, (N, 2), I32, 9),
             loss_acc=_t(d, (1,), I64), blocks=0)
    muts = [("z", wider), ("z", pinned), ("z", strided), ("z", column),
            ("labels", wider), ("labels", pinned), ("labels", strided), ("labels", short), ("labels", column),
            ("gh", wider), ("gh", pinned), ("gh", strided), ("gh", short), ("gh", flat),
            ("gh", value(lambda dv: _t(dv, (N, 3), I32))),
            ("loss_acc", narrower), ("loss_acc", pinned), ("loss_acc", value(lambda dv: _t(dv, (0,), I64))),
            ("loss_acc", value(lambda dv: _t(dv, (2,), I64))), ("loss_acc", column)] + BLOCKS_MUTS
    return a, muts


@entry("gbdt_hist")
def _(d):
    a = dict(bins=_bins(d), node=_node(d), gh=_gh(d), hist=_t(d, (NODES, NF, NB, 3), I64), path=0, blocks=0)
    muts = BINS_MUTS + [("node", wider), ("node", pinned), ("node", strided), ("node", column),
                        ("gh", wider), ("gh", pinned), ("gh", strided), ("gh", short), ("gh", flat),
                        ("hist", narrower), ("hist", pinned), ("hist", strided), ("hist", flat),
                        ("hist", value(lambda dv: _t(dv, (3, NF, NB, 3), I64))),  # nodes: no power of two
                        ("hist", value(lambda dv: _t(dv, (256, NF, NB, 3), I64))),
                        ("hist", value(lambda dv: _t(dv, (NODES, NF, 1, 3), I64))),
                        ("hist", value(lambda dv: _t(dv, (NODES, NF, 257, 3), I64))),
                        ("hist", value(lambda dv: _t(dv, (NODES, NF, NB, 4), I64))),
                        ("path", value(-1)), ("path", value(3))] + BLOCKS_MUTS
    return a, muts


def _hist(d):
    h = _t(d, (NODES, NF, NB, 3), I64)
    h[..., 2] = 2
    h[..., 1] = 1 << 19
    h[:, :, :2, 0] = 1 << 19
    h[:, :, 2:, 0] = -(1 << 19)
    return h


@entry("gbdt_split")
def _(d):
    a = dict(hist=_hist(d), reg_lambda=1.0, min_child_count=1, min_gain=0.0, feat=_t(d, (NODES,), I32, 9),
             thr=_t(d, (NODES,), I32, 9), gain=_t(d, (NODES,), F64, 9.0), child=_t(d, (NODES, 2, 3), I64, 9))
    muts = [("hist", narrower), ("hist", pinned), ("hist", strided), ("hist", flat),
            ("hist", value(lambda dv: _t(dv, (3, NF, NB, 3), I64))),
            ("hist", value(lambda dv: _t(dv, (NODES, NF, 1, 3), I64))),
            ("hist", value(lambda dv: _t(dv, (NODES, NF, NB, 2), I64))),
            ("reg_lambda", value(0.0)), ("reg_lambda", value(-1.0)), ("reg_lambda", value(float("nan"))),
            ("reg_lambda", value(float("inf"))),
            ("min_child_count", value(0)), ("min_child_count", value(-3)),
            ("min_gain", value(-0.5)), ("min_gain", value(float("nan"))), ("min_gain", value(float("inf"))),
            ("feat", wider), ("feat", pinned), ("feat", strided), ("feat", short), ("feat", column),
            ("thr", wider), ("thr", pinned), ("thr", strided), ("thr", short), ("thr", column),
            ("gain", narrower), ("gain", pinned), ("gain", strided), ("gain", short), ("gain", column),
            ("child", narrower), ("child", pinned), ("child", strided), ("child", short), ("child", flat),
            ("child", value(lambda dv: _t(dv, (NODES, 3, 2), I64)))]
    return a, muts


@entry("gbdt_leaf")
def _(d):
    c = _t(d, (NODES, 2, 3), I64)
    c[..., 0], c[..., 1], c[..., 2] = 1 << 20, 1 << 20, 4
    a = dict(child=c, reg_lambda=1.0, lr=0.5, leaf=_t(d, (2 * NODES,), F32, 9.0))
    muts = [("child", narrower), ("child", pinned), ("child", strided), ("child", flat),
            ("child", value(lambda dv: _t(dv, (3, 2, 3), I64))),
            ("child", value(lambda dv: _t(dv, (NODES, 2, 2), I64))),
            ("reg_lambda", value(0.0)), ("reg_lambda", value(float("nan"))),
            ("lr", value(0.0)), ("lr", value(-0.1)), ("lr", value(float("inf"))),
            ("leaf", wider), ("leaf", pinned), ("leaf", strided), ("leaf", short), ("leaf", column)]
    return a, muts


@entry("gbdt_advance")
def _(d):
    a = dict(bins=_bins(d), node=_node(d), feat=torch.tensor([1, -1], dtype=I32, device=d),
             thr=torch.tensor([1, 0], dtype=I32, device=d), F=NF, leaf=torch.tensor([0.5, 1.0, 2.0, 4.0], device=d),
             z=_t(d, (N,), F32, 1.0), blocks=0)
    muts = BINS_MUTS + [("node", wider), ("node", pinned), ("node", strided), ("node", column),
                        ("feat", wider), ("feat", pinned), ("feat", strided), ("feat", column),
                        ("feat", value(lambda dv: _t(dv, (3,), I32))), ("feat", value(lambda dv: _t(dv, (0,), I32))),
                        ("thr", wider), ("thr", pinned), ("thr", strided), ("thr", short), ("thr", column),
                        ("F", value(0)), ("F", value(-1)), ("F", value(4097)),
                        ("leaf", wider), ("leaf", pinned), ("leaf", strided), ("leaf", short), ("leaf", column),
                        ("leaf", value(None)),  # leaf and z come together
                        ("z", wider), ("z", pinned), ("z", strided), ("z", short), ("z", column),
                        ("z", value(None))] + BLOCKS_MUTS
    return a, muts


@entry("gbdt_predict")
def _(d):
    nn = (1 << DEPTH) - 1
    a = dict(bins=_bins(d), feat=torch.tensor([[0, 1, -1], [2, 2, 0]], dtype=I32, device=d),
             thr=torch.tensor([[1, 0, 0], [2, 1, 0]], dtype=U8, device=d),
             leaf=torch.tensor([[1.0, 2.0, 4.0, 8.0], [16.0, 32.0, 64.0, 128.0]], device=d), F=NF, depth=DEPTH,
             base=0.5, z=_t(d, (N,), F32, 9.0), leaf_index=_t(d, (N, T), I32, 9), blocks=0)
    muts = BINS_MUTS + [("feat", wider), ("feat", pinned), ("feat", strided), ("feat", flat),
                        ("feat", value(lambda dv: _t(dv, (T, nn + 1), I32))),
                        ("thr", wider), ("thr", pinned), ("thr", strided), ("thr", short), ("thr", flat),
                        ("leaf", wider), ("leaf", pinned), ("leaf", strided), ("leaf", short), ("leaf", flat),
                        ("leaf", value(lambda dv: _t(dv, (T, nn), F32))),
                        ("F", value(0)), ("F", value(4097)),
                        ("depth", value(0)), ("depth", value(9)), ("depth", value(-1)),
                        ("base", value(float("nan"))), ("base", value(float("inf"))),
                        ("z", wider), ("z", pinned), ("z", strided), ("z", column),
                        ("leaf_index", wider), ("leaf_index", pinned), ("leaf_index", strided),
                        ("leaf_index", short), ("leaf_index", flat)] + BLOCKS_MUTS
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
    K_ = _native.gbdtk()  # a missing build is an error here, not a skip: build() makes it
    exported = {n for n in dir(K_) if not n.startswith("_") and callable(getattr(K_, n))}
    assert exported == set(TABLE) == {"gbdt_bin", "gbdt_grad", "gbdt_hist", "gbdt_split", "gbdt_leaf", "gbdt_advance",
                                      "gbdt_predict"}, sorted(exported ^ set(TABLE))
    from minips_amd import ops as O

    # the limits of the rule and the flush bound of the LDS accumulators (csrc/kernels/gbdt.h)
    assert (K_.MAX_BINS, K_.MAX_DEPTH, K_.MAX_F) == (O.GBDT_MAX_BINS, O.GBDT_MAX_DEPTH, O.GBDT_MAX_F) == (256, 8, 4096)
    assert 1 << K_.SCALE_BITS == O.GBDT_SCALE == 1 << 20
    assert K_.FLUSH_ROWS << K_.SCALE_BITS < 1 << 31 and K_.LDS_BYTES <= 160 * 1024


def test_the_other_modules_export_none_of_them():
    for K_ in (_native.kernels(), _native.evalk(), _native.optk(), _native.ftrlk(), _native.wdftrlk(), _native.fmk(),
               _native.dfmk(), _native.dcnk(), _native.ffmk()):
        assert not set(TABLE) & set(dir(K_))


@pytest.mark.gpu
def test_valid_arguments_are_accepted(dev):
    K_ = _native.gbdtk()
    args = {name: TABLE[name](dev)[0] for name in TABLE}
    for name in sorted(TABLE):
        getattr(K_, name)(*args[name].values())
    torch.cuda.synchronize()
    # bin: x = (-1, 0, 1) against cuts (-0.5, 0.5, inf): bins 0, 1, 2; the other columns untouched
    b = args["gbdt_bin"]["bins"].cpu()
    assert b[:, :NF].tolist() == [[0, 1, 2]] * N and bool((b[:, NF:] == 9).all())
    # grad: z = 0, y = 1: p = 0.5 exactly
    g = args["gbdt_grad"]
    assert g["gh"][0].tolist() == [-(1 << 19), 1 << 18] and int(g["gh"][:, 1].min()) >= 1
    assert g["gh"][3].tolist() == [1 << 20, 1] and int(g["loss_acc"]) > 0  # z = 40 clamps to 30, y = 0
    # hist: every sample once per feature
    h = args["gbdt_hist"]["hist"].cpu()
    assert h[..., 2].sum(2).tolist() == [[3] * NF, [3] * NF] and int(h[..., 0].sum()) == 0 and \
        int(h[0, 0, 0, 1]) == 1 and int(h[1, 0, 0, 1]) == 5
    # split: bins 0, 1 hold +2^19 each, bins 2, 3 -2^19 each, 2 samples a bin: the cut after bin 1, feature 0
    s = args["gbdt_split"]
    assert s["feat"].tolist() == [0, 0] and s["thr"].tolist() == [1, 1]
    assert s["child"][0].tolist() == [[1 << 20, 1 << 20, 4], [-(1 << 20), 1 << 20, 4]]
    assert s["gain"].tolist() == [1.0, 1.0]  # 1 / 2 + 1 / 2 - 0 / 3
    # leaf: -(1) / (1 + 1) * 0.5
    assert args["gbdt_leaf"]["leaf"].tolist() == [-0.25] * 4
    # advance: node 0 splits on feature 1 at 1, node 1 passes everything left; z += leaf
    a = args["gbdt_advance"]
    assert a["node"].tolist() == [0, 2, 1, 2, 2, 1] and a["z"].tolist() == [1.5, 3.0, 2.0, 3.0, 3.0, 2.0]
    # predict: tree 0 = (f0 > 1; left: f1 > 0; right: all left), tree 1 = (f2 > 2; left: f2 > 1; right: f0 > 0)
    p = args["gbdt_predict"]
    assert p["leaf_index"].tolist() == [[1, 1], [1, 3], [2, 0], [2, 0], [0, 0], [2, 3]]
    assert p["z"].tolist() == [0.5 + 2 + 32, 0.5 + 2 + 128, 0.5 + 4 + 16, 0.5 + 4 + 16, 0.5 + 1 + 16, 0.5 + 4 + 128]


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    args, muts = TABLE[name](dev)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native.gbdtk(), name)(*args.values())
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    args, _ = TABLE[name](torch.device("cpu"))
    with pytest.raises(RuntimeError) as e:
        getattr(_native.gbdtk(), name)(*args.values())
    assert any(_names(a).search(str(e.value)) for a in args), f"{name}: {e.value}"
