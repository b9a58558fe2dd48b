"""Argument validation of the _kernels bindings (csrc/bindings/ops_py.cpp, tensor_access.h).

One table entry per registered op and per LaunchList op: a tiny valid argument set and mutations
of it. GPU part: every mutation raises RuntimeError naming the mutated argument and launches
nothing (no tensor argument changes); the valid set is accepted. Every mutation is harmless even
if its check were missing -- the mutated argument is backed by memory the kernel may touch at the
valid extent and still holds valid indices, keys and device addresses (a wider or reinterpreted
dtype at the same element count with the original values readable, a narrow view of the full-size
buffer, a transposed same-size buffer of float data, a pinned host copy, or a scalar that only
shrinks what is addressed) -- so a missing check shows up as "did not raise", never as a GPU fault.
CPU part (no GPU): every entry's valid set on pageable
CPU tensors raises RuntimeError naming a tensor argument (the device check).
"""
import re
import types

import pytest
import torch

from minips_amd import _native

BF, F32, F64, I32, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
WIDER = {BF: F32, F32: F64}  # float data only: what a kernel reads from it are values, never indices

# host objects and stream helpers: no tensors to validate (LaunchList's ops are table entries)
EXEMPT = {"Rccl", "AsyncServer", "FastEvent", "HostWord", "LaunchList", "new_stream", "wire_spin", "ipc_alloc",
          "ipc_open", "ps_set_fences", "rccl_unique_id"}
LAUNCHLIST_EXEMPT = {"fork", "run", "size"}
EPI_STORE_BF16 = 4  # (asserted against the module's attribute below)


# ---- mutations ------------------------------------------------------------------------------------
def wider(t):
    """A dtype of equal or larger element size at the same element count, whose memory read with the
    ORIGINAL element type still holds valid indices / keys / addresses: int64 is reinterpreted (same
    bits), int32 -> int64 words whose two halves both read as the original value, floats are converted."""
    if t.dtype == I64:
        return t.view(F64)
    if t.dtype == I32:
        low = t.to(I64) & 0xFFFFFFFF
        return low | (low << 32)
    return t.to(WIDER[t.dtype])


def short(t):  # one element (row) less: a narrow view of the full-size buffer
    return t[:-1]


def transposed(t):  # same shape, a non-contiguous view of a same-size buffer
    assert t.dim() == 2 and min(t.shape) > 1
    return torch.zeros(t.shape[1], t.shape[0], dtype=t.dtype, device=t.device).t()


def pinned(t):  # the same contents (indices and addresses stay valid) in page-locked host memory
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)


def value(v):  # replaces a scalar, or None by a tensor (v may be a callable taking the device)
    return lambda old, dev=None: v


class Case:
    def __init__(self, dev):
        self.dev = dev
        self.keep = []  # buffers addressed through raw device addresses

    def t(self, shape, dtype, fill=None):
        x = torch.zeros(shape, dtype=dtype, device=self.dev)
        if fill is not None:
            x += torch.as_tensor(fill, dtype=dtype, device=self.dev)
        return x

    def v(self, vals, dtype=I64):
        return torch.tensor(vals, dtype=dtype, device=self.dev)

    def addr(self, *bufs):  # int64 tensor of the buffers' device addresses
        self.keep += bufs
        return self.v([b.data_ptr() for b in bufs])


TABLE = {}


def entry(name):
    def reg(fn):
        TABLE[name] = fn
        return fn
    return reg


# every entry returns (args: dict in positional order, mutations: [(argument, mutation)])
def _gemm_args(c):
    return dict(A=c.t((8, 8), BF, 1), B=c.t((8, 8), BF, 1), C=c.t((8, 8), BF, 3), M=8, N=8, K=8, a_km=False,
                b_kn=False, epi=EPI_STORE_BF16, bias=None, mask=None, colsum=None, alpha=1.0, split_k=1)


_GEMM_MUTS = [("A", wider), ("A", short), ("A", pinned), ("B", wider), ("B", transposed), ("C", wider), ("C", short),
              ("K", value(4)), ("bias", value(lambda d: torch.zeros(8, dtype=F32, device=d))),
              ("bias", value(lambda d: torch.zeros(8, dtype=BF, device=d)[:7])),
              ("colsum", value(lambda d: torch.zeros(8, dtype=F64, device=d)))]


@entry("gemm")
def _(c):
    a = _gemm_args(c)
    a.update(batch=1, inner=1, lda=0, ldb=0, ldc=0, strides=[], perm=None, seg=0, tile=0)
    return a, _GEMM_MUTS + [("perm", value(lambda d: torch.zeros(8, dtype=I64, device=d)))]


@entry("LaunchList.gemm")
def _(c):
    a = _gemm_args(c)
    a.update(perm=None, seg=0, tile=0)
    return a, _GEMM_MUTS


def _gemm_slab(c):
    a = dict(A=c.t((8, 8), BF, 1), B=c.t((8, 8), BF, 1), slab=c.t((64,), F32, 3), M=8, N=8, K=8, a_km=True, b_kn=True,
             split_k=1)
    return a, [("A", wider), ("A", short), ("A", pinned), ("B", wider), ("B", short), ("slab", wider), ("slab", short),
               ("K", value(4)), ("M", value(4)), ("N", value(4))]


TABLE["gemm_slab"] = TABLE["LaunchList.gemm_slab"] = _gemm_slab


def _colsum(c):
    a = dict(x=c.t((8, 16), BF, 1), out=c.t((16,), F32, 3))
    return a, [("x", wider), ("x", pinned), ("x", transposed), ("out", wider), ("out", short)]


TABLE["colsum_bf16"] = TABLE["LaunchList.colsum_bf16"] = _colsum


def _head_fold(c):
    a = dict(B=8, Hd=64, dw=c.t((64,), F32, 3), db=c.t((1,), F32, 3), loss_sum=c.t((1,), F32, 3), dH_colsum=None)
    return a, [("dw", wider), ("dw", short), ("db", wider), ("db", pinned), ("loss_sum", wider), ("loss_sum", pinned),
               ("dH_colsum", value(lambda d: torch.zeros(64, dtype=F64, device=d))),
               ("dH_colsum", value(lambda d: torch.zeros(64, dtype=F32, device=d)[:63]))]


TABLE["wd_head_fold"] = TABLE["LaunchList.wd_head_fold"] = _head_fold


@entry("layernorm_fwd")
def _(c):
    a = dict(x=c.t((8, 16), BF, 1), C=16, gamma=c.t((16,), BF, 1), beta=c.t((16,), BF), eps=1e-5, y=c.t((8, 16), BF, 3),
             mean=c.t((8,), F32, 3), rstd=c.t((8,), F32, 3))
    return a, [("x", wider), ("gamma", wider), ("gamma", short), ("beta", pinned), ("y", wider), ("y", short),
               ("mean", wider), ("rstd", short), ("C", value(6))]


@entry("layernorm_bwd")
def _(c):
    a = dict(x=c.t((8, 16), BF, 1), dy=c.t((8, 16), BF, 1), C=16, gamma=c.t((16,), BF, 1), mean=c.t((8,), F32),
             rstd=c.t((8,), F32, 1), dx=c.t((8, 16), BF, 3), dgamma=c.t((16,), F32, 3), dbeta=c.t((16,), F32, 3),
             accumulate=False)
    return a, [("dy", wider), ("gamma", wider), ("gamma", pinned), ("gamma", short), ("mean", wider), ("mean", pinned),
               ("rstd", wider), ("rstd", pinned), ("dx", short), ("dgamma", wider), ("dgamma", short),
               ("dgamma", pinned), ("dbeta", wider), ("dbeta", short), ("dbeta", pinned)]


@entry("softmax_xent")
def _(c):
    a = dict(logits=c.t((8, 16), BF, 1), V=16, labels=c.v(list(range(8))), scale=1.0, loss_sum=c.t((1,), F32, 3),
             correct=None)
    return a, [("logits", wider), ("labels", wider), ("labels", short), ("loss_sum", wider), ("loss_sum", pinned),
               ("correct", value(lambda d: torch.zeros(1, dtype=F64, device=d)))]


@entry("causal_softmax_fwd")
def _(c):
    a = dict(S=c.t((8, 8), F32, 1), T=8, P=c.t((8, 8), BF, 3))
    return a, [("S", wider), ("S", pinned), ("P", wider), ("P", short)]


@entry("causal_softmax_bwd")
def _(c):
    a = dict(P=c.t((8, 8), BF, 1), dP=c.t((8, 8), F32, 1), T=8, scale=1.0, dS=c.t((8, 8), BF, 3))
    return a, [("P", wider), ("dP", wider), ("dP", short), ("dS", wider), ("dS", short)]


@entry("gelu_bwd")
def _(c):
    a = dict(dh=c.t((64,), BF, 1), u=c.t((64,), BF, 1), du=c.t((64,), BF, 3))
    return a, [("dh", wider), ("dh", pinned), ("dh", short), ("u", wider), ("u", pinned), ("u", short), ("du", wider),
               ("du", pinned), ("du", short)]


@entry("add_bf16")
def _(c):
    a = dict(a=c.t((64,), BF, 1), b=c.t((64,), BF, 1), out=c.t((64,), BF, 3))
    return a, [("a", wider), ("b", wider), ("b", short), ("out", wider), ("out", short)]


@entry("dlrm_interact_fwd")
def _(c):
    a = dict(V=c.t((8, 48), BF, 1), NV=3, D=16, dense_idx=0, out=c.t((8, 24), BF, 3))
    return a, [("V", wider), ("out", wider), ("out", short)]


@entry("dlrm_interact_bwd")
def _(c):
    a = dict(V=c.t((8, 48), BF, 1), NV=3, D=16, dense_idx=0, dout=c.t((8, 24), BF, 1), dV=c.t((8, 48), F32, 3),
             d_dense=c.t((8, 16), BF, 3))
    return a, [("V", wider), ("dout", wider), ("dout", short), ("dV", wider), ("dV", short), ("d_dense", wider),
               ("d_dense", short)]


@entry("unique_bucketize")
def _(c):
    a = dict(keys=c.v([5, 3, 5, 9, 1, 3, 7, 7]), bounds=c.v([0, 1 << 40]), F=1, route_mult=0, route_n=0,
             extra_zero_ints=0, csr_counts=False)
    return a, [("keys", wider), ("keys", pinned), ("bounds", wider), ("bounds", short)]


@entry("bitmap_plan")
def _(c):
    a = dict(keys=c.v([5, 3, 5, 9, 1, 3, 7, 7]), bounds=c.v([0, 32]), num_rows=32, route_mult=0, route_n=0, oor=None)
    return a, [("keys", wider), ("bounds", wider), ("bounds", short),
               ("oor", value(lambda d: torch.zeros(1, dtype=F64, device=d)))]


@entry("plan_sorted")
def _(c):
    keys = torch.stack([torch.arange(8) % 5, 16 + torch.arange(8) % 3], 1).to(c.dev)
    a = dict(keys=keys.contiguous(), col_base=c.v([0, 16]), col_bits=c.v([4, 4], I32), col_bits_host=[4, 4],
             route_mult=0, route_n=0, bounds=c.v([0, 1 << 40]), with_positions=False)
    return a, [("keys", wider), ("col_base", wider), ("col_base", short), ("col_bits", wider), ("col_bits", short),
               ("bounds", wider), ("col_bits_host", value([4, 40]))]


@entry("gather_rows")
def _(c):
    a = dict(table=c.t((32, 16), F32, 1), keys=c.v([0, 3, 31, 7, 7, 2, 1, 30]), base=0, out=c.t((8, 16), F32, 3),
             n_dev=None)
    return a, [("table", transposed), ("table", pinned), ("keys", wider), ("out", wider), ("out", short),
               ("n_dev", value(lambda d: torch.ones(1, dtype=F64, device=d)))]


@entry("sparse_apply_bf16")
def _(c):
    a = dict(opt=0, table=c.t((32, 16), BF, 1), state=c.t((32,), F32), state2=None, D1=16,
             keys=c.v([0, 3, 31, 7, 9, 2, 1, 30]), base=0, grads=c.t((8, 16), F32, 1), lr=0.1, eps=1e-8, scale=1.0,
             step=1, seed=0, n_dev=None)
    return a, [("table", wider), ("state", wider), ("state", short), ("keys", wider), ("grads", wider),
               ("grads", short), ("grads", pinned)]


@entry("lookup_rows")
def _(c):
    a = dict(rows=c.t((4, 16), BF, 1), inv=c.v([i % 4 for i in range(16)]), F=2, D=8, out=c.t((8, 16), BF, 3))
    return a, [("rows", wider), ("inv", wider), ("inv", short), ("out", wider), ("out", transposed)]


@entry("scatter_add_rows")
def _(c):
    a = dict(src=c.t((8, 16), F32, 1), idx=c.v([i % 4 for i in range(8)]), acc=c.t((4, 16), F32, 3))
    return a, [("src", transposed), ("src", pinned), ("idx", wider), ("idx", short), ("acc", wider)]


@entry("owner_slots")
def _(c):
    a = dict(own_inv=c.v([0, 1, 0, 2]), splits=[2, 2], cap=4)
    return a, [("own_inv", wider), ("own_inv", pinned)]


@entry("owner_rows_adagrad")
def _(c):
    a = dict(table=c.t((8, 20), F32, 1), state=c.t((8,), F32), state2=None, D1=20, keys=c.v([0, 1]), n=2, n_dev=None,
             base=0, recv=c.t((4, 20), F32, 1), P=2, slots=c.v([0, 2, 1, 3], I32), lr=0.1, eps=1e-8)
    return a, [("table", wider), ("state", wider), ("keys", wider), ("keys", short), ("recv", wider),
               ("slots", wider), ("slots", short)]


@entry("owner_push_adagrad")
def _(c):
    a = dict(table=c.t((8, 20), F32, 1), state=c.t((8,), F32), state2=None, D1=20, keys=c.v([0, 1, 0, 2]), base=0,
             recv=c.t((4, 20), F32, 1), splits=[2, 2], rs=c.t((32,), I32), stamp=1, lr=0.1, eps=1e-8)
    return a, [("table", wider), ("state", wider), ("keys", wider), ("recv", short), ("recv", wider), ("rs", wider),
               ("rs", short)]


@entry("sparse_rowwise_adagrad")
def _(c):
    a = dict(table=c.t((32, 16), F32, 1), state=c.t((32,), F32), state2=None, D1=16,
             keys=c.v([0, 3, 31, 7, 9, 2, 1, 30]), base=0, grads=c.t((8, 16), F32, 1), lr=0.1, eps=1e-8, n_dev=None,
             zero_g=False)
    return a, [("table", wider), ("state", wider), ("state", pinned), ("keys", wider), ("grads", wider),
               ("grads", short), ("state2", value(lambda d: torch.zeros(32, dtype=F64, device=d)))]


@entry("sparse_sgd")
def _(c):
    a = dict(table=c.t((32, 16), F32, 1), keys=c.v([0, 3, 31, 7, 9, 2, 1, 30]), base=0, grads=c.t((8, 16), F32, 1),
             scale=1.0, n_dev=None)
    return a, [("table", transposed), ("keys", wider), ("grads", wider), ("grads", short)]


@entry("embedding_bag_fwd")
def _(c):
    a = dict(rows=c.t((8, 16), F32, 1), idx=c.v([0, 1, 2, 3, 4, 5]), offsets=c.v([0, 2, 4, 6]), mean=False,
             out=c.t((3, 16), F32, 3))
    return a, [("rows", wider), ("idx", wider), ("offsets", wider), ("out", wider), ("out", short)]


@entry("embedding_bag_bwd")
def _(c):
    a = dict(grad_out=c.t((3, 16), F32, 1), idx=c.v([0, 1, 2, 3, 4, 5]), offsets=c.v([0, 2, 4, 6]), mean=False,
             grad_rows=c.t((8, 16), F32, 3))
    return a, [("grad_out", wider), ("idx", wider), ("idx", pinned), ("offsets", wider), ("offsets", short),
               ("offsets", pinned), ("grad_rows", wider)]


def _wd_in(c):
    return dict(dense=c.t((8, 4), F32, 1), rows=c.t((4, 24), BF, 1), inv=c.v([i % 4 for i in range(16)]), F=2, D=16,
                X=c.t((8, 40), BF, 3), wide_logit=c.t((8,), F32, 3), ones_col=-1, zero=None)


@entry("wd_assemble")
def _(c):
    return _wd_in(c), [("dense", wider), ("rows", wider), ("inv", wider), ("inv", short), ("X", wider),
                       ("wide_logit", wider), ("wide_logit", short), ("wide_logit", pinned),
                       ("zero", value(lambda d: torch.zeros(1, dtype=F64, device=d)))]


@entry("wd_assemble_tab")
def _(c):
    a = _wd_in(c)
    a = dict(dense=a["dense"], tab=c.t((8, 20), F32, 1), uniq=c.v([0, 2, 5, 7]), base=0, inv=a["inv"], F=2, D=16,
             X=a["X"], wide_logit=a["wide_logit"], ones_col=-1, zero=None, rowidx=None)
    return a, [("dense", wider), ("dense", pinned), ("tab", wider), ("uniq", wider), ("inv", wider), ("X", wider),
               ("wide_logit", wider), ("wide_logit", short),
               ("rowidx", value(lambda d: torch.zeros(16, dtype=I64, device=d)))]


@entry("wd_head")
def _(c):
    a = dict(H=c.t((8, 64), BF, 1), w=c.t((64,), BF, 1), b0=c.t((1,), BF), wide_logit=c.t((8,), F32),
             labels=c.t((8,), F32, 1), dH=c.t((8, 64), BF, 3), dw=c.t((64,), F32, 3), db=c.t((1,), F32, 3),
             dwide=c.t((8,), F32, 3), loss_sum=c.t((1,), F32, 3), dH_colsum=None, grad_scale=1.0, defer_fold=False)
    return a, [("H", wider), ("w", wider), ("b0", wider), ("wide_logit", wider), ("wide_logit", short),
               ("labels", wider), ("labels", short), ("labels", pinned), ("dH", pinned), ("dw", wider),
               ("dw", short), ("dw", pinned),
               ("db", wider), ("db", pinned), ("dwide", wider), ("dwide", short), ("dwide", pinned),
               ("loss_sum", wider), ("loss_sum", pinned), ("db", short), ("loss_sum", short)]


@entry("emb_build_csr")
def _(c):
    a = dict(inv=c.v([i % 4 for i in range(16)]), F=2, U=4, zeroed=None, counts_ready=False)
    return a, [("inv", wider), ("inv", pinned), ("zeroed", value(lambda d: torch.zeros(8, dtype=I64, device=d))),
               ("zeroed", value(lambda d: torch.zeros(8, dtype=I32, device=d)[:7]))]


@entry("emb_csr_positions")
def _(c):
    return dict(members=c.v([3, 1, 0, 2, 7, 5, 4, 6], I32)), [("members", wider), ("members", pinned)]


@entry("wd_emb_backward")
def _(c):
    a = dict(dX=c.t((8, 32), F32, 1), dwide=c.t((8,), F32, 1), inv=c.v([i % 4 for i in range(16)]), F=2, D=16,
             grad_rows=c.t((4, 20), F32, 3), x_off=0, members=None, memrow=None, sorted_rows=False)
    return a, [("dX", wider), ("dwide", wider), ("dwide", short), ("inv", wider), ("inv", short),
               ("grad_rows", wider),
               ("members", value(lambda d: torch.zeros(16, dtype=I32, device=d)))]


def _bad_slabs(n):
    """Slab lists the bindings refuse for a gradient of n elements (test_optk_validation.py's): each is refused
    by the launcher's own check as well, so none could reach a kernel."""
    h = n // 2

    def mk(d, ns=3, plane=h, off=0):
        return [(torch.zeros(ns * plane, device=d), ns, plane, off)]

    return [("slabs", value(lambda d: mk(d, off=n - h + 4))),  # the region ends past the gradient
            ("slabs", value(lambda d: mk(d, plane=h - 2))),  # plane: no multiple of 4
            ("slabs", value(lambda d: mk(d, off=2))),  # offset: no multiple of 4
            ("slabs", value(lambda d: mk(d, ns=0))),
            # misaligned planes
            ("slabs", value(lambda d: [(torch.zeros(3 * h + 8, device=d)[1: 1 + 3 * h], 3, h, 0)])),
            ("slabs", value(lambda d: mk(d) * 5))]  # more than 4 regions


@entry("adam_apply")
def _(c):
    a = dict(w=c.t((16,), F32, 1), m=c.t((16,), F32), v=c.t((16,), F32), g=c.t((16,), F32, 1), lr=0.1, beta1=0.9,
             beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, grad_scale=1.0, w_bf16=None, step_dev=None,
             zero_g=False, slabs=[])
    return a, [("w", wider), ("m", short), ("v", wider), ("g", wider),
               ("step_dev", value(lambda d: torch.ones(1, dtype=I64, device=d))),
               ("step_dev", value(lambda d: torch.ones(1, dtype=I32, pin_memory=True))),
               ("w_bf16", value(lambda d: torch.zeros(16, dtype=F32, device=d))),
               ("slabs", value(lambda d: [(torch.zeros(16, device=d)[:15], 1, 16, 0)])),
               ("slabs", value(lambda d: [(torch.zeros(16, dtype=F64, device=d), 1, 16, 0)])),
               ("slabs", value(lambda d: [(torch.zeros(16, device=d), 1, 16, -4)]))] + _bad_slabs(16)


@entry("slab_pack")
def _(c):
    a = dict(g=c.t((16,), F32, 1), out=c.t((16,), F32, 3), slabs=[])
    return a, [("g", wider), ("g", pinned), ("out", wider), ("out", short),
               ("slabs", value(lambda d: [(torch.zeros(16, device=d)[:15], 1, 16, 0)]))] + _bad_slabs(16)


@entry("sgd_apply")
def _(c):
    a = dict(w=c.t((16,), F32, 1), g=c.t((16,), F32, 1), lr=0.1, grad_scale=1.0, w_bf16=None)
    return a, [("w", wider), ("w", pinned), ("g", wider), ("g", short)]


@entry("adagrad_apply")
def _(c):
    a = dict(w=c.t((16,), F32, 1), acc=c.t((16,), F32), g=c.t((16,), F32, 1), lr=0.1, eps=1e-8, grad_scale=1.0,
             w_bf16=None)
    return a, [("w", wider), ("acc", wider), ("acc", short), ("g", wider)]


@entry("cast_f32_bf16")
def _(c):
    return dict(x=c.t((16,), F32, 1), y=c.t((16,), BF, 3)), [("x", wider), ("y", wider), ("y", short)]


@entry("emu_sum_slices")
def _(c):
    a = {"in": c.t((32,), F32, 1), "out": c.t((16,), F32, 3), "P": 2}
    return a, [("in", wider), ("in", pinned), ("out", wider), ("out", short)]


@entry("emu_rebase")
def _(c):
    return dict(keys=c.v([0, 1, 4, 5, 2, 3, 6, 7]), step=4, P=2, base=0), [("keys", wider), ("keys", pinned)]


@entry("lr_sparse_step")
def _(c):
    a = dict(rowptr=c.v([0, 2, 4]), cols=c.v([0, 3, 5, 7]), vals=c.t((4,), F32, 1), labels=c.t((2,), F32, 1),
             w=c.t((8,), F32), alpha=0.1, delta=c.t((8,), F32, 3), correct=c.t((1,), F32, 3))
    return a, [("rowptr", wider), ("cols", wider), ("vals", short), ("labels", wider), ("labels", pinned),
               ("delta", wider), ("delta", short), ("correct", wider)]


@entry("kmeans_assign")
def _(c):
    a = dict(X=c.t((8, 4), F32, 1), C=c.t((2, 4), F32), assign=c.t((8,), I32, 3), dist=c.t((8,), F32, 3))
    return a, [("X", wider), ("C", wider), ("assign", wider), ("assign", short), ("dist", wider), ("dist", short)]


@entry("kmeans_split3")
def _(c):
    a = dict(src=c.t((8, 4), F32, 1), out=c.t((8, 16), BF, 3), order=0, norms=c.t((8,), F32, 3))
    return a, [("src", wider), ("out", wider), ("out", short), ("norms", wider), ("norms", short)]


@entry("kmeans_argmin")
def _(c):
    a = dict(S=c.t((8, 2), F32, 1), cn=c.t((2,), F32), xn=c.t((8,), F32), assign=c.t((8,), I32, 3), dist=None)
    return a, [("S", wider), ("cn", short), ("xn", wider), ("assign", wider), ("assign", pinned), ("assign", short)]


@entry("kmeans_assign_csr")
def _(c):
    a = dict(rowptr=c.v([0, 2, 4]), cols=c.v([0, 3, 1, 2]), vals=c.t((4,), F32, 1), C=c.t((2, 4), F32),
             cnorm=c.t((2,), F32, 3), assign=c.t((2,), I32, 3), dist=None)
    return a, [("rowptr", wider), ("cols", wider), ("vals", wider), ("cnorm", wider), ("assign", wider),
               ("assign", short)]


@entry("kmeans_csr_accum")
def _(c):
    a = dict(rowptr=c.v([0, 2, 4]), cols=c.v([0, 3, 1, 2]), vals=c.t((4,), F32, 1), assign=c.v([0, 1], I32),
             sums=c.t((2, 4), F32, 3))
    return a, [("rowptr", wider), ("cols", wider), ("vals", wider), ("vals", short), ("assign", wider),
               ("sums", wider)]


@entry("criteo_synth")
def _(c):
    a = dict(seed=0, step=0, step_dev=None, cards=c.v([10, 20]), offsets=c.v([0, 10]), w=c.t((4,), F32, 1),
             dense=c.t((8, 4), F32, 3), keys=c.t((8, 2), I64, 3), labels=c.t((8,), F32, 3))
    return a, [("cards", wider), ("offsets", wider), ("offsets", short), ("w", wider), ("w", short), ("dense", wider),
               ("dense", short), ("keys", wider), ("labels", wider),
               ("step_dev", value(lambda d: torch.zeros(1, dtype=F64, device=d)))]


@entry("uniform_synth")
def _(c):
    a = dict(seed=0, step=0, rows=100, dense=c.t((8, 4), F32, 3), keys=c.t((8, 2), I64, 3), labels=c.t((8,), F32, 3))
    return a, [("dense", wider), ("keys", wider), ("labels", wider), ("labels", short)]


@entry("multi_copy")
def _(c):
    a = dict(dst=[c.t((16,), F32, 3)], src=[c.t((16,), F32, 1)])
    return a, [("src", lambda s: [pinned(s[0])]), ("dst", lambda s: [short(s[0])]),
               ("src", lambda s: [transposed(s[0].view(4, 4))])]


@entry("clock_probe")
def _(c):
    return dict(out=c.t((2,), I64, 3), spin_ticks=10, stream=0), [("out", wider), ("out", short), ("out", pinned)]


@entry("hash_slots")
def _(c):
    a = dict(tab_keys=c.t((16,), I64, -1), q=c.v([5, 9, 5, 1]), slots=c.t((4,), I64, 3), vals=c.t((16, 4), F32),
             init_scale=0.0, seed=0, counters=c.t((2,), I32), n_dev=None)
    return a, [("tab_keys", wider), ("q", wider), ("slots", wider), ("slots", short), ("vals", wider),
               ("counters", wider), ("counters", short)]


@entry("hash_rehash")
def _(c):
    a = dict(old_keys=c.t((16,), I64, -1), old_vals=c.t((16, 4), F32), old_state=c.t((16,), F32),
             new_keys=c.t((32,), I64, -1), new_vals=c.t((32, 4), F32), new_state=c.t((32,), F32),
             counters=c.t((1,), I32))  # (the rehash counts inserts only: one counter)
    return a, [("counters", short), ("old_keys", pinned), ("old_vals", wider), ("old_vals", pinned),
               ("old_state", wider),
               ("old_state", short), ("old_state", pinned), ("new_keys", pinned), ("new_vals", wider),
               ("new_vals", pinned), ("new_state", wider), ("new_state", short), ("new_state", pinned),
               ("counters", wider), ("counters", pinned)]


def _attn(c):
    return dict(qkv=c.t((64, 192), BF, 0.5), O=c.t((64, 64), BF, 0.5), lse=c.t((64,), F32, 1))


@entry("attn_fwd")
def _(c):
    t = _attn(c)
    a = dict(qkv=t["qkv"], B=1, T=64, H=1, scale=0.125, O=t["O"], lse=t["lse"])
    return a, [("qkv", wider), ("O", wider), ("O", short), ("lse", wider), ("lse", short), ("lse", pinned)]


@entry("attn_bwd")
def _(c):
    t = _attn(c)
    a = dict(qkv=t["qkv"], O=t["O"], dO=c.t((64, 64), BF, 0.5), lse=t["lse"], delta=c.t((64,), F32, 3), B=1, T=64,
             H=1, scale=0.125, dqkv=c.t((64, 192), BF, 3))
    return a, [("dO", wider), ("lse", wider), ("lse", pinned), ("delta", wider), ("delta", short), ("delta", pinned),
               ("dqkv", wider), ("dqkv", short)]


@entry("embed_fwd")
def _(c):
    a = dict(wte=c.t((32, 16), BF, 1), wpe=c.t((8, 16), BF, 1), tok=c.v([0, 3, 31, 7, 9, 2, 1, 30]), T=8,
             out=c.t((8, 16), BF, 3))
    return a, [("wte", wider), ("wpe", wider), ("wpe", short), ("tok", wider), ("out", wider), ("out", short)]


@entry("embed_bwd")
def _(c):
    a = dict(dx=c.t((8, 16), BF, 1), tok=c.v([0, 3, 31, 7, 9, 2, 1, 30]), T=8, dwte=c.t((32, 16), F32, 3),
             dwpe=c.t((8, 16), F32, 3))
    return a, [("dx", wider), ("dx", short), ("tok", wider), ("dwte", wider), ("dwpe", wider), ("dwpe", short)]


def _inbox(c, nbytes=256):
    return c.addr(c.t((nbytes,), U8))


@entry("ps_push_rows")
def _(c):
    a = dict(uniq=c.v([1, 2, 3, 4]), counts=c.v([4]), U_dev=None, n=4, g=c.t((4, 4), F32, 1), inbox=_inbox(c),
             slot_off=0, cap=4)
    return a, [("uniq", wider), ("uniq", short), ("counts", wider), ("g", wider), ("g", short), ("inbox", wider),
               ("inbox", pinned), ("U_dev", value(lambda d: torch.ones(1, dtype=F64, device=d))), ("n", value(-1))]


@entry("ps_set_headers")
def _(c):
    return dict(inbox=_inbox(c), slot_off=0, value=0), [("inbox", wider), ("inbox", pinned)]


@entry("ps_push_dense")
def _(c):
    a = dict(grad=c.t((8,), F32, 1), inbox=_inbox(c), data_off=64, S=8, slabs=[])
    return a, [("grad", wider), ("grad", short), ("inbox", wider), ("inbox", pinned), ("S", value(-4)),
               ("slabs", value(lambda d: [(torch.zeros(8, device=d)[:7], 1, 8, 0)]))] + _bad_slabs(8)


def _ps_gather(dtype):
    def build(c):
        a = dict(bases=c.addr(c.t((8, 16), dtype, 1)), bounds=c.v([0, 8]), keys=c.v([0, 7, 3, 3]), n_dev=None, W=16,
                 out=c.t((4, 16), F32, 3))
        return a, [("bases", wider), ("bases", pinned), ("bounds", wider), ("bounds", short), ("keys", wider),
                   ("out", wider), ("out", short), ("W", value(8))]
    return build


TABLE["ps_gather_rows"] = _ps_gather(F32)
TABLE["ps_gather_rows_bf16tab"] = _ps_gather(BF)


@entry("ps_hash_gather")
def _(c):
    a = dict(hkeys=c.addr(c.t((16,), I64, -1)), hvals=c.addr(c.t((16, 4), F32)), bounds=c.v([0, 1 << 40]), cap=16,
             keys=c.v([5, 9, 5, 1]), n_dev=None, W=4, out=c.t((4, 4), F32, 3))
    return a, [("hkeys", wider), ("hvals", wider), ("hvals", pinned), ("bounds", wider), ("keys", wider),
               ("out", wider), ("out", short)]


@entry("ps_pull")
def _(c):
    a = dict(srcs=c.addr(c.t((64,), U8, 1)), owners=[0], shard_bytes=64, dst=c.t((64,), U8, 3))
    return a, [("srcs", wider), ("srcs", pinned), ("dst", short), ("dst", pinned)]


@entry("ps_read_lock")
def _(c):
    held = c.t((16,), I32)
    a = dict(locks=c.addr(c.t((16,), I32)), held=held.data_ptr(), err=0)
    c.keep.append(held)
    return a, [("locks", wider), ("locks", pinned)]


@entry("ps_read_unlock")
def _(c):
    held = c.t((16,), I32)  # mask 0: no lock held, nothing to release
    a = dict(locks=c.addr(c.t((16,), I32)), held=held.data_ptr())
    c.keep.append(held)
    return a, [("locks", wider), ("locks", pinned)]


# ---- the harness ----------------------------------------------------------------------------------
def _tensors(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _tensors(y)


def _bytes(t):  # bit comparison (reinterpreted keys may read as NaN)
    return t.contiguous().view(-1).view(U8) if t.numel() else t.reshape(0)


def _call(name, c, args):
    K = _native.kernels()
    if name.startswith("LaunchList."):
        main = torch.cuda.current_stream().cuda_stream if c.dev.type == "cuda" else 0
        side = torch.cuda.Stream(c.dev).cuda_stream if c.dev.type == "cuda" else 1
        c.keep.append(K.LaunchList(main, side))
        return getattr(c.keep[-1], name.split(".")[1])(*args.values())
    return getattr(K, name)(*args.values())


def _names(arg):
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(arg) + r"(?![A-Za-z0-9_])")


def _cases():
    for name in sorted(TABLE):
        _, muts = TABLE[name](Case(torch.device("cpu")))
        for i, m in enumerate(muts):
            yield pytest.param(name, i, id=f"{name}-{m[0]}-{i}")


def test_every_registered_op_is_in_the_table():
    if not _native.kernels_available():
        pytest.skip("_kernels is not built")
    K = _native.kernels()
    assert K.EPI_STORE_BF16 == EPI_STORE_BF16
    ops = {n for n in dir(K) if not n.startswith("_") and callable(getattr(K, n))}
    assert ops - EXEMPT == {n for n in TABLE if "." not in n}, sorted(ops - EXEMPT ^ {n for n in TABLE if "." not in n})
    lst = {n for n in dir(K.LaunchList) if not n.startswith("_")} - LAUNCHLIST_EXEMPT
    assert lst == {n.split(".")[1] for n in TABLE if n.startswith("LaunchList.")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_valid_arguments_are_accepted(name, dev):
    c = Case(dev)
    args, _ = TABLE[name](c)
    _call(name, c, args)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _cases())
def test_bad_argument_raises_and_launches_nothing(name, i, dev):
    c = Case(dev)
    args, muts = TABLE[name](c)
    arg, mut = muts[i]
    new = mut(args[arg])
    args[arg] = new(dev) if isinstance(new, types.FunctionType) else new
    before = [t.clone() for t in _tensors(list(args.values()) + c.keep)]
    with pytest.raises(RuntimeError) as e:
        _call(name, c, args)
    assert _names(arg).search(str(e.value)), f"{name}: the message does not name {arg}: {e.value}"
    torch.cuda.synchronize()
    for t, b in zip(_tensors(list(args.values()) + c.keep), before):
        assert torch.equal(_bytes(t), _bytes(b)), f"{name}: a tensor changed although the call raised"


@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_rejected(name):
    if torch.cuda.is_available():
        pytest.skip("the pageable-memory device check is exercised where no GPU can be reached")
    if not _native.kernels_available():
        pytest.skip("_kernels is not built")
    c = Case(torch.device("cpu"))
    args, _ = TABLE[name](c)
    tensor_args = [a for a, v in args.items() if any(True for _ in _tensors(v))]
    with pytest.raises(RuntimeError) as e:
        _call(name, c, args)
    assert any(_names(a).search(str(e.value)) for a in tensor_args), f"{name}: {e.value}"
