"""Data-plane ops of minips_amd.

Every op has ONE device implementation: GPU tensors go to the hand-written gfx950 HIP
kernels in ``minips_amd._kernels`` (the evaluation, gradient-clipping, FTRL, Adagrad + FTRL and factorization-machine
ops: in the small extensions ``_evalk`` / ``_optk`` / ``_ftrlk`` / ``_wdftrlk`` / ``_fmk``; the LDA ops: in
``_ldak``) and raise if that extension is missing -- there is no silent eager fallback on a GPU. CPU tensors run a
plain PyTorch reference of the same math; that path exists for the CPU/gloo plumbing configuration (BASELINE
config 1) and as the fp32 oracle the GPU numerics tests compare against.
"""
from __future__ import annotations

import math

import torch

from .._native import dcnk, dfmk, evalk, ffmk, fmk, ftrlk, gbdtk, kernels, ldak, optk, w2vk, wdftrlk

EPI_STORE_F32 = 0
EPI_ATOMIC_F32 = 1
EPI_BIAS_RELU_BF16 = 2
EPI_BIAS_BF16 = 3
EPI_STORE_BF16 = 4
EPI_RELU_MASK_BF16 = 5
EPI_BIAS_GELU_BF16 = 6
EPI_BIAS_GELU_AUX_BF16 = 7  # C = gelu(u), mask(aux) = u  (pre-activation saved for backward)
EPI_GELU_GRAD_BF16 = 8      # C = acc * gelu'(mask)
EPI_PERM_ROWS_BF16 = 9      # C rows of `seg` columns permuted by `perm` (embedding dgrad in planner order)
EPI_BIAS_GELU_DAUX_BF16 = 13  # C = gelu(u), mask(aux) = gelu'(u)  (the derivative saved for backward)
EPI_MUL_AUX_BF16 = 14       # C = acc * mask(aux)
_L2E = 1.4426950408889634


def _gelu_grad(u):
    # with s = sigmoid(2z) = (1 + t) / 2 and 1 - t^2 = 4 s (1 - s): from e = exp(-2|z|) and r = 1 / (1 + e), without
    # the cancellation of 1 + t at t -> -1 (gemm_kernels.h gelu_grad_stable)
    k, c = 0.7978845608, 0.044715
    z = k * (u + c * u ** 3)
    e = torch.exp(-2 * z.abs())
    r = 1 / (1 + e)
    return torch.where(z >= 0, r, e * r) + 2 * u * (e * r * r) * k * (1 + 3 * c * u * u)


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ----------------------------------------------------------------------------- GEMM
_NO_STRIDES: list = []
_REC = None  # the active ops.recording, if any


class recording:
    """Inside ``with ops.recording(lst):`` the GEMM-family ops (gemm, linear_fwd / dgrad / wgrad,
    colsum_add) run through ``lst``, a native LaunchList (csrc/bindings/ops_py.cpp): each launches
    as usual AND is appended, validated, for ``lst.run()`` to replay with no Python or binding cost.
    ``sink_adds`` collects the slab-sink registrations the replay must repeat (linear_wgrad defer)."""

    def __init__(self, lst):
        self.lst = lst
        self.sink_adds: list = []

    def __enter__(self):
        global _REC
        self.prev, _REC = _REC, self
        return self

    def __exit__(self, *exc):
        global _REC
        _REC = self.prev
        return False


def gemm(A, B, C, M, N, K, a_km=False, b_kn=False, epi=EPI_STORE_F32, bias=None, mask=None, colsum=None,
         alpha=1.0, split_k=1, perm=None, seg=0, tile=0):
    """C[M,N] (op)= A.B.  A is [M][K] (a_km=False) or [K][M]; B is [N][K] (b_kn=False) or [K][N].
    EPI_PERM_ROWS_BF16: C is [M*N/seg, seg] and output (row, col) goes to row perm[row*N/seg + col//seg].
    ``tile`` (GPU): 128 / 200 (256x128) / 256 forces the workgroup tile, 0 lets the launcher pick."""
    if _gpu(A):
        if _REC is not None:
            _REC.lst.gemm(A, B, C, M, N, K, a_km, b_kn, epi, bias, mask, colsum, float(alpha), int(split_k), perm,
                          int(seg), int(tile))
            return C
        # (all positional: pybind's keyword / default-argument path costs ~1 us per call)
        kernels().gemm(A, B, C, M, N, K, a_km, b_kn, epi, bias, mask, colsum, float(alpha), int(split_k), 1, 1, 0, 0,
                       0, _NO_STRIDES, perm, int(seg), int(tile))
        return C
    a = (A[:K, :M].t() if a_km else A[:M, :K]).float()
    b = (B[:K, :N] if b_kn else B[:N, :K].t()).float()
    acc = (a @ b) * alpha
    if epi == EPI_STORE_F32:
        C[:M, :N] = acc
    elif epi == EPI_ATOMIC_F32:
        C[:M, :N] += acc
    elif epi == EPI_BIAS_GELU_AUX_BF16:
        if bias is not None:
            acc = acc + bias[:N].float()
        mask[:M, :N] = acc.to(torch.bfloat16)
        C[:M, :N] = torch.nn.functional.gelu(acc, approximate="tanh").to(torch.bfloat16)
    elif epi == EPI_GELU_GRAD_BF16:
        C[:M, :N] = (acc * _gelu_grad(mask[:M, :N].float())).to(torch.bfloat16)
    elif epi == EPI_BIAS_GELU_DAUX_BF16:
        if bias is not None:
            acc = acc + bias[:N].float()
        mask[:M, :N] = _gelu_grad(acc).to(torch.bfloat16)
        C[:M, :N] = torch.nn.functional.gelu(acc, approximate="tanh").to(torch.bfloat16)
    elif epi == EPI_MUL_AUX_BF16:
        C[:M, :N] = (acc * mask[:M, :N].float()).to(torch.bfloat16)
    elif epi in (EPI_BIAS_RELU_BF16, EPI_BIAS_BF16, EPI_BIAS_GELU_BF16):
        if bias is not None:
            acc = acc + bias[:N].float()
        if epi == EPI_BIAS_RELU_BF16:
            acc = torch.relu(acc)
        elif epi == EPI_BIAS_GELU_BF16:
            acc = torch.nn.functional.gelu(acc, approximate="tanh")
        C[:M, :N] = acc.to(torch.bfloat16)
    elif epi == EPI_STORE_BF16:
        C[:M, :N] = acc.to(torch.bfloat16)
    elif epi == EPI_PERM_ROWS_BF16:
        C.view(-1, seg)[perm[: M * (N // seg)].long()] = acc.to(torch.bfloat16).reshape(-1, seg)
    elif epi == EPI_RELU_MASK_BF16:
        out = torch.where(mask[:M, :N].float() > 0, acc, torch.zeros_like(acc)).to(torch.bfloat16)
        C[:M, :N] = out
        if colsum is not None:
            colsum[:N] += out.float().sum(0)
    else:
        raise ValueError(f"unknown epilogue {epi}")
    return C


def gemm_batched(A, B, C, M, N, K, a_km, b_kn, epi, batch, inner, lda, ldb, ldc, strides, alpha=1.0, bias=None,
                 tile=0):
    """``batch`` GEMMs over flat buffers; operand z starts at (z//inner)*s_outer + (z%inner)*s_inner
    (strides = [sa_o, sa_i, sb_o, sb_i, sc_o, sc_i] in elements), leading dims lda/ldb/ldc. ``tile``: gemm's."""
    if _gpu(A):
        if _REC is not None:
            raise RuntimeError("ops.recording: batched GEMMs are not recordable")
        kernels().gemm(A, B, C, M, N, K, a_km, b_kn, epi, bias, None, None, float(alpha), 1, int(batch), int(inner),
                       int(lda), int(ldb), int(ldc), [int(x) for x in strides], None, 0, int(tile))
        return C
    Af, Bf, Cf = A.reshape(-1), B.reshape(-1), C.reshape(-1)
    for z in range(batch):
        zo, zi = divmod(z, inner)
        oa, ob, oc = (zo * strides[0] + zi * strides[1], zo * strides[2] + zi * strides[3],
                      zo * strides[4] + zi * strides[5])
        ar, ac = (K, M) if a_km else (M, K)
        br, bc = (K, N) if b_kn else (N, K)
        a = Af[oa: oa + (ar - 1) * lda + ac].as_strided((ar, ac), (lda, 1))
        b = Bf[ob: ob + (br - 1) * ldb + bc].as_strided((br, bc), (ldb, 1))
        c = Cf[oc: oc + (M - 1) * ldc + N].as_strided((M, N), (ldc, 1))
        gemm(a, b, c, M, N, K, a_km, b_kn, epi, bias=bias, alpha=alpha)
    return C


_FWD_EPI = {"relu": EPI_BIAS_RELU_BF16, "none": EPI_BIAS_BF16, "gelu": EPI_BIAS_GELU_BF16}


def linear_fwd(x, w, bias=None, act="relu", out=None):
    """y = act(x w^T + b) in bf16 (x [M,K], w [N,K])."""
    M, K = x.shape[0], w.shape[1]
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    return gemm(x, w, out, M, N, K, False, False, _FWD_EPI[act], bias=bias)


def colsum_add(x, out):
    """out[:N] += x.sum(0) in fp32 (x bf16 [M, N]): a Linear's bias gradient from its dy."""
    if _gpu(x):
        (kernels() if _REC is None else _REC.lst).colsum_bf16(x, out)
        return out
    out[: x.shape[1]] += x.float().sum(0)
    return out


def linear_dgrad(dy, w, mask=None, colsum=None, out_f32=False, n_cols=None, out=None, perm=None, seg=0, tile=0):
    """dx = dy w (dy [M,N], w [N,K]) -> bf16 masked by (mask > 0) (+colsum), or fp32. ``perm`` /
    ``seg``: dx's row segments of ``seg`` columns go to rows perm[...] of out [M*K/seg, seg] (the
    embedding gradient written straight into the key planner's row-sorted order). ``tile``: gemm's."""
    M, N = dy.shape
    K = w.shape[1] if n_cols is None else n_cols
    if perm is not None:
        if out is None:
            out = torch.empty(M * K // seg, seg, dtype=torch.bfloat16, device=dy.device)
        return gemm(dy, w, out, M, K, N, False, True, EPI_PERM_ROWS_BF16, perm=perm, seg=seg, tile=tile)
    if out is None:
        out = torch.empty(M, K, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dy.device)
    epi = EPI_STORE_F32 if out_f32 else (EPI_RELU_MASK_BF16 if mask is not None else EPI_STORE_BF16)
    return gemm(dy, w, out, M, K, N, False, True, epi, mask=mask, colsum=colsum, tile=tile)


# Split-K weight gradients: about one 128x128 workgroup per CU pair (512 blocks), but a minimum number
# of reduction rows per split (profiles/r2/gpt2_wgrad_sweep.txt: shorter slices lose to their fixed
# prologue/epilogue cost). 640 rows is the isolated-kernel optimum (a wgrad on the critical path, e.g.
# the MLP); a wgrad forked onto a side stream beside the dgrad chain (SideStream sets overlap_mode)
# favours throughput: fewer, longer splits with less slab traffic -- 1024 rows measured best there
# (W&D 0.461 ms vs 0.490 at 2048; tools/gpu_round.sh ab, profiles/r2/gemm_round2.txt). A block-count floor
# for overlapped wgrads with few tiles measured worse (W&D 0.528 -> 0.539 ms at 128 blocks) and is gone;
# so are the 256x256 wgrad tile and the phase-split v3 wgrad (profiles/r4/ab_gpt2_knobs.txt).
_WGRAD_BLOCKS = 512
_WGRAD_MIN_ROWS = 640
_WGRAD_MIN_ROWS_OVERLAP = 1024
_overlap_state = __import__("threading").local()


def overlap_mode(on: bool) -> bool:
    """Mark GEMMs issued from now on as overlapped side-stream work (returns the previous mode)."""
    prev = getattr(_overlap_state, "on", False)
    _overlap_state.on = on
    return prev


def linear_wgrad(dy, x, dw, split_k=None, blocks=None, defer=None, tile=0):
    """dw[N,K] += dy^T x (dy [M,N], x [M,K]); fp32 accumulate. ``blocks``: the workgroup target of
    the split-K choice (default _WGRAD_BLOCKS; a model may tune its own). ``defer``: a
    DenseTable slab sink (DenseTable.slab_sink()): the K slices stay in fp32 slab planes that the
    table's next Adam folds in (no reduce kernel); dw must be a contiguous [N, K] region of the
    table's gradient, which the sum then never passes through. ``tile``: gemm's tile hint."""
    M, N = dy.shape
    K = x.shape[1]
    if split_k is None:
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        overlapped = getattr(_overlap_state, "on", False)
        min_rows = _WGRAD_MIN_ROWS_OVERLAP if overlapped else _WGRAD_MIN_ROWS
        target = _WGRAD_BLOCKS if blocks is None else int(blocks)
        split_k = max(1, min(M // min_rows, (target + tiles - 1) // tiles))
    if (defer is not None and _gpu(dy) and split_k > 1 and K % 4 == 0 and dw.dim() == 2
            and dw.stride(1) == 1 and dw.stride(0) == K and defer.accepts(dw)):
        slab = defer.slab(dw, split_k)
        nsplit = (kernels() if _REC is None else _REC.lst).gemm_slab(dy, x, slab, N, K, M, True, True, int(split_k))
        defer.add(dw, slab, nsplit)
        if _REC is not None:
            _REC.sink_adds.append((defer, dw, slab, nsplit))
        return dw
    return gemm(dy, x, dw, N, K, M, True, True, EPI_ATOMIC_F32, split_k=split_k, tile=tile)


# ----------------------------------------------------------------------------- sparse keys
def unique_bucketize(keys: torch.Tensor, bounds: torch.Tensor, F: int = 1):
    """Dedupe ``keys`` and group the unique keys by owner shard.

    Returns (uniq [n] with the first sum(counts) valid, inverse [n], counts [P]) where
    ``bounds`` [P+1] are the shard key boundaries and uniq[inverse[i]] == keys[i]. ``F`` > 1
    declares the flat keys as a [B, F] batch (the GPU kernel then dedupes feature-major tiles).
    """
    uniq, inv, counts, _ = unique_bucketize_n(keys, bounds, F)
    return uniq, inv, counts


def unique_bucketize_n(keys: torch.Tensor, bounds: torch.Tensor, F: int = 1, route_mult: int = 0,
                       route_n: int = 0, extra_zero_ints: int = 0, csr_counts: bool = False):
    """unique_bucketize plus the total unique count U as a 1-element device tensor, so that
    consumers (gather_rows / sparse_* with ``n_dev``, wd_emb_backward with ``U_dev``) bound
    their work on the GPU without a host round trip. ``route_mult`` != 0 first maps every key to
    key * route_mult mod route_n (fused into the GPU kernel). ``csr_counts`` (GPU, with
    extra_zero_ints >= n): the first n ints of the zeroed block receive each unique key's lookup
    count, for emb_build_csr(..., counts_ready=True)."""
    if _gpu(keys):
        out = kernels().unique_bucketize(keys.contiguous(), bounds.contiguous(), int(F), int(route_mult),
                                         int(route_n), int(extra_zero_ints), bool(csr_counts))
        if extra_zero_ints:  # (..., zeroed int32 workspace cleared by the same memset)
            return tuple(out[:4]), out[4]
        return tuple(out)
    keys = keys.reshape(-1)
    if route_mult:
        keys = (keys * route_mult) % route_n
    u, inv = torch.unique(keys, sorted=True, return_inverse=True)
    owner = torch.bucketize(u, bounds[1:-1], right=True)
    counts = torch.bincount(owner, minlength=bounds.numel() - 1)
    # sorted unique keys are already grouped by owner (ranges are contiguous)
    out = torch.empty_like(keys)
    out[: u.numel()] = u
    return out, inv, counts, torch.tensor([u.numel()], dtype=torch.int64)


def bitmap_plan(keys: torch.Tensor, bounds: torch.Tensor, num_rows: int, route_mult: int = 0, oor=None):
    """unique_bucketize_n for a bounded key space: keys (after the optional routing
    key * route_mult mod num_rows) in [0, num_rows). GPU: an N-bit map + popcount ranks
    (csrc/kernels/bitmap.hip), no hash table; the unique keys come out sorted, so the CPU
    reference (torch.unique) produces the identical plan. Returns (uniq, inverse, counts, U).
    ``oor`` (device int64 [1], optional): accumulates the number of keys outside the key space
    (they would alias row 0); the caller checks it at a host sync point (no sync here)."""
    if _gpu(keys):
        return tuple(kernels().bitmap_plan(keys.reshape(-1).contiguous(), bounds.contiguous(), int(num_rows),
                                           int(route_mult), int(num_rows) if route_mult else 0, oor))
    flat = keys.reshape(-1)
    k = (flat * route_mult) % num_rows if route_mult else flat
    bad = (k < 0) | (k >= num_rows)
    if bool(bad.any()):
        if oor is None:
            raise ValueError(f"keys outside [0, {num_rows})")
        oor += int(bad.sum())
    return unique_bucketize_n(flat, bounds, 1, int(route_mult), int(num_rows) if route_mult else 0)


def plan_sorted(keys, col_base, col_bits, route_mult=0, route_n=0, bits_dev=None, bounds=None, positions=False):
    """Key planning of a [B, F] batch whose columns hold disjoint key ranges (column f's keys in
    [col_base[f], col_base[f] + 2**col_bits[f])): per-column radix sort, no global atomics
    (plan.hip). ``col_bits``: a list of ints (or one int for every column); ``bounds`` [P+1]: the
    owners' routed-key ranges (None: one owner). Returns (uniq [n] (first U valid, routed; column-
    major, inside a column by (owner, key) -- ascending keys for one owner -- then stably grouped by
    owner), inv [n], counts [P], U_dev [1], members [n] int32, memrow [n] int32) -- the
    unique_bucketize_n outputs plus the lookup CSR of emb_build_csr (rows contiguous, in that
    column-major order)."""
    if bounds is None:
        bounds = torch.tensor([0, (1 << 62)], dtype=torch.int64, device=keys.device)
    if _gpu(keys):
        bits = [int(col_bits)] * keys.shape[1] if isinstance(col_bits, int) else [int(b) for b in col_bits]
        if bits_dev is None:  # (tables pass their cached device copy: no H2D copy per plan)
            bits_dev = torch.tensor(bits, dtype=torch.int32, device=keys.device)
        return tuple(kernels().plan_sorted(keys.contiguous(), col_base.contiguous(), bits_dev, bits,
                                           int(route_mult), int(route_n), bounds.contiguous(), bool(positions)))
    B, F = keys.shape
    P = bounds.numel() - 1
    uniq_l, inv_l = [], []
    base = 0
    for f in range(F):
        u, i = torch.unique(keys[:, f], sorted=True, return_inverse=True)
        if P > 1:  # inside a column the keys sort by (owner shard of the routed key, key)
            r = (u * route_mult) % route_n if route_mult else u
            o = torch.sort(torch.bucketize(r, bounds[1:-1], right=True), stable=True).indices
            rank = torch.empty_like(o)
            rank[o] = torch.arange(o.numel())
            u, i = u[o], rank[i]
        uniq_l.append(u)
        inv_l.append(i + base)
        base += u.numel()
    U = base
    uniq = torch.cat(uniq_l)
    if route_mult:
        uniq = (uniq * route_mult) % route_n
    owner = torch.bucketize(uniq, bounds[1:-1], right=True)
    perm_order = torch.sort(owner, stable=True).indices      # regrouped position -> u
    perm = torch.empty(U, dtype=torch.int64)
    perm[perm_order] = torch.arange(U)                         # u -> regrouped position
    out = torch.empty(B * F, dtype=torch.int64)
    out[:U] = uniq[perm_order]
    inv_u = torch.stack(inv_l, 1).reshape(-1)                  # column-major u of each lookup
    order = torch.sort(inv_u, stable=True).indices             # lookups grouped by u (ascending)
    counts = torch.bincount(owner, minlength=P).to(torch.int64)
    res = (out, perm[inv_u], counts, torch.tensor([U], dtype=torch.int64), order.to(torch.int32),
           perm[inv_u[order]].to(torch.int32))
    pos = None
    if positions:  # members = order: pos[order[m]] = m
        pos = torch.empty(B * F, dtype=torch.int32)
        pos[order] = torch.arange(B * F, dtype=torch.int32)
    if P == 1:  # row u's lookups are members [rowstart[u], rowstart[u + 1]): (.., positions or None, rowstart,
        # rowidx or None) -- rowidx: each lookup's table row (routed key) when routed keys fit int32
        rs = torch.full((B * F + 1,), B * F, dtype=torch.int32)
        rs[0] = 0
        rs[1: U + 1] = torch.cumsum(torch.bincount(inv_u, minlength=U), 0).to(torch.int32)
        ri = uniq[inv_u].to(torch.int32) if route_mult and 0 < route_n <= 0x7FFFFFFF else None
        return res + (pos, rs, ri)
    return res + (pos,) if positions else res


def gather_rows(table, keys, base, out, n_dev=None):
    """out[i] = table[keys[i] - base] for i < n (n = keys.numel(), or the device count n_dev)."""
    if _gpu(keys):
        kernels().gather_rows(table, keys, int(base), out, n_dev)
        return out
    if n_dev is not None:
        keys = keys[: int(n_dev.reshape(-1)[0])]
    rows = table[(keys - base), : out.shape[1]]
    out[: keys.numel()] = rows.to(out.dtype)
    return out


def lookup_rows(rows, inv, F, D, out):
    """out[b, f*D:(f+1)*D] = rows[inv[b*F+f], :D] (bf16; out may be a row-major column slice)."""
    if _gpu(rows):
        kernels().lookup_rows(rows, inv, int(F), int(D), out)
        return out
    B = out.shape[0]
    out[:, : F * D] = rows[inv, :D].reshape(B, F * D).to(out.dtype)
    return out


def scatter_add_rows(src, idx, acc):
    """acc[idx[i]] += src[i] (src fp32 or bf16, acc fp32; or both fp64)."""
    if _gpu(src):
        kernels().scatter_add_rows(src, idx, acc)
        return acc
    acc.index_add_(0, idx, src.to(acc.dtype))
    return acc


def _sr_bf16(x: torch.Tensor, gen: torch.Generator | None = None) -> torch.Tensor:
    """Stochastic rounding of fp32 to bf16 (CPU reference of bf16rows.hip): add 16 random bits
    below the bf16 mantissa, truncate."""
    b = x.contiguous().view(torch.int32)
    r = torch.randint(0, 1 << 16, b.shape, dtype=torch.int32, generator=gen)
    finite = (b & 0x7F800000) != 0x7F800000
    b = torch.where(finite, b + r, b)
    return (b & -65536).view(torch.float32).to(torch.bfloat16)


def sparse_apply_bf16(opt, table, state, keys, base, grads, lr, eps=1e-8, scale=1.0, state2=None, split=None,
                      step=0, seed=0, n_dev=None):
    """fp32 gradient rows into a bf16 table with stochastic rounding (opt "rowwise_adagrad" |
    "add" (w += scale * g))."""
    D = table.shape[1]
    D1 = D if split is None else split
    code = 0 if opt == "rowwise_adagrad" else 1
    if _gpu(table):
        kernels().sparse_apply_bf16(code, table, state, state2, int(D1), keys, int(base), grads, float(lr), float(eps),
                                    float(scale), int(step) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, n_dev)
        return
    if n_dev is not None:
        n = int(n_dev.reshape(-1)[0])
        keys, grads = keys[:n], grads[:n]
    rows = keys - base
    w = table[rows].float()
    g = grads[:, :D].float()
    if code == 0:
        s1 = state[rows] + (g[:, :D1] ** 2).mean(1)
        state[rows] = s1
        w[:, :D1] -= lr * g[:, :D1] / (s1.sqrt() + eps).unsqueeze(1)
        if D1 < D:
            s2 = state2[rows] + (g[:, D1:] ** 2).mean(1)
            state2[rows] = s2
            w[:, D1:] -= lr * g[:, D1:] / (s2.sqrt() + eps).unsqueeze(1)
    else:
        w += scale * g
    table[rows] = _sr_bf16(w, torch.Generator().manual_seed((int(seed) * 1000003 + int(step)) & 0x7FFFFFFF))


def sparse_rowwise_adagrad(table, state, keys, base, grads, lr, eps=1e-8, state2=None, split=None, n_dev=None,
                           zero_g=False):
    """Row-wise Adagrad on table rows keys - base. ``zero_g``: the kernel clears the gradient rows
    after reading them (a persistent, pre-zeroed push buffer stays zero for the next push)."""
    D = grads.shape[1]
    D1 = D if split is None else split
    if _gpu(table):
        kernels().sparse_rowwise_adagrad(table, state, state2, D1, keys, int(base), grads, float(lr), float(eps),
                                         n_dev, bool(zero_g))
        return
    if n_dev is not None:
        n = int(n_dev.reshape(-1)[0])
        keys, grads = keys[:n], grads[:n]
    rows = keys - base
    g1 = grads[:, :D1]
    s1 = state[rows] + (g1 * g1).mean(1)
    state[rows] = s1
    table[rows, :D1] -= lr * g1 / (s1.sqrt() + eps).unsqueeze(1)
    if D1 < D:
        g2 = grads[:, D1:]
        s2 = state2[rows] + (g2 * g2).mean(1)
        state2[rows] = s2
        table[rows, D1:D] -= lr * g2 / (s2.sqrt() + eps).unsqueeze(1)


def owner_slots(own_inv, splits, cap):
    """Owner side of a multi-rank push: the received rows come grouped by requester (``splits``,
    host ints); returns int32 slots [cap * P] with slots[u * P + s] = the received row requester s
    sent for owned unique row u (own_inv[i] = u), -1 where s sent none."""
    P = len(splits)
    if _gpu(own_inv):
        return kernels().owner_slots(own_inv, [int(c) for c in splits], int(cap))
    slots = torch.full((max(int(cap), 1) * P,), -1, dtype=torch.int32)
    seg = torch.repeat_interleave(torch.arange(P), torch.tensor([int(c) for c in splits], dtype=torch.int64))
    slots[own_inv * P + seg] = torch.arange(own_inv.numel(), dtype=torch.int32)
    return slots


def owner_push_adagrad(table, state, keys, base, recv, splits, rs, stamp, lr, eps=1e-8, state2=None, split=None):
    """Owner apply of one push without an owner-side dedupe: received key i (requester segments
    ``splits``, each requester's keys distinct) carries gradient row recv[i]; every touched row gets
    the row-wise Adagrad of the sum of its received rows in requester order -- owner_rows_adagrad's
    arithmetic. ``rs``: a persistent int32 [rows * P * 2] {stamp, row} table (GPU), ``stamp`` this
    push's number (increasing, >= 0)."""
    D = recv.shape[1]
    D1 = D if split is None else split
    if _gpu(table):
        kernels().owner_push_adagrad(table, state, state2, int(D1), keys, int(base), recv.contiguous(),
                                     [int(c) for c in splits], rs, int(stamp), float(lr), float(eps))
        return
    M = keys.numel()
    if M == 0:
        return
    uniq, inv = torch.unique(keys, sorted=True, return_inverse=True)
    P = len(splits)
    seg = torch.repeat_interleave(torch.arange(P), torch.tensor([int(c) for c in splits], dtype=torch.int64))
    slots = torch.full((uniq.numel() * P,), -1, dtype=torch.int32)
    slots[inv * P + seg] = torch.arange(M, dtype=torch.int32)
    owner_rows_adagrad(table, state, uniq, uniq.numel(), base, recv, slots, P, lr, eps, state2=state2, split=split)


def owner_rows_adagrad(table, state, keys, n, base, recv, slots, P, lr, eps=1e-8, state2=None, split=None, n_dev=None):
    """Row-wise Adagrad of owned rows keys[:n] (n_dev: device bound) with the gradient of row u =
    sum over s in 0..P-1 of recv[slots[u * P + s]] (bf16 / fp32 rows, fp32 sum in requester order)
    -- ops.sparse_rowwise_adagrad of the owner-side segment sums, in one pass."""
    D = recv.shape[1]
    D1 = D if split is None else split
    if _gpu(table):
        kernels().owner_rows_adagrad(table, state, state2, int(D1), keys, int(n), n_dev, int(base), recv, int(P), slots,
                                     float(lr), float(eps))
        return
    if n_dev is not None:
        n = min(int(n), int(n_dev.reshape(-1)[0]))
    sl = slots[: n * P].view(n, P).long()
    g = torch.zeros(n, D, dtype=torch.float32)
    for s in range(P):  # requester order (the GPU sum's order)
        m = sl[:, s]
        hit = m >= 0
        g[hit] += recv[m[hit]].float()
    sparse_rowwise_adagrad(table, state, keys[:n], base, g, lr, eps, state2=state2, split=split)


def sparse_sgd(table, keys, base, grads, scale, n_dev=None):
    if _gpu(table):
        kernels().sparse_sgd(table, keys, int(base), grads, float(scale), n_dev)
        return
    if n_dev is not None:
        n = int(n_dev.reshape(-1)[0])
        keys, grads = keys[:n], grads[:n]
    table.index_add_(0, keys - base, scale * grads, alpha=1.0) if grads.shape[1] == table.shape[1] else \
        table[:, : grads.shape[1]].index_add_(0, keys - base, scale * grads)


def _sqrt_f32(x):
    """The correctly rounded fp32 square root (the kernel's sqrtf): through fp64, whose 53 bits make the
    second rounding exact. torch's vectorised fp32 sqrt on the CPU is off by one ulp on about 0.6 % of
    inputs, which would show in z after the rule's division by alpha."""
    return x.double().sqrt().to(torch.float32)


def ftrl_weights(z, n, alpha, beta=1.0, l1=0.0, l2=0.0):
    """The closed form w = f(z, n) of FTRL-Proximal in fp32, the rule's own operation order:
    w = |z| <= l1 ? 0 : -(z - sign(z) * l1) / ((beta + sqrt(n)) / alpha + l2)."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=z.device)  # noqa: E731
    shrunk = z - torch.sign(z) * f(l1)
    scale = (f(beta) + _sqrt_f32(n)) / f(alpha) + f(l2)
    return torch.where(z.abs() <= f(l1), torch.zeros_like(z), -shrunk / scale)


def sparse_ftrl(table, zn, keys, base, grads, alpha, beta=1.0, l1=0.0, l2=0.0, n_dev=None, oor=None, blocks=0):
    """Per-coordinate FTRL-Proximal (McMahan et al. 2013, Algorithm 1) on table rows keys - base, in fp32:
        g2 = g * g;  n' = n + g2;  s' = sqrt(n');  s = sqrt(n);  den = alpha * (s' + s)
        sigma = den > 0 ? g2 / den : 0;  z' = z + (g - sigma * w)
        w' = |z'| <= l1 ? 0 : -(z' - sign(z') * l1) / ((beta + s') / alpha + l2)
    ``zn`` [rows, 2W]: z in columns [0, W), n in [W, 2W) of the table's row. ``keys`` distinct; ``n_dev``
    (device int64) bounds the prefix without a host sync; a key whose row is outside [0, rows) is skipped
    and counted into ``oor`` (int64 [1]). ``blocks`` > 0 forces the GPU grid size. The CPU path is the
    reference of the same operation sequence (g * g its own rounded product)."""
    alpha, beta, l1, l2 = float(alpha), float(beta), float(l1), float(l2)
    if _gpu(table):
        ftrlk().sparse_ftrl(table, zn, keys, int(base), grads, alpha, beta, l1, l2, n_dev, oor, int(blocks))
        return
    if not alpha > 0 or not (beta >= 0 and l1 >= 0 and l2 >= 0):
        raise RuntimeError(f"sparse_ftrl: alpha {alpha} must be positive, beta {beta}, l1 {l1}, l2 {l2} non-negative")
    W, nrows = grads.shape[1], table.shape[0]
    if table.dtype != torch.float32 or zn.dtype != torch.float32 or tuple(zn.shape) != (nrows, 2 * W):
        raise RuntimeError(f"sparse_ftrl: fp32 table and zn [{nrows}, {2 * W}] expected, got {table.dtype} / "
                           f"{zn.dtype} {tuple(zn.shape)}")
    n = keys.numel()
    if n_dev is not None:
        n = min(n, int(n_dev.reshape(-1)[0]))
    rows, g = keys[:n] - base, grads[:n].float()
    ok = (rows >= 0) & (rows < nrows)
    if oor is not None:
        oor += int((~ok).sum())
    rows, g = rows[ok], g[ok]
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    w, z, nn = table[rows, :W], zn[rows, :W], zn[rows, W:]
    g2 = g * g
    n1 = nn + g2
    s1, s0 = _sqrt_f32(n1), _sqrt_f32(nn)
    den = f(alpha) * (s1 + s0)
    sigma = torch.where(den > 0, g2 / den, torch.zeros_like(den))
    z1 = z + (g - sigma * w)
    table[rows, :W] = ftrl_weights(z1, n1, alpha, beta, l1, l2)
    zn[rows, :W] = z1
    zn[rows, W:] = n1


def sparse_adagrad_ftrl(table, state, zn, split, keys, base, grads, lr, eps, alpha, beta=1.0, l1=0.0, l2=0.0,
                        grad_scale=1.0, n_dev=None, oor=None, blocks=0):
    """Split rows with two rules, one pass: columns [0, split) of table rows keys - base take
    sparse_rowwise_adagrad's rule (``state`` [rows], ``lr``, ``eps``), columns [split, W) take sparse_ftrl's
    coordinate rule on ``grads[:, split:] * grad_scale`` (the scaling its own rounded product) with ``alpha``,
    ``beta``, ``l1``, ``l2``. ``zn`` [rows, 2 * (W - split)]: z | n of the wide columns, sparse_ftrl's layout.
    ``grad_scale``: the step pushes gradients of the mean loss; batch size x world gives the FTRL columns
    the summed-loss gradient the paper's hyper-parameters assume (exact for a power of two). ``keys``
    distinct; ``n_dev`` bounds the prefix without a host sync; a key whose row is outside [0, rows) is skipped
    whole and counted into ``oor`` (int64 [1]). ``blocks`` > 0 forces the GPU grid size. The CPU path is the
    composition of the two CPU references."""
    lr, eps, alpha, beta, l1, l2, grad_scale = (float(v) for v in (lr, eps, alpha, beta, l1, l2, grad_scale))
    D1 = int(split)
    if _gpu(table):
        wdftrlk().sparse_adagrad_ftrl(table, state, zn, D1, keys, int(base), grads, lr, eps, alpha, beta, l1, l2,
                                      grad_scale, n_dev, oor, int(blocks))
        return
    W, nrows = grads.shape[1], table.shape[0]
    if not 1 <= D1 < W:
        raise RuntimeError(f"sparse_adagrad_ftrl: split {D1} outside [1, {W})")
    if not (grad_scale > 0 and math.isfinite(grad_scale)):
        raise RuntimeError(f"sparse_adagrad_ftrl: grad_scale {grad_scale} must be finite and positive")
    if tuple(state.shape) != (nrows,):
        raise RuntimeError(f"sparse_adagrad_ftrl: state [{nrows}] expected, got {tuple(state.shape)}")
    n = keys.numel()
    if n_dev is not None:
        n = min(n, int(n_dev.reshape(-1)[0]))
    rows, g = keys[:n] - base, grads[:n].float()
    ok = (rows >= 0) & (rows < nrows)
    if oor is not None:
        oor += int((~ok).sum())
    rows, g = rows[ok], g[ok]
    sparse_rowwise_adagrad(table, state, rows, 0, g[:, :D1], lr, eps)
    sparse_ftrl(table[:, D1:W], zn, rows, 0, g[:, D1:] * torch.tensor(grad_scale, dtype=torch.float32), alpha, beta,
                l1, l2)


def embedding_bag_fwd(rows, idx, offsets, mean=False, out=None):
    B = offsets.numel() - 1
    if out is None:
        out = torch.empty(B, rows.shape[1], dtype=torch.float32, device=rows.device)
    if _gpu(rows):
        kernels().embedding_bag_fwd(rows, idx, offsets, bool(mean), out)
        return out
    mode = "mean" if mean else "sum"
    out.copy_(torch.nn.functional.embedding_bag(idx, rows, offsets[:-1], mode=mode, include_last_offset=False))
    return out


def embedding_bag_bwd(grad_out, idx, offsets, grad_rows, mean=False):
    if _gpu(grad_out):
        kernels().embedding_bag_bwd(grad_out, idx, offsets, bool(mean), grad_rows)
        return grad_rows
    lens = (offsets[1:] - offsets[:-1])
    bag = torch.repeat_interleave(torch.arange(lens.numel(), device=idx.device), lens)
    g = grad_out[bag]
    if mean:
        g = g / lens[bag].clamp_min(1).unsqueeze(1).to(g.dtype)
    grad_rows.index_add_(0, idx, g)
    return grad_rows


# ----------------------------------------------------------------------------- Wide&Deep
def wd_assemble(dense, rows, inv, F, D, X, wide_logit, ones_col=-1, zero=None):
    """X = [emb_0..emb_{F-1} | dense | 1 at ones_col | 0-pad] (bf16);
    wide_logit[b] = sum_f rows[inv, D]. ``zero`` (fp32 [1], optional) is set to 0 on the way
    (the step's loss accumulator: no separate fill kernel)."""
    if _gpu(X):
        kernels().wd_assemble(dense, rows, inv, int(F), int(D), X, wide_logit, int(ones_col), zero)
        return X, wide_logit
    if zero is not None:
        zero.zero_()
    B = X.shape[0]
    r = rows[inv].view(B, F, rows.shape[1]).float()
    X.zero_()
    X[:, : F * D] = r[:, :, :D].reshape(B, F * D).to(torch.bfloat16)
    X[:, F * D: F * D + dense.shape[1]] = dense.to(torch.bfloat16)
    if ones_col >= 0:
        X[:, ones_col] = 1.0
    wide_logit.copy_(r[:, :, D].sum(1))
    return X, wide_logit


def wd_assemble_tab(dense, table, index, base, inv, F, D, X, wide_logit, ones_col=-1, zero=None, rowidx=None):
    """wd_assemble with the rows read in place: the row of unique u is table[index[u] - base]
    (fp32), rounded to bf16 exactly as gather_rows(out bf16) does. ``rowidx`` (plan_sorted, one
    owner): lookup j's row + base directly (the same rows, one index load per lookup)."""
    if _gpu(X):
        kernels().wd_assemble_tab(dense, table, index, int(base), inv, int(F), int(D), X, wide_logit, int(ones_col),
                                  zero, rowidx)
        return X, wide_logit
    U = int(inv.max()) + 1 if inv.numel() else 0
    rows = table[index[:U] - base].to(torch.bfloat16)
    return wd_assemble(dense, rows, inv, F, D, X, wide_logit, ones_col, zero)


def wd_head(H, w, b0, wide_logit, labels, dH, dw, db, dwide, loss_sum, dH_colsum=None, grad_scale=1.0,
            defer_fold=False):
    """Last layer + BCE forward/backward. ``defer_fold`` (GPU): the batch sums into dw / db /
    loss_sum / dH_colsum are left as per-block partials for wd_head_fold (a later kernel, e.g. on
    the weight-gradient stream, off the dgrad chain); on the CPU they are added here and the fold
    is a no-op."""
    if _gpu(H):
        kernels().wd_head(H, w, b0, wide_logit, labels, dH, dw, db, dwide, loss_sum, dH_colsum, float(grad_scale),
                          bool(defer_fold))
        return
    h = H.float()
    z = h @ w.float() + b0.float() + wide_logit
    y = (labels > 0.5).float()
    p = torch.sigmoid(z)
    dz = (p - y) * grad_scale
    dwide.copy_(dz)
    db += dz.sum()
    loss_sum += (torch.clamp_min(z, 0) - z * y + torch.log1p(torch.exp(-z.abs()))).sum()
    g = torch.where(h > 0, dz.unsqueeze(1) * w.float().unsqueeze(0), torch.zeros_like(h)).to(torch.bfloat16)
    dH.copy_(g)
    dw += (dz.unsqueeze(1) * h).sum(0)
    if dH_colsum is not None:
        dH_colsum += g.float().sum(0)


def wd_head_fold(B, Hd, dw, db, loss_sum, dH_colsum=None):
    """The totals of the device's last wd_head(defer_fold=True) (same B, Hd), on the current
    stream (recordable into a LaunchList). No-op on the CPU (wd_head added them)."""
    if _gpu(dw):
        (kernels() if _REC is None else _REC.lst).wd_head_fold(int(B), int(Hd), dw, db, loss_sum, dH_colsum)


# ----------------------------------------------------------------------------- DeepFM's interaction term
def _wd_fm_check(X, F, D):
    if not 1 <= D <= 64 or F < 1:
        raise RuntimeError(f"wd_fm: D is {D} and F is {F}, expected 1 <= D <= 64 and F >= 1")
    if X.dim() != 2 or X.shape[1] < F * D:
        raise RuntimeError(f"wd_fm: X has shape {tuple(X.shape)}, expected [B, >= F * D = {F * D}]")


def wd_fm_forward(X, F, D, wide, S=None, blocks=0):
    """DeepFM's second-order term over the assembled Wide&Deep input (the rule: csrc/kernels/deepfm.h). X bf16
    [B, >= F*D] holds sample b's F field embeddings in columns [f*D, f*D + D); with v = X[:, :F*D].float():
      S_bc = sum_f v_fc,  q_bc = sum_f v_fc^2,  wide[b] += 0.5 * sum_c (S_bc^2 - q_bc)   (all fp32).
    Returns S fp32 [B, D] (``S``: written in place when given, no allocation). Columns >= F*D of X are never
    read. ``blocks`` > 0 forces the GPU grid size. One gfx950 launch on the GPU (one wave per sample, no atomics,
    the same bits for every grid size); the CPU path is the fp32 PyTorch reference of the same rule."""
    F, D, B = int(F), int(D), X.shape[0]
    if S is None:
        S = torch.empty(B, D, dtype=torch.float32, device=X.device)
    if _gpu(X):
        dfmk().wd_fm_forward(X, F, D, wide, S, int(blocks))
        return S
    _wd_fm_check(X, F, D)
    v = X[:, : F * D].float().reshape(B, F, D)
    s = v.sum(1)
    S.copy_(s)
    wide += 0.5 * (s * s - (v * v).sum(1)).sum(1)
    return S


def wd_fm_backward(X, S, dwide, dX, F, D, perm=None, blocks=0):
    """The interaction term's gradient added to the embedding gradient (csrc/kernels/deepfm.h): for every lookup
    (b, f), row r = perm[b*F + f] (b*F + f without ``perm``) of ``dX`` (bf16, B*F*D contiguous elements) viewed as
    [B*F, D] becomes bf16(dX[r].float() + dwide[b] * (S[b] - v_bf)) -- three fp32 roundings and one to bf16. A
    ``perm`` (int32) entry outside [0, B*F) is skipped. In place; the CPU path computes the same bits."""
    F, D, B = int(F), int(D), X.shape[0]
    if _gpu(X):
        dfmk().wd_fm_backward(X, S, dwide, perm, dX, F, D, int(blocks))
        return dX
    _wd_fm_check(X, F, D)
    n = B * F
    if dX.numel() != n * D or not dX.is_contiguous():
        raise RuntimeError(f"wd_fm_backward: dX {tuple(dX.shape)}, expected {n * D} contiguous elements")
    v = X[:, : F * D].float().reshape(n, D)
    dx = dX.view(n, D)
    Sb = S.repeat_interleave(F, 0)
    dz = dwide.repeat_interleave(F)[:, None]
    if perm is None:
        dx.copy_((dx.float() + dz * (Sb - v)).to(torch.bfloat16))
        return dX
    r = perm.long()
    ok = (r >= 0) & (r < n)
    r = r[ok]
    dx[r] = (dx[r].float() + dz[ok] * (Sb[ok] - v[ok])).to(torch.bfloat16)
    return dX


# ----------------------------------------------------------------------------- Deep & Cross layers
CROSS_MAX_D = 2048   # csrc/kernels/dcn.h: kDcnMaxD, kDcnMaxL, kDcnChunk, kDcnTrailer (the binding exports them too)
CROSS_MAX_L = 4
CROSS_CHUNK = 32
CROSS_TRAILER = 8


def wd_cross_part_shape(B, d, L):
    """Shape of wd_cross_backward's per-chunk partial batch sums: one row per CROSS_CHUNK samples holding the L+1
    partial T_j rows of align8(d) columns and a trailer whose first L+1 slots are the partial scalar sums."""
    return (int(B) + CROSS_CHUNK - 1) // CROSS_CHUNK, (int(L) + 1) * ((int(d) + 7) // 8 * 8) + CROSS_TRAILER


def _wd_cross_check(X, d, Pc, L):
    if not 1 <= L <= CROSS_MAX_L:
        raise RuntimeError(f"wd_cross: L is {L}, expected 1 <= L <= {CROSS_MAX_L}")
    if not 1 <= d <= CROSS_MAX_D:
        raise RuntimeError(f"wd_cross: d is {d}, expected 1 <= d <= {CROSS_MAX_D}")
    if X is not None and (X.dim() != 2 or X.shape[1] < d):
        raise RuntimeError(f"wd_cross: X has shape {tuple(X.shape)}, expected [B, >= d = {d}]")
    if tuple(Pc.shape) != (2 * L + 1, (d + 7) // 8 * 8):
        raise RuntimeError(f"wd_cross: Pc has shape {tuple(Pc.shape)}, expected [{2 * L + 1}, {(d + 7) // 8 * 8}]")


def _wd_cross_a(p, k, L):
    """a_0 .. a_L of the scalar rule (csrc/kernels/dcn.h), one rounded fp32 operation per line."""
    a = [torch.ones_like(p[:, 0])]
    for l in range(L):
        t = a[l] * p[:, l]
        s = t + k[l]
        a.append(a[l] + s)
    return a


def wd_cross_forward(X, d, Pc, L, wide, p=None, k=None, blocks=0):
    """Deep & Cross layers over the assembled Wide&Deep input (the rule: csrc/kernels/dcn.h). X bf16 [B, >= d],
    x_0 = X[:, :d]; Pc bf16 [(2L+1), align8(d)] holds w_0, b_0, ..., w_{L-1}, b_{L-1}, w_c. With p_j = <x_0, w_j>
    and k_j = <b_0 + ... + b_{j-1}, w_j> (w_L = w_c):  a = 1; s_l = a p_l + k_l; a += s_l (l < L);
    wide[b] += a p_L + k_L -- the recurrence x_{l+1} = x_0 <x_l, w_l> + b_l + x_l, wide += <x_L, w_c>, exactly.
    Returns (p fp32 [B, L+1], k fp32 [L+1]) for the backward (written in place when given, no allocation). Columns
    >= d of X and of Pc are never read. ``blocks`` > 0 forces the GPU grid size. One gfx950 launch on the GPU (one
    wave per sample, no atomics, the same bits for every grid size); the CPU path is the fp32 PyTorch reference of
    the same rule (its dot products are summed in PyTorch's order)."""
    d, L, B = int(d), int(L), X.shape[0]
    if p is None:
        p = torch.empty(B, L + 1, dtype=torch.float32, device=X.device)
    if k is None:
        k = torch.empty(L + 1, dtype=torch.float32, device=X.device)
    if _gpu(X):
        dcnk().wd_cross_forward(X, d, Pc, L, wide, p, k, int(blocks))
        return p, k
    _wd_cross_check(X, d, Pc, L)
    if B == 0:
        return p, k
    x = X[:, :d].float()
    W, bb = Pc[0::2, :d].float(), Pc[1::2, :d].float()
    p.copy_(x @ W.t())
    Bj = torch.cat([torch.zeros(1, d), torch.cumsum(bb, 0)])  # B_0 .. B_L
    k.copy_((Bj * W).sum(1))
    a = _wd_cross_a(p, k, L)
    t = a[L] * p[:, L]
    wide += t + k[L]
    return p, k


def wd_cross_backward(X, d, p, k, dwide, Pc, L, dX, F, D, part, perm=None, blocks=0):
    """The cross layers' backward (csrc/kernels/dcn.h) from the forward's ``p`` and ``k``: nothing is recomputed
    over d. Per sample dz = dwide[b], ds_L = dz, r = dz p_L, ds_l = r, r += ds_l p_l (l = L-1 .. 0), m_j = ds_j a_j.
    Embedding gradient: for every lookup (b, f), row r = perm[b*F + f] (b*F + f without ``perm``) of ``dX`` (bf16,
    B*F*D contiguous elements) viewed as [B*F, D] becomes bf16(dX[r].float() + sum_j m_j w_j[f*D:(f+1)*D]), the sum
    in the order j = 0 .. L; a ``perm`` (int32) entry outside [0, B*F) is skipped, the dense-feature columns get no
    gradient. Batch sums: ``part`` (fp32, wd_cross_part_shape) receives per chunk of CROSS_CHUNK samples the partial
    T_j = sum_b m_j x_0 and sum_b ds_j for ops.wd_cross_fold. In place; the CPU path computes the same dX bits."""
    d, L, F, D, B = int(d), int(L), int(F), int(D), X.shape[0]
    if _gpu(X):
        dcnk().wd_cross_backward(X, d, p, k, dwide, Pc, L, perm, dX, F, D, part, int(blocks))
        return dX
    _wd_cross_check(X, d, Pc, L)
    if not 1 <= D <= 64 or F < 1 or F * D > d:
        raise RuntimeError(f"wd_cross_backward: D is {D} and F is {F}, expected 1 <= D <= 64, F >= 1, F * D <= d")
    n = B * F
    if dX.numel() != n * D or not dX.is_contiguous():
        raise RuntimeError(f"wd_cross_backward: dX {tuple(dX.shape)}, expected {n * D} contiguous elements")
    if tuple(part.shape) != wd_cross_part_shape(B, d, L):
        raise RuntimeError(f"wd_cross_backward: part {tuple(part.shape)}, expected {wd_cross_part_shape(B, d, L)}")
    if B == 0:
        return dX
    L1, dp = L + 1, (d + 7) // 8 * 8
    x = X[:, :d].float()
    W = Pc[0::2, :d].float()
    a = _wd_cross_a(p, k, L)
    ds = [None] * L1
    ds[L] = dwide
    r = dwide * p[:, L]
    for l in range(L - 1, -1, -1):
        ds[l] = r
        t = ds[l] * p[:, l]
        r = r + t
    m = torch.stack([ds[j] * a[j] for j in range(L1)], 1)  # [B, L+1]
    ds = torch.stack(ds, 1)
    g = m[:, 0:1] * W[0, : F * D]
    for j in range(1, L1):
        t = m[:, j: j + 1] * W[j, : F * D]
        g = g + t
    g = g.reshape(n, D)
    dx = dX.view(n, D)
    if perm is None:
        dx.copy_((dx.float() + g).to(torch.bfloat16))
    else:
        r = perm.long()
        ok = (r >= 0) & (r < n)
        r = r[ok]
        dx[r] = (dx[r].float() + g[ok]).to(torch.bfloat16)
    nch = part.shape[0]
    pad = nch * CROSS_CHUNK - B
    mc = torch.cat([m, m.new_zeros(pad, L1)]).view(nch, CROSS_CHUNK, L1)
    xc = torch.cat([x, x.new_zeros(pad, d)]).view(nch, CROSS_CHUNK, d)
    part.zero_()
    part[:, : L1 * dp].view(nch, L1, dp)[:, :, :d] = torch.einsum("cbj,cbd->cjd", mc, xc)
    part[:, L1 * dp: L1 * dp + L1] = torch.cat([ds, ds.new_zeros(pad, L1)]).view(nch, CROSS_CHUNK, L1).sum(1)
    return dX


def wd_cross_fold(part, Pc, d, L, Gc):
    """The cross parameters' gradients from the backward's partial batch sums, ADDED into ``Gc`` (fp32
    [(2L+1), align8(d)], rows as Pc's): with T_j and Sd_j the sums of the chunks in chunk order and B_l = b_0 + ...
    + b_{l-1}:  dw_l = T_l + B_l Sd_l (l = 0 .. L, w_L = w_c),  db_l = Sd_L w_c + sum_{j>l} Sd_j w_j (added in the
    order j = L-1 .. l+1). One gfx950 launch; the CPU path is the fp32 reference of the same rule."""
    d, L = int(d), int(L)
    nch = part.shape[0]
    if _gpu(part):
        dcnk().wd_cross_fold(part, nch, Pc, d, L, Gc)
        return Gc
    _wd_cross_check(None, d, Pc, L)
    L1, dp = L + 1, (d + 7) // 8 * 8
    if part.dim() != 2 or part.shape[1] != L1 * dp + CROSS_TRAILER or tuple(Gc.shape) != (2 * L + 1, dp):
        raise RuntimeError(f"wd_cross_fold: part {tuple(part.shape)} / Gc {tuple(Gc.shape)}, expected "
                           f"[nchunks, {L1 * dp + CROSS_TRAILER}] / [{2 * L + 1}, {dp}]")
    if nch == 0:
        return Gc
    T = part[:, : L1 * dp].view(nch, L1, dp)[:, :, :d]
    S = part[:, L1 * dp: L1 * dp + L1]
    Tt, Sd = torch.zeros(L1, d), torch.zeros(L1)
    for c in range(nch):
        Tt = Tt + T[c]
        Sd = Sd + S[c]
    W, bb = Pc[0::2, :d].float(), Pc[1::2, :d].float()
    Bc = torch.zeros(d)
    for l in range(L1):
        t = Bc * Sd[l]
        Gc[2 * l, :d] += Tt[l] + t
        if l < L:
            Bc = Bc + bb[l]
    r = Sd[L] * W[L]
    for l in range(L - 1, -1, -1):
        Gc[2 * l + 1, :d] += r
        t = Sd[l] * W[l]
        r = r + t
    return Gc


# ----------------------------------------------------------------------------- held-out evaluation
EVAL_LOSS_SCALE = float(1 << 24)  # loss_fx counts units of 2^-24


def _eval_bins(acc) -> int:
    NB = (acc.numel() - 2) // 2
    if acc.dtype != torch.int64 or acc.numel() != 2 * NB + 2 or not 32 <= NB <= 8192 or NB & (NB - 1):
        raise RuntimeError(f"acc must be int64 [2*NB + 2] with NB a power of two in [32, 8192], got "
                           f"{acc.dtype} [{acc.numel()}]")
    return NB


def binary_hist(logits, labels, acc):
    """Accumulate fp32 ``logits`` [n] with 0/1 float ``labels`` into ``acc`` (int64, neg[NB] | pos[NB] |
    loss_fx | n_nan). Per sample: a NaN logit only counts in n_nan; y = label > 0.5;
    bin = min(NB-1, floor((clamp(z, -16, 16) + 16) * (NB/32))) (the logit is binned, not the probability:
    no transcendental, so CPU and GPU bins agree bit for bit); loss_fx += round(l * 2^24) with
    l = max(zl,0) - zl*y + log1p(exp(-|zl|)), zl = clamp(z, -64, 64). Integer sums: independent of order."""
    NB = _eval_bins(acc)
    if _gpu(logits):
        evalk().binary_hist(logits, labels, acc)
        return
    z = logits.reshape(-1).to(torch.float32)
    y = labels.reshape(-1).to(torch.float32) > 0.5
    ok = ~torch.isnan(z)
    acc[2 * NB + 1] += int((~ok).sum())
    z, y = z[ok], y[ok]
    zc = torch.clamp(z, -16.0, 16.0)
    bins = torch.clamp_max(torch.floor((zc + 16.0) * float(NB // 32)).to(torch.int64), NB - 1)
    acc[:NB] += torch.bincount(bins[~y], minlength=NB)
    acc[NB:2 * NB] += torch.bincount(bins[y], minlength=NB)
    zl = torch.clamp(z, -64.0, 64.0)
    l = torch.clamp_min(zl, 0) - zl * y.to(torch.float32) + torch.log1p(torch.exp(-zl.abs()))
    acc[2 * NB] += torch.round(l * EVAL_LOSS_SCALE).to(torch.int64).sum()


def eval_head(H, w, b0, wide, labels, acc, logits_out=None):
    """The forward half of wd_head fused with binary_hist: z = H . w + b0 + wide (fp32 accumulate; ``wide``
    may be None) goes through binary_hist's rule into ``acc``; ``logits_out`` (fp32 [B], optional)
    receives z. H: bf16 [B, Hd] rows (a column-sliced view is fine), Hd % 8 == 0, 8 <= Hd <= 1024."""
    if _gpu(H):
        evalk().eval_head_hist(H, w, b0, wide, labels, acc, logits_out)
        return
    z = H.float() @ w.float() + b0.float()
    if wide is not None:
        z = z + wide
    if logits_out is not None:
        logits_out.copy_(z)
    binary_hist(z, labels, acc)


def emb_csr_positions(members):
    """pos[members[m]] = m (int32): the member-order row of every lookup (the dgrad's permutation)."""
    if _gpu(members):
        return kernels().emb_csr_positions(members)
    pos = torch.empty_like(members)
    pos[members.long()] = torch.arange(members.numel(), dtype=members.dtype)
    return pos


def emb_build_csr(inv, F, U, zeroed=None, counts_ready=False):
    """Lookups grouped by unique row: (members, memrow) int32 [n] with memrow sorted and
    members[i] the lookup id (b*F + f) of the i-th entry. Depends on ``inv`` only, so the PS
    builds it while planning a batch (off the critical path). ``zeroed``: an already-zero int32
    block of >= 2U (from unique_bucketize_n's extra_zero_ints) saves the counter memset."""
    if _gpu(inv):
        return tuple(kernels().emb_build_csr(inv, int(F), int(max(U, 1)), zeroed, bool(counts_ready)))
    order = torch.sort(inv, stable=True).indices
    return order.to(torch.int32), inv[order].to(torch.int32)


def wd_emb_backward(dX, dwide, inv, F, D, grad_rows, x_off=0, csr=None, sorted_rows=False):
    """grad_rows[u, :D] = sum of dX[b, x_off + f*D : ...] over the lookups (b, f) with
    inv[b*F+f] == u; column D likewise sums dwide[b] when given, columns D+1.. are 0. On the GPU
    (D 16 / 32 / 64) every row that has lookups (every unique row of a plan) is written exactly
    once, in a fixed summation order -- the same bits on every run; rows without lookups are left
    untouched -- and ``grad_rows`` may be fp32 or bf16 (the multi-rank push payload);
    the CPU reference adds into grad_rows, so callers pass a zeroed buffer. ``sorted_rows``: dX is
    [B*F, D] in the CSR's member order (row m = lookup csr[0][m]; linear_dgrad(perm=csr[2]) writes it)."""
    if _gpu(dX):
        members, memrow = (csr[0], csr[1]) if csr is not None else (None, None)
        kernels().wd_emb_backward(dX, dwide, inv, int(F), int(D), grad_rows, int(x_off), members, memrow,
                                  bool(sorted_rows))
        return grad_rows
    if sorted_rows:  # back to lookup order
        un = torch.empty_like(dX)
        un[csr[0].long()] = dX
        dX, x_off = un.reshape(-1, F * D), 0
    B = dX.shape[0]
    g = dX[:, x_off: x_off + F * D].float().reshape(B * F, D)
    acc = grad_rows if grad_rows.dtype == torch.float32 else grad_rows.float()
    acc[:, :D].index_add_(0, inv, g)
    if dwide is not None:
        acc[:, D].index_add_(0, inv, dwide.repeat_interleave(F))
    if acc is not grad_rows:
        grad_rows.copy_(acc)
    return grad_rows


# ----------------------------------------------------------------------------- factorization machine
def _fm_check_k(k: int, width: int):
    if k % 4 or not 4 <= k <= 60:
        raise RuntimeError(f"fm: k is {k}, expected k % 4 == 0 and 4 <= k <= 60")
    if width < k + 4:
        raise RuntimeError(f"fm: rows are {width} wide, expected >= k + 4 = {k + 4}")


def fm_forward(rowptr, inv, vals, labels, rows, k, w0=None, gscale=1.0, blocks=0):
    """2-way factorization machine over a CSR batch of pulled rows [v_0 .. v_{k-1} | w | pad] (the rule:
    csrc/kernels/fm.h). Sample b holds the lookups j in [rowptr[b], rowptr[b+1]); lookup j reads rows[inv[j]]
    with value vals[j]. y = labels > 0.5. Returns fp32 (S [B, k], z [B], dz [B], loss [B]) and rowid int32 [n]:
      S_bf = sum_j v_f x,  z = w0 + sum_j w x + (sum_f S_bf^2 - sum_j sum_f (v_f x)^2) / 2,
      loss = max(z, 0) - z y + log1p(exp(-|z|)),  dz = (sigmoid(z) - y) * gscale,  rowid[j] = b.
    ``w0``: fp32 tensor whose first element is the bias (None: 0). ``blocks`` > 0 forces the GPU grid size.
    One fused gfx950 launch on the GPU (no atomics, the same bits for every grid size); the CPU path is
    the fp32 PyTorch reference of the same rule."""
    k, B, n = int(k), rowptr.numel() - 1, inv.numel()
    if _gpu(rows):
        dev = rows.device
        S = torch.empty(B, k, dtype=torch.float32, device=dev)
        z, dz, loss = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        rowid = torch.empty(n, dtype=torch.int32, device=dev)
        fmk().fm_forward(rowptr, inv, vals, labels, rows, k, w0, float(gscale), S, z, dz, loss, rowid, int(blocks))
        return S, z, dz, loss, rowid
    _fm_check_k(k, rows.shape[1])
    rowid = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), rowptr[1:] - rowptr[:-1])
    x = vals.float()
    p = rows[inv, :k].float() * x[:, None]
    S = torch.zeros(B, k, dtype=torch.float32).index_add_(0, rowid, p)
    Q = torch.zeros(B, dtype=torch.float32).index_add_(0, rowid, (p * p).sum(1))
    lin = torch.zeros(B, dtype=torch.float32).index_add_(0, rowid, rows[inv, k].float() * x)
    z = lin + 0.5 * ((S * S).sum(1) - Q)
    if w0 is not None:
        z = z + w0.reshape(-1)[0].float()
    y = (labels > 0.5).float()
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    dz = (torch.sigmoid(z) - y) * torch.tensor(float(gscale), dtype=torch.float32)
    return S, z, dz, loss, rowid.to(torch.int32)


def fm_backward(inv, rowid, vals, dz, S, rows, k, grad_rows, csr=None, blocks=0):
    """Gradient of every unique pulled row of fm_forward's batch (csrc/kernels/fm.h): with c_m = dz[rowid[m]] *
    vals[m] over the lookups m of row u (inv[m] == u), grad_rows[u, f] = sum_m c_m (S[rowid[m], f] - rows[u, f]
    vals[m]) for f < k, grad_rows[u, k] = sum_m c_m, columns k+1.. are 0; rows without lookups are left
    untouched. ``csr`` = (members, memrow): the lookups grouped by unique row (a plan's lookup CSR; built from
    ``inv`` here when absent on the GPU, ignored on the CPU). On the GPU every such row is written exactly once
    in a fixed summation order -- no atomics, the same bits on every run and for every grid size (``blocks``);
    the CPU reference sums with index_add_ over ``inv``."""
    k = int(k)
    if _gpu(rows):
        if csr is None:
            csr = emb_build_csr(inv, 1, max(rows.shape[0], 1))
        fmk().fm_backward(csr[0], csr[1], rowid, vals, dz, S, rows, k, grad_rows, int(blocks))
        return grad_rows
    _fm_check_k(k, rows.shape[1])
    W = k + 4
    if grad_rows.shape[1] != W or grad_rows.shape[0] < rows.shape[0]:
        raise RuntimeError(f"fm_backward: grad_rows {tuple(grad_rows.shape)}, expected [>= {rows.shape[0]}, {W}]")
    if inv.numel() == 0:
        return grad_rows
    b, x = rowid.long(), vals.float()
    c = dz[b] * x
    acc = torch.zeros(rows.shape[0], W, dtype=torch.float32)
    acc[:, :k].index_add_(0, inv, c[:, None] * (S[b] - rows[inv, :k].float() * x[:, None]))
    acc[:, k].index_add_(0, inv, c)
    touched = torch.zeros(rows.shape[0], dtype=torch.bool)
    touched[inv] = True
    grad_rows[: rows.shape[0]][touched] = acc[touched]
    return grad_rows


# ----------------------------------------------------------------------------- field-aware factorization machine
FFM_MAX_F, FFM_MAX_K, FFM_MAX_FK = 64, 16, 512   # csrc/kernels/ffm.h (the binding exports them too)


def _ffm_check(F: int, k: int, width: int):
    if k % 4 or not 4 <= k <= FFM_MAX_K or not 1 <= F <= FFM_MAX_F or F * k > FFM_MAX_FK:
        raise RuntimeError(f"ffm: F is {F} and k is {k}, expected k % 4 == 0, 4 <= k <= {FFM_MAX_K}, 1 <= F <= "
                           f"{FFM_MAX_F} and F * k <= {FFM_MAX_FK}")
    if width < F * k + 4:
        raise RuntimeError(f"ffm: rows are {width} wide, expected >= F * k + 4 = {F * k + 4}")


def _ffm_padded(rowptr, inv, vals, fields, cap, F):
    """The batch padded to its max nnz: (pos [B, Mx] lookup index, ok [B, Mx] a lookup that counts, r / f / x
    [B, Mx] its row, field and value (0 where not ok)) and rowid [n]. rowptr is clamped to [0, n]."""
    B, n = rowptr.numel() - 1, inv.numel()
    rp = rowptr.clamp(0, n)
    st, cnt = rp[:-1], (rp[1:] - rp[:-1]).clamp(min=0)
    Mx = int(cnt.max()) if B else 0
    pos = st[:, None] + torch.arange(Mx, dtype=torch.int64)[None, :]
    inside = torch.arange(Mx)[None, :] < cnt[:, None]
    pos = torch.where(inside, pos, torch.zeros_like(pos))
    r, f = inv[pos], fields[pos].long()
    ok = inside & (r >= 0) & (r < cap) & (f >= 0) & (f < F)
    zero = torch.zeros_like(pos)
    x = torch.where(ok, vals.float()[pos], torch.zeros(()))
    rowid = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), cnt)
    if rowid.numel() != n or int(st[0] if B else 0) != 0:  # a rowptr that does not cover [0, n)
        full = torch.zeros(n, dtype=torch.int64)
        full[pos[inside]] = torch.arange(B)[:, None].expand(B, Mx)[inside]
        rowid = full
    return pos, inside, ok, torch.where(ok, r, zero), torch.where(ok, f, zero), x, rowid


def _ffm_chunks(B, Mx, k):
    """Sample ranges whose [b, Mx, Mx, k] intermediates stay near 2^24 elements."""
    step = max(1, (1 << 24) // max(1, Mx * Mx * k))
    return [(lo, min(B, lo + step)) for lo in range(0, B, step)]


def ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0=None, gscale=1.0, blocks=0):
    """Field-aware factorization machine over a CSR batch of pulled rows [v_0 | v_1 | ... | v_{F-1} | w | pad]
    (the rule: csrc/kernels/ffm.h): slot g (k columns) of a row is the vector its feature uses against a partner
    of field g. Sample b holds the lookups j in [rowptr[b], rowptr[b+1]); lookup j reads rows[inv[j]] with value
    vals[j] and field fields[j] (int32 in [0, F)). y = labels > 0.5. Returns fp32 (z [B], dz [B], loss [B]) and
    rowid int32 [n]:
      z = w0 + sum_j w x + sum_{i<j} <v_{inv[i], fields[j]}, v_{inv[j], fields[i]}> x_i x_j,
      loss = max(z, 0) - z y + log1p(exp(-|z|)),  dz = (sigmoid(z) - y) * gscale,  rowid[j] = b.
    A lookup whose inv is outside [0, cap) or whose field is outside [0, F) contributes nothing. ``w0``: fp32
    tensor whose first element is the bias (None: 0). ``blocks`` > 0 forces the GPU grid size. One fused gfx950
    launch on the GPU (no atomics, the same bits for every grid size); the CPU path is the fp32 PyTorch
    reference of the same rule, samples padded to the batch's max nnz."""
    F, k, B, n = int(F), int(k), rowptr.numel() - 1, inv.numel()
    if _gpu(rows):
        dev = rows.device
        z, dz, loss = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        rowid = torch.empty(n, dtype=torch.int32, device=dev)
        ffmk().ffm_forward(rowptr, inv, vals, fields, labels, rows, F, k, w0, float(gscale), z, dz, loss, rowid,
                           int(blocks))
        return z, dz, loss, rowid
    _ffm_check(F, k, rows.shape[1])
    cap, FK = rows.shape[0], F * k
    pos, inside, ok, r, f, x, rowid = _ffm_padded(rowptr, inv, vals, fields, cap, F)
    Mx = pos.shape[1]
    slots = rows[:, :FK].float().reshape(cap * F, k)
    # (the linear term summed as fm_forward's reference sums it: in lookup order, by index_add_)
    z = torch.zeros(B, dtype=torch.float32).index_add_(
        0, torch.arange(B)[:, None].expand(B, Mx)[ok], rows[:, FK].float()[r[ok]] * x[ok])
    upper = torch.triu(torch.ones(Mx, Mx, dtype=torch.bool), diagonal=1)
    for lo, hi in _ffm_chunks(B, Mx, k):
        rr, ff, xx = r[lo:hi], f[lo:hi], x[lo:hi]
        A = slots[rr[:, :, None] * F + ff[:, None, :]]  # A[b, i, j] = v_{inv[i], fields[j]}
        P = (A * A.transpose(1, 2)).sum(-1) * (xx[:, :, None] * xx[:, None, :])
        z[lo:hi] += (P * upper).sum((1, 2))
    if w0 is not None:
        z = z + w0.reshape(-1)[0].float()
    y = (labels > 0.5).float()
    loss = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    dz = (torch.sigmoid(z) - y) * torch.tensor(float(gscale), dtype=torch.float32)
    return z, dz, loss, rowid.to(torch.int32)


def ffm_backward(inv, rowid, rowptr, vals, fields, dz, rows, F, k, grad_rows, csr=None, blocks=0):
    """Gradient of every unique pulled row of ffm_forward's batch (csrc/kernels/ffm.h): with c_m = dz[rowid[m]] *
    vals[m] over the lookups m of row u (inv[m] == u), grad_rows[u, g k + c] = sum_m c_m sum_j rows[inv[j],
    fields[m] k + c] vals[j] over the other lookups j of m's sample with fields[j] == g, grad_rows[u, F k] =
    sum_m c_m, the three pad columns are 0; rows without lookups are left untouched. Self is skipped, not
    subtracted. ``csr`` = (members, memrow): the lookups grouped by unique row (a plan's lookup CSR; built from
    ``inv`` here when absent on the GPU, ignored on the CPU). On the GPU every such row is written exactly once
    in a fixed summation order -- no atomics, the same bits on every run and for every grid size (``blocks``) --
    and everything is recomputed from ``rows``, a member or sample index (``csr``, ``rowid``) out of range is
    skipped. The CPU reference sums with index_add_ and takes every lookup's sample from ``rowptr``: it reads
    neither ``rowid`` nor ``csr``."""
    F, k = int(F), int(k)
    if _gpu(rows):
        if csr is None:
            csr = emb_build_csr(inv, 1, max(rows.shape[0], 1))
        ffmk().ffm_backward(csr[0], csr[1], rowid, rowptr, inv, vals, fields, dz, rows, F, k, grad_rows, int(blocks))
        return grad_rows
    _ffm_check(F, k, rows.shape[1])
    cap, FK, W = rows.shape[0], F * k, F * k + 4
    if grad_rows.shape[1] != W or grad_rows.shape[0] < cap:
        raise RuntimeError(f"ffm_backward: grad_rows {tuple(grad_rows.shape)}, expected [>= {cap}, {W}]")
    if inv.numel() == 0 or dz.numel() == 0:
        return grad_rows
    pos, inside, ok, r, f, x, _ = _ffm_padded(rowptr, inv, vals, fields, cap, F)
    B, Mx = pos.shape
    c = dz.float()[:, None] * x  # [B, Mx]: 0 where the lookup does not count
    slots = rows[:, :FK].float().reshape(cap * F, k)
    acc = torch.zeros(cap * F, k, dtype=torch.float32)
    lin = torch.zeros(cap, dtype=torch.float32).index_add_(0, r[ok], c[ok])
    off = ~torch.eye(Mx, dtype=torch.bool)
    for lo, hi in _ffm_chunks(B, Mx, k):
        rr, ff, xx, oo = r[lo:hi], f[lo:hi], x[lo:hi], ok[lo:hi]
        pair = oo[:, :, None] & oo[:, None, :] & off  # [b, member i, partner j]
        # member i of row inv[i] receives, in slot fields[j], c_i x_j v_{inv[j], fields[i]}
        src = (rr[:, None, :] * F + ff[:, :, None]).expand(-1, Mx, Mx)[pair]
        dst = (rr[:, :, None] * F + ff[:, None, :]).expand(-1, Mx, Mx)[pair]
        s = (c[lo:hi][:, :, None] * xx[:, None, :]).expand(-1, Mx, Mx)[pair]
        acc.index_add_(0, dst, slots[src] * s[:, None])
    touched = torch.zeros(cap, dtype=torch.bool)  # every row of the lookup CSR is written, as on the GPU
    touched[inv[(inv >= 0) & (inv < cap)]] = True
    out = torch.zeros(cap, W, dtype=torch.float32)
    out[:, :FK] = acc.reshape(cap, FK)
    out[:, FK] = lin
    grad_rows[:cap][touched] = out[touched]
    return grad_rows


# ----------------------------------------------------------------------------- histogram GBDT in fixed point
GBDT_MAX_BINS, GBDT_MAX_DEPTH, GBDT_MAX_F = 256, 8, 4096  # csrc/kernels/gbdt.h (the binding exports them too)
GBDT_SCALE = 1 << 20
_GBDT_ROWS = 1 << 16  # samples per pass of the CPU references


def _gbdt_hist_dims(hist):
    if hist.dim() != 4 or hist.shape[3] != 3 or hist.dtype != torch.int64:
        raise RuntimeError(f"gbdt: hist must be int64 [nodes, F, NB, 3], got {hist.dtype} {tuple(hist.shape)}")
    nodes, F, NB = hist.shape[:3]
    if not (1 <= nodes <= 1 << (GBDT_MAX_DEPTH - 1) and nodes & (nodes - 1) == 0 and 1 <= F <= GBDT_MAX_F
            and 2 <= NB <= GBDT_MAX_BINS):
        raise RuntimeError(f"gbdt: hist {tuple(hist.shape)}: nodes a power of two <= 128, 1 <= F <= {GBDT_MAX_F}, "
                           f"2 <= NB <= {GBDT_MAX_BINS}")
    return nodes, F, NB


def gbdt_bin(X, cuts, out=None, blocks=0):
    """bins uint8 [N, ldb] of fp32 features X [N, F] against cuts fp32 [F, NB - 1] (ascending per feature, padded
    with +inf; the rule: csrc/kernels/gbdt.h): bin(x, f) = #{j : x > cuts[f, j]}, comparisons only (NaN -> 0).
    ``out``: a uint8 [N, >= F] matrix to fill (columns >= F untouched); None allocates zeros with ldb =
    align16(F). ``blocks`` > 0 forces the GPU grid size."""
    N, F = X.shape[0], cuts.shape[0]
    if out is None:
        out = torch.zeros(N, (F + 15) & ~15, dtype=torch.uint8, device=X.device)
    if _gpu(X):
        gbdtk().gbdt_bin(X, cuts, out, int(blocks))
        return out
    NB = cuts.shape[1] + 1
    if X.dim() != 2 or X.shape[1] != F or not (1 <= F <= GBDT_MAX_F and 2 <= NB <= GBDT_MAX_BINS) or \
            out.shape[0] != N or out.shape[1] < F:
        raise RuntimeError(f"gbdt_bin: X {tuple(X.shape)}, cuts {tuple(cuts.shape)}, bins {tuple(out.shape)}")
    step = max(1, (1 << 24) // (F * NB))
    for lo in range(0, N, step):
        x = X[lo:lo + step].float()
        out[lo:lo + step, :F] = (x[:, :, None] > cuts[None]).sum(-1).to(torch.uint8)
    return out


def gbdt_grad(z, labels, gh, loss_acc, blocks=0):
    """Fixed-point gradients of the logistic loss (csrc/kernels/gbdt.h): gh int32 [N, 2] = (llrint((p - y) 2^20),
    llrint(max(p (1 - p), 2^-20) 2^20)) with p = sigmoid(clamp(z, -30, 30)) in fp32, y = labels > 0.5; adds
    sum llrint(loss 2^24) to the int64 ``loss_acc`` [1] (loss: the evalmetrics formula)."""
    if _gpu(z):
        gbdtk().gbdt_grad(z, labels, gh, loss_acc, int(blocks))
        return gh
    N = z.numel()
    if gh.shape != (N, 2) or gh.dtype != torch.int32 or labels.numel() != N or loss_acc.dtype != torch.int64:
        raise RuntimeError(f"gbdt_grad: z [{N}], labels [{labels.numel()}], gh {gh.dtype} {tuple(gh.shape)}")
    S = float(GBDT_SCALE)
    y = (labels > 0.5).float()
    p = 1.0 / (1.0 + torch.exp(-z.float().clamp(-30.0, 30.0)))
    gh[:, 0] = torch.round((p - y) * S).to(torch.int32)
    gh[:, 1] = torch.round((p * (1.0 - p)).clamp(min=1.0 / S) * S).to(torch.int32)
    zl = z.float().clamp(-64.0, 64.0)
    l = zl.clamp(min=0.0) - zl * y + torch.log1p(torch.exp(-zl.abs()))
    loss_acc += torch.round(l * 16777216.0).to(torch.int64).sum()
    return gh


def gbdt_hist(bins, node, gh, hist, path=0, blocks=0):
    """ADDS the level's gradient histograms into ``hist`` int64 [nodes, F, NB, 3] (sum qg, sum qh, count): sample
    i with 0 <= node[i] < nodes contributes once per feature f at bins[i, f]; a node id out of range or a bin >=
    NB contributes nothing. Integer sums only: the same bits for every ``path`` (0 auto, 1 LDS accumulators, 2
    global atomics) and ``blocks`` (> 0 forces the workgroups along the samples) and on the CPU."""
    if _gpu(hist):
        gbdtk().gbdt_hist(bins, node, gh, hist, int(path), int(blocks))
        return hist
    if path not in (0, 1, 2):
        raise RuntimeError(f"gbdt_hist: path {path}: 0 auto, 1 LDS, 2 global")
    return _gbdt_hist_ref(bins, node, gh, hist)


def _gbdt_hist_ref(bins, node, gh, hist):
    """The PyTorch composition of gbdt_hist (index_add_ into int64), on the tensors' device."""
    nodes, F, NB = _gbdt_hist_dims(hist)
    N = node.numel()
    if bins.dim() != 2 or bins.shape[0] != N or bins.shape[1] < F or gh.shape != (N, 2):
        raise RuntimeError(f"gbdt_hist: bins {tuple(bins.shape)}, node [{N}], gh {tuple(gh.shape)}")
    flat = hist.view(-1, 3)
    fs = torch.arange(F, dtype=torch.int64, device=hist.device)
    for lo in range(0, N, _GBDT_ROWS):
        nd = node[lo:lo + _GBDT_ROWS].long()
        b = bins[lo:lo + _GBDT_ROWS, :F].long()
        g = gh[lo:lo + _GBDT_ROWS].long()
        ok = ((nd >= 0) & (nd < nodes))[:, None] & (b < NB)
        idx = ((nd[:, None] * F + fs[None, :]) * NB + b)[ok]
        v = torch.cat([g, torch.ones(g.shape[0], 1, dtype=torch.int64, device=g.device)],
                      1)[:, None, :].expand(-1, F, -1)[ok]
        flat.index_add_(0, idx, v)
    return hist


def gbdt_split(hist, reg_lambda, min_child_count, min_gain, feat, thr, gain, child):
    """The best split of every node from ``hist`` alone (csrc/kernels/gbdt.h): candidates (f, t), left = bins <= t;
    gain = (GL GL / (HL + lambda) + GR GR / (HR + lambda)) - G G / (H + lambda) in fp64, every operation rounded
    on its own; valid with both counts >= min_child_count and gain > min_gain; largest gain, then lowest f, then
    lowest t. Writes feat / thr int32 [nodes] (feat -1, thr 0, gain 0: no valid split), gain fp64 [nodes], child
    int64 [nodes, 2, 3] (left and right sums; no split: feature 0's totals | zeros)."""
    if _gpu(hist):
        gbdtk().gbdt_split(hist, float(reg_lambda), int(min_child_count), float(min_gain), feat, thr, gain, child)
        return feat, thr, gain, child
    return _gbdt_split_ref(hist, reg_lambda, min_child_count, min_gain, feat, thr, gain, child)


def _gbdt_split_ref(hist, reg_lambda, min_child_count, min_gain, feat, thr, gain, child):
    """The PyTorch composition of gbdt_split (cumsum, the gain in fp64 op by op, the first maximum), on the
    tensors' device."""
    nodes, F, NB = _gbdt_hist_dims(hist)
    if not reg_lambda > 0 or min_child_count < 1 or not min_gain >= 0:
        raise RuntimeError(f"gbdt_split: reg_lambda {reg_lambda} > 0, min_child_count {min_child_count} >= 1, "
                           f"min_gain {min_gain} >= 0")
    sc = 1.0 / GBDT_SCALE
    cum = hist.cumsum(2)
    tot, L = cum[:, :, -1, :], cum[:, :, :NB - 1, :]
    R = tot[:, :, None, :] - L
    GL, HL, GR, HR = L[..., 0].double() * sc, L[..., 1].double() * sc, R[..., 0].double() * sc, R[..., 1].double() * sc
    G, H = tot[..., 0].double() * sc, tot[..., 1].double() * sc
    g = (GL * GL / (HL + reg_lambda) + GR * GR / (HR + reg_lambda)) - (G * G / (H + reg_lambda))[:, :, None]
    ok = (L[..., 2] >= min_child_count) & (R[..., 2] >= min_child_count) & (g > min_gain)
    g = torch.where(ok, g, torch.full_like(g, -math.inf)).reshape(nodes, F * (NB - 1))
    mx = g.max(1).values
    ids = torch.arange(F * (NB - 1), dtype=torch.int64, device=hist.device)
    first = torch.where(g == mx[:, None], ids[None, :], torch.full_like(ids, F * NB)[None, :]).min(1).values
    some = mx > -math.inf
    first = torch.where(some, first, torch.zeros_like(first))
    f, t = first // (NB - 1), first % (NB - 1)
    n = torch.arange(nodes, device=hist.device)
    left = torch.where(some[:, None], L[n, f, t], tot[:, 0])
    right = torch.where(some[:, None], tot[n, f] - left, torch.zeros_like(left))
    feat.copy_(torch.where(some, f, torch.full_like(f, -1)))
    thr.copy_(torch.where(some, t, torch.zeros_like(t)))
    gain.copy_(torch.where(some, mx, torch.zeros_like(mx)))
    child[:, 0], child[:, 1] = left, right
    return feat, thr, gain, child


def gbdt_leaf(child, reg_lambda, lr, leaf):
    """leaf fp32 [2 nodes] from a level's ``child`` [nodes, 2, 3]: leaf[2 n + s] = (float)(-(Gs 2^-20) / (Hs 2^-20 +
    lambda) * lr) in fp64 with every operation rounded on its own; a child with count 0 gets +0.0."""
    if _gpu(child):
        gbdtk().gbdt_leaf(child, float(reg_lambda), float(lr), leaf)
        return leaf
    if child.dim() != 3 or child.shape[1:] != (2, 3) or leaf.numel() != 2 * child.shape[0] or not reg_lambda > 0 \
            or not lr > 0:
        raise RuntimeError(f"gbdt_leaf: child {tuple(child.shape)}, leaf {tuple(leaf.shape)}, reg_lambda "
                           f"{reg_lambda}, lr {lr}")
    c = child.reshape(-1, 3)
    sc = 1.0 / GBDT_SCALE
    v = (-(c[:, 0].double() * sc)) / (c[:, 1].double() * sc + reg_lambda) * lr
    leaf.copy_(torch.where(c[:, 2] == 0, torch.zeros_like(v), v).float())
    return leaf


def gbdt_advance(bins, node, feat, thr, F, leaf=None, z=None, blocks=0):
    """node[i] <- 2 node[i] + (feat[node[i]] >= 0 and bins[i, feat] > thr), in place (a node id outside [0, nodes)
    or a feat >= F gives -1). With ``leaf`` [2 nodes] and ``z`` [N] (the last level) also z[i] += leaf[node'[i]]."""
    if (leaf is None) != (z is None):
        raise RuntimeError("gbdt_advance: leaf and z come together")
    if _gpu(node):
        gbdtk().gbdt_advance(bins, node, feat, thr, int(F), leaf, z, int(blocks))
        return node
    return _gbdt_advance_ref(bins, node, feat, thr, F, leaf, z)


def _gbdt_advance_ref(bins, node, feat, thr, F, leaf=None, z=None):
    """The PyTorch composition of gbdt_advance, on the tensors' device."""
    N, nodes = node.numel(), feat.numel()
    if bins.dim() != 2 or bins.shape[0] != N or bins.shape[1] < F or thr.numel() != nodes:
        raise RuntimeError(f"gbdt_advance: bins {tuple(bins.shape)}, node [{N}], feat [{nodes}], thr [{thr.numel()}]")
    if N == 0:
        return node
    nd = node.long()
    ok = (nd >= 0) & (nd < nodes)
    ndc = nd.clamp(0, nodes - 1)
    f = feat.long()[ndc]
    ok &= f < F
    b = bins[torch.arange(N, device=node.device), f.clamp(0, F - 1)].long()
    right = (f >= 0) & (b > thr.long()[ndc])
    out = torch.where(ok, 2 * nd + right.long(), torch.full_like(nd, -1))
    node.copy_(out)
    if leaf is not None:
        m = out >= 0
        z[m] = z[m] + leaf[out[m]]
    return node


def gbdt_predict(bins, feat, thr, leaf, F, depth, base, z, leaf_index=None, blocks=0):
    """z[i] = base + sum_t leaf[t, leaf of sample i in tree t], summed in fp32 in tree order, over complete
    level-major trees feat int32 / thr uint8 [T, 2^depth - 1], leaf fp32 [T, 2^depth]; optionally ``leaf_index``
    int32 [N, T]."""
    if _gpu(z):
        gbdtk().gbdt_predict(bins, feat, thr, leaf, int(F), int(depth), float(base), z, leaf_index, int(blocks))
        return z
    N, T, nn = z.numel(), feat.shape[0], (1 << depth) - 1
    if not 1 <= depth <= GBDT_MAX_DEPTH or feat.shape != (T, nn) or thr.shape != (T, nn) or \
            leaf.shape != (T, nn + 1) or bins.shape[0] != N or bins.shape[1] < F or \
            (leaf_index is not None and leaf_index.shape != (N, T)):
        raise RuntimeError(f"gbdt_predict: depth {depth}, feat {tuple(feat.shape)}, thr {tuple(thr.shape)}, leaf "
                           f"{tuple(leaf.shape)}, bins {tuple(bins.shape)}, z [{N}]")
    s = torch.full((N,), float(base), dtype=torch.float32)
    rows = torch.arange(N)
    for t in range(T):
        n = torch.zeros(N, dtype=torch.int64)
        for d in range(depth):
            at = (1 << d) - 1 + n
            f = feat[t].long()[at]
            b = bins[rows, f.clamp(0, F - 1)].long() if N else n
            n = 2 * n + ((f >= 0) & (f < F) & (b > thr[t].long()[at])).long()
        s = s + leaf[t][n]
        if leaf_index is not None:
            leaf_index[:, t] = n.to(torch.int32)
    z.copy_(s)
    return z


# ----------------------------------------------------------------------------- LDA collapsed Gibbs in fixed point
LDA_MIN_K, LDA_MAX_K, LDA_MAX_DOC_LEN = 2, 1024, 4096  # csrc/kernels/lda.h (the binding exports them too)
LDA_MAX_PRIOR = 64.0
LDA_LOGLIK_SCALE = float(1 << 24)
_LDA_GOLD = 0x9E3779B97F4A7C15
_LDA_M64 = (1 << 64) - 1
_LDA_M32 = (1 << 32) - 1


def _lda_s64(x: int) -> int:
    """The int64 that holds the bits of the uint64 x."""
    x &= _LDA_M64
    return x - (1 << 64) if x >> 63 else x


def lda_mix_int(x: int) -> int:
    """mix of csrc/kernels/lda.h on a Python integer (mod 2^64)."""
    x &= _LDA_M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _LDA_M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _LDA_M64
    x ^= x >> 31
    return x


def _lda_lsr(x: torch.Tensor, s: int) -> torch.Tensor:
    return (x >> s) & ((1 << (64 - s)) - 1)  # the logical shift of the uint64 held in an int64


def _lda_mix(x: torch.Tensor) -> torch.Tensor:
    """mix on int64 tensors holding uint64 bits (torch's int64 products wrap mod 2^64)."""
    x = x ^ _lda_lsr(x, 30)
    x = x * _lda_s64(0xBF58476D1CE4E5B9)
    x = x ^ _lda_lsr(x, 27)
    x = x * _lda_s64(0x94D049BB133111EB)
    return x ^ _lda_lsr(x, 31)


def mulhi_u64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The high 64 bits of the 128-bit product of two uint64 held in int64 tensors, from 32-bit limbs."""
    al, ah, bl, bh = a & _LDA_M32, _lda_lsr(a, 32), b & _LDA_M32, _lda_lsr(b, 32)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = _lda_lsr(ll, 32) + (lh & _LDA_M32) + (hl & _LDA_M32)
    return hh + _lda_lsr(lh, 32) + _lda_lsr(hl, 32) + _lda_lsr(mid, 32)


def _lda_check(op, K, alpha, beta, Vbeta, rows, blocks=0):
    if not LDA_MIN_K <= K <= LDA_MAX_K:
        raise RuntimeError(f"{op}: nk says K = {K}, expected {LDA_MIN_K} <= K <= {LDA_MAX_K}")
    if not (0 < alpha <= LDA_MAX_PRIOR and 0 < beta <= LDA_MAX_PRIOR):
        raise RuntimeError(f"{op}: alpha is {alpha} and beta {beta}, expected both in (0, 64]")
    if not 0 < Vbeta < float("inf"):
        raise RuntimeError(f"{op}: Vbeta is {Vbeta}, expected a positive finite V * beta")
    if rows.dim() != 2 or rows.shape[1] < K or rows.dtype != torch.float32:
        raise RuntimeError(f"{op}: rows must be fp32 [cap, >= {K}], got {rows.dtype} {tuple(rows.shape)}")
    if not 0 <= blocks <= 65535:
        raise RuntimeError(f"{op}: blocks is {blocks}, expected 0 <= blocks <= 65535")


def _lda_tokens(rowptr, n):
    """The tokens the documents cover: (lo [B], lens [B], doc [m], pos [m], t [m]) with t = lo[doc] + pos."""
    lo = rowptr[:-1].clamp(0, n)
    hi = torch.maximum(rowptr[1:].clamp(0, n), lo)
    lens = hi - lo
    B = lens.numel()
    doc = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), lens)
    start = torch.cumsum(lens, 0) - lens
    pos = torch.arange(doc.numel(), dtype=torch.int64) - start[doc]
    return lo, lens, doc, pos, lo[doc] + pos


def lda_sample(rowptr, gid, inv, z_old, rows, nk, alpha, beta, Vbeta, seed, it, z_new=None, dk=None, blocks=0):
    """One clock of delayed-update collapsed Gibbs sampling for LDA against the snapshot (rows, nk) (the rule:
    csrc/kernels/lda.h). Document d holds the tokens [rowptr[d], rowptr[d+1]) and has the global id gid[d]; token t
    reads rows[inv[t]] (fp32 counts [cap, >= K]); nk int64 [K]; z_old int16 [n], or None at the initialisation
    (it == 0). Returns (z_new int16 [n], dk int64 [K]); ``dk`` is ADDED to: -1 at the old and +1 at the new topic
    of every token whose topic changed (+1 only at the initialisation). A token whose inv lies outside [0, cap)
    keeps its topic and contributes nothing. The same bits on the GPU (one wave per document; ``blocks`` > 0 forces
    the grid) and in this PyTorch reference, which is vectorised across documents and loops over positions."""
    B, n, K = rowptr.numel() - 1, inv.numel(), nk.numel()
    alpha, beta, Vbeta, seed, it = float(alpha), float(beta), float(Vbeta), int(seed), int(it)
    if z_new is None:
        z_new = torch.empty(n, dtype=torch.int16, device=rows.device)
    if dk is None:
        dk = torch.zeros(K, dtype=torch.int64, device=rows.device)
    if _gpu(rows):
        ldak().lda_sample(rowptr, gid, inv, z_old, rows, nk, alpha, beta, Vbeta, _lda_s64(seed), it, z_new, dk,
                          int(blocks))
        return z_new, dk
    _lda_check("lda_sample", K, alpha, beta, Vbeta, rows, blocks)
    if it < 0 or (z_old is None) != (it == 0):
        raise RuntimeError(f"lda_sample: it is {it}: 0 is the initialisation and takes no z_old, a sweep needs one")
    if gid.numel() != B or z_new.numel() != n or dk.numel() != K or (z_old is not None and z_old.numel() != n):
        raise RuntimeError(f"lda_sample: gid [{gid.numel()}] for {B} documents, z_new [{z_new.numel()}] for {n} "
                           f"tokens, dk [{dk.numel()}] for K = {K}")
    cap = rows.shape[0]
    lo, lens, doc, pos, t = _lda_tokens(rowptr, n)
    base = _lda_s64(lda_mix_int(seed + it * _LDA_GOLD))
    one = torch.ones(1, dtype=torch.int64)
    if z_old is None:
        r = _lda_mix(base ^ (gid[doc] * 4096 + pos))
        kn = mulhi_u64(r, torch.full_like(r, K))
        live = (inv[t] >= 0) & (inv[t] < cap)
        z_new[t] = torch.where(live, kn, torch.full_like(kn, -1)).to(torch.int16)
        dk.index_add_(0, kn[live], one.expand(int(live.sum())))
        return z_new, dk
    z = z_old.long()
    live_t = (inv >= 0) & (inv < cap) & (z >= 0) & (z < K)
    z_new[t] = z_old[t]
    lt = live_t[t]
    ndk = torch.zeros(B, K, dtype=torch.int64)
    ndk.view(-1).index_add_(0, (doc * K + z[t])[lt], one.expand(int(lt.sum())))
    cinv0 = 1.0 / (nk.clamp(min=0).double() + Vbeta)
    for j in range(int(lens.max()) if B else 0):
        act = torch.nonzero(lens > j).squeeze(1)
        tj = lo[act] + j
        lv = live_t[tj]
        act, tj = act[lv], tj[lv]
        a = act.numel()
        if a == 0:
            continue
        A = torch.arange(a)
        ko, uu = z[tj], inv[tj]
        nd = ndk[act]
        nd[A, ko] -= 1
        av = nd.double() + alpha
        bv = rows[uu, :K].double()
        bv[A, ko] -= 1.0
        bv = bv.clamp(min=0.0) + beta
        cv = cinv0.expand(a, K).clone()
        cv[A, ko] = 1.0 / ((nk[ko] - 1).clamp(min=0).double() + Vbeta)
        x = (av * bv) * cv
        wt = (x * 1099511627776.0).to(torch.int64) + 1
        cs = torch.cumsum(wt, 1)
        r = _lda_mix(base ^ (gid[act] * 4096 + j))
        target = mulhi_u64(r, cs[:, -1])
        kn = (cs <= target[:, None]).sum(1).clamp(max=K - 1)
        nd[A, kn] += 1
        ndk[act] = nd
        z_new[tj] = kn.to(torch.int16)
        ch = kn != ko
        c = int(ch.sum())
        dk.index_add_(0, ko[ch], -one.expand(c))
        dk.index_add_(0, kn[ch], one.expand(c))
    return z_new, dk


def lda_delta(inv, z_old, z_new, K, delta, csr=None, blocks=0):
    """The count deltas of every unique pulled row of lda_sample's batch (csrc/kernels/lda.h): over the member
    tokens m of row u (inv[m] == u), delta[u, k] = #{z_new[m] == k} - #{z_old[m] == k} for k < K and 0 for the pad
    columns of delta fp32 [cap, align4(K)]; z_old None: +1 only (the initialisation). The whole row is written
    (explicit zeros included); rows without members are left untouched. ``csr`` = (members, memrow): a plan's
    lookup CSR (built from ``inv`` here when absent on the GPU, ignored on the CPU). On the GPU every such row is
    written exactly once from an integer LDS histogram -- no global atomics, the same bits for every grid size
    (``blocks``)."""
    K = int(K)
    W = (K + 3) & ~3
    if _gpu(delta):
        if csr is None:  # (not the model's path: a plan carries its CSR) rows outside [0, cap) go to a row past the
            cap = delta.shape[0]  # end, which the kernel ignores: emb_build_csr trusts its rows
            ok = (inv >= 0) & (inv < cap)
            csr = emb_build_csr(torch.where(ok, inv, torch.full_like(inv, cap)), 1, cap + 1)
        ldak().lda_delta(csr[0], csr[1], z_old, z_new, K, delta, int(blocks))
        return delta
    n, cap = inv.numel(), delta.shape[0]
    if not LDA_MIN_K <= K <= LDA_MAX_K or delta.dim() != 2 or delta.shape[1] != W or z_new.numel() != n or \
            (z_old is not None and z_old.numel() != n):
        raise RuntimeError(f"lda_delta: K {K}, delta {tuple(delta.shape)} (expected [cap, {W}]), z_new "
                           f"[{z_new.numel()}] for {n} tokens")
    if n == 0 or cap == 0:
        return delta
    ok = (inv >= 0) & (inv < cap)
    acc = torch.zeros(cap * W, dtype=torch.int64)
    for zz, sign in ((z_new, 1), (z_old, -1)):
        if zz is None:
            continue
        zz = zz.long()
        m = ok & (zz >= 0) & (zz < K)
        acc.index_add_(0, inv[m] * W + zz[m], torch.full((1,), sign, dtype=torch.int64).expand(int(m.sum())))
    touched = torch.zeros(cap, dtype=torch.bool)
    touched[inv[ok]] = True
    delta[touched] = acc.view(cap, W)[touched].float()
    return delta


def lda_loglik(rowptr, inv, z, rows, nk, alpha, beta, Vbeta, acc, blocks=0):
    """ADDS the batch's fixed-point log likelihood into acc int64 [2] (csrc/kernels/lda.h): per live token, in
    fp64, l = log(sum_k ((ndk[k] + alpha) / (L + K alpha)) * ((rows[inv][k] + beta) / (nk[k] + Vbeta))) with the
    document's own counts ndk and length L; acc[0] += sum llrint(-l 2^24), acc[1] += tokens. The GPU and this
    reference may differ by one unit per token (the order of the fp64 sum, ``log``)."""
    B, n, K = rowptr.numel() - 1, inv.numel(), nk.numel()
    alpha, beta, Vbeta = float(alpha), float(beta), float(Vbeta)
    if _gpu(rows):
        ldak().lda_loglik(rowptr, inv, z, rows, nk, alpha, beta, Vbeta, acc, int(blocks))
        return acc
    _lda_check("lda_loglik", K, alpha, beta, Vbeta, rows, blocks)
    if z.numel() != n or acc.numel() != 2 or acc.dtype != torch.int64:
        raise RuntimeError(f"lda_loglik: z [{z.numel()}] for {n} tokens, acc {acc.dtype} [{acc.numel()}]")
    cap = rows.shape[0]
    _, _, doc, _, t = _lda_tokens(rowptr, n)
    zl = z.long()
    live = ((inv >= 0) & (inv < cap) & (zl >= 0) & (zl < K))[t]
    doc, t = doc[live], t[live]
    ndk = torch.zeros(B, K, dtype=torch.int64)
    ndk.view(-1).index_add_(0, doc * K + zl[t], torch.ones(1, dtype=torch.int64).expand(t.numel()))
    theta = (ndk.double() + alpha) / (ndk.sum(1).double() + K * alpha)[:, None]
    den = nk.double() + Vbeta
    step = max(1, (1 << 22) // K)
    for s in range(0, t.numel(), step):
        phi = (rows[inv[t[s:s + step]], :K].double() + beta) / den
        p = (theta[doc[s:s + step]] * phi).sum(1)
        acc[0] += torch.round(-torch.log(p) * LDA_LOGLIK_SCALE).to(torch.int64).sum()
    acc[1] += t.numel()
    return acc


# ----------------------------------------------------------------------------- word2vec: skip-gram, negative sampling
SGNS_MIN_DIM, SGNS_MAX_DIM, SGNS_MAX_NEG = 4, 512, 64  # csrc/kernels/sgns.h (the binding exports them too)
SGNS_MAX_TOKENS = 1 << 40
SGNS_Q_SCALE = float(1 << 20)
_SGNS_ROWS = 1 << 13  # pairs per pass of the CPU references


def _sgns_check(op, d, N, rows, blocks=0):
    if d % 4 or not SGNS_MIN_DIM <= d <= SGNS_MAX_DIM:
        raise RuntimeError(f"{op}: rows are {d} wide, expected d % 4 == 0 and {SGNS_MIN_DIM} <= d <= {SGNS_MAX_DIM}")
    if not 1 <= N <= SGNS_MAX_NEG:
        raise RuntimeError(f"{op}: N is {N}, expected 1 <= N <= {SGNS_MAX_NEG}")
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise RuntimeError(f"{op}: rows must be fp32 [cap, d], got {rows.dtype} {tuple(rows.shape)}")
    if not 0 <= blocks <= 65535:
        raise RuntimeError(f"{op}: blocks is {blocks}, expected 0 <= blocks <= 65535")


def sgns_alias(counts):
    """The integer alias table of word2vec's negative sampler (the rule: csrc/kernels/sgns.h), built on the host
    with Python integers in a fixed order from the int64 word counts [V]: q_w = c_w > 0 ? max(1, rint(c_w^0.75
    2^20)) : 0 in fp64, T = sum q_w, Vose's method over V buckets of capacity T with the masses q_w V. Returns
    (thr int64 [V], alias int32 [V], T, q): thr[w] + sum_{i: alias[i] == w} (T - thr[i]) == q_w V exactly."""
    c = counts.detach().to("cpu", torch.int64).reshape(-1)
    V = c.numel()
    if V < 1 or V >= 1 << 31 or bool((c < 0).any()):
        raise ValueError(f"w2v: {V} word counts, expected 1 <= V < 2^31 and no negative count")
    if int(c.sum()) >= SGNS_MAX_TOKENS:
        raise ValueError(f"w2v: the counts hold {int(c.sum())} tokens, expected fewer than 2^40")
    qt = torch.where(c > 0, torch.round(c.double().pow(0.75) * SGNS_Q_SCALE).clamp_(min=1.0),
                     torch.zeros((), dtype=torch.float64))
    q = [int(v) for v in qt.to(torch.int64).tolist()]
    T = sum(q)
    if T < 1:
        raise ValueError("w2v: every word count is 0: there is nothing to draw negatives from")
    m = [v * V for v in q]
    thr, alias = [T] * V, list(range(V))
    small = [w for w in range(V) if m[w] < T]
    large = [w for w in range(V) if m[w] >= T]
    while small and large:
        s, big = small.pop(), large[-1]
        thr[s], alias[s] = m[s], big
        m[big] -= T - m[s]
        if m[big] < T:
            large.pop()
            small.append(big)
    assert not small and all(m[w] == T for w in large)  # integers: what is left fills its bucket exactly
    return torch.tensor(thr, dtype=torch.int64), torch.tensor(alias, dtype=torch.int32), T, q


def sgns_keep(counts, sample: float) -> torch.Tensor:
    """word2vec's subsampling as integers: int64 [V] holding uint32 thresholds kt; a token of word w with the
    32-bit draw x is kept iff x <= kt[w]. kt = min(2^32 - 1, floor(p 2^32)) with p = min(1, (sqrt(f / s) + 1) s / f)
    in fp64, f = c_w / sum c; ``sample`` 0 (and a word of count 0) keeps everything."""
    c = counts.detach().to("cpu", torch.int64).reshape(-1).double()
    full = float((1 << 32) - 1)
    if not sample > 0:
        return torch.full((c.numel(),), (1 << 32) - 1, dtype=torch.int64)
    f = c / c.sum().clamp(min=1.0)
    p = torch.where(f > 0, (torch.sqrt(f / sample) + 1.0) * sample / f.clamp(min=1e-300), torch.ones_like(f))
    return torch.floor(p.clamp(max=1.0) * float(1 << 32)).clamp_(max=full).to(torch.int64)


def sgns_lookups(centres, contexts, thr, alias, T, seed, epoch, pair_base, N, negatives=None):
    """The int64 key matrix [P, N + 2] of P skip-gram pairs (csrc/kernels/sgns.h): column 0 is 2 c (the centre's
    input row), column 1 is 2 o + 1 (the context's output row), column 2 + t is 2 neg + 1, where neg is draw t of the
    global pair pair_base + p in ``epoch`` from the alias table (thr int64 [V] holding uint64 bits, alias int32 [V],
    T), or negatives[p, t] when the explicit int32 [P, N] ``negatives`` are given. A word outside [0, V) gives the
    key -1. One launch on the GPU; the CPU path is the same integer arithmetic on int64 tensors."""
    N, T, P, V = int(N), int(T), centres.numel(), thr.numel()
    if _gpu(centres):
        keys = torch.empty(P, N + 2, dtype=torch.int64, device=centres.device)
        w2vk().sgns_lookups(centres, contexts, thr, alias, T, int(seed), int(epoch), int(pair_base), N, negatives, keys)
        return keys
    if not 1 <= N <= SGNS_MAX_NEG or not 1 <= V < 1 << 31 or alias.numel() != V or contexts.numel() != P or \
            not 1 <= T < 1 << 59 or epoch < 0 or pair_base < 0:
        raise RuntimeError(f"sgns_lookups: N {N}, V {V}, alias [{alias.numel()}], contexts [{contexts.numel()}] for "
                           f"{P} centres, T {T}, epoch {epoch}, pair_base {pair_base}")
    if negatives is None:
        base = lda_mix_int(int(seed) + int(epoch) * _LDA_GOLD)
        g = torch.arange(P, dtype=torch.int64) + int(pair_base)
        r = _lda_mix((g[:, None] * 64 + torch.arange(N, dtype=torch.int64)[None, :]) ^ _lda_s64(base))
        i = mulhi_u64(r, torch.full_like(r, V))
        x = mulhi_u64(_lda_mix(r), torch.full_like(r, T))
        neg = torch.where(x < thr[i], i, alias[i].long())
    else:
        if tuple(negatives.shape) != (P, N):
            raise RuntimeError(f"sgns_lookups: negatives {tuple(negatives.shape)}, expected [{P}, {N}]")
        neg = negatives.long()
    words = torch.cat([centres.long().reshape(P, 1), contexts.long().reshape(P, 1), neg], 1)
    odd = torch.ones(N + 2, dtype=torch.int64)
    odd[0] = 0
    return torch.where((words >= 0) & (words < V), 2 * words + odd, torch.full_like(words, -1))


def _sgns_head(s, first, gscale):
    """member_rows.h's logistic head on fp32 tensors: (e, loss) of the logits s against y = ``first``."""
    ex = torch.exp(-s.abs())
    big, small = 1.0 / (1.0 + ex), ex / (1.0 + ex)
    sg, one_m = torch.where(s >= 0, big, small), torch.where(s >= 0, small, big)
    e = torch.where(first, -one_m, sg) * torch.tensor(float(gscale), dtype=torch.float32)
    loss = s.clamp(min=0) - torch.where(first, s, torch.zeros_like(s)) + torch.log1p(ex)
    return e, loss


def sgns_forward(inv, rows, N, gscale=1.0, blocks=0):
    """Skip-gram with negative sampling over pulled rows (the rule: csrc/kernels/sgns.h). inv int64 [P (N + 2)] are a
    plan's row indices of sgns_lookups' keys, rows fp32 [cap, d]. Pair p has the centre row a = inv[p (N + 2)] and
    the targets t = 0 .. N with rows b_t = inv[p (N + 2) + 1 + t], y_t = [t == 0]; a target t >= 1 with b_t == b_0 is
    masked, a row index outside [0, cap) makes its target (or, for the centre, the whole pair) not exist. Returns
    fp32 (e [P, N + 1], loss [P], h [P, d]): s_t = <rows[a], rows[b_t]>, e_t = (sigmoid(s_t) - y_t) gscale (exactly 0
    when masked), loss = the sum of the live targets' logistic losses, h = sum_t e_t rows[b_t]. One fused gfx950
    launch on the GPU (no atomics, the same bits for every grid size, ``blocks``); the CPU path is the fp32
    PyTorch reference of the same rule."""
    N = int(N)
    K2 = N + 2
    P, d = inv.numel() // K2, rows.shape[1] if rows.dim() == 2 else 0
    if _gpu(rows):
        dev = rows.device
        e = torch.empty(P, N + 1, dtype=torch.float32, device=dev)
        loss = torch.empty(P, dtype=torch.float32, device=dev)
        h = torch.empty(P, d, dtype=torch.float32, device=dev)
        w2vk().sgns_forward(inv, rows, N, float(gscale), e, loss, h, int(blocks))
        return e, loss, h
    _sgns_check("sgns_forward", d, N, rows, blocks)
    if inv.numel() != P * K2:
        raise RuntimeError(f"sgns_forward: inv holds {inv.numel()} lookups, not a multiple of N + 2 = {K2}")
    cap = rows.shape[0]
    e = torch.zeros(P, N + 1, dtype=torch.float32)
    loss = torch.zeros(P, dtype=torch.float32)
    h = torch.zeros(P, d, dtype=torch.float32)
    if P == 0 or cap == 0:
        return e, loss, h
    iv = inv.view(P, K2)
    first = torch.zeros(1, N + 1, dtype=torch.bool)
    first[0, 0] = True
    for lo in range(0, P, _SGNS_ROWS):
        a, b = iv[lo:lo + _SGNS_ROWS, 0], iv[lo:lo + _SGNS_ROWS, 1:]
        ok = ((a >= 0) & (a < cap))[:, None] & (b >= 0) & (b < cap)
        ok[:, 1:] &= b[:, 1:] != b[:, :1]
        va, u = rows[a.clamp(0, cap - 1)], rows[b.clamp(0, cap - 1)]
        ee, ll = _sgns_head((va[:, None, :] * u).sum(-1), first, gscale)
        ee = torch.where(ok, ee, torch.zeros_like(ee))
        e[lo:lo + _SGNS_ROWS] = ee
        loss[lo:lo + _SGNS_ROWS] = torch.where(ok, ll, torch.zeros_like(ll)).sum(1)
        h[lo:lo + _SGNS_ROWS] = (ee[:, :, None] * u).sum(1)
    return e, loss, h


def sgns_backward(inv, e, h, rows, N, grad_rows, csr=None, blocks=0):
    """Gradient of every unique pulled row of sgns_forward's batch (csrc/kernels/sgns.h): over the lookups j of row
    r (inv[j] == r), p = j // (N + 2), col = j % (N + 2), grad_rows[r] = sum of h[p] (col == 0) or e[p, col - 1] *
    rows[inv[p (N + 2)]] (col >= 1); rows without lookups are left untouched. ``csr`` = (members, memrow): the
    lookups grouped by unique row (a plan's lookup CSR; built from ``inv`` here when absent on the GPU, ignored on
    the CPU). On the GPU every such row is written exactly once in a fixed summation order -- no atomics, the same
    bits on every run and for every grid size (``blocks``); the CPU reference sums with index_add_ over ``inv``."""
    N = int(N)
    K2 = N + 2
    if _gpu(rows):
        if csr is None:  # (not the model's path) rows outside [0, cap) go to a row past the end, which the kernel
            cap = rows.shape[0]  # ignores: emb_build_csr trusts its rows
            ok = (inv >= 0) & (inv < cap)
            csr = emb_build_csr(torch.where(ok, inv, torch.full_like(inv, cap)), 1, cap + 1)
        w2vk().sgns_backward(csr[0], csr[1], inv, e, h, rows, N, grad_rows, int(blocks))
        return grad_rows
    P, d = h.shape[0], h.shape[1]
    _sgns_check("sgns_backward", d, N, rows, blocks)
    cap = rows.shape[0]
    if inv.numel() != P * K2 or tuple(e.shape) != (P, N + 1) or rows.shape[1] < d or grad_rows.dim() != 2 or \
            grad_rows.shape[1] != d or grad_rows.shape[0] < cap:
        raise RuntimeError(f"sgns_backward: inv [{inv.numel()}], e {tuple(e.shape)}, h {tuple(h.shape)}, rows "
                           f"{tuple(rows.shape)}, grad_rows {tuple(grad_rows.shape)} for {P} pairs of {K2} lookups")
    if P == 0 or cap == 0:
        return grad_rows
    iv = inv.view(P, K2)
    acc = torch.zeros(cap, d, dtype=torch.float32)
    for lo in range(0, P, _SGNS_ROWS):
        a, b = iv[lo:lo + _SGNS_ROWS, 0], iv[lo:lo + _SGNS_ROWS, 1:]
        cen = (a >= 0) & (a < cap)
        acc.index_add_(0, a[cen], h[lo:lo + _SGNS_ROWS][cen])
        ok = cen[:, None] & (b >= 0) & (b < cap)
        va = rows[a.clamp(0, cap - 1)][:, :d]
        acc.index_add_(0, b[ok], (e[lo:lo + _SGNS_ROWS][:, :, None] * va[:, None, :])[ok])
    touched = torch.zeros(cap, dtype=torch.bool)
    touched[inv[(inv >= 0) & (inv < cap)]] = True
    grad_rows[:cap][touched] = acc[touched]
    return grad_rows


# ----------------------------------------------------------------------------- optimizers
def _slab_args(slabs):
    return [(s, int(n), int(p), int(o)) for s, n, p, o in slabs]


def _fold_slabs(g, slabs, group4=True):
    """g + its split-K planes ((slab, nsplit, plane, offset) each), an exact fp32 model of the kernels' fold
    (slab_fold in csrc/kernels/dense_update.h); ``g`` itself when there are none. ``group4``: the order of what
    an Adam consumes (adam_apply, adam_clip_apply, grad_sumsq) -- groups of four planes as (a0+a1)+(a2+a3),
    then the remainder one by one. Otherwise plane by plane, the order of what is shipped (slab_pack, the
    one-sided dense push). The two round differently from 4 planes on."""
    if not slabs:
        return g
    x = g.clone()
    for s, n, p, o in slabs:
        P, r = s[: n * p].view(n, p), x[o: o + p]
        z = 0
        while group4 and z + 3 < n:
            r += (P[z] + P[z + 1]) + (P[z + 2] + P[z + 3])
            z += 4
        while z < n:
            r += P[z]
            z += 1
    return x


def adam_apply(w, m, v, g, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, grad_scale=1.0,
               w_bf16=None, step_dev=None, zero_g=False, slabs=()):
    """Fused Adam(W). ``step_dev`` (int32 [1] device tensor): the bias-correction step is read on the
    device, so a captured (HIP graph) clock stays correct on replay. ``zero_g``: the kernel also
    clears ``g`` after reading it (the gradient accumulator of the next clock; no fill kernel).
    ``slabs``: (slab, nsplit, plane, offset) split-K gradient planes folded into g[offset:offset+plane]."""
    if _gpu(w):
        kernels().adam_apply(w, m, v, g, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                             int(step), float(grad_scale), w_bf16, step_dev, bool(zero_g), _slab_args(slabs))
        return
    g_in, g = g, _fold_slabs(g, slabs)
    if step_dev is not None:
        step = int(step_dev.reshape(-1)[0])
    gg = g * grad_scale
    m.mul_(beta1).add_((1 - beta1) * gg)
    v.mul_(beta2).add_((1 - beta2) * gg * gg)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    w.sub_(lr * ((m / bc1) / ((v / bc2).sqrt() + eps) + weight_decay * w))
    if w_bf16 is not None:
        w_bf16.copy_(w.to(torch.bfloat16))
    if zero_g:
        g_in.zero_()


# ----------------------------------------------------------------------------- global-norm clipping
def grad_sumsq(g, part, L=None, slabs=()):
    """part[0:L] (fp64) = partial sums of squares of the fp32 gradient ``g`` (+ ``slabs``, as adam_apply's),
    squared and accumulated in fp64: their sum is the squared l2 norm, non-finite exactly when an element is.
    GPU: workgroup b of L writes part[b] -- no atomics, a function of the data and L only (g.numel() % 4 == 0,
    16-byte aligned, 1 <= L <= 1024). CPU: the whole sum lands in part[0]."""
    L = part.numel() if L is None else int(L)
    if _gpu(g):
        optk().grad_sumsq(g, _slab_args(slabs), part, L)
        return part
    if not 1 <= L <= 1024 or part.numel() < L or part.dtype != torch.float64:
        raise RuntimeError(f"grad_sumsq: part must be float64 with 1 <= L <= 1024 entries, got {part.dtype} "
                           f"[{part.numel()}], L {L}")
    part[:L] = 0
    part[0] = _fold_slabs(g, slabs).double().square().sum()
    return part


def clip_scale(total: float, max_norm: float):
    """The rule's host form: (norm, scale, skip) of a squared norm ``total``. scale is torch's
    clip_grad_norm_ coefficient max_norm / (norm + 1e-6), rounded to fp32 below 1, else exactly 1."""
    if not math.isfinite(total):
        return math.sqrt(total) if total > 0 else float("nan"), 0.0, True
    norm = math.sqrt(total)
    sd = max_norm / (norm + 1e-6)
    return norm, (float(torch.tensor(sd, dtype=torch.float32)) if sd < 1.0 else 1.0), False


def adam_clip_apply(w, m, v, g, lr, part, max_norm, stats, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                    step=1, np=None, w_bf16=None, step_dev=None, zero_g=False, slabs=(), write_stats=True):
    """adam_apply with the gradient clipped to the global l2 norm ``max_norm``. total = sum(part[0:np]) (the
    grad_sumsq partials of the WHOLE gradient, every bucket and rank; np <= 4096) is folded on the device in
    one fixed order; scale = clip_scale(total); the update is adam_apply's with grad_scale = scale. A
    non-finite total skips the clock: w, m, v and w_bf16 stay bit for bit, ``g`` is still cleared on
    ``zero_g``. ``stats`` (fp64 [4]: norm, scale, n_clipped, n_skipped; scale 0 on a skip) is updated when
    ``write_stats``. No host sync on the GPU."""
    np = part.numel() if np is None else int(np)
    if _gpu(w):
        optk().adam_clip_apply(w, m, v, g, _slab_args(slabs), float(lr), float(beta1), float(beta2), float(eps),
                               float(weight_decay), int(step), step_dev, w_bf16, bool(zero_g), part, np,
                               float(max_norm), stats, bool(write_stats))
        return
    if not 1 <= np <= 4096 or part.numel() < np:
        raise RuntimeError(f"adam_clip_apply: np {np} outside [1, 4096] or beyond part [{part.numel()}]")
    norm, scale, skip = clip_scale(float(part[:np].sum()), float(max_norm))
    if write_stats:
        stats[0], stats[1] = norm, scale
        stats[3 if skip else 2] += 1.0 if skip or scale < 1.0 else 0.0
    if not skip:
        adam_apply(w, m, v, _fold_slabs(g, slabs), lr, beta1, beta2, eps, weight_decay, step, scale, w_bf16,
                   step_dev=step_dev)
    if zero_g:
        g.zero_()


def slab_pack(g, out, slabs=()):
    """out = g + the split-K planes ``slabs`` ((slab, nsplit, plane, offset), as adam_apply) folded
    into their regions; g cleared -- a several-rank dense clock's reduce-scatter input in one pass."""
    if _gpu(g):
        kernels().slab_pack(g, out, _slab_args(slabs))
        return out
    out.copy_(_fold_slabs(g, slabs, group4=False))
    g.zero_()
    return out


def sgd_apply(w, g, lr, grad_scale=1.0, w_bf16=None):
    if _gpu(w):
        kernels().sgd_apply(w, g, float(lr), float(grad_scale), w_bf16)
        return
    w.sub_(lr * grad_scale * g)
    if w_bf16 is not None:
        w_bf16.copy_(w.to(torch.bfloat16))


def adagrad_apply(w, acc, g, lr, eps=1e-10, grad_scale=1.0, w_bf16=None):
    if _gpu(w):
        kernels().adagrad_apply(w, acc, g, float(lr), float(eps), float(grad_scale), w_bf16)
        return
    gg = g * grad_scale
    acc.add_(gg * gg)
    w.sub_(lr * gg / (acc.sqrt() + eps))
    if w_bf16 is not None:
        w_bf16.copy_(w.to(torch.bfloat16))


def cast_f32_bf16(x, y):
    if _gpu(x):
        kernels().cast_f32_bf16(x, y)
        return y
    y.copy_(x.to(torch.bfloat16))
    return y


# ----------------------------------------------------------------------------- LR / K-Means
def lr_sparse_step(rowptr, cols, vals, labels, w, alpha, delta=None, correct=None):
    """Sparse LR gradient (lr_example.cpp:291-312): delta[col] += alpha*x*(y - sigmoid(w.x))."""
    if _gpu(w):
        kernels().lr_sparse_step(rowptr, cols, vals, labels, w, float(alpha), delta, correct)
        return
    B = labels.numel()
    lens = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(B, device=w.device), lens)
    dot = torch.zeros(B, dtype=w.dtype, device=w.device).index_add_(0, row, w[cols] * vals)
    p = torch.sigmoid(dot)
    y = labels.clamp_min(0)
    err = alpha * (y - p)
    if delta is not None:
        delta.index_add_(0, cols, err[row] * vals)
    if correct is not None:
        correct += ((p > 0.5) == (y > 0.5)).float().sum()


def kmeans_assign_csr(rowptr, cols, vals, C, assign=None, dist=None):
    """Nearest centre of every sparse point (CSR rowptr [n+1], cols / vals [nnz]) among the dense
    centres C [k, d] fp32 (kmeans_helper.hpp:45-66); optional squared distances. int32 assign."""
    n = rowptr.numel() - 1
    if assign is None:
        assign = torch.empty(n, dtype=torch.int32, device=C.device)
    if _gpu(C):
        cnorm = torch.empty(C.shape[0], dtype=torch.float32, device=C.device)
        kernels().kmeans_assign_csr(rowptr, cols, vals, C, cnorm, assign, dist)
        return assign
    lens = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n, device=C.device), lens)
    ok = cols < C.shape[1]
    xn = torch.zeros(n, dtype=torch.float32).index_add_(0, row, vals * vals)
    dots = torch.zeros(n, C.shape[0], dtype=torch.float32)
    dots.index_add_(0, row[ok], vals[ok, None] * C[:, cols[ok]].t())
    d2 = xn[:, None] - 2 * dots + (C * C).sum(1)[None]
    best, idx = d2.min(1)
    assign.copy_(idx.to(torch.int32))
    if dist is not None:
        dist.copy_(best.clamp_min(0))
    return assign


def kmeans_csr_accum(rowptr, cols, vals, assign, sums):
    """sums[assign[i], col] += val for every non-zero of every point."""
    if _gpu(sums):
        kernels().kmeans_csr_accum(rowptr, cols, vals, assign, sums)
        return sums
    n = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=sums.device), rowptr[1:] - rowptr[:-1])
    ok = cols < sums.shape[1]
    sums.index_put_((assign.to(torch.int64)[row[ok]], cols[ok]), vals[ok], accumulate=True)
    return sums


_KMEANS_CHUNK = 16384  # rows of S = X.C^T per GEMM (keeps the fp32 score block L2/MALL-sized)


def kmeans_assign(X, C, assign=None, dist=None, mfma=None):
    """Nearest centre of every row of X (fp32 [n, d]) among C (fp32 [k, d]); optional squared
    distance. GPU: the MFMA form (hi/lo-split bf16 GEMM for x.c, argmin kernel) unless the
    problem is tiny (or mfma=False: the one-wave-per-point fp32 kernel)."""
    if assign is None:
        assign = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    if _gpu(X):
        n, d = X.shape
        k = C.shape[0]
        if mfma is None:
            mfma = n * k >= 1 << 16 and k >= 16
        if not mfma:
            kernels().kmeans_assign(X, C, assign, dist)
            return assign
        ld = (3 * d + 7) // 8 * 8
        Xc, Cc = X.contiguous(), C.contiguous()
        Cs = torch.empty(k, ld, dtype=torch.bfloat16, device=X.device)
        cn = torch.empty(k, dtype=torch.float32, device=X.device)
        kernels().kmeans_split3(Cc, Cs, 1, cn)
        xn = torch.empty(n, dtype=torch.float32, device=X.device)
        for r0 in range(0, n, _KMEANS_CHUNK):
            r1 = min(n, r0 + _KMEANS_CHUNK)
            Xs = torch.empty(r1 - r0, ld, dtype=torch.bfloat16, device=X.device)
            kernels().kmeans_split3(Xc[r0:r1], Xs, 0, xn[r0:r1])
            S = torch.empty(r1 - r0, k, dtype=torch.float32, device=X.device)
            gemm(Xs, Cs, S, r1 - r0, k, ld, False, False, EPI_STORE_F32)
            kernels().kmeans_argmin(S, cn, xn[r0:r1], assign[r0:r1], None if dist is None else dist[r0:r1])
        return assign
    d = torch.cdist(X.double(), C.double()) ** 2
    best, idx = d.min(1)
    assign.copy_(idx.to(torch.int32))
    if dist is not None:
        dist.copy_(best.to(dist.dtype))
    return assign


# ----------------------------------------------------------------------------- dense models
def layernorm_fwd(x, C, gamma, beta, eps, y, mean, rstd):
    if _gpu(x):
        kernels().layernorm_fwd(x, int(C), gamma, beta, float(eps), y, mean, rstd)
        return y
    xf = x[:, :C].float()
    mu = xf.mean(1)
    xc = xf - mu[:, None]
    # two passes, as the kernel: E[x^2] - mean^2 cancels in fp32 once |mean| >> std
    rs = torch.rsqrt((xc * xc).mean(1) + eps)
    y[:, :C] = (xc * rs[:, None] * gamma.float() + beta.float()).to(torch.bfloat16)
    mean.copy_(mu)
    rstd.copy_(rs)
    return y


def layernorm_bwd(x, dy, C, gamma, mean, rstd, dx, dgamma, dbeta, accumulate=False):
    if _gpu(x):
        kernels().layernorm_bwd(x, dy, int(C), gamma, mean, rstd, dx, dgamma, dbeta, bool(accumulate))
        return dx
    xh = (x[:, :C].float() - mean[:, None]) * rstd[:, None]
    d = dy[:, :C].float()
    g = d * gamma.float()
    a = g.mean(1, keepdim=True)
    b = (g * xh).mean(1, keepdim=True)
    v = rstd[:, None] * (g - a - xh * b)
    if accumulate:
        v = v + dx[:, :C].float()
    dx[:, :C] = v.to(torch.bfloat16)
    dgamma += (d * xh).sum(0)
    dbeta += d.sum(0)
    return dx


def softmax_xent(logits, V, labels, scale, loss_sum, correct=None):
    """In place: logits[:, :V] <- (softmax - onehot) * scale (bf16); loss_sum += sum CE."""
    if _gpu(logits):
        kernels().softmax_xent(logits, int(V), labels, float(scale), loss_sum, correct)
        return logits
    z = logits[:, :V].float()
    lse = torch.logsumexp(z, 1)
    loss_sum += (lse - z.gather(1, labels[:, None]).squeeze(1)).sum()
    if correct is not None:
        correct += (z.argmax(1) == labels).float().sum()
    p = torch.softmax(z, 1)
    p[torch.arange(z.shape[0]), labels] -= 1.0
    logits[:, :V] = (p * scale).to(torch.bfloat16)
    return logits


def causal_softmax_fwd(S, T, P):
    if _gpu(S):
        kernels().causal_softmax_fwd(S, int(T), P)
        return P
    s = S.reshape(-1, T, T).float()
    mask = torch.ones(T, T, dtype=torch.bool).triu(1)
    P.view(-1, T, T).copy_(torch.softmax(s.masked_fill(mask, float("-inf")), -1).to(P.dtype))
    return P


def causal_softmax_bwd(P, dP, T, scale, dS):
    if _gpu(P):
        kernels().causal_softmax_bwd(P, dP, int(T), float(scale), dS)
        return dS
    p = P.reshape(-1, T, T).float()
    dp = dP.reshape(-1, T, T).float()
    mask = torch.ones(T, T, dtype=torch.bool).triu(1)
    dp = dp.masked_fill(mask, 0.0)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    dS.view(-1, T, T).copy_(ds.to(dS.dtype))
    return dS


def gelu_bwd(dh, u, du):
    if _gpu(u):
        kernels().gelu_bwd(dh, u, du)
        return du
    du.copy_((dh.float() * _gelu_grad(u.float())).to(du.dtype))
    return du


def add_bf16(a, b, out):
    if _gpu(a):
        kernels().add_bf16(a, b, out)
        return out
    out.copy_((a.float() + b.float()).to(out.dtype))
    return out


def _attn_heads(x, B, T, H, col0):
    hd = 64
    return x[:, col0: col0 + H * hd].float().reshape(B, T, H, hd).transpose(1, 2)


def attn_fwd(qkv, B, T, H, scale, O, lse):
    """Fused causal attention (head dim 64): O[:, h*64:] = softmax(mask(Q K^T scale)) V per head,
    lse [B*H*T] = log2-sum-exp2 of the scaled scores (log2 units, for the backward)."""
    if _gpu(qkv):
        kernels().attn_fwd(qkv, int(B), int(T), int(H), float(scale), O, lse)
        return O
    d = H * 64
    q, k, v = (_attn_heads(qkv, B, T, H, c) for c in (0, d, 2 * d))
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    lse.view(B, H, T).copy_(torch.logsumexp(s, -1) * (1.0 / math.log(2.0)))
    o = torch.softmax(s, -1) @ v
    O[:, :d] = o.transpose(1, 2).reshape(B * T, d).to(O.dtype)
    return O


def attn_bwd(qkv, O, dO, lse, delta, B, T, H, scale, dqkv):
    """Backward of attn_fwd: writes dQ|dK|dV into dqkv [B*T, 3*H*64]; delta is [B*H*T] scratch."""
    if _gpu(qkv):
        kernels().attn_bwd(qkv, O, dO, lse, delta, int(B), int(T), int(H), float(scale), dqkv)
        return dqkv
    d = H * 64
    q, k, v = (_attn_heads(qkv, B, T, H, c) for c in (0, d, 2 * d))
    o = _attn_heads(O, B, T, H, 0)
    do = _attn_heads(dO, B, T, H, 0)
    s = (q @ k.transpose(-1, -2)) * scale
    mask = torch.ones(T, T, dtype=torch.bool, device=s.device).triu(1)
    p = torch.exp2(s * (1.0 / math.log(2.0)) - lse.view(B, H, T, 1)).masked_fill(mask, 0.0)
    dl = (do * o).sum(-1, keepdim=True)
    delta.view(B, H, T).copy_(dl.squeeze(-1))
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - dl)
    dq = ds @ k * scale
    dk = ds.transpose(-1, -2) @ q * scale
    for i, t in enumerate((dq, dk, dv)):
        dqkv[:, i * d: (i + 1) * d] = t.transpose(1, 2).reshape(B * T, d).to(dqkv.dtype)
    return dqkv


_U64 = (1 << 64) - 1


def _mix64_int(x: int) -> int:
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _U64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _U64
    x ^= x >> 33
    return x


def hash_slots(tab_keys, q, slots, vals, init_scale, seed, counters, n_dev=None):
    """Lookup-or-insert of q in the open-addressing table (EMPTY = -1), linear probing from
    mix64(key); new rows are zero or uniform[-a, a) from mix64(key*golden + seed + c). With
    ``n_dev`` (device int64 count) only q[:n_dev] is resolved; the rest get slot -1."""
    if _gpu(q):
        kernels().hash_slots(tab_keys, q, slots, vals, float(init_scale), int(seed), counters, n_dev)
        return slots
    if n_dev is not None:
        n = int(n_dev.reshape(-1)[0])
        slots[n:] = -1
        q, slots = q[:n], slots[:n]
    cap = tab_keys.numel()
    W = vals.shape[1]
    tk = tab_keys.tolist()
    out = []
    for k in q.tolist():
        s = _mix64_int(k & _U64) & (cap - 1)
        found = -1
        for _ in range(cap):
            if tk[s] == k:
                found = s
                break
            if tk[s] == -1:
                tk[s] = k
                tab_keys[s] = k
                if init_scale != 0.0:
                    row = []
                    for c in range(W):
                        h = _mix64_int(((k & _U64) * 0x9E3779B97F4A7C15 + seed + c) & _U64)
                        row.append(init_scale * (2.0 * float(h >> 40) / 16777216.0 - 1.0))
                    vals[s] = torch.tensor(row, dtype=vals.dtype)
                else:
                    vals[s] = 0
                counters[0] += 1
                found = s
                break
            s = (s + 1) & (cap - 1)
        if found < 0:
            counters[1] += 1
        out.append(found)
    slots[: len(out)] = torch.tensor(out, dtype=torch.int64)
    return slots


def hash_rehash(old_keys, old_vals, old_state, new_keys, new_vals, new_state, counters):
    if _gpu(old_keys):
        kernels().hash_rehash(old_keys, old_vals, old_state, new_keys, new_vals, new_state, counters)
        return
    occ = (old_keys != -1).nonzero().reshape(-1)
    slots = torch.empty(occ.numel(), dtype=torch.int64)
    hash_slots(new_keys, old_keys[occ], slots, new_vals, 0.0, 0, counters)
    new_vals[slots] = old_vals[occ]
    if old_state is not None:
        new_state[slots] = old_state[occ]


def embed_fwd(wte, wpe, tok, T, out):
    """out[m, :C] = wte[tok[m]] + wpe[m % T] (bf16)."""
    if _gpu(wte):
        kernels().embed_fwd(wte, wpe, tok.reshape(-1), int(T), out)
        return out
    t = tok.reshape(-1)
    C = wte.shape[1]
    pos = torch.arange(t.numel()) % T
    out[:, :C] = (wte[t].float() + wpe[pos].float()).to(out.dtype)
    return out


def embed_bwd(dx, tok, T, dwte, dwpe):
    """dwte[tok[m]] += dx[m, :C]; dwpe[m % T] += dx[m, :C] (fp32 accumulators)."""
    if _gpu(dx):
        kernels().embed_bwd(dx, tok.reshape(-1), int(T), dwte, dwpe)
        return
    t = tok.reshape(-1)
    C = dwte.shape[1]
    d = dx[:, :C].float()
    dwte.index_add_(0, t, d)
    dwpe.index_add_(0, torch.arange(t.numel()) % T, d)


def dlrm_interact_fwd(V, NV, D, out, dense_idx=0):
    """V [B, NV, D] bf16 -> out[b] = [V[b,dense_idx] | V_i . V_j for i > j (lower triangle, row-major)]."""
    if _gpu(V):
        kernels().dlrm_interact_fwd(V, int(NV), int(D), int(dense_idx), out)
        return out
    v = V.reshape(-1, NV, D).float()
    z = v @ v.transpose(1, 2)
    ii, jj = torch.tril_indices(NV, NV, -1)
    out[:, :D] = V.reshape(-1, NV, D)[:, dense_idx]
    out[:, D: D + ii.numel()] = z[:, ii, jj].to(out.dtype)
    return out


def dlrm_interact_bwd(V, NV, D, dout, dV, d_dense, dense_idx=0):
    """dV fp32 [B, NV*D]; d_dense bf16 [B, D] = dV[:, dense_idx] * (V[:, dense_idx] > 0)."""
    if _gpu(V):
        kernels().dlrm_interact_bwd(V, int(NV), int(D), int(dense_idx), dout, dV, d_dense)
        return dV
    v = V.reshape(-1, NV, D).float()
    B = v.shape[0]
    ii, jj = torch.tril_indices(NV, NV, -1)
    dz = torch.zeros(B, NV, NV)
    g = dout[:, D: D + ii.numel()].float()
    dz[:, ii, jj] = g
    dz[:, jj, ii] = g
    d = dz @ v
    d[:, dense_idx] += dout[:, :D].float()
    dV.view(B, NV, D).copy_(d)
    d_dense.copy_(torch.where(v[:, dense_idx] > 0, d[:, dense_idx], torch.zeros_like(d[:,
                                                                                       dense_idx])).to(d_dense.dtype))
    return dV


def kaiming_uniform_(w: torch.Tensor, fan_in: int, gen=None):
    bound = 1.0 / math.sqrt(fan_in)
    return w.uniform_(-bound, bound, generator=gen)
