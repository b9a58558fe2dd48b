"""Shared pieces of the GEMM epilogue tests: an independent fp64 reference of every fused epilogue (it never
calls ops.gemm), round-to-nearest-even bf16 rounding, the two input regimes, the padded case layouts, and the
runner that drives one device / kernel variant through every (epilogue, layout, shape, C layout) cell.

Exact regime: small integer operands, so every product, partial sum and epilogue input is exactly representable
in fp32 and the result cannot depend on accumulation order, split-K, atomics or FMA contraction: the bf16 outputs
must be bit-equal to round_bf16(reference), the fp32 outputs equal to the reference.
GELU regime: integer operands with a power-of-two alpha, so the activation's input x is exact and only tanh /
the polynomial around it round: |out - ref| <= 2^-8 |ref| + 2^-18 (half a bf16 ulp, plus an assumed 5 fp32 ulp of
tanhf carried through 0.5 x (1 + t) and the derivative for |x| <= 16).
"""
import functools
import json
import math
import sys
import time

import torch

from minips_amd import ops as E  # the EPI_* codes (and, in the runner, the op under test)

GELU_K, GELU_C3 = 0.7978845608, 0.044715  # csrc/kernels/gemm_kernels.h
LAYOUTS = {"nt": (False, False), "nn": (False, True), "tn": (True, True), "tt": (True, False)}
# M, N, K (KN layouts round N down to a multiple of 8): a tile that is almost all tail with one partial K
# stage; second 256 tile in M and N, N tail inside an 8-column lane group, K tail in the second 64-stage;
# second 128 tile, double-buffer wrap over 4 stages; v1's BK = 64 path with a fully vector-aligned N
SHAPES = [(8, 8, 8), (264, 331, 72), (136, 203, 200), (264, 328, 264)]
EXACT_EPIS = [E.EPI_STORE_F32, E.EPI_ATOMIC_F32, E.EPI_BIAS_RELU_BF16, E.EPI_BIAS_BF16, E.EPI_STORE_BF16,
              E.EPI_RELU_MASK_BF16, E.EPI_MUL_AUX_BF16, E.EPI_PERM_ROWS_BF16]
GELU_EPIS = [E.EPI_BIAS_GELU_BF16, E.EPI_BIAS_GELU_AUX_BF16, E.EPI_BIAS_GELU_DAUX_BF16, E.EPI_GELU_GRAD_BF16]
F32_EPIS = (E.EPI_STORE_F32, E.EPI_ATOMIC_F32)
BIAS_EPIS = (E.EPI_BIAS_RELU_BF16, E.EPI_BIAS_BF16, E.EPI_BIAS_GELU_BF16, E.EPI_BIAS_GELU_AUX_BF16,
             E.EPI_BIAS_GELU_DAUX_BF16)
READ_MASK_EPIS = (E.EPI_RELU_MASK_BF16, E.EPI_MUL_AUX_BF16, E.EPI_GELU_GRAD_BF16)
WRITE_AUX_EPIS = (E.EPI_BIAS_GELU_AUX_BF16, E.EPI_BIAS_GELU_DAUX_BF16)
EPI_NAMES = {getattr(E, n): n[4:] for n in dir(E) if n.startswith("EPI_")}
GELU_RTOL, GELU_ATOL = 2.0 ** -8, 2.0 ** -18
GUARD = 8  # NaN guard rows before and after every matrix (8 rows keep any leading dimension 16-byte aligned)
NAN = float("nan")


# ----------------------------------------------------------------------------- reference
def gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(GELU_K * (x + GELU_C3 * x ** 3)))


def gelu_grad64(x):
    t = torch.tanh(GELU_K * (x + GELU_C3 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_K * (1.0 + 3.0 * GELU_C3 * x * x)


def _f32_bits(x64):
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "round_bf16 / is_tie take values that are exact in fp32"
    return x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def round_bf16(x64):
    """Round-to-nearest-even to bf16, on the fp32 bit pattern (x64 must be exact in fp32: the exact regime)."""
    u = _f32_bits(x64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return r.view(torch.float32).to(torch.bfloat16)  # the low 16 bits are zero: this conversion is exact


def is_tie(x64):
    """Exactly halfway between two bf16 values (where truncation, round-half-up and RNE all differ)."""
    return (_f32_bits(x64) & 0xFFFF) == 0x8000


def ref(epi, A, B, M, N, K, a_km, b_kn, alpha=1.0, bias=None, mask=None, C0=None, perm=None, seg=0):
    """fp64 acc = alpha (A . B) of the stored operands and the epilogue's real-valued results: ``c`` (for
    EPI_PERM_ROWS_BF16 in logical [M, N] order; ``dest`` holds the destination row of every segment), ``aux``
    for the *_AUX / *_DAUX forms, ``colsum`` (the increment: column sums of the bf16-rounded output) for the
    relu mask."""
    a = (A[:K, :M].t() if a_km else A[:M, :K]).double()
    b = (B[:K, :N] if b_kn else B[:N, :K].t()).double()
    acc = alpha * (a @ b) + 0.0  # (+ 0.0: an all-cancelling sum is +0, as in an accumulator that starts at +0)
    out = {"acc": acc, "c": None, "aux": None, "colsum": None, "dest": None}
    x = acc + bias[:N].double() if (epi in BIAS_EPIS and bias is not None) else acc
    m = mask[:M, :N].double() if mask is not None else None
    if epi in (E.EPI_STORE_F32, E.EPI_STORE_BF16, E.EPI_BIAS_BF16):
        out["c"] = x
    elif epi == E.EPI_ATOMIC_F32:
        out["c"] = C0[:M, :N].double() + acc
    elif epi == E.EPI_BIAS_RELU_BF16:
        out["c"] = torch.clamp(x, min=0.0)
    elif epi == E.EPI_RELU_MASK_BF16:
        out["c"] = torch.where(m > 0, acc, torch.zeros_like(acc))
        out["colsum"] = round_bf16(out["c"]).double().sum(0)
    elif epi == E.EPI_MUL_AUX_BF16:
        out["c"] = acc * m
    elif epi == E.EPI_PERM_ROWS_BF16:
        out["c"] = acc
        out["dest"] = perm[: M * (N // seg)].long().view(M, N // seg)
    elif epi == E.EPI_BIAS_GELU_BF16:
        out["c"] = gelu64(x)
    elif epi == E.EPI_BIAS_GELU_AUX_BF16:
        out["c"], out["aux"] = gelu64(x), x
    elif epi == E.EPI_BIAS_GELU_DAUX_BF16:
        out["c"], out["aux"] = gelu64(x), gelu_grad64(x)
    elif epi == E.EPI_GELU_GRAD_BF16:
        out["c"] = acc * gelu_grad64(m)
    else:
        raise ValueError(f"no reference for epilogue {epi}")
    return out


# ----------------------------------------------------------------------------- inputs
def _seed(layout, M, N, K, salt):
    return (sorted(LAYOUTS).index(layout) * 1000003 + M * 10007 + N * 101 + K) * 16 + salt


def _int_operands(M, N, K, lim, gen, boost):
    """Logical A [M, K] and B [K, N] of integers in [-lim, lim]. ``boost`` is the share of elements that take a
    large magnitude and a sign coherent along k (sign_i * sign_k): below K ~ 128 uniform draws never reach
    |acc| >= 256, where integer sums start to fall on bf16 ties."""
    A = torch.randint(-lim, lim + 1, (M, K), generator=gen).double()
    B = torch.randint(-lim, lim + 1, (K, N), generator=gen).double()
    if boost > 0:
        sk = torch.randint(0, 2, (K,), generator=gen).double() * 2 - 1
        for X, rows in ((A, M), (B.t(), N)):  # (B.t() is a view: the assignment below writes B)
            sr = torch.randint(0, 2, (rows,), generator=gen).double() * 2 - 1
            big = torch.randint(lim - lim // 2 + 1, lim + 1, (rows, K), generator=gen).double() * sr[:, None] * sk
            pick = torch.rand(rows, K, generator=gen) < boost
            X[pick] = big[pick]
    return A, B


def _boost(K):
    return min(1.0, math.sqrt(7.2 / K)) if K < 128 else 0.0


def n_of(layout, N):
    return N // 8 * 8 if LAYOUTS[layout][1] else N


@functools.lru_cache(maxsize=None)
def exact_case(layout, M, N, K):
    """The exact regime's inputs (CPU, logical orientation, fp64 holding small integers) and the references of
    every non-GELU epilogue; shared by every test and variant, never modified."""
    assert K <= 264 and M <= 264
    a_km, b_kn = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(_seed(layout, M, N, K, 0))
    A, B = _int_operands(M, N, K, 8, gen, _boost(K))
    d = {"M": M, "N": N, "K": K, "layout": layout, "regime": "exact"}
    d["alpha"] = 0.5 if (K in (72, 264)) != a_km else 1.0  # every layout and epilogue meets both values
    d["A"], d["B"] = (A.t() if a_km else A).contiguous(), (B if b_kn else B.t()).contiguous()  # stored layout
    d["bias"] = torch.randint(-64, 65, (N,), generator=gen).double()
    r = torch.rand(M, N, generator=gen)
    pos = torch.randint(1, 3, (M, N), generator=gen).double()
    # relu mask: 70 % positive, 10 % negative, 10 % +0.0, 10 % -0.0
    d["mask"] = {E.EPI_RELU_MASK_BF16: torch.where(r < 0.7, pos, torch.where(r < 0.8, -pos, torch.where(
        r < 0.9, torch.zeros_like(pos), -torch.zeros_like(pos)))),
        E.EPI_MUL_AUX_BF16: torch.randint(-2, 3, (M, N), generator=gen).double()}
    d["C0"] = torch.randint(-1024, 1025, (M, N), generator=gen).double()
    d["colsum0"] = torch.randint(1, 100, (N,), generator=gen).double()
    d["perm"], d["ref"] = {}, {}
    for seg in (8, 40):
        if N % 8 == 0 and N >= seg:  # N rounded down to a multiple of seg (328 -> 320 at seg = 40)
            Np = N // seg * seg
            rows = M * (Np // seg)
            d["perm"][seg] = (Np, rows + 16, torch.randperm(rows + 16, generator=gen)[:rows].to(torch.int32))
    sign = d["mask"][E.EPI_RELU_MASK_BF16]
    assert bool((sign == 0).any()) and bool(torch.signbit(sign[sign == 0]).any()) and \
        bool((~torch.signbit(sign[sign == 0])).any()) and bool((sign > 0).any())
    for epi in EXACT_EPIS:
        if epi == E.EPI_PERM_ROWS_BF16:
            continue
        o = ref(epi, d["A"], d["B"], M, N, K, a_km, b_kn, d["alpha"], d["bias"], d["mask"].get(epi), d["C0"])
        d["ref"][epi] = o
        # every quantity exact in fp32: below 2^23 (all are multiples of 1/2), the colsum included
        assert float(o["acc"].abs().max()) + 64 < 2 ** 23 and float(o["c"].abs().max()) < 2 ** 23
        if epi not in F32_EPIS:
            ties = float(is_tie(o["c"]).double().mean())
            assert ties >= 0.05, (layout, M, N, K, EPI_NAMES[epi], "bf16 ties", ties)
        if epi in (E.EPI_BIAS_RELU_BF16, E.EPI_RELU_MASK_BF16):
            zeros = float((o["c"] == 0).double().mean())
            assert 0.2 <= zeros <= 0.8, (layout, M, N, K, EPI_NAMES[epi], "zero share", zeros)
        if o["colsum"] is not None:
            assert float(round_bf16(o["c"]).double().abs().sum(0).max() + d["colsum0"].max()) < 2 ** 23
    return d


@functools.lru_cache(maxsize=None)
def gelu_case(layout, M, N, K):
    """The GELU regime: integers in [-4, 4], a power-of-two alpha that puts x = alpha acc + bias at a standard
    deviation near 3 (2^-5 at K = 200), integer bias in [-2, 2]; GELU_GRAD reads a bf16 u on the same grid."""
    a_km, b_kn = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(_seed(layout, M, N, K, 1))
    A, B = _int_operands(M, N, K, 4, gen, 0.0)
    d = {"M": M, "N": N, "K": K, "layout": layout, "regime": "gelu"}
    d["alpha"] = 2.0 ** -math.ceil(math.log2(math.sqrt(K * (20.0 / 3.0) ** 2) / 3.0))
    d["A"], d["B"] = (A.t() if a_km else A).contiguous(), (B if b_kn else B.t()).contiguous()
    d["bias"] = torch.randint(-2, 3, (N,), generator=gen).double()
    u = torch.clamp(torch.round(torch.randn(M, N, generator=gen) * 3.0 * 32) / 32, -16, 16)
    d["mask"] = {E.EPI_GELU_GRAD_BF16: u.to(torch.bfloat16).double()}
    d["ref"] = {}
    for epi in GELU_EPIS:
        o = ref(epi, d["A"], d["B"], M, N, K, a_km, b_kn, d["alpha"], d["bias"], d["mask"].get(epi))
        d["ref"][epi] = o
        x = d["mask"][epi] if epi == E.EPI_GELU_GRAD_BF16 else o["acc"] + d["bias"]
        assert torch.equal(x.float().double(), x) and torch.equal(o["acc"].float().double(), o["acc"])
        inside = float((x.abs() <= 6).double().mean())
        assert inside >= 0.9 and float(x.abs().max()) <= 16, (layout, M, N, K, EPI_NAMES[epi], inside, x.abs().max())
    return d


@functools.lru_cache(maxsize=None)
def gauss_case(layout, M, N, K):
    """bf16 gaussian operands (stored layout) with the fp64 product and the elementwise |A| . |B|."""
    a_km, b_kn = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(_seed(layout, M, N, K, 2))
    A = torch.randn(K if a_km else M, M if a_km else K, generator=gen).to(torch.bfloat16).double()
    B = torch.randn(K if b_kn else N, N if b_kn else K, generator=gen).to(torch.bfloat16).double()
    o = ref(E.EPI_STORE_F32, A, B, M, N, K, a_km, b_kn)
    mag = ref(E.EPI_STORE_F32, A.abs(), B.abs(), M, N, K, a_km, b_kn)["acc"]
    return {"A": A, "B": B, "ref": o["c"], "mag": mag}


# ----------------------------------------------------------------------------- case layouts
def padded(mat, rows, cols, ld, dtype, dev):
    """A [GUARD + rows + GUARD, ld] buffer of NaN holding ``mat`` (or nothing) at [GUARD:, :cols]; returns the
    buffer and the [rows, cols] view the op gets (its base stays 16-byte aligned for any ld)."""
    buf = torch.full((GUARD + rows + GUARD, ld), NAN, dtype=dtype)
    if mat is not None:
        buf[GUARD:GUARD + rows, :cols] = mat.to(dtype)
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + rows, :cols]


def ld_of(cols, variant):
    """variant 0: a multiple of 8 above cols (vector body, scalar tail when cols % 8); 1: odd (all scalar)."""
    return (cols // 8 + 1) * 8 if variant == 0 else cols + 1 + cols % 2


def _vec(vals, n, variant, dtype, dev):
    """A length-n vector inside a NaN store: 16-byte aligned (variant 0) or store[1 : 1 + n]."""
    store = torch.full((n + 16,), NAN, dtype=dtype)
    off = 0 if variant == 0 else 1
    store[off:off + n] = vals.to(dtype)
    store = store.to(dev)
    return store, store[off:off + n]


_OPERANDS = {}


def operands(d, dev):
    """The case's A and B on ``dev`` in NaN-padded buffers with lda / ldb a multiple of 8 above the extent."""
    key = (d["regime"], d["layout"], d["M"], d["N"], d["K"], str(dev))
    if key not in _OPERANDS:
        out = []
        for X in (d["A"], d["B"]):
            r, c = X.shape
            out.append(padded(X, r, c, (c // 8 + 1) * 8 + 8, torch.bfloat16, dev))
        _OPERANDS[key] = out
    return _OPERANDS[key][0][1], _OPERANDS[key][1][1]


def _inside(rows, cols, ld):
    m = torch.zeros(GUARD + rows + GUARD, ld, dtype=torch.bool)
    m[GUARD:GUARD + rows, :cols] = True
    return m


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_matrix(what, buf, rows, cols, expect=None, ref64=None, rel_ref=None, stats=None):
    """``buf`` (CPU copy of a padded buffer) against bit-exact ``expect`` [rows, cols] or, in the GELU regime,
    against ``ref64`` within the bound; every padding element must still be NaN and nothing inside may be."""
    fails = []
    ins = _inside(rows, cols, buf.shape[1])
    nan = torch.isnan(buf)
    if not bool(nan[~ins].all()):
        fails.append(f"{what}: {int((~nan[~ins]).sum())} padding elements overwritten")
    got = buf[GUARD:GUARD + rows, :cols]
    if bool(torch.isnan(got).any()):
        fails.append(f"{what}: {int(torch.isnan(got).sum())} NaN inside [M, N]")
    elif expect is not None:
        bad = _bits(got) != _bits(expect)
        if bool(bad.any()):
            i, j = [int(v) for v in bad.nonzero()[0]]
            fails.append(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at ({i}, {j}): "
                         f"{float(got[i, j])!r} vs {float(expect[i, j])!r}")
    else:
        err = (got.double() - ref64).abs()
        bound = GELU_RTOL * (ref64 if rel_ref is None else rel_ref).abs() + GELU_ATOL
        ratio = float((err / bound).max())
        if stats is not None:
            stats["gelu_worst_err_over_bound"] = max(stats.get("gelu_worst_err_over_bound", 0.0), ratio)
        if ratio > 1.0:
            i, j = [int(v) for v in (err / bound == (err / bound).max()).nonzero()[0]]
            fails.append(f"{what}: error {float(err[i, j]):.3e} over bound {float(bound[i, j]):.3e} at ({i}, {j}), "
                         f"ref {float(ref64[i, j])!r}")
    return fails


def run_cell(ops, dev, d, epi, variant, tile=0, split_k=1, seg=0, ldc=None, stats=None):
    """One GEMM of case ``d`` with epilogue ``epi`` in C / mask / bias / colsum layout ``variant``; returns the
    list of failed checks (empty: the cell passed)."""
    M, N, K, layout = d["M"], d["N"], d["K"], d["layout"]
    a_km, b_kn = LAYOUTS[layout]
    A, B = operands(d, dev)
    name = f"{EPI_NAMES[epi]} {layout} {M}x{N}x{K} v{variant} tile={tile} split={split_k}"
    name += f" seg={seg}" if seg else ""
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + 1
    if epi == E.EPI_PERM_ROWS_BF16:
        Np, rows, perm = d["perm"][seg]
        Bp = B[:, :Np] if b_kn else B[:Np]
        Cbuf = torch.full((rows, seg), NAN, dtype=torch.bfloat16).to(dev)
        ops.gemm(A, Bp, Cbuf, M, Np, K, a_km, b_kn, epi, alpha=d["alpha"], perm=perm.to(dev), seg=seg, tile=tile)
        o = ref(epi, d["A"], d["B"][:, :Np] if b_kn else d["B"][:Np], M, Np, K, a_km, b_kn, d["alpha"], perm=perm,
                seg=seg)
        want = torch.full((rows, seg), NAN, dtype=torch.bfloat16)
        want[o["dest"].reshape(-1)] = round_bf16(o["c"]).reshape(-1, seg)
        bad = _bits(Cbuf.cpu()) != _bits(want)  # destination rows bit-exact, every other row still NaN
        return [f"{name}: {int(bad.sum())} of {bad.numel()} elements differ"] if bool(bad.any()) else []
    o = d["ref"][epi]
    f32 = epi in F32_EPIS
    dt = torch.float32 if f32 else torch.bfloat16
    ldc = ld_of(N, variant) if ldc is None else ldc
    Cbuf, C = padded(d["C0"] if epi == E.EPI_ATOMIC_F32 else None, M, N, ldc, dt, dev)
    kw = {}
    ldm = ld_of(N, variant)
    if epi in READ_MASK_EPIS or epi in WRITE_AUX_EPIS:
        Mbuf, kw["mask"] = padded(d["mask"][epi] if epi in READ_MASK_EPIS else None, M, N, ldm, torch.bfloat16, dev)
    if epi in BIAS_EPIS:
        _, kw["bias"] = _vec(d["bias"], N, variant, torch.bfloat16, dev)
    if epi == E.EPI_RELU_MASK_BF16:
        if variant == 0:
            csbuf, kw["colsum"] = _vec(d["colsum0"], N, 0, torch.float32, dev)
        else:  # a column of an [N, 5] matrix
            csbuf = torch.full((N, 5), NAN)
            csbuf[:, 2] = d["colsum0"].float()
            csbuf = csbuf.to(dev)
            kw["colsum"] = csbuf[:, 2]
    ops.gemm(A, B, C, M, N, K, a_km, b_kn, epi, alpha=d["alpha"], split_k=split_k, tile=tile, **kw)
    got = Cbuf.cpu()
    exact = d["regime"] == "exact"
    expect = (o["c"].float() if f32 else round_bf16(o["c"])) if exact else None
    fails = check_matrix(f"{name} C", got, M, N, expect=expect, ref64=o["c"], stats=stats)
    if epi in WRITE_AUX_EPIS:
        fails += check_matrix(f"{name} aux", Mbuf.cpu(), M, N, ref64=o["aux"], stats=stats)
    if epi in READ_MASK_EPIS:  # an input: unchanged, padding included
        before = padded(d["mask"][epi], M, N, ldm, torch.bfloat16, "cpu")[0]
        if not torch.equal(_bits(Mbuf.cpu()), _bits(before)):
            fails.append(f"{name}: the mask / aux input was written")
    if epi == E.EPI_RELU_MASK_BF16:
        cs = csbuf.cpu()
        val = cs[:N] if variant == 0 else cs[:, 2]
        # against the device's own C (pinned above): integers (or halves) below 2^23, so any order is exact
        want = d["colsum0"] + got[GUARD:GUARD + M, :N].double().sum(0)
        if not torch.equal(val.double(), want):
            bad = val.double() != want
            j = int(bad.nonzero()[0])
            fails.append(f"{name} colsum: {int(bad.sum())} of {N} columns differ, first {j}: {float(val[j])} vs "
                         f"{float(want[j])}")
        rest = cs[N:] if variant == 0 else cs[:, [0, 1, 3, 4]]
        if not bool(torch.isnan(rest).all()):
            fails.append(f"{name} colsum: neighbouring elements overwritten")
    return fails


# ----------------------------------------------------------------------------- the cases beyond the grid
def run_splitk(ops, dev, tile=0, stats=None):
    """Split-K in the exact regime: the in-kernel atomic epilogue (N % 4 != 0), the fp32 slab reduce and the bf16
    slab reduce, each into a padded C (ldc = 336 for N = 328)."""
    fails = []
    d = exact_case("nt", 264, 331, 200)
    for variant in (0, 1):
        fails += run_cell(ops, dev, d, E.EPI_ATOMIC_F32, variant, tile, split_k=3, stats=stats)
    for layout in ("nt", "tn"):
        fails += run_cell(ops, dev, exact_case(layout, 264, 328, 200), E.EPI_ATOMIC_F32, 0, tile, split_k=3,
                          ldc=336, stats=stats)
    fails += run_cell(ops, dev, exact_case("nn", 264, 328, 200), E.EPI_STORE_BF16, 0, tile, split_k=3, ldc=336,
                      stats=stats)
    return fails


def run_batched(ops, dev, tile=0, stats=None):
    """2 outer x 3 inner GEMMs of 136 x 72 x 40 with a bias, the inner index interleaved inside the rows, a padded
    ldc, and an outer C stride that leaves the second outer block only 8-byte aligned (its scalar store path)."""
    outer, inner, M, N, K = 2, 3, 136, 72, 40
    lda = ldb = inner * 48
    ldc = inner * 80
    st = [M * lda + 16, 48, N * ldb + 8, 48, M * ldc + 4, 80]
    gen = torch.Generator().manual_seed(77)
    bias = torch.randint(-64, 65, (N,), generator=gen).double()
    Af = torch.full((outer * st[0] + 8,), NAN, dtype=torch.bfloat16)
    Bf = torch.full((outer * st[2] + 8,), NAN, dtype=torch.bfloat16)
    want = torch.full((outer * st[4] + 8,), NAN, dtype=torch.bfloat16)
    ties = []
    for z in range(outer * inner):
        zo, zi = divmod(z, inner)
        A, B = _int_operands(M, N, K, 8, gen, _boost(K))
        Af[zo * st[0] + zi * st[1]:].as_strided((M, K), (lda, 1)).copy_(A)
        Bf[zo * st[2] + zi * st[3]:].as_strided((N, K), (ldb, 1)).copy_(B.t())
        c = ref(E.EPI_BIAS_BF16, A, B.t().contiguous(), M, N, K, False, False, 0.5, bias)["c"]
        ties.append(float(is_tie(c).double().mean()))
        want[zo * st[4] + zi * st[5]:].as_strided((M, N), (ldc, 1)).copy_(round_bf16(c))
    assert min(ties) >= 0.05, ties
    Cf = torch.full_like(want, NAN).to(dev)
    ops.gemm_batched(Af.to(dev), Bf.to(dev), Cf, M, N, K, False, False, E.EPI_BIAS_BF16, outer * inner, inner, lda,
                     ldb, ldc, st, alpha=0.5, bias=bias.to(torch.bfloat16).to(dev), tile=tile)
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + 1
    bad = _bits(Cf.cpu()) != _bits(want)
    return [f"batched BIAS_BF16 tile={tile}: {int(bad.sum())} of {bad.numel()} elements differ (padding "
            f"included)"] if bool(bad.any()) else []


def run_gauss(ops, dev, layout, tile=0, stats=None):
    """Gaussian bf16 data, fp32 store: |C - ref| <= K 2^-23 (|A| . |B|) elementwise, the fp32 accumulation bound
    (a reduced-precision accumulate passes the integer data and fails here)."""
    M, N, K = 264, 328, 264
    a_km, b_kn = LAYOUTS[layout]
    g = gauss_case(layout, M, N, K)
    bufs = [padded(X, X.shape[0], X.shape[1], (X.shape[1] // 8 + 1) * 8 + 8, torch.bfloat16, dev)
            for X in (g["A"], g["B"])]
    Cbuf, C = padded(None, M, N, ld_of(N, 0), torch.float32, dev)
    ops.gemm(bufs[0][1], bufs[1][1], C, M, N, K, a_km, b_kn, E.EPI_STORE_F32, tile=tile)
    got = Cbuf.cpu()[GUARD:GUARD + M, :N].double()
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + 1
    if bool(torch.isnan(got).any()):
        return [f"gauss {layout} tile={tile}: NaN in C"]
    ratio = float(((got - g["ref"]).abs() / (K * 2.0 ** -23 * g["mag"])).max())
    if stats is not None:
        stats["gauss_worst_err_over_bound"] = max(stats.get("gauss_worst_err_over_bound", 0.0), ratio)
    return [f"gauss {layout} tile={tile}: error {ratio:.3f} x the fp32 accumulation bound"] if ratio > 1.0 else []


def run_grid(ops, dev, layout, shape, tile=0, stats=None):
    """Every epilogue x both C / mask / bias / colsum variants at one (layout, shape)."""
    M, N, K = shape
    N = n_of(layout, N)
    fails = []
    de, dg = exact_case(layout, M, N, K), gelu_case(layout, M, N, K)
    for variant in (0, 1):
        for epi in EXACT_EPIS:
            if epi != E.EPI_PERM_ROWS_BF16:
                fails += run_cell(ops, dev, de, epi, variant, tile, stats=stats)
        for epi in GELU_EPIS:
            fails += run_cell(ops, dev, dg, epi, variant, tile, stats=stats)
    # the permuted rows need N % seg == 0: the case's own N for the KN layouts, else N rounded down to 8
    dp = de if N % 8 == 0 else exact_case(layout, M, N // 8 * 8, K)
    for seg in sorted(dp["perm"]):
        fails += run_cell(ops, dev, dp, E.EPI_PERM_ROWS_BF16, 0, tile, seg=seg, stats=stats)
    return fails


def run_variant(ops, dev, tile=0):
    """Everything one kernel variant has to pass; returns (failures, stats)."""
    stats = {}
    t0 = time.time()
    fails = []
    for layout in LAYOUTS:
        for shape in SHAPES:
            fails += run_grid(ops, dev, layout, shape, tile, stats)
        fails += run_gauss(ops, dev, layout, tile, stats)
    fails += run_splitk(ops, dev, tile, stats)
    fails += run_batched(ops, dev, tile, stats)
    stats["seconds"] = round(time.time() - t0, 2)
    return fails, stats


def child_main():
    """The body of a fresh process that runs one variant on cuda:0 (the forced-kernel knob is read once per
    process): prints one JSON line {"fails": [...], "stats": {...}} and exits 1 if anything failed."""
    from minips_amd import _native, ops

    _native.kernels()
    fails, stats = run_variant(ops, torch.device("cuda", 0), 0)
    print(json.dumps({"fails": fails[:40], "nfails": len(fails), "stats": stats}))
    sys.exit(1 if fails else 0)
