"""Shared pieces of the GPT-2 kernel tests (fused causal attention, LayerNorm, token + position embedding): plain
float64 CPU references that never call the op under test, the magnitude every error is judged against, the input
regimes, and the runners that drive one device (the HIP kernels, or the CPU path of minips_amd.ops) through a case.
The dense counterpart of tests/_gemm_ref.py.

Error model. Every reference returns the exact result and its MAGNITUDE: the same expression with absolute values
inside the sums. A structural mistake (a wrong mask, a dropped tile, a swapped index) makes an error of the order of
the magnitude; rounding makes one of a few bf16 units of it, so a bound between the two is not met by accident.
Every output element is checked, component-wise, with u = 2^-8 (the bf16 unit roundoff).

Attention (all from the same bf16 inputs; P the fp64 probabilities, scale > 0):
  O    |O - O64|   <= 4u (P |V|)
  dV   |dV - dV64| <= 4u (P^T |dO|)
  dQ   |dQ - dQ64| <= 4u scale (D |K|)       D = P o (|dP| + |delta|), dP = dO V^T, delta = sum_d dO O
  dK   |dK - dK64| <= 4u scale (D^T |Q|)
  lse  (log2 units) <= 2^-20 max(1, |lse|) + T 2^-23
4u = one bf16 rounding of P (or dS) as the MFMA operand + one bf16 rounding of the output, times a margin of 2 for
the fp32 accumulation order and the hardware exp2. D bounds |dS| from above without the cancellation of dP - delta:
in peaked rows that difference cancels in fp32, and a bound on |dS| itself is several times too tight for a correct
kernel. Underflow (the term the derivation above leaves out; the CPU path needs it as the kernels do): under a
spike a probability is e^-100 and a whole output element can lie below the normal range of fp32 and bf16, where P,
a product or the stored value may flush to zero. Every such flush is an absolute error of at most eta = 2^-126 times
the weight of the term, so each bound gains eta (1 + sum over the visible terms of (1 + weight)): the magnitude with
P replaced by 1 and |V| (or |dO|, |K|, |Q|, |dP| + |delta|) by 1 + itself. At 1e-35 it cannot hide a mistake in a
value that does not underflow. The lse bound is its fp32 storage, the fp32 sum of at most T terms, and log2f. The
backward reference takes the O (bf16) and the lse (fp32) it is given, as the kernel does, so the backward is judged
alone.

LayerNorm (C columns, M rows, xh = (x - mean) rstd, g = dy gamma):
  mean   <= (C + 16) 2^-24 mean|x|           rstd   relative <= (C + 16) 2^-23
  y      <= 3u (|xh gamma| + |beta|)
  dx     <= 3u (rstd (|g| + |mean g| + |xh mean(g xh)|) + |prev|)       (|prev| only with accumulate)
  dgamma <= (M + 16) 2^-23 (sum_rows |dy xh| + |dgamma0|)   dbeta <= (M + 16) 2^-23 (sum_rows |dy| + |dbeta0|)
The backward reference uses the mean and rstd it is given, so the forward's error does not leak into it. With
integer dy (and an integer dbeta0) dbeta is an exact integer sum in any order and must be bit-exact: that pins the
row partition (no row dropped or counted twice), which the rounding bound alone could miss for one row in 33000.

Embedding: the forward is bit-exact against bf16(fp64 sum) on inputs whose exponents differ by less than 16 (the
fp32 sum is then exact: no double rounding); the backward is bit-exact on small-integer dx and within
(n + 16) 2^-23 sum|dx| per element on gaussian dx, n the number of contributing rows.
"""
import functools
import math

import torch

from _gemm_ref import round_bf16

U = 2.0 ** -8
ETA = 2.0 ** -126    # the smallest normal fp32 / bf16 number
HD = 64
L2E = 1.0 / math.log(2.0)
SENT = 77.0          # the sentinel of pad columns and of every output before the op runs (exact in bf16)
BF = torch.bfloat16
WORST = {}           # tensor name -> worst error / bound this process has seen (the GPU run reports it)

ATTN_T1 = (1, 16, 17, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 161, 255, 257)
ATTN_SHAPES = [(1, 1, T) for T in ATTN_T1] + [(2, 3, T) for T in (33, 129, 257)]
ATTN_REGIMES = ("flat", "peaked", "spike_early", "spike_late", "zero_q")
SCALE = 0.125
LN_SHAPES = [(1, 4), (7, 8), (64, 252), (300, 256), (300, 260), (504, 768), (505, 768), (520, 1024), (33000, 8)]
LN_RATIOS = (16, 64, 200)
LN_EPS = 1e-5
EMB_SHAPES = [(1, 1, 8, 3), (3, 5, 24, 7), (2, 64, 128, 500)]


# ----------------------------------------------------------------------------- bookkeeping
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == torch.float32
                               else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def worst_ratio(err, bound):
    """max err / bound over all elements (0 where the error is 0, inf where only the bound is, NaN if any is)."""
    if err.numel() == 0:
        return 0.0
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def judge(name, got, ref, bound, fails, what=""):
    """Component-wise |got - ref| <= bound; records the worst ratio under ``name`` and appends a failure line."""
    got = got.detach().cpu().double().reshape(ref.shape)
    r = worst_ratio((got - ref).abs(), bound)
    if name not in WORST or not r <= WORST[name]:
        WORST[name] = r
    if not r <= 1.0:
        fails.append(f"{what}{name}: error {r:.3g} x bound")
    return r


def judge_bits(name, got, want, fails, what=""):
    got = got.detach().cpu()
    if not same_bits(got, want):
        bad = _bits(got) != _bits(want) if got.shape == want.shape else None
        fails.append(f"{what}{name}: {'shape' if bad is None else int(bad.sum())} of {want.numel()} differ bitwise")


def padbuf(mat, rows, cols, ld, dtype, dev):
    """A [rows, ld] buffer of SENT holding ``mat`` (or SENT) in [:, :cols], on ``dev``."""
    buf = torch.full((rows, ld), SENT, dtype=dtype)
    if mat is not None:
        buf[:, :cols] = mat.to(dtype)
    return buf.to(dev)


def pads_intact(name, buf, cols, fails, what=""):
    pad = buf.detach().cpu()[:, cols:]
    if not same_bits(pad, torch.full_like(pad, SENT)):
        fails.append(f"{what}{name}: pad columns overwritten")


# ----------------------------------------------------------------------------- attention reference
def _heads(x, B, T, H, col0):
    return x[:, col0: col0 + H * HD].double().reshape(B, T, H, HD).transpose(1, 2)  # [B, H, T, 64]


def _rows(t, B, T, H):
    return t.transpose(1, 2).reshape(B * T, H * HD)


def _causal(T):
    return torch.ones(T, T, dtype=torch.bool).triu(1)  # True where key > query


def attn_fwd_ref(qkv, B, T, H, scale):
    """O [B*T, d], its magnitude P |V|, and lse [B*H*T] in log2 units, in fp64 from the bf16 qkv."""
    d = H * HD
    q, k, v = (_heads(qkv, B, T, H, c) for c in (0, d, 2 * d))
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(_causal(T), float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    seen = (~_causal(T)).double()
    return {"O": _rows(p @ v, B, T, H), "O_mag": _rows(p @ v.abs(), B, T, H), "lse": (lse * L2E).reshape(-1),
            "O_floor": ETA * (1 + _rows(seen @ (1 + v.abs()), B, T, H))}


def attn_bwd_ref(qkv, O, dO, lse, B, T, H, scale):
    """dqkv [B*T, 3d] = dQ | dK | dV and its magnitude, from the O (bf16) and lse (fp32, log2 units) given."""
    d = H * HD
    q, k, v = (_heads(qkv, B, T, H, c) for c in (0, d, 2 * d))
    o, do = _heads(O, B, T, H, 0), _heads(dO, B, T, H, 0)
    s2 = (q @ k.transpose(-1, -2)) * (scale * L2E)
    p = torch.exp2(s2 - lse.double().reshape(B, H, T, 1)).masked_fill(_causal(T), 0.0)
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - delta)
    w = dp.abs() + delta.abs()
    dmag = p * w
    out = [scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ do]
    mag = [scale * (dmag @ k.abs()), scale * (dmag.transpose(-1, -2) @ q.abs()), p.transpose(-1, -2) @ do.abs()]
    seen = (~_causal(T)).double()
    w1 = seen * (1 + w)
    floor = [w1 @ (1 + k.abs()), w1.transpose(-1, -2) @ (1 + q.abs()), seen.transpose(-1, -2) @ (1 + do.abs())]
    return {"dqkv": torch.cat([_rows(t, B, T, H) for t in out], 1),
            "mag": torch.cat([_rows(t, B, T, H) for t in mag], 1),
            "floor": ETA * (1 + torch.cat([_rows(t, B, T, H) for t in floor], 1))}


def lse_bound(lse, T):
    return 2.0 ** -20 * lse.abs().clamp_min(1.0) + T * 2.0 ** -23


def check_attn_fwd(ref, O, lse, T, fails, what=""):
    judge("O", O, ref["O"], 4 * U * ref["O_mag"] + ref["O_floor"], fails, what)
    judge("lse", lse, ref["lse"], lse_bound(ref["lse"], T), fails, what)


def check_attn_bwd(ref, dqkv, fails, what=""):
    d = ref["dqkv"].shape[1] // 3
    got = dqkv.detach().cpu().double()
    for i, name in enumerate(("dQ", "dK", "dV")):
        c = slice(i * d, (i + 1) * d)
        judge(name, got[:, c], ref["dqkv"][:, c], 4 * U * ref["mag"][:, c] + ref["floor"][:, c], fails, what)


# ----------------------------------------------------------------------------- attention cases
def _attn_seed(B, H, T, regime):
    return ((B * 7 + H) * 1000 + T) * 8 + ATTN_REGIMES.index(regime)


@functools.lru_cache(maxsize=None)
def attn_case(B, H, T, regime):
    """bf16 qkv [B*T, 3d] and dO [B*T, d] of one regime with the forward reference, the bf16 O and fp32 lse the
    backward is fed, and the backward reference from those; shared by every test, never modified.
      flat         unit gaussians: scores of std 1, a nearly flat softmax
      peaked       Q x 8: scores reach about +-30
      spike_early  key min(3, T-1) scores about +100 against every query: the running maximum is fixed in tile 0
      spike_late   the same at key T-1: the maximum jumps on the last tile and the rescale factor underflows to 0
      zero_q       some query rows exactly zero: lse = log2(q + 1), O = the running mean of V"""
    d = H * HD
    g = torch.Generator().manual_seed(_attn_seed(B, H, T, regime))
    qkv = torch.randn(B * T, 3 * d, generator=g)
    dO = torch.randn(B * T, d, generator=g).to(BF)
    c = {"B": B, "H": H, "T": T, "d": d, "regime": regime, "scale": SCALE}
    if regime == "peaked":
        qkv[:, :d] *= 8
    elif regime in ("spike_early", "spike_late"):
        key = min(3, T - 1) if regime == "spike_early" else T - 1
        qkv[:, 0:d:HD] = 8.0                                        # column 0 of every head's Q
        qkv.view(B, T, 3 * d)[:, key, d:2 * d:HD] = 100.0           # ... and of that key: 0.125 * 8 * 100
    elif regime == "zero_q":
        zero = sorted({0, T // 2, T - 1, min(T - 1, 31), min(T - 1, 64)})
        qkv.view(B, T, 3 * d)[:, zero, :d] = 0.0
        c["zero_rows"] = zero
    c["qkv"] = qkv = qkv.to(BF)
    c["dO"] = dO
    c["fwd"] = f = attn_fwd_ref(qkv, B, T, H, SCALE)
    if regime == "peaked":
        assert T < 64 or float(_scores(c).abs().max()) > 20
    elif regime.startswith("spike"):
        assert float(_scores(c).max()) > 80
    elif regime == "zero_q":  # the closed forms the zero rows must meet
        v = _heads(qkv, B, T, H, 2 * d)
        run = _rows(v.cumsum(2) / torch.arange(1, T + 1).double()[:, None], B, T, H).view(B, T, d)
        want = torch.log2(torch.arange(1, T + 1).double())
        for r in zero:
            assert float((f["lse"].view(B, H, T)[:, :, r] - want[r]).abs().max()) < 1e-12
            assert float((f["O"].view(B, T, d)[:, r] - run[:, r]).abs().max()) < 1e-12
    c["O_in"], c["lse_in"] = f["O"].to(BF), f["lse"].float()
    c["bwd"] = attn_bwd_ref(qkv, c["O_in"], dO, c["lse_in"], B, T, H, SCALE)
    return c


def _scores(c):
    q, k = (_heads(c["qkv"], c["B"], c["T"], c["H"], col) for col in (0, c["d"]))
    return ((q @ k.transpose(-1, -2)) * c["scale"]).masked_fill(_causal(c["T"]), 0.0)


def run_attn(ops, dev, c, padded, chained=False):
    """attn_fwd, then attn_bwd twice (fed the reference's O and lse, or with ``chained`` the forward's own
    outputs) on ``dev``, with default pitches or every pitch padded; returns the list of failed checks."""
    B, H, T, d, scale = c["B"], c["H"], c["T"], c["d"], c["scale"]
    what = f"attn B={B} H={H} T={T} {c['regime']}{' padded' if padded else ''}{' chained' if chained else ''}: "
    pq, po, pdo, pdq = (8, 8, 16, 8) if padded else (0, 0, 0, 0)
    fails = []
    qbuf = padbuf(c["qkv"], B * T, 3 * d, 3 * d + pq, BF, dev)
    q0 = qbuf.cpu()
    Obuf = padbuf(None, B * T, d, d + po, BF, dev)
    lse = torch.full((B * H * T,), SENT, device=dev)
    ops.attn_fwd(qbuf[:, :3 * d], B, T, H, scale, Obuf[:, :d], lse)
    check_attn_fwd(c["fwd"], Obuf[:, :d], lse, T, fails, what)
    pads_intact("O", Obuf, d, fails, what)
    if chained:
        O_in, lse_in = Obuf, lse
        bref = attn_bwd_ref(c["qkv"], Obuf[:, :d].cpu(), c["dO"], lse.cpu(), B, T, H, scale)
    else:
        O_in, lse_in = padbuf(c["O_in"], B * T, d, d + po, BF, dev), c["lse_in"].to(dev)
        bref = c["bwd"]
    O0, lse0 = O_in.cpu(), lse_in.cpu()
    dObuf = padbuf(c["dO"], B * T, d, d + pdo, BF, dev)
    dO0 = dObuf.cpu()
    outs = []
    for _ in range(2):
        dq = padbuf(None, B * T, 3 * d, 3 * d + pdq, BF, dev)
        delta = torch.full((B * H * T,), SENT, device=dev)
        ops.attn_bwd(qbuf[:, :3 * d], O_in[:, :d], dObuf[:, :d], lse_in, delta, B, T, H, scale, dq[:, :3 * d])
        outs.append(dq.cpu())
    check_attn_bwd(bref, outs[0][:, :3 * d], fails, what)
    pads_intact("dqkv", outs[0], 3 * d, fails, what)
    if not same_bits(outs[0], outs[1]):
        fails.append(what + "dqkv differs between two runs of the backward")
    for name, buf, before in (("qkv", qbuf, q0), ("O", O_in, O0), ("dO", dObuf, dO0), ("lse", lse_in, lse0)):
        if not same_bits(buf.cpu(), before):
            fails.append(what + f"the input {name} was written")
    return fails


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd_ref(x, gamma, beta, eps):
    x, gm, bt = x.double(), gamma.double(), beta.double()
    mean = x.mean(1)
    xc = x - mean[:, None]
    rstd = ((xc * xc).mean(1) + eps) ** -0.5
    xh = xc * rstd[:, None]
    return {"mean": mean, "rstd": rstd, "y": xh * gm + bt, "y_mag": (xh * gm).abs() + bt.abs(),
            "absmean": x.abs().mean(1)}


def ln_bwd_ref(x, dy, gamma, mean, rstd, prev, dg0, db0):
    """dx, dgamma, dbeta and their magnitudes from the mean / rstd (fp32) given; ``prev`` (the dx accumulated
    into) and dg0 / db0 (the initial parameter gradients) may be None."""
    x, dy, gm = x.double(), dy.double(), gamma.double()
    rs = rstd.double()[:, None]
    xh = (x - mean.double()[:, None]) * rs
    g = dy * gm
    a, b = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx, mag = rs * (g - a - xh * b), rs * (g.abs() + a.abs() + (xh * b).abs())
    if prev is not None:
        dx, mag = dx + prev.double(), mag + prev.double().abs()
    dg, dgm, db, dbm = (dy * xh).sum(0), (dy * xh).abs().sum(0), dy.sum(0), dy.abs().sum(0)
    if dg0 is not None:
        dg, dgm, db, dbm = dg + dg0.double(), dgm + dg0.double().abs(), db + db0.double(), dbm + db0.double().abs()
    return {"dx": dx, "dx_mag": mag, "dgamma": dg, "dgamma_mag": dgm, "dbeta": db, "dbeta_mag": dbm}


def check_ln_fwd(ref, C, y, mean, rstd, fails, what=""):
    judge("mean", mean, ref["mean"], (C + 16) * 2.0 ** -24 * ref["absmean"], fails, what)
    judge("rstd", rstd, ref["rstd"], (C + 16) * 2.0 ** -23 * ref["rstd"], fails, what)
    judge("y", y, ref["y"], 3 * U * ref["y_mag"], fails, what)


def check_ln_bwd(ref, M, dx, dgamma, dbeta, fails, what=""):
    judge("dx", dx, ref["dx"], 3 * U * ref["dx_mag"], fails, what)
    judge("dgamma", dgamma, ref["dgamma"], (M + 16) * 2.0 ** -23 * ref["dgamma_mag"], fails, what)
    judge("dbeta", dbeta, ref["dbeta"], (M + 16) * 2.0 ** -23 * ref["dbeta_mag"], fails, what)


def ln_rows(M, C, gen):
    """bf16 rows cycling through: 2 randn + 0.5; mean / std = 16, 64, 200 (as bf16 values, so the ratio of the
    stored row is what counts: it is returned); a constant row (variance 0, rstd = eps^-1/2)."""
    x = torch.randn(M, C, generator=gen)
    kind = torch.arange(M) % 5
    x[kind == 0] = x[kind == 0] * 2 + 0.5
    for i, ratio in enumerate(LN_RATIOS, 1):
        s = 0.37 * 2.0 ** i
        x[kind == i] = (x[kind == i] + ratio) * s
    x[kind == 4] = (torch.randn(M, 1, generator=gen) * 3).expand(M, C)[kind == 4]
    x = x.to(BF)
    xd = x.double()
    real = xd.mean(1).abs() / xd.std(1, unbiased=False)
    return x, kind, real


@functools.lru_cache(maxsize=None)
def ln_case(M, C, int_dy=False):
    g = torch.Generator().manual_seed(M * 2048 + C + (1 << 30) * int_dy)
    x, kind, real = ln_rows(M, C, g)
    c = {"M": M, "C": C, "x": x, "int_dy": int_dy}
    if C >= 252:  # (a handful of columns make no statistics)
        for i, ratio in enumerate(LN_RATIOS, 1):
            r = real[kind == i]
            assert r.numel() and 0.5 * ratio < float(r.min()) and float(r.max()) < 1.5 * ratio, (ratio, r)
    if M >= 5:
        assert float(x[kind == 4].double().std(1).max()) == 0.0
    c["gamma"], c["beta"] = torch.randn(C, generator=g).to(BF), torch.randn(C, generator=g).to(BF)
    if int_dy:
        c["dy"] = torch.randint(-3, 4, (M, C), generator=g).to(BF)
    else:
        c["dy"] = torch.randn(M, C, generator=g).to(BF)
    c["prev"] = (torch.randn(M, C, generator=g) * 2).to(BF)
    c["dg0"] = torch.randn(C, generator=g) * 3
    c["db0"] = torch.randint(-50, 51, (C,), generator=g).float()
    assert float(c["prev"].abs().mean()) > 0.5 and float(c["dg0"].abs().min()) > 0
    c["fwd"] = ln_fwd_ref(x, c["gamma"], c["beta"], LN_EPS)
    return c


def run_ln(ops, dev, c, accumulate):
    """layernorm_fwd and layernorm_bwd (fed the forward's own mean / rstd) at pitch C + 4."""
    M, C = c["M"], c["C"]
    what = f"layernorm M={M} C={C}{' int dy' if c['int_dy'] else ''}{' accumulate' if accumulate else ''}: "
    ld = C + 4
    fails = []
    xb, dyb = padbuf(c["x"], M, C, ld, BF, dev), padbuf(c["dy"], M, C, ld, BF, dev)
    gm, bt = c["gamma"].to(dev), c["beta"].to(dev)
    yb = padbuf(None, M, C, ld, BF, dev)
    mean, rstd = torch.full((M,), SENT, device=dev), torch.full((M,), SENT, device=dev)
    ops.layernorm_fwd(xb, C, gm, bt, LN_EPS, yb, mean, rstd)
    check_ln_fwd(c["fwd"], C, yb[:, :C], mean, rstd, fails, what)
    pads_intact("y", yb, C, fails, what)
    dxb = padbuf(c["prev"], M, C, ld, BF, dev)
    dg, db = c["dg0"].clone().to(dev), c["db0"].clone().to(dev)
    ops.layernorm_bwd(xb, dyb, C, gm, mean, rstd, dxb, dg, db, accumulate=accumulate)
    ref = ln_bwd_ref(c["x"], c["dy"], c["gamma"], mean.cpu(), rstd.cpu(), c["prev"] if accumulate else None,
                     c["dg0"], c["db0"])
    check_ln_bwd(ref, M, dxb[:, :C], dg, db, fails, what)
    pads_intact("dx", dxb, C, fails, what)
    if c["int_dy"]:
        assert float(ref["dbeta_mag"].max()) < 2 ** 24
        judge_bits("dbeta (integer sums)", db, ref["dbeta"].float(), fails, what)
    for name, buf, src in (("x", xb, c["x"]), ("dy", dyb, c["dy"])):
        if not same_bits(buf.cpu(), padbuf(src, M, C, ld, BF, "cpu")):
            fails.append(what + f"the input {name} was written")
    return fails


# ----------------------------------------------------------------------------- embedding
def _exponents(t):
    return torch.frexp(t.float())[1]


@functools.lru_cache(maxsize=None)
def emb_case(B, T, C, vocab, hot):
    """wte [vocab, C] and wpe [T + 3, C] (bf16, magnitudes in [2^-4, 2^4]) and the tokens: every one 0 with
    ``hot`` (one row takes all the atomics), else spread and including 0 and vocab - 1 where two tokens fit."""
    g = torch.Generator().manual_seed(((B * 100 + T) * 1000 + C) * 2 + hot)
    M = B * T

    def table(rows):
        w = torch.randn(rows, C, generator=g) * 2
        return (torch.sign(w) * w.abs().clamp(2.0 ** -4, 2.0 ** 4)).to(BF)

    wte, wpe = table(vocab), table(T + 3)
    e = torch.cat([_exponents(wte).reshape(-1), _exponents(wpe).reshape(-1)])
    assert bool((wte != 0).all()) and bool((wpe != 0).all()) and int(e.max() - e.min()) < 16
    tok = torch.zeros(M, dtype=torch.int64) if hot else torch.randint(0, vocab, (M,), generator=g)
    if not hot:
        tok[-1] = vocab - 1
        if M >= 2:
            tok[0] = 0
    pos = torch.arange(M) % T
    c = {"B": B, "T": T, "C": C, "vocab": vocab, "hot": hot, "M": M, "wte": wte, "wpe": wpe, "tok": tok, "pos": pos}
    c["out"] = round_bf16(wte[tok].double() + wpe[pos].double())  # (round_bf16 asserts the sum is exact in fp32)
    c["dx_int"] = torch.randint(-4, 5, (M, C), generator=g).to(BF)
    c["dx_gauss"] = torch.randn(M, C, generator=g).to(BF)
    c["dwte0"] = torch.randint(-9, 10, (vocab, C), generator=g).float()
    c["dwpe0"] = torch.randint(-9, 10, (T + 3, C), generator=g).float()
    assert bool((c["dwte0"] != 0).any()) and bool((c["dwpe0"] != 0).any())
    return c


def _emb_sums(c, dx, w0, p0):
    dw, dp = w0.double().clone(), p0.double().clone()
    dw.index_add_(0, c["tok"], dx.double())
    dp.index_add_(0, c["pos"], dx.double())
    return dw, dp


def run_embed(ops, dev, c):
    M, T, C, vocab = c["M"], c["T"], c["C"], c["vocab"]
    what = f"embed B={c['B']} T={T} C={C} vocab={vocab}{' hot' if c['hot'] else ''}: "
    fails = []
    out = padbuf(None, M, C, C + 8, BF, dev)
    ops.embed_fwd(c["wte"].to(dev), c["wpe"].to(dev), c["tok"].to(dev), T, out)
    judge_bits("out", out[:, :C], c["out"], fails, what)
    pads_intact("out", out, C, fails, what)
    # backward, integer dx into non-zero integer accumulators: an order-independent exact sum
    tok_d = c["tok"].to(dev)
    dxb = padbuf(c["dx_int"], M, C, C + 8, BF, dev)
    dw, dp = c["dwte0"].clone().to(dev), c["dwpe0"].clone().to(dev)
    ops.embed_bwd(dxb, tok_d, T, dw, dp)
    rw, rp = _emb_sums(c, c["dx_int"], c["dwte0"], c["dwpe0"])
    assert float(rw.abs().max()) < 2 ** 24 and float(rp.abs().max()) < 2 ** 24
    judge_bits("dwte (integer sums)", dw, rw.float(), fails, what)  # untouched rows and dwpe[T:] included
    judge_bits("dwpe (integer sums)", dp, rp.float(), fails, what)
    # gaussian dx into zeroed touched rows (the bound has no term for an initial value); every other row holds SENT
    w0, p0 = torch.full((vocab, C), SENT), torch.full((T + 3, C), SENT)
    w0[c["tok"].unique()] = 0.0
    p0[c["pos"].unique()] = 0.0
    dxb = padbuf(c["dx_gauss"], M, C, C + 8, BF, dev)
    dw, dp = w0.clone().to(dev), p0.clone().to(dev)
    ops.embed_bwd(dxb, tok_d, T, dw, dp)
    for name, got, init, idx in (("dwte", dw, w0, c["tok"]), ("dwpe", dp, p0, c["pos"])):
        got = got.cpu()
        touched = torch.zeros(init.shape[0], dtype=torch.bool)
        touched[idx] = True
        n = torch.zeros(init.shape[0], dtype=torch.float64).index_add_(0, idx, torch.ones(M, dtype=torch.float64))
        zero = torch.zeros(init.shape, dtype=torch.float64)
        ref = zero.clone().index_add_(0, idx, c["dx_gauss"].double())
        mag = zero.clone().index_add_(0, idx, c["dx_gauss"].double().abs())
        judge("dwte/dwpe", got[touched], ref[touched], ((n + 16) * 2.0 ** -23)[touched, None] * mag[touched], fails,
              what + name + " ")
        judge_bits(name + " untouched rows", got[~touched], init[~touched], fails, what)
    return fails
