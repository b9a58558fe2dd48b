"""The checker of tests/_nn_ref.py, tested on the CPU. (1) The CPU path of minips_amd.ops (attn_fwd / attn_bwd,
layernorm_*, embed_*) passes the same checks at the same shapes as the HIP kernels in test_gpt2_kernels_gpu.py.
(2) The checker rejects seeded mistakes: each is applied to a local fp64 copy of the reference arithmetic (never to
a kernel), its outputs are rounded as a kernel stores them, and the same check_* calls must fail, while the
unmodified copy passes. That is what shows the magnitude bounds can see a subtle error."""
import pytest
import torch

import _nn_ref as R
from minips_amd import ops

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- the CPU path passes
@pytest.mark.parametrize("regime", R.ATTN_REGIMES)
@pytest.mark.parametrize("B,H,T", R.ATTN_SHAPES)
def test_attention_cpu_path(B, H, T, regime):
    c = R.attn_case(B, H, T, regime)
    fails = R.run_attn(ops, CPU, c, padded=False) + R.run_attn(ops, CPU, c, padded=True)
    assert not fails, fails


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
def test_attention_chained_cpu_path(B, H):
    fails = R.run_attn(ops, CPU, R.attn_case(B, H, 129, "peaked"), padded=True, chained=True)
    assert not fails, fails


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm_cpu_path(M, C, accumulate):
    fails = R.run_ln(ops, CPU, R.ln_case(M, C), accumulate)
    assert not fails, fails


@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm_integer_dy_cpu_path(M, C):
    fails = R.run_ln(ops, CPU, R.ln_case(M, C, int_dy=True), accumulate=True)
    assert not fails, fails


@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("B,T,C,vocab", R.EMB_SHAPES)
def test_embedding_cpu_path(B, T, C, vocab, hot):
    fails = R.run_embed(ops, CPU, R.emb_case(B, T, C, vocab, hot))
    assert not fails, fails


def test_one_pass_variance_misses_the_rstd_bound():
    """The formula the kernels used before (E[x^2] - mean^2 in fp32) fails the rstd bound on the mean / std = 200
    rows; this is why the forward takes the mean first and sums (v - mean)^2."""
    c = R.ln_case(300, 256)
    x = c["x"].float()
    mu = x.mean(1)
    rs = torch.rsqrt(((x * x).mean(1) - mu * mu).clamp_min(0) + R.LN_EPS)
    fails = []
    worst = dict(R.WORST)
    R.judge("rstd", rs, c["fwd"]["rstd"], (256 + 16) * 2.0 ** -23 * c["fwd"]["rstd"], fails)
    R.WORST.clear()
    R.WORST.update(worst)  # (a deliberate failure is not an observed error of the code under test)
    assert fails


# ----------------------------------------------------------------------------- seeded mistakes are rejected
ATTN_MISTAKES = ("mask_ge", "skip_last_key_tile", "row_unwritten", "lse_hbt", "dk_unscaled", "dq_no_delta")


def _attn_copy(c, mistake=None):
    """A local fp64 copy of the attention arithmetic with one seeded mistake; returns O (bf16), lse (fp32) and
    dqkv (bf16) as a kernel would store them. The backward is fed the case's reference O and lse."""
    B, H, T, d, scale = c["B"], c["H"], c["T"], c["d"], c["scale"]
    q, k, v = (R._heads(c["qkv"], B, T, H, col) for col in (0, d, 2 * d))
    causal = torch.ones(T, T, dtype=torch.bool).triu(1)
    mask = torch.ones(T, T, dtype=torch.bool).triu(0) if mistake == "mask_ge" else causal.clone()  # > became >=
    if mistake == "skip_last_key_tile":
        mask[:, 64 * ((T - 1) // 64):] = True
    s = (q @ k.transpose(-1, -2)) * scale
    sm = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(sm, -1, keepdim=True)
    O = torch.exp(sm - lse) @ v
    if mistake == "row_unwritten":  # the last query row of the second 128-row block keeps what the buffer held
        O[:, :, min(T, 256) - 1] = 0.0
    lse2 = (lse * R.L2E).squeeze(-1)  # [B, H, T]
    if mistake == "lse_hbt":
        lse2 = lse2.transpose(0, 1)
    o, do = R._heads(c["O_in"], B, T, H, 0), R._heads(c["dO"], B, T, H, 0)
    p = torch.exp2(s * R.L2E - c["lse_in"].double().reshape(B, H, T, 1)).masked_fill(causal, 0.0)
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    dq = scale * ((p * (dp if mistake == "dq_no_delta" else dp - delta)) @ k)
    dk = (1.0 if mistake == "dk_unscaled" else scale) * ((p * (dp - delta)).transpose(-1, -2) @ q)
    dv = p.transpose(-1, -2) @ do
    dqkv = torch.cat([R._rows(t, B, T, H) for t in (dq, dk, dv)], 1)
    return R._rows(O, B, T, H).to(R.BF), lse2.reshape(-1).float(), dqkv.to(R.BF)


def _attn_verdict(c, mistake):
    O, lse, dqkv = _attn_copy(c, mistake)
    worst = dict(R.WORST)
    fails = []
    R.check_attn_fwd(c["fwd"], O, lse, c["T"], fails)
    R.check_attn_bwd(c["bwd"], dqkv, fails)
    if mistake is not None:  # (a seeded mistake is not an observed error of the code under test)
        R.WORST.clear()
        R.WORST.update(worst)
    return fails


@pytest.mark.parametrize("regime", ["flat", "zero_q", "spike_late"])
@pytest.mark.parametrize("T", [129, 257])
def test_attention_copy_passes_and_every_mistake_fails(T, regime):
    """(In the regimes where every mistake changes the result: under an early spike or a peaked softmax the
    probability of a dropped key can be below the rounding, so there is nothing to see.)"""
    c = R.attn_case(2, 3, T, regime)
    assert not _attn_verdict(c, None)
    for mistake in ATTN_MISTAKES:
        fails = _attn_verdict(c, mistake)
        assert fails, (mistake, "passed the checker")
        hit = {"mask_ge": "O", "skip_last_key_tile": "lse", "row_unwritten": "O", "lse_hbt": "lse",
               "dk_unscaled": "dK", "dq_no_delta": "dQ"}[mistake]
        assert any(f.startswith(hit + ":") for f in fails), (mistake, fails)


def _ln_copy(c, mistake=None, accumulate=True):
    """A local fp64 copy of the LayerNorm backward (fed the reference's mean and rstd) with one seeded mistake:
    one of the 16 slices of partial rows missing from dgamma (row r goes to partial row r % G, G = ceil(M / 8)
    of them, slice j takes partial rows [j G/16, (j+1) G/16)), or the accumulate flag ignored."""
    M, C, f = c["M"], c["C"], c["fwd"]
    x, dy, gm = c["x"].double(), c["dy"].double(), c["gamma"].double()
    mean, rs = f["mean"].float().double()[:, None], f["rstd"].float().double()[:, None]
    xh = (x - mean) * rs
    g = dy * gm
    dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if accumulate and mistake != "accumulate_ignored":
        dx = dx + c["prev"].double()
    keep = torch.ones(M, dtype=torch.bool)
    if mistake == "slice_dropped":
        G = (M + 7) // 8
        assert G >= 64
        per = (G + 15) // 16
        part = torch.arange(M) % G
        keep = ~((part >= 5 * per) & (part < 6 * per))
        assert 0 < int((~keep).sum()) < M // 8
    dg = c["dg0"].double() + (dy * xh)[keep].sum(0)
    db = c["db0"].double() + dy.sum(0)
    return dx.to(R.BF), dg.float(), db.float()


@pytest.mark.parametrize("M,C", [(505, 768), (520, 1024)])
def test_layernorm_copy_passes_and_every_mistake_fails(M, C):
    c = R.ln_case(M, C)
    f = c["fwd"]
    ref = R.ln_bwd_ref(c["x"], c["dy"], c["gamma"], f["mean"].float(), f["rstd"].float(), c["prev"], c["dg0"],
                       c["db0"])
    worst = dict(R.WORST)
    for mistake, hit in ((None, None), ("slice_dropped", "dgamma"), ("accumulate_ignored", "dx")):
        fails = []
        R.check_ln_bwd(ref, M, *_ln_copy(c, mistake), fails)
        if mistake is None:
            assert not fails, fails
            worst = dict(R.WORST)
        else:
            assert fails and all(f.startswith(hit + ":") for f in fails), (mistake, fails)
    R.WORST.clear()
    R.WORST.update(worst)
