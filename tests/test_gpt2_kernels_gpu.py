"""GPT-2's non-GEMM HIP kernels (fused causal attention: attn_fwd, attn_prep, attn_bwd_dq, attn_bwd_dkv; LayerNorm
forward / backward / column sums; token + position embedding) against the fp64 references and component-wise
magnitude bounds of tests/_nn_ref.py, at the kernels' edges: 16 / 32 (rows per wave), 64 (LDS tile), 128 (rows per
workgroup) and one past each, padded pitches with sentinel pad columns, flat / peaked / spiked / zero-query softmax
rows, both sides of LayerNorm's sliced atomic reduction (M = 504 / 505), grid-stride rows, and bit-exact integer
reductions. tests/test_nn_ref.py runs the same checks on the CPU path and shows they reject seeded mistakes."""
import json

import pytest
import torch

import _nn_ref as R
from minips_amd import _native, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _require_kernels(dev):
    _native.kernels()


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nworst error / bound per tensor:", json.dumps({k: round(v, 4) for k, v in sorted(R.WORST.items())}))


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize("regime", R.ATTN_REGIMES)
@pytest.mark.parametrize("B,H,T", R.ATTN_SHAPES)
def test_attention(dev, B, H, T, regime):
    """Forward, and the backward fed the reference's O (bf16) and lse (fp32) so it is judged alone, with default
    pitches and with every pitch padded (qkv 3d + 8, O d + 8, dO d + 16, dqkv 3d + 8); the backward run twice
    must give the same bits (dQ has its own sweep: no float atomics)."""
    c = R.attn_case(B, H, T, regime)
    fails = R.run_attn(ops, dev, c, padded=False) + R.run_attn(ops, dev, c, padded=True)
    assert not fails, fails


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
def test_attention_chained(dev, B, H):
    """The backward fed the GPU forward's own O and lse."""
    fails = R.run_attn(ops, dev, R.attn_case(B, H, 129, "peaked"), padded=True, chained=True)
    assert not fails, fails


@pytest.mark.parametrize("B,T", [(0, 5), (2, 0)])
def test_attention_empty_launch(dev, B, T):
    """B * T == 0 returns before any launch and writes nothing."""
    H, d = 2, 128
    bf = dict(dtype=torch.bfloat16, device=dev)
    qkv, O, dO, dqkv = (torch.empty(0, w, **bf) for w in (3 * d, d, d, 3 * d))
    lse, delta = torch.full((8,), R.SENT, device=dev), torch.full((8,), R.SENT, device=dev)
    ops.attn_fwd(qkv, B, T, H, 0.125, O, lse)
    ops.attn_bwd(qkv, O, dO, lse, delta, B, T, H, 0.125, dqkv)
    torch.cuda.synchronize()
    want = torch.full((8,), R.SENT)
    assert R.same_bits(lse.cpu(), want) and R.same_bits(delta.cpu(), want)


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm(dev, M, C, accumulate):
    """Rows of 2 randn + 0.5, of mean / std = 16, 64, 200 and constant rows, at pitch C + 4 with sentinel pads, into
    a non-trivial dx and non-zero dgamma / dbeta. (504, 768) has 63 partial rows (one colsum slice, plain +=),
    (505, 768) 64 (16 slices, fp32 atomics); (33000, 8) runs grid-stride rows at the 4096-block cap."""
    fails = R.run_ln(ops, dev, R.ln_case(M, C), accumulate)
    assert not fails, fails


@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm_integer_dy_dbeta_bit_exact(dev, M, C):
    """Integer dy: dbeta is an exact integer sum in any order, so it is bit-exact on both reduction paths: no row
    is dropped or counted twice."""
    fails = R.run_ln(ops, dev, R.ln_case(M, C, int_dy=True), accumulate=True)
    assert not fails, fails


# ----------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("B,T,C,vocab", R.EMB_SHAPES)
def test_embedding(dev, B, T, C, vocab, hot):
    """embed_fwd bit-exact against bf16(fp64 sum) at output pitch C + 8; embed_bwd bit-exact on integer dx into
    non-zero accumulators and within (n + 16) 2^-23 sum|dx| on gaussian dx; rows of dwte whose token never occurs
    and rows of dwpe at positions >= T unchanged bitwise. ``hot``: every token equal (one row takes all atomics)."""
    fails = R.run_embed(ops, dev, R.emb_case(B, T, C, vocab, hot))
    assert not fails, fails
