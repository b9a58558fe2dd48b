"""ops.gemm's CPU path (the reference every model-level GPU test compares against) for every EPI_* code, all four
operand layouts and the padded / odd-stride case layouts, against the independent fp64 reference of
tests/_gemm_ref.py: bit-exact in the exact regime, |out - ref| <= 2^-8 |ref| + 2^-18 in the GELU regime. The same
runner drives the GPU kernels in tests/test_gemm_epilogues_gpu.py, so this also validates the helper itself."""
import pytest
import torch

import _gemm_ref as G
from minips_amd import ops

CPU = torch.device("cpu")


def test_round_bf16_is_rne():
    # 1 + 2^-8 is halfway between bf16 1.0 and 1.0078125: ties go to the even mantissa, in both directions
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 257.0, 259.0, 0.0, -0.0,
                      1.0 + 2.0 ** -9], dtype=torch.float64)
    want = torch.tensor([1.0, 1.015625, -1.0, 256.0, 260.0, 0.0, -0.0, 1.0], dtype=torch.float64)
    got = G.round_bf16(x)
    assert got.dtype == torch.bfloat16 and torch.equal(G._bits(got), G._bits(want.to(torch.bfloat16)))
    assert G.is_tie(x).tolist() == [True, True, True, True, True, False, False, False]
    g = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=g).double()  # (fp32 values: exact in fp64)
    assert torch.equal(G._bits(G.round_bf16(r.float().double())), G._bits(r.float().to(torch.bfloat16)))


def test_reference_gelu_matches_closed_form():
    x = torch.linspace(-16, 16, 4097, dtype=torch.float64).requires_grad_()
    y = torch.nn.functional.gelu(x, approximate="tanh")
    (dy,) = torch.autograd.grad(y.sum(), x)
    # (the kernel's 0.7978845608 is sqrt(2 / pi) to 10 digits)
    torch.testing.assert_close(G.gelu64(x.detach()), y.detach(), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(G.gelu_grad64(x.detach()), dy, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_cpu_gemm_every_epilogue(layout, shape):
    stats = {}
    fails = G.run_grid(ops, CPU, layout, shape, stats=stats)
    print(layout, shape, stats)
    assert not fails, fails[:10]
    assert stats["cells"] >= 2 * 11 + 1


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_cpu_gemm_gaussian_f32(layout):
    stats = {}
    fails = G.run_gauss(ops, CPU, layout, stats=stats)
    print(layout, stats)
    assert not fails, fails


def test_cpu_gemm_accumulate_into_padded_c():
    # (the CPU path has one K slice; the cases are the GPU split-K ones: pre-filled, padded, odd-stride C)
    fails = G.run_splitk(ops, CPU)
    assert not fails, fails


def test_cpu_gemm_batched_with_bias():
    fails = G.run_batched(ops, CPU)
    assert not fails, fails
