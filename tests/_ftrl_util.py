"""Shared pieces of the FTRL-Proximal tests: the independent fp64 oracle (the textbook form of
McMahan et al. 2013, Algorithm 1), the near-threshold mask of the zero-pattern comparison, input makers."""
import torch

RTOL, ATOL = 1e-5, 1e-6  # the single-apply tolerance of tests/test_kernels_gpu.py's sparse optimizers
HYPERS = [dict(alpha=0.1, beta=1.0, l1=0.0, l2=0.0), dict(alpha=0.1, beta=1.0, l1=0.5, l2=0.0),
          dict(alpha=0.05, beta=0.5, l1=0.0, l2=0.01), dict(alpha=0.1, beta=1.0, l1=0.5, l2=0.01)]


def oracle_apply(w, z, n, g, alpha, beta=1.0, l1=0.0, l2=0.0):
    """One FTRL-Proximal step on fp64 tensors of equal shape, sigma = (sqrt(n + g^2) - sqrt(n)) / alpha."""
    w, z, n, g = (t.double() for t in (w, z, n, g))
    n1 = n + g * g
    sigma = (n1.sqrt() - n.sqrt()) / alpha
    z1 = z + g - sigma * w
    w1 = torch.where(z1.abs() <= l1, torch.zeros_like(z1),
                     -(z1 - torch.sign(z1) * l1) / ((beta + n1.sqrt()) / alpha + l2))
    return w1, z1, n1


def oracle_rows(table, zn, keys, base, grads, **hp):
    """oracle_apply on rows keys - base of an fp64 (table [rows, W], zn [rows, 2W]) pair, in place."""
    W = grads.shape[1]
    r = keys - base
    w1, z1, n1 = oracle_apply(table[r, :W], zn[r, :W], zn[r, W:], grads, **hp)
    table[r, :W], zn[r, :W], zn[r, W:] = w1, z1, n1


def decided(z64, l1):
    """Where the zero / non-zero decision |z| <= l1 is not within rounding of its threshold."""
    a = z64.abs()
    return (a - l1).abs() > 1e-4 * torch.clamp(a, min=l1)


def check_zero_pattern(w, z64, l1, what=""):
    """w's zero pattern equals the oracle's wherever the decision is clear; at most 1 % is unclear."""
    ok = decided(z64, l1)
    excluded = 1.0 - float(ok.double().mean())
    print(f"{what} zero pattern: excluded share {excluded:.3g}")
    assert excluded <= 0.01, excluded
    assert torch.equal((w == 0)[ok], (z64.abs() <= l1)[ok])
    return int((~ok).sum())


def eighths(shape, gen, lim=4.0):
    """Multiples of 1/8 in [-lim, lim]: sums of a few of them are exact in fp32 in any order."""
    k = int(lim * 8)
    return torch.randint(-k, k + 1, shape, generator=gen).float() / 8.0


def distinct_keys(n, rows, base, gen):
    return torch.randperm(rows, generator=gen)[:n].to(torch.int64) + base
