"""The CIN kernels (csrc/kernels/cin.hip, module _cink) on the GPU against an fp64 evaluation of cin.h's rule on the
same bf16 inputs, one layer at a time: the reference of layer k reads the X^{k-1} (and dX^k, g0) the test supplies,
so no error compounds.

Bounds, derived (u = 2^-8, M the same sum on absolute values, K the length of the fp32 accumulation):
  forward   z is rounded once per term (<= u M in all), the MFMA accumulates in fp32 (<= K 2^-23 M), the stored
            X^k is rounded once more: |X^k - ref| <= e + u (|ref| + e), e = (u + K 2^-23) M, K = H_{k-1} mp.
  p, wide   fp32 sums of D (of Hs) exact inputs against fp64 on the kernel's own X^k: (D + Hs + 8) 2^-24 M.
  backward  dX^T = bf16(dz w_out) is an MFMA operand: that rounding, u M, exists at the last layer only (a stored
            dX^k is an exact input). dZ accumulates over H_k, the contractions over mp and H_{k-1} terms in fp32:
            e = (u_last + (H_k + H_{k-1} + mp + 8) 2^-23) M; a stored dX^{k-1} or dX row adds its rounding,
            u (|ref| + e).
  weights   z rounded (u M), dX^T rounded at the last layer (u M), fp32 over chunk D + nchunks terms.
A structural mistake is of order M: the reference without the last (i, j) terms of the K sweep misses the bound."""
import math

import pytest
import torch

from minips_amd import ops
from minips_amd.data.synthetic import CriteoSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu
BF, U, E23 = torch.bfloat16, 2.0 ** -8, 2.0 ** -23
SHAPES = [(1, 1), (3, 3), (26, 26), (48, 26)]  # (H_{k-1}, m): layer 1 where they agree, else layer 2


def _case(B, hp, m, H, D, drop=0):
    """Inputs and fp64 references of one layer. B == 5 makes the layer a middle one (a stored dX^k, a g0 from above);
    otherwise it is the last (dX^T on the fly). drop > 0 zeroes the last ``drop`` (i, j) terms of the same inputs'
    reference only."""
    g = torch.Generator().manual_seed(B + hp + m + H + D)
    first, last = hp == m, B != 5
    layers = (() if first else (hp,)) + (H,) + (() if last else (16,))
    k, mp, Hs = 1 if first else 2, (m + 7) // 8 * 8, sum(layers)
    off = 0 if first else hp
    X = torch.full((B, m * D + 11), float("nan"), dtype=BF)  # an unaligned leading dimension; NaN where not read
    X[:, : m * D] = torch.randn(B, m * D, generator=g).to(BF)
    XK = torch.zeros(B, Hs, D, dtype=BF)
    XK[:, :off] = torch.randn(B, off, D, generator=g).to(BF)
    dXK = torch.zeros(B, Hs, D, dtype=BF)
    dXK[:, off: off + H] = torch.randn(B, H, D, generator=g).to(BF)
    W = torch.zeros(H, hp, mp, dtype=BF)
    W[:, :, :m] = ((torch.rand(H, hp, m, generator=g) * 2 - 1) / math.sqrt(hp * m)).to(BF)
    w_out = (torch.randn(Hs, generator=g) * 0.5).to(BF)
    dz, g0 = torch.randn(B, generator=g), torch.randn(B, m, D, generator=g)
    c = dict(B=B, m=m, D=D, H=H, hp=hp, k=k, layers=layers, off=off, first=first, last=last, X=X, XK=XK, dXK=dXK, W=W,
             w_out=w_out, dz=dz, g0=g0, K=hp * mp)
    Wd = W[:, :, :m].double().clone()
    if drop:
        Wd.view(H, -1)[:, -drop:] = 0
    for tag, f in (("", lambda t: t), ("M_", torch.abs)):
        x0 = f(X[:, : m * D].double().view(B, m, D))
        xp = x0 if first else f(XK[:, :off].double())
        Wf, wo, dzf = f(Wd), f(w_out.double()), f(dz.double())
        z = xp[:, :, None, :] * x0[:, None, :, :]
        c[tag + "xk"] = torch.einsum("hij,bijc->bhc", Wf, z)
        dxk = f(dXK[:, off: off + H].double())
        if last:
            dxk = (dzf[:, None] * wo[off: off + H])[:, :, None].expand(B, H, D)
        dZ = torch.einsum("hij,bhc->bijc", Wf, dxk)
        dxp = (dZ * x0[:, None]).sum(2)
        gg = (dZ * xp[:, :, None]).sum(1)
        if first:
            gg = gg + dxp
        else:
            c[tag + "dxp"] = dxp + (dzf[:, None] * wo[:hp])[:, :, None]
        c[tag + "g"] = gg if last else gg + f(g0.double())
        c[tag + "dW"] = torch.einsum("bhc,bijc->hij", dxk, z)
    return c


def _within(got, ref, e, rounded):
    err = (got.double().cpu() - ref).abs()
    bound = e + (U * (ref.abs() + e) if rounded else 0)
    return bool((err <= bound).all())


def _w(c, dev):
    """W on the device; at B == 5 two bytes off a 16-byte boundary (the kernels' element-wise load of W)."""
    W = c["W"].to(dev)
    return torch.cat([W.new_zeros(1), W.flatten()])[1:].view(W.shape) if c["B"] == 5 else W


def _forward(c, dev, blocks=0):
    XK = c["XK"].to(dev)
    ops.wd_cin_layer_forward(c["X"].to(dev), c["m"], c["D"], _w(c, dev), c["layers"], c["k"], XK, blocks=blocks)
    return XK


def _backward(c, dev, perm=None, blocks=0, dX=None):
    B, m, D = c["B"], c["m"], c["D"]
    XK, dXK, g0 = _forward(c, dev), c["dXK"].to(dev), c["g0"].to(dev)
    dX = torch.zeros(B * m, D, dtype=BF, device=dev) if dX is None else dX.to(dev)
    ops.wd_cin_layer_backward(c["X"].to(dev), m, D, _w(c, dev), c["layers"], c["k"], XK, dXK, c["w_out"].to(dev),
                              c["dz"].to(dev), g0, dX, perm=None if perm is None else perm.to(dev), blocks=blocks)
    return dXK, g0, dX


@pytest.mark.parametrize("B", [1, 5, ops.CIN_CHUNK + 3])
@pytest.mark.parametrize("D", [8, 32])
@pytest.mark.parametrize("H", [16, 48, 128])
@pytest.mark.parametrize("hp,m", SHAPES)
def test_layer_against_fp64(B, hp, m, H, D, dev):
    c = _case(B, hp, m, H, D)
    off, K, mp = c["off"], c["K"], (m + 7) // 8 * 8
    # forward, with the same bits for every grid
    XK = _forward(c, dev)
    assert torch.equal(XK, _forward(c, dev, blocks=1)) and torch.equal(XK, _forward(c, dev, blocks=7))
    assert torch.equal(XK[:, :off].cpu(), c["XK"][:, :off]) and bool((XK[:, off + H:] == 0).all())
    assert _within(XK[:, off: off + H], c["xk"], (U + K * E23) * c["M_xk"], rounded=True)
    # pooled maps and the wide term on the stored values
    wide0 = torch.randn(B, generator=torch.Generator().manual_seed(1))
    outs = []
    for blocks in (0, 1, 7):
        wide, p = wide0.clone().to(dev), torch.full((B, XK.shape[1]), float("nan"), device=dev)
        ops.wd_cin_output(XK, c["w_out"].to(dev), wide, p, blocks=blocks)
        outs.append((wide, p))
        assert torch.equal(wide, outs[0][0]) and torch.equal(p, outs[0][1])
    x64, wo = XK.double().cpu(), c["w_out"].double()
    e_p = (D + XK.shape[1] + 8) * 2.0 ** -24
    assert _within(outs[0][1], x64.sum(2), e_p * x64.abs().sum(2), rounded=False)
    assert _within(outs[0][0], wide0.double() + x64.sum(2) @ wo,
                   e_p * (wide0.abs().double() + x64.abs().sum(2) @ wo.abs()), rounded=False)
    # backward: dX^{k-1}, g0 / dX, the same bits for every grid
    e_b = ((U if c["last"] else 0) + (H + hp + mp + 8) * E23)
    dXK, g0, dX = _backward(c, dev)
    for blocks in (1, 7):
        again = _backward(c, dev, blocks=blocks)
        assert all(torch.equal(a, b) for a, b in zip((dXK, g0, dX), again))
    if c["first"]:
        assert _within(dX.view(B, m, D), c["g"], e_b * c["M_g"], rounded=True)
        assert torch.equal(dXK.cpu(), c["dXK"])
    else:
        assert _within(g0, c["g"], e_b * c["M_g"], rounded=False) and bool((dX == 0).all())
        assert _within(dXK[:, :hp], c["dxp"], e_b * c["M_dxp"], rounded=True)
        assert torch.equal(dXK[:, hp:].cpu(), c["dXK"][:, hp:])
    # weight gradient: partials, folded in chunk order and added
    nch = ops.wd_cin_nchunks(B)
    part = torch.full((nch, H, K), float("nan"), device=dev)
    ops.wd_cin_layer_wgrad(c["X"].to(dev), m, D, c["layers"], c["k"], XK, c["dXK"].to(dev), c["w_out"].to(dev),
                           c["dz"].to(dev), part)
    G = torch.full((H, hp, mp), 0.5, device=dev)
    ops.wd_cin_fold(part, G)
    e_w = (U + (U if c["last"] else 0) + (ops.wd_cin_chunk(B) * D + nch + 8) * E23)
    assert _within(G[:, :, :m] - 0.5, c["dW"], e_w * c["M_dW"] + E23 * (0.5 + c["dW"].abs()), rounded=False)
    assert bool((G[:, :, m:] == 0.5).all()) and nch == (2 if B > ops.CIN_CHUNK else 1)


@pytest.mark.parametrize("hp,m", SHAPES[1:])
def test_a_dropped_k_tail_misses_the_bound(hp, m, dev):
    """The reference of the same inputs without the last whole i -- the sweep's last K step at mp = 32."""
    H, D, B = 16, 8, 1
    c, bad = _case(B, hp, m, H, D), _case(B, hp, m, H, D, drop=m)
    assert torch.equal(c["X"][:, : m * D], bad["X"][:, : m * D]) and torch.equal(c["W"], bad["W"])
    XK, (_, g0, dX) = _forward(c, dev), _backward(c, dev)
    e_f, e_b = (U + c["K"] * E23) * c["M_xk"], (U + (H + hp + c["K"] // hp + 8) * E23) * c["M_g"]
    got = dX.view(B, m, D) if c["first"] else g0
    assert _within(XK[:, c["off"]:], c["xk"], e_f, True) and not _within(XK[:, c["off"]:], bad["xk"], e_f, True)
    assert _within(got, c["g"], e_b, c["first"]) and not _within(got, bad["g"], e_b, c["first"])


def test_perm_and_a_skipped_entry(dev):
    c, n = _case(7, 3, 3, 16, 8), 21
    gen = torch.Generator().manual_seed(2)
    dX0 = torch.randn(n, 8, generator=gen).to(BF)
    plain = _backward(c, dev, dX=dX0)[2].cpu()
    perm = torch.randperm(n, generator=gen).to(torch.int32)
    srt = torch.empty_like(dX0)
    srt[perm.long()] = dX0
    assert torch.equal(_backward(c, dev, perm=perm, dX=srt)[2].cpu()[perm.long()], plain)
    hole, keep = perm.clone(), torch.arange(n) != 4
    hole[4] = n  # out of range: the lookup is skipped and its row keeps its value
    got = _backward(c, dev, perm=hole, dX=srt)[2].cpu()
    assert torch.equal(got[perm.long()[keep]], plain[keep]) and torch.equal(got[perm[4]], srt[perm[4]])


CARDS = [100, 50, 3000, 7, 300, 20, 5, 60, 90, 10, 11, 12]


def _run(device, steps=6):
    m = WideDeep(WideDeepConfig(cards=CARDS, hidden=(128, 64, 64), emb_dim=16, row_width=20, cin_layers=(32, 16)),
                 Comm(device=torch.device(device)))
    data = CriteoSynth(320, cards=CARDS, device="cpu", seed=3)
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        losses.append(float(m.train_step(dense.to(device), keys.to(device), y.to(device)).item()) / 320)
    held = data.holdout(5)
    ev = m.evaluate((t.to(device) for t in held.next()) for _ in range(2))
    m.drain()
    return losses + [ev["logloss"]]


def test_xdeepfm_on_the_gpu_matches_the_cpu(dev):
    l_cpu, l_gpu = _run("cpu"), _run(dev)
    for a, b in zip(l_gpu, l_cpu):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (l_gpu, l_cpu)
