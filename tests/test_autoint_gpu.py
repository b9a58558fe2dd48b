"""AutoInt's kernels on the GPU, one layer at a time against an fp64 evaluation of the plain formula on the same bf16
inputs (the test supplies E^{l-1}, dE^l and the incoming dX, so nothing compounds across layers), and the model.

Bounds (derived, not fitted; u = 2^-8, f = 2^-23 per fp32 accumulation step, |.| = the same expression on absolute
values, all evaluated in fp64 by the reference):
  scores   Q and K carry one rounding each: e_s = ((1 + u)^2 - 1 + (Din + d) f) (|Q| |K|^T). The inputs are scaled so
           that e_s <= 0.05 (asserted): a dropped mask, head or tile changes an output by the order of its magnitude
           M and cannot hide inside a bound of a few percent of M.
  P        softmax of scores off by e_s: relative exp(2 e_s) - 1, + 2^-20 for the fast exponential, + u for P's own
           rounding: r_P = exp(2 e_s) (1 + 2^-20) (1 + u) - 1.
  forward  err = ((1 + r_P)(1 + u) - 1 + (m + Din) f) (P |V|) + Din f (|E| |W_R|); the stored value adds
           u (|O + R| + err).
  dV       ((1 + r_P)(1 + u) - 1) (P^T |dY|);  dP: V's rounding, u (|dY| |V|^T) = u M_dP
  dS       M_dS = P (M_dP + sum_j P M_dP), relative r_S = (1 + r_P)^2 (1 + u)^2 - 1 (two factors P, dP, own rounding)
  dQ, dK   ((1 + r_S)(1 + u)^2 - 1) (M_dS |K|) and (M_dS^T |Q|) (dS, the other operand's rounding, own rounding)
  dE^{l-1} err_G |W|^T + 4 A f (|G| |W|^T); the bf16 store adds u (|value| + err) (for dX: of the updated value)
  dW       sum_b |E|^T err_G + (32 chunk) f (|E|^T |G|): per chunk, compared after the in-order fold
  wide, dw_out   fp32 sums of exact products: n f M.
The largest observed error / bound ratios are recorded in profiles/autoint/bounds.txt."""
import math

import pytest
import torch

from minips_amd import ops
from minips_amd.data.synthetic import CriteoSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu
BF, U, FE = torch.bfloat16, 2.0 ** -8, 2.0 ** -23
CH = ops.ATTN_CHUNK
# m, D, H, d, B, T, l, perm: every value of the issue's table, first / middle / last layers
CASES = [(1, 8, 1, 16, 1, 1, 1, False), (3, 32, 2, 32, 5, 2, 1, True), (16, 64, 4, 16, CH + 3, 3, 1, True),
         (17, 8, 2, 32, 5, 3, 2, False), (26, 32, 2, 32, CH + 3, 3, 3, False), (32, 64, 1, 16, 5, 2, 2, False),
         (26, 32, 4, 16, 1, 3, 2, False), (32, 32, 2, 32, CH + 3, 2, 1, True), (17, 8, 3, 16, 5, 2, 2, False)]


def _heads(t, H, d):
    return t.view(t.shape[0], t.shape[1], H, d).transpose(1, 2)


def _merge(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)


def _reference(E, W, H, d, dE, mask):
    """fp64: the layer's output with its bound, and (dE^{l-1}, G, their bounds) for dY = dE where mask."""
    m, A, din = E.shape[1], H * d, E.shape[2]
    Y = E @ W
    Q, K, V = (_heads(Y[..., i * A:(i + 1) * A], H, d) for i in range(3))
    R, aW = Y[..., 3 * A:], W.abs()
    aY = E.abs() @ aW
    aQ, aK, aV = (_heads(aY[..., i * A:(i + 1) * A], H, d) for i in range(3))
    e_s = (((1 + U) ** 2 - 1 + (din + d) * FE) * (aQ @ aK.transpose(-1, -2))).max().item()
    P = torch.softmax(Q @ K.transpose(-1, -2), -1)
    r_p = math.exp(2 * e_s) * (1 + 2.0 ** -20) * (1 + U) - 1
    out = _merge(P @ V) + R
    err = ((1 + r_p) * (1 + U) - 1 + (m + din) * FE) * _merge(P @ aV) + din * FE * aY[..., 3 * A:]
    fwd = (torch.relu(out), err + U * (out.abs() + err))
    dY = torch.where(mask, dE, torch.zeros_like(dE))
    dYh, aV_ = _heads(dY, H, d), V.abs()
    dV, e_dV = P.transpose(-1, -2) @ dYh, ((1 + r_p) * (1 + U) - 1) * (P.transpose(-1, -2) @ dYh.abs())
    dP, m_dP = dYh @ V.transpose(-1, -2), dYh.abs() @ aV_.transpose(-1, -2)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    m_dS = P * (m_dP + (m_dP * P).sum(-1, keepdim=True))
    r_q = ((1 + r_p) ** 2 * (1 + U) ** 2) * (1 + U) ** 2 - 1
    dQ, dK = dS @ K, dS.transpose(-1, -2) @ Q
    e_dQ, e_dK = r_q * (m_dS @ K.abs()), r_q * (m_dS.transpose(-1, -2) @ Q.abs())
    G = torch.cat([_merge(dQ), _merge(dK), _merge(dV), dY], -1)
    eG = torch.cat([_merge(e_dQ), _merge(e_dK), _merge(e_dV), torch.zeros_like(dY)], -1)
    dEp = G @ W.t()
    e_dEp = eG @ aW.t() + 4 * A * FE * (G.abs() @ aW.t())
    return e_s, fwd, (dEp, e_dEp, G, eG)


def _ratio(name, got, want, bound):
    r = ((got.double().cpu() - want).abs() / (bound + 1e-30)).max().item()
    print(f"{name}: max error / bound = {r:.3f}")
    assert r <= 1.0, f"{name}: error exceeds the derived bound ({r:.3f} of it)"


@pytest.mark.parametrize("m,D,H,d,B,T,l,use_perm", CASES)
def test_layer_against_fp64(m, D, H, d, B, T, l, use_perm, dev):
    g = torch.Generator().manual_seed(1000 * m + D + l)
    A, cfg = H * d, (T, H, d)
    din = D if l == 1 else A
    X = torch.randn(B, m * D + 3, generator=g).to(BF)  # an odd leading dimension, NaN in the unread columns
    X[:, m * D:] = float("nan")
    EK = torch.randn(B, T, m, A, generator=g).to(BF)
    dEK = (0.5 * torch.randn(B, T, m, A, generator=g)).to(BF)
    W = torch.randn(din, 4 * A, generator=g) / din ** 0.5
    w_out, dwide = torch.randn(m * A, generator=g).to(BF), torch.randn(B, generator=g)
    dX0 = torch.randn(B * m, D, generator=g).to(BF)
    perm = torch.randperm(B * m, generator=g).int()
    perm[0] = -1 if m * B == 1 else B * m + 5  # one entry outside [0, B F): skipped
    E = (X[:, :m * D].view(B, m, D) if l == 1 else EK[:, l - 2]).double()
    for _ in range(8):  # the condition e_s <= 0.05, by scaling the Q | K columns
        if _reference(E, W.to(BF).double(), H, d, torch.zeros(B, m, A, dtype=torch.float64),
                      torch.ones(B, m, A, dtype=torch.bool))[0] <= 0.05:
            break
        W[:, :2 * A] *= 0.6
    W = W.to(BF)
    nch = ops.wd_attn_nchunks(B)

    def run(blocks):
        t = dict(X=X.to(dev), EK=EK.to(dev), dEK=dEK.to(dev), dX=dX0.to(dev).clone(),
                 part=torch.full((nch, din, 4 * A), 7.0, device=dev), wide=torch.ones(B, device=dev),
                 part_o=torch.full((nch, m * A), 7.0, device=dev), G=torch.ones(din, 4 * A, device=dev))
        Wd, wo, dw = W.to(dev), w_out.to(dev), dwide.to(dev)
        ops.wd_attn_layer_forward(t["X"], m, D, Wd, cfg, l, t["EK"], blocks=blocks)
        ops.wd_attn_layer_backward(t["X"], m, D, Wd, cfg, l, t["EK"], t["dEK"], wo, dw, t["dX"], t["part"],
                                   perm=perm.to(dev) if use_perm else None, blocks=blocks)
        ops.wd_attn_fold(t["part"], t["G"])
        ops.wd_attn_output(t["EK"], d, wo, t["wide"], blocks=blocks)
        ops.wd_attn_wout_partial(t["EK"], d, dw, t["part_o"])
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in t.items() if k != "X"}

    out = run(0)
    for blocks in (0, 1, 7):  # the same bits for every grid and run
        again = run(blocks)
        for k in out:
            assert torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)), (k, blocks)

    El = out["EK"][:, l - 1].double()
    dE = dEK[:, l - 1].double() if l < T else (dwide[:, None] * w_out.float()).to(BF).double().view(B, m, A)
    e_s, (ref, b_fwd), (dEp, e_dEp, G, eG) = _reference(E, W.double(), H, d, dE, El > 0)
    assert e_s <= 0.05
    _ratio("E^l", El, ref, b_fwd)
    for k in range(T):  # the other slots are untouched
        if k != l - 1:
            assert torch.equal(out["EK"][:, k], EK[:, k])
    if l > 1:
        _ratio("dE^{l-1}", out["dEK"][:, l - 2], dEp, e_dEp + U * (dEp.abs() + e_dEp))
        assert torch.equal(out["dX"], dX0)
    else:
        want, rows = dX0.double().clone(), torch.arange(B * m)
        if use_perm:
            ok = (perm >= 0) & (perm < B * m)
            rows, dEp, e_dEp = perm[ok].long(), dEp.reshape(B * m, D)[ok], e_dEp.reshape(B * m, D)[ok]
        want[rows] += dEp.reshape(-1, D)
        bound = torch.zeros_like(want)
        bound[rows] = e_dEp.reshape(-1, D) + U * (want[rows].abs() + e_dEp.reshape(-1, D))
        _ratio("dX", out["dX"], want, bound)
    dW = torch.einsum("bik,bin->kn", E, G)
    b_dW = torch.einsum("bik,bin->kn", E.abs(), eG) + 32 * CH * FE * torch.einsum("bik,bin->kn", E.abs(), G.abs())
    _ratio("dW", out["G"] - 1.0, dW, b_dW + FE * (1 + dW.abs()) * (nch + 1))
    ET = out["EK"][:, T - 1].double().reshape(B, -1)
    _ratio("wide", out["wide"] - 1.0, ET @ w_out.double(), m * A * FE * (ET.abs() @ w_out.double().abs()) + 2 * FE)
    chunks = [slice(c * CH, (c + 1) * CH) for c in range(nch)]
    _ratio("dw_out", out["part_o"], torch.stack([dwide[s].double() @ ET[s] for s in chunks]),
           torch.stack([CH * FE * (dwide[s].double().abs() @ ET[s].abs()) for s in chunks]))


CARDS = [100, 50, 3000, 7, 300, 20, 5, 60, 90, 10, 11, 12]


def _run(device, steps=6):
    m = WideDeep(WideDeepConfig(cards=CARDS, hidden=(128, 64, 64), emb_dim=16, row_width=20, attn_layers=2,
                                attn_heads=2, attn_dim=16), Comm(device=torch.device(device)))
    data = CriteoSynth(320, cards=CARDS, device="cpu", seed=3)
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        losses.append(float(m.train_step(dense.to(device), keys.to(device), y.to(device)).item()) / 320)
    held = data.holdout(5)
    m.drain()
    before = (m.emb.shard.clone(), m.dense.full_master().clone())
    ev = m.evaluate((t.to(device) for t in held.next()) for _ in range(2))
    m.drain()  # evaluate() writes no table value
    assert torch.equal(before[0], m.emb.shard) and torch.equal(before[1], m.dense.full_master())
    m.drain()
    return losses + [ev["logloss"]]


def test_autoint_on_the_gpu_matches_the_cpu(dev):
    l_cpu, l_gpu = _run("cpu"), _run(dev)
    for a, b in zip(l_gpu, l_cpu):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (l_gpu, l_cpu)
