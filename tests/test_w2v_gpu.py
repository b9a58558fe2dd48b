"""The skip-gram negative-sampling kernels (csrc/kernels/sgns.hip through ops.sgns_lookups / sgns_forward /
sgns_backward) on the GPU (csrc/kernels/sgns.h states the rule). The lookups are integers: torch.equal to the CPU
reference. The forward and the backward are judged against fp64 references with derived bounds, u = 2^-24:
  forward   s_t = <v, u_t> is d products summed in some order (a lane's own in column order, then the lanes' by a
            butterfly): every product is rounded once and every partial sum at most d - 1 times, so
              |s - s64| <= (d + 2) u sum_f |v_f u_f|                                        =: b_s
            e = head(s) gscale: the logistic function's slope is at most 1/4, and exp, the quotient and the product
            with gscale round a value of at most 1 a few times:
              |e - e64| <= gscale (b_s / 4 + 4 u)
            a term of the loss has slope at most 1 in s and is max + product + log1p(exp) of values of at most
            |s| + 1:  b_s + 4 u (|s| + 1); the N + 1 terms are non-negative and summed in t order, each partial sum
            rounded once:
              |loss - loss64| <= sum_t (b_s,t + 4 u (|s_t| + 1)) + (N + 1) u sum_t loss64_t
            h = sum_t e_t u_t is judged against the fp64 sum of the kernel's OWN e times the rows, so that only its
            own N + 1 products and additions count:
              |h - h64| <= (N + 3) u sum_t |e_t u_t|
            a masked or missing target's e is exactly 0, a pair without a centre is exactly 0 everywhere.
  backward  alone, on the outputs of the fp32 CPU reference forward, so only its own summation is judged: a member
            contributes h_p (exact) or e v (one rounding), and the M_r members of a row are summed in some order, a
            partial sum rounded at most M_r times:
              |g - g64| <= (M_r + 4) u sum_m |contribution_m|
            rows without lookups keep a sentinel.
Shapes: the smallest that reach every path -- every lane shape (d 4 / 8 / 32 / 128 / 256 / 512), N 1 / 5 / 64,
P 1 / 3 / 257 (more than one block at the forced grid sizes), cap > U, rows contiguous, strided with ld = d + 4 (still
the float4 kernels), with ld = d + 1 and misaligned by 4 bytes (both the one-lane-per-element fallback, at every one
of its lane shapes: d 4 / 8 / 16 / 32 / 64 / 128 / 256 / 512), member counts on both sides of every backward switch
(32 | 33, 512 | 513), one batch whose pairs all share one centre (a heavy input row of col == 0 members), one whose
negatives are all one word (a heavy output row), a heavy row first and last in memrow. Results are bit-identical
across repeats and at blocks = 1, 7 and the default. Then the model: GPU against CPU, no host sync in a steady
step, two ranks on one card."""
import math

import pytest
import torch

from test_multirank_gpu import run_world
from test_w2v import _w2v_world, _power_law

from minips_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
I64, I32 = torch.int64, torch.int32


# ------------------------------------------------------------------------------ lookups
@pytest.mark.parametrize("V,N,P", [(1000, 5, 257), (7, 64, 1), (1000, 1, 1), (37, 64, 257)])
def test_lookups_equal_the_cpu_reference(V, N, P, dev):
    thr, alias, T, _ = ops.sgns_alias(_power_law(V, seed=2))
    g = torch.Generator().manual_seed(V + N)
    cen, ctx = torch.randint(0, V, (P,), generator=g), torch.randint(0, V, (P,), generator=g)
    seed, epoch, base = (1 << 61) + 99, 5, (1 << 40) + 3
    want = ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch, base, N)
    got = ops.sgns_lookups(cen.to(dev), ctx.to(dev), thr.to(dev), alias.to(dev), T, seed, epoch, base, N)
    assert got.dtype == I64 and torch.equal(got.cpu(), want)
    neg = torch.randint(0, V, (P, N), generator=g, dtype=I32)
    neg[0, 0], cen[0] = V, -1                      # words outside [0, V): the key -1
    want = ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch, base, N, negatives=neg)
    got = ops.sgns_lookups(cen.to(dev), ctx.to(dev), thr.to(dev), alias.to(dev), T, seed, epoch, base, N,
                           negatives=neg.to(dev))
    assert torch.equal(got.cpu(), want) and want[0, 0] == -1 and want[0, 2] == -1


# ------------------------------------------------------------------------------ forward and backward
def _case(d, N, P, seed, cap_extra=5, num_rows=None):
    """P pairs on the CPU: row indices drawn from few rows (duplicates, masked negatives by chance and on purpose),
    some indices out of range, cap > U. Vectors of std d^-1/4: the logits have std 1."""
    g = torch.Generator().manual_seed(seed)
    K2 = N + 2
    num_rows = num_rows or max(4, P * K2 // 4)
    cap = num_rows + cap_extra
    inv = torch.randint(0, num_rows, (P, K2), generator=g)
    inv[P // 2, K2 - 1] = inv[P // 2, 1]           # a masked negative
    if P >= 3:
        inv[1, 2] = -1                             # targets that do not exist
        inv[2, K2 - 1] = cap
        inv[P - 1, 0] = cap + 7                    # a pair without a centre
    inv[0, 0] = num_rows - 1                       # memrow[n - 1] + 1 reaches num_rows
    rows = torch.randn(cap, d, generator=g) * d ** -0.25
    return inv.reshape(-1).contiguous(), rows


def _layout(rows, how, dev):
    """rows on the GPU as a contiguous matrix, a strided view (ld = d + 4: float4 loads still), one whose ld = d + 1
    is no multiple of 4, or a misaligned one (base + 4 bytes); the last two take the one-lane-per-element kernels."""
    cap, W = rows.shape
    if how == "contig":
        return rows.to(dev)
    if how in ("strided", "odd_ld"):
        buf = torch.full((cap, W + (4 if how == "strided" else 1)), float("nan"), device=dev)
        buf[:, :W] = rows.to(dev)
        return buf[:, :W]
    flat = torch.full((cap * W + 1,), float("nan"), device=dev)
    v = flat[1:].view(cap, W)
    v.copy_(rows.to(dev))
    assert v.data_ptr() % 16 == 4
    return v


def _forward64(inv, rows, N, gscale):
    cap, d = rows.shape
    K2 = N + 2
    iv = inv.view(-1, K2)
    a, b = iv[:, 0], iv[:, 1:]
    cen = (a >= 0) & (a < cap)
    ok = cen[:, None] & (b >= 0) & (b < cap)
    ok[:, 1:] &= b[:, 1:] != b[:, :1]
    va, u = rows[a.clamp(0, cap - 1)].double(), rows[b.clamp(0, cap - 1)].double()
    prod = va[:, None, :] * u
    s, sabs = prod.sum(-1), prod.abs().sum(-1)
    y = torch.zeros_like(s)
    y[:, 0] = 1
    e = torch.where(ok, (torch.sigmoid(s) - y) * gscale, torch.zeros_like(s))
    lt = torch.where(ok, s.clamp(min=0) - s * y + torch.log1p(torch.exp(-s.abs())), torch.zeros_like(s))
    bs = (d + 2) * U * sabs
    be = torch.where(ok, gscale * (bs / 4 + 4 * U), torch.zeros_like(s))
    bl = torch.where(ok, bs + 4 * U * (s.abs() + 1), torch.zeros_like(s)).sum(1) + (N + 1) * U * lt.sum(1)
    return dict(s=s, ok=ok, e=e, be=be, loss=lt.sum(1), bloss=bl, u=u)


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - bound).max()) if err.numel() else 0.0
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"  {name}: max err {float(err.max()) if err.numel() else 0.0:.3e}, max err / bound {ratio:.3f}")
    assert worst <= 0, f"{name}: error exceeds the bound by {worst:.3e} (err / bound {ratio:.3f})"


def _csr(inv, cap):
    """The lookup CSR built on the host: rows outside [0, cap) go to a row past the end, which the kernel ignores."""
    r = torch.where((inv >= 0) & (inv < cap), inv, torch.full_like(inv, cap))
    order = torch.sort(r, stable=True).indices
    return order.to(I32), r[order].to(I32)


def _backward64(inv, e, h, rows, N):
    """fp64 of the backward rule on fp32 inputs, its bound per element, and which rows have lookups."""
    cap, d = rows.shape
    K2 = N + 2
    P = inv.numel() // K2
    iv = inv.view(P, K2)
    a = iv[:, 0]
    cen = (a >= 0) & (a < cap)
    g = torch.zeros(cap, d, dtype=torch.float64)
    mag = torch.zeros(cap, d, dtype=torch.float64)
    g.index_add_(0, a[cen], h.double()[cen])
    mag.index_add_(0, a[cen], h.double()[cen].abs())
    b = iv[:, 1:]
    ok = cen[:, None] & (b >= 0) & (b < cap)
    c = e.double()[:, :, None] * rows[a.clamp(0, cap - 1)].double()[:, None, :]
    g.index_add_(0, b[ok], c[ok])
    mag.index_add_(0, b[ok], c[ok].abs())
    inr = inv[(inv >= 0) & (inv < cap)]
    M = torch.zeros(cap, dtype=torch.float64).index_add_(0, inr, torch.ones(inr.numel(), dtype=torch.float64))
    return g, (M + 4)[:, None] * U * mag, M > 0


def _check_backward(inv, rows, N, dev, how="contig", blocks=(0, 1, 7)):
    P = inv.numel() // (N + 2)
    cap, d = rows.shape
    e, loss, h = ops.sgns_forward(inv, rows, N, 1.0 / max(P, 1))  # the fp32 CPU reference
    g64, bound, touched = _backward64(inv, e, h, rows, N)
    members, memrow = _csr(inv, cap)
    rows_d = _layout(rows, how, dev)
    h_d = _layout(h, "misaligned", dev) if how == "misaligned" else h.to(dev)
    outs = []
    for bl in blocks + (blocks[0],):
        grad = _layout(torch.full((cap, d), 7.0), "misaligned" if how == "misaligned" else "contig", dev)
        ops.sgns_backward(inv.to(dev), e.to(dev), h_d, rows_d, N, grad, csr=(members.to(dev), memrow.to(dev)),
                          blocks=bl)
        outs.append(grad)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])  # every grid size and every launch: the same bits
    g = outs[0].cpu()
    _within("grad", g[touched], g64[touched], bound[touched])
    assert bool((g[~touched] == 7.0).all())  # rows without lookups keep the sentinel


CASES = [(d, 5, 257, "contig") for d in (4, 8, 32, 128, 256, 512)] + \
        [(d, N, P, "contig") for d in (4, 32, 512) for N, P in ((1, 1), (64, 3), (1, 3))] + \
        [(d, 5, 257, how) for d in (4, 32, 128, 256, 512) for how in ("strided", "misaligned")] + \
        [(8, 64, 257, "contig"), (128, 64, 3, "misaligned")] + \
        [(d, 5, 257, "misaligned") for d in (8, 16, 64)] + [(d, 5, 257, "odd_ld") for d in (16, 64, 512)]


@pytest.mark.parametrize("d,N,P,how", CASES)
def test_forward_and_backward_against_fp64(d, N, P, how, dev):
    inv, rows = _case(d, N, P, seed=1000 * d + 10 * N + P)
    gscale = 1.0 / P
    ref = _forward64(inv, rows, N, gscale)
    assert float(ref["s"].abs().max()) < 60  # no underflow anywhere
    rows_d = _layout(rows, how, dev)
    outs = [ops.sgns_forward(inv.to(dev), rows_d, N, gscale, blocks=bl) for bl in (0, 1, 7, 0)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(x, y)  # every grid size and every launch: the same bits
    e, loss, h = outs[0]
    print(f"d {d} N {N} P {P} {how}: {int(ref['ok'].sum())} live targets of {P * (N + 1)}")
    assert e.shape == (P, N + 1) and loss.shape == (P,) and h.shape == (P, d)
    _within("e", e, ref["e"], ref["be"])
    assert bool((e.cpu()[~ref["ok"]] == 0).all())  # masked and missing targets: exactly 0
    _within("loss", loss, ref["loss"], ref["bloss"])
    eu = e.cpu().double()[:, :, None] * ref["u"]
    _within("h", h, eu.sum(1), (N + 3) * U * eu.abs().sum(1))
    if P >= 3:  # the pair without a centre
        assert not bool(e[P - 1].any()) and float(loss[P - 1]) == 0.0 and not bool(h[P - 1].any())
    _check_backward(inv, rows, N, dev, how)


def test_csr_built_on_the_device(dev):
    """ops.sgns_backward without a CSR builds it with the plan's kernel: any member order is inside the bound."""
    d, N = 32, 5
    inv, rows = _case(d, N, 40, seed=9)
    e, loss, h = ops.sgns_forward(inv, rows, N, 1.0 / 40)
    g64, bound, touched = _backward64(inv, e, h, rows, N)
    grad = torch.full((rows.shape[0], d), 7.0, device=dev)
    ops.sgns_backward(inv.to(dev), e.to(dev), h.to(dev), rows.to(dev), N, grad)
    g = grad.cpu()
    _within("grad", g[touched], g64[touched], bound[touched])
    assert bool((g[~touched] == 7.0).all())


def _members_case(d, N, counts, seed):
    """Row r has counts[r] member lookups, scattered over the pairs' columns."""
    g = torch.Generator().manual_seed(seed)
    inv = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    n = inv.numel()
    assert n % (N + 2) == 0
    inv = inv[torch.randperm(n, generator=g)]
    rows = torch.randn(len(counts) + 3, d, generator=g) * d ** -0.25
    return inv.contiguous(), rows


@pytest.mark.parametrize("d,how", [(4, "contig"), (32, "contig"), (128, "contig"), (512, "contig"),
                                   (32, "misaligned"), (512, "misaligned")])
def test_backward_member_count_switches(d, how, dev):
    """Both sides of the lane-group | wave switch (32 | 33) and of the wave | workgroup switch (512 | 513); two
    heavy rows side by side (one chunk holds the end of one and the start of the next), a heavy row that starts on
    a chunk boundary (row 0) and light rows between them."""
    counts = [3072, 1, 32, 33, 2, 512, 513, 2500, 31, 64, 5, 511, 1025, 3]
    inv, rows = _members_case(d, 2, counts, seed=d)
    _check_backward(inv, rows, 2, dev, how, blocks=(0, 2))


@pytest.mark.parametrize("how", ["contig", "misaligned"])
@pytest.mark.parametrize("counts", [[513], [3, 513], [513, 3]])
def test_backward_heavy_row_at_the_edges_of_memrow(counts, how, dev):
    """The smallest heavy row as the only row, as the last row after a light one (it ends at n: the last chunk has
    no member after it) and as the first row before a light one."""
    inv, rows = _members_case(8, 1, counts, seed=len(counts) + counts[0])
    _check_backward(inv, rows, 1, dev, how, blocks=(0, 2))


@pytest.mark.parametrize("d", [8, 256])
def test_backward_heavy_input_and_output_rows(d, dev):
    """One batch whose pairs all share one centre -- a heavy input row, every member a col == 0 lookup (h_p) -- and
    one whose negatives are all one word -- a heavy output row of P N members (e v)."""
    g = torch.Generator().manual_seed(d)
    N, P, R = 3, 2100, 50
    rows = torch.randn(R + 2, d, generator=g) * d ** -0.25
    inv = torch.randint(1, R, (P, N + 2), generator=g)
    inv[:, 0] = 0                                   # one centre: 2100 > 512 members
    _check_backward(inv.reshape(-1).contiguous(), rows, N, dev, blocks=(0, 2))
    inv = torch.randint(1, R, (P, N + 2), generator=g)
    inv[:, 2:] = R                                  # one negative word, the last row: 6300 members
    _check_backward(inv.reshape(-1).contiguous(), rows, N, dev, blocks=(0, 2))


def test_empty_inputs_launch_nothing(dev):
    d, N = 8, 3
    rows = torch.zeros(4, d, device=dev)
    e64 = torch.zeros(0, dtype=I64, device=dev)
    e, loss, h = ops.sgns_forward(e64, rows, N, 1.0)
    assert e.shape == (0, N + 1) and loss.shape == (0,) and h.shape == (0, d)
    grad = torch.full((4, d), 7.0, device=dev)
    e32 = torch.zeros(0, dtype=I32, device=dev)
    ops.sgns_backward(e64, e, h, rows, N, grad, csr=(e32, e32))
    thr, alias, T, _ = ops.sgns_alias(torch.ones(4, dtype=I64))
    keys = ops.sgns_lookups(e64, e64, thr.to(dev), alias.to(dev), T, 0, 0, 0, N)
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and keys.shape == (0, N + 2)


# ------------------------------------------------------------------------------ the model
MV, MP = 64, 256


def _models(dev):
    from minips_amd.models.word2vec import Word2Vec, Word2VecConfig
    from minips_amd.ps.comm import Comm

    c = Word2VecConfig(vocab=MV, dim=16, negatives=5, lr=0.05, seed=2)
    cpu, gpu = Word2Vec(c, Comm(device=torch.device("cpu"))), Word2Vec(c, Comm(device=dev))
    gpu.table.shard.copy_(cpu.table.shard.to(dev))
    counts = _power_law(MV, seed=3) + 1
    cpu.set_counts(counts)
    gpu.set_counts(counts)
    return cpu, gpu


def _pairs(step, dev=None):
    g = torch.Generator().manual_seed(100 + step)
    cen, ctx = torch.randint(0, MV, (MP,), generator=g), torch.randint(0, MV, (MP,), generator=g)
    return (cen, ctx) if dev is None else (cen.to(dev), ctx.to(dev))


def test_model_gpu_matches_cpu(dev):
    cpu, gpu = _models(dev)
    assert torch.equal(gpu.thr.cpu(), cpu.thr) and torch.equal(gpu.alias.cpu(), cpu.alias)
    for step in range(3):
        lc = float(cpu.train_step(*_pairs(step), pair_base=step * MP, epoch=1)) / MP
        lg = float(gpu.train_step(*_pairs(step, dev), pair_base=step * MP, epoch=1)) / MP
        print(f"step {step}: cpu {lc:.6f} gpu {lg:.6f}")
        assert abs(lg - lc) <= 3e-3 * max(1.0, abs(lc))
    gpu.drain()
    assert (gpu.vectors().cpu() - cpu.vectors()).abs().max() < 1e-3


def test_steady_step_has_no_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    _, gpu = _models(dev)
    batches = [_pairs(s, dev) for s in range(6)]
    for s, b in enumerate(batches[:3]):  # warm-up: first plans, scratch allocations
        gpu.train_step(*b, pair_base=s * MP)
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for s, b in enumerate(batches[3:]):
            audit.step_begin()
            gpu.train_step(*b, pair_base=(3 + s) * MP)
            audit.step_end()
    rep = audit.report()
    gpu.drain()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep


def test_epoch_on_the_gpu_builds_the_cpu_pairs(dev):
    """make_pairs is integer arithmetic: the GPU's pairs are the CPU's, with and without subsampling."""
    from minips_amd.data.synthetic import W2VSynth
    from minips_amd.models.word2vec import Word2Vec, Word2VecConfig
    from minips_amd.ps.comm import Comm

    s = W2VSynth(4, 8, sentences=40, length=9, seed=2)
    for sample in (0.0, 0.02):
        c = Word2VecConfig(vocab=s.vocab, dim=8, negatives=2, window=3, sample=sample, batch_pairs=128, seed=5)
        cpu, gpu = Word2Vec(c, Comm(device=torch.device("cpu"))), Word2Vec(c, Comm(device=dev))
        for m in (cpu, gpu):
            m.set_counts(s.counts())
            m.attach(*s.corpus(), token_base=77)
        counts = []
        for ep in range(2):
            (cc, co), (gc, go) = cpu.make_pairs(ep), gpu.make_pairs(ep)
            assert torch.equal(gc.cpu(), cc) and torch.equal(go.cpu(), co) and cc.numel() > 0
            counts.append(cc.numel())
        first = gpu.epoch()  # epoch 0: several clocks of 128 pairs
        assert 0 < first <= 3 * math.log(2.0) and gpu.total_pairs == counts[0] > 128


def _w2v_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _w2v_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_match_one_rank(dev):
    many = run_world(_w2v_two_ranks_gpu, world=2)
    one = _w2v_world(0, 1, dev=dev)
    print(f"2 ranks on one card {many[0]} vs one rank {one}")
    assert many[1] == many[0]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert all(math.isfinite(v) for v in many[0])
