"""Word2vec by skip-gram with negative sampling on the sparse PS (minips_amd/models/word2vec.py, ops.sgns_*), CPU
side: the fp32 reference ops against fp64 autograd of the loss written with loops, the integer alias table's exact
identity and the lookups against a Python-integer loop, epoch()'s pairs against a brute-force loop, the start loss,
learning of planted groups, ranks over gloo against one rank, and every refusal and driver flag."""
import json
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import W2VSynth
from minips_amd.models import word2vec as W
from minips_amd.models.word2vec import Word2Vec, Word2VecConfig, purity
from minips_amd.ps.comm import Comm

CPU = torch.device("cpu")
I64, I32 = torch.int64, torch.int32
LN2 = math.log(2.0)


# ------------------------------------------------------------------------------ a. ops against autograd
def _case(d=8, N=3, seed=0):
    """6 pairs over 9 pulled rows (cap 11 > U). Pair 0: plain. Pair 1: negatives 0 and 2 repeat the context's row
    (masked). Pair 2: the centre word is the context word -- different rows (4: input, 5: output). Pairs 3 and 4: the
    same pair twice. Pair 5: a negative's row index out of range (the target does not exist). Row 8 is read by
    nobody; rows 9 and 10 are beyond the unique count."""
    g = torch.Generator().manual_seed(seed)
    inv = torch.tensor([[0, 1, 2, 3, 6],
                        [0, 3, 3, 2, 3],
                        [4, 5, 1, 2, 7],
                        [6, 7, 1, 1, 2],
                        [6, 7, 1, 1, 2],
                        [2, 5, 99, 1, -1]], dtype=I64)[:, : N + 2].contiguous()
    rows = torch.randn(11, d, generator=g) * 0.7
    return inv.reshape(-1), rows


def _loss64(inv, rows64, N, gscale):
    """The loss with explicit loops in fp64: sum over pairs and live targets of logistic(<v, u>, y) * gscale."""
    cap, K2 = rows64.shape[0], N + 2
    total = rows64.new_zeros(())
    for p in range(inv.numel() // K2):
        a = int(inv[p * K2])
        if not 0 <= a < cap:
            continue
        b0 = int(inv[p * K2 + 1])
        for t in range(N + 1):
            b = int(inv[p * K2 + 1 + t])
            if not 0 <= b < cap or (t >= 1 and b == b0):
                continue
            s = (rows64[a] * rows64[b]).sum()
            y = 1.0 if t == 0 else 0.0
            total = total + (s.clamp(min=0) - s * y + torch.log1p(torch.exp(-s.abs()))) * gscale
    return total


@pytest.mark.parametrize("d,N", [(4, 1), (8, 3), (36, 3)])
def test_cpu_ops_match_fp64_autograd(d, N):
    inv, rows = _case(d, N)
    P, gscale = inv.numel() // (N + 2), 1.0 / 6
    e, loss, h = ops.sgns_forward(inv, rows, N, gscale)
    assert e.shape == (P, N + 1) and loss.shape == (P,) and h.shape == (P, d)
    r64 = rows.double().requires_grad_(True)
    total = _loss64(inv, r64, N, gscale)
    total.backward()
    assert abs(float(loss.double().sum()) * gscale - float(total.detach())) < 1e-5
    grad = torch.full((11, d), float("nan"))
    ops.sgns_backward(inv, e, h, rows, N, grad)
    ok = inv[(inv >= 0) & (inv < 11)]
    touched = torch.zeros(11, dtype=torch.bool)
    touched[ok] = True
    assert touched.tolist() == [True] * 8 + [False] * 3
    assert bool(torch.isnan(grad[~touched]).all())           # rows without lookups are untouched
    assert not bool(r64.grad[~touched].any())
    assert (grad[touched].double() - r64.grad[touched]).abs().max() < 1e-6
    iv = inv.view(P, N + 2)
    if N == 3:
        assert e[1, 1] == 0 and e[1, 3] == 0 and e[1, 2] != 0    # masked negatives are exactly 0
        assert e[5, 1] == 0 and e[5, 3] == 0 and e[5, 2] != 0    # targets that do not exist
        assert torch.equal(e[3], e[4]) and torch.equal(h[3], h[4])
    # h is the centre's gradient contribution: sum_t e_t u_t
    for p in range(P):
        want = sum(e[p, t].double() * rows[iv[p, 1 + t].clamp(0, 10)].double() for t in range(N + 1))
        assert (h[p].double() - want).abs().max() < 1e-6


def test_a_centre_out_of_range_contributes_nothing():
    inv, rows = _case(8, 3)
    inv = inv.clone()
    inv[0] = 11                                    # pair 0's centre: one past the rows
    e, loss, h = ops.sgns_forward(inv, rows, 3, 0.5)
    assert not bool(e[0].any()) and loss[0] == 0 and not bool(h[0].any())
    grad = torch.zeros(11, 8)
    ops.sgns_backward(inv, e, h, rows, 3, grad)
    r64 = rows.double().requires_grad_(True)
    _loss64(inv, r64, 3, 0.5).backward()
    assert (grad.double() - r64.grad).abs().max() < 1e-6
    # empty inputs are fine
    e, loss, h = ops.sgns_forward(torch.zeros(0, dtype=I64), rows, 3, 1.0)
    assert e.shape == (0, 4) and h.shape == (0, 8)
    assert ops.sgns_backward(torch.zeros(0, dtype=I64), e, h, rows, 3, grad) is grad


# ------------------------------------------------------------------------------ b. the alias table and the lookups
def _power_law(V, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = (1e6 / torch.arange(1, V + 1, dtype=torch.float64) ** 1.1).long() + torch.randint(0, 3, (V,), generator=g)
    if V >= 7:
        c[torch.tensor([2, V - 1, V // 2])] = 0          # some words never occur
    return c


@pytest.mark.parametrize("V", [1, 2, 7, 1000])
def test_alias_table_is_exact(V):
    c = _power_law(V)
    thr, alias, T, q = ops.sgns_alias(c)
    assert thr.dtype == I64 and alias.dtype == I32 and thr.shape == alias.shape == (V,)
    for w in range(V):
        want = 0 if int(c[w]) == 0 else max(1, round(float(c[w]) ** 0.75 * 2 ** 20))
        assert q[w] == want
    assert T == sum(q) and 1 <= T < 1 << 59
    th, al = thr.tolist(), alias.tolist()
    mass = list(th)
    for i in range(V):
        assert 0 <= th[i] <= T and 0 <= al[i] < V
        mass[al[i]] += T - th[i]
    assert mass == [qw * V for qw in q]                    # thr[w] + sum_{alias[i] == w} (T - thr[i]) == q_w V
    # a word of count 0 is never drawn: nothing of any bucket is its own
    for w in range(V):
        if q[w] == 0:
            assert th[w] == 0 and all(al[i] != w or th[i] == T for i in range(V))


def _mulhi(a, b):
    return (a * b) >> 64


def _lookups_loop(centres, contexts, thr, alias, T, seed, epoch, pair_base, N, negatives=None):
    """sgns.h's draw with Python integers."""
    V = len(thr)
    base = ops.lda_mix_int(seed + epoch * 0x9E3779B97F4A7C15)
    out = []
    for p, (c, o) in enumerate(zip(centres, contexts)):
        words = [c, o]
        for t in range(N):
            if negatives is not None:
                words.append(negatives[p][t])
                continue
            r = ops.lda_mix_int(base ^ ((pair_base + p) * 64 + t))
            i = _mulhi(r, V)
            x = _mulhi(ops.lda_mix_int(r), T)
            words.append(i if x < thr[i] else alias[i])
        out.append([(2 * w + (j > 0)) if 0 <= w < V else -1 for j, w in enumerate(words)])
    return out


@pytest.mark.parametrize("V,N", [(1, 1), (7, 5), (1000, 64)])
def test_lookups_match_the_python_integer_loop(V, N):
    c = _power_law(V, seed=1)
    thr, alias, T, q = ops.sgns_alias(c)
    g = torch.Generator().manual_seed(V)
    P = 37
    cen, ctx = torch.randint(0, V, (P,), generator=g), torch.randint(0, V, (P,), generator=g)
    seed, epoch, base = (1 << 61) + 12345, 3, (1 << 33) + 7
    keys = ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch, base, N)
    assert keys.dtype == I64 and keys.shape == (P, N + 2)
    assert keys.tolist() == _lookups_loop(cen.tolist(), ctx.tolist(), thr.tolist(), alias.tolist(), T, seed, epoch,
                                          base, N)
    drawn = set(((keys[:, 2:] - 1) // 2).reshape(-1).tolist())
    assert not any(q[w] == 0 for w in drawn)
    # another epoch and another pair_base draw other negatives (V large enough to tell)
    if V == 1000:
        assert not torch.equal(keys, ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch + 1, base, N))
        assert not torch.equal(keys, ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch, base + 1, N))
    # explicit negatives replace the draws; a word outside [0, V) gives the key -1
    neg = torch.randint(0, V, (P, N), generator=g, dtype=I32)
    neg[0, 0], cen[1] = V, -1
    keys = ops.sgns_lookups(cen, ctx, thr, alias, T, seed, epoch, base, N, negatives=neg)
    assert keys.tolist() == _lookups_loop(cen.tolist(), ctx.tolist(), thr.tolist(), alias.tolist(), T, seed, epoch,
                                          base, N, neg.tolist())
    assert keys[0, 2] == -1 and keys[1, 0] == -1


def test_draws_follow_the_unigram_power():
    """The frequency of word w among 2^18 draws is q_w / T within 5 binomial standard deviations."""
    c = torch.tensor([1000, 0, 10, 100, 1, 500, 50])
    thr, alias, T, q = ops.sgns_alias(c)
    P, N = 4096, 64
    z = torch.zeros(P, dtype=I64)
    keys = ops.sgns_lookups(z, z, thr, alias, T, 5, 0, 0, N)
    got = torch.bincount(((keys[:, 2:] - 1) // 2).reshape(-1), minlength=7).double()
    n = P * N
    for w in range(7):
        pw = q[w] / T
        assert abs(float(got[w]) - n * pw) <= 5 * math.sqrt(n * pw * (1 - pw)), (w, got, q)


# ------------------------------------------------------------------------------ c. pair generation
def _model(V=12, d=8, N=2, window=3, sample=0.0, batch_pairs=16, seed=4, **kw):
    return Word2Vec(Word2VecConfig(vocab=V, dim=d, negatives=N, window=window, sample=sample, batch_pairs=batch_pairs,
                                   seed=seed, **kw), Comm(device=CPU))


def _pairs_loop(tokens, rowptr, keep, window, seed, epoch, token_base):
    """make_pairs with Python integers: subsample, then every kept token with the up to b kept tokens before and
    after it in its sentence, b = 1 + mulhi(mix(r), window); ordered by centre, then by offset."""
    tb = W.token_base(seed, epoch)
    cen, ctx = [], []
    for s in range(len(rowptr) - 1):
        kept = []
        for i in range(rowptr[s], rowptr[s + 1]):
            r = ops.lda_mix_int(tb ^ (token_base + i))
            if (r >> 32) <= keep[tokens[i]]:
                kept.append((tokens[i], 1 + _mulhi(ops.lda_mix_int(r), window)))
        for i, (w, b) in enumerate(kept):
            for o in list(range(-b, 0)) + list(range(1, b + 1)):
                if 0 <= i + o < len(kept):
                    cen.append(w)
                    ctx.append(kept[i + o][0])
    return cen, ctx


@pytest.mark.parametrize("sample", [0.0, 0.05])
def test_epoch_pairs_match_the_brute_force_loop(sample):
    tokens = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6])
    rowptr = torch.tensor([0, 9, 10, 21])            # the middle sentence has length 1
    m = _model(sample=sample)
    m.set_counts(torch.bincount(tokens, minlength=12))
    m.attach(tokens, rowptr, token_base=1000)
    keep = m.keep.tolist()
    dropped = 0
    for ep in range(3):
        cen, ctx = m.make_pairs(ep)
        want = _pairs_loop(tokens.tolist(), rowptr.tolist(), keep, 3, 4, ep, 1000)
        assert (cen.tolist(), ctx.tolist()) == want
        tb = W.token_base(4, ep)
        dropped += sum((ops.lda_mix_int(tb ^ (1000 + i)) >> 32) > keep[int(tokens[i])] for i in range(21))
    if sample == 0.0:
        assert dropped == 0 and all(k == (1 << 32) - 1 for k in keep)
    else:
        assert dropped > 0                               # this sample does drop tokens
    # the threshold is word2vec's (sqrt(f / s) + 1) s / f in fp64, clamped to 1
    if sample:
        c = torch.bincount(tokens, minlength=12).double()
        for w in range(12):
            f = float(c[w]) / 21
            p = 1.0 if f == 0 else min(1.0, (math.sqrt(f / sample) + 1) * sample / f)
            assert keep[w] == min((1 << 32) - 1, math.floor(p * 2 ** 32))


# ------------------------------------------------------------------------------ d. the start loss
def test_start_loss_is_n_plus_one_ln2():
    """The output vectors start at zero, so every s_t = 0: a clock without masked negatives has the mean pair loss
    (N + 1) ln 2; a masked negative makes it smaller by ln 2."""
    V, N, P = 12, 4, 10
    m = _model(V=V, N=N)
    g = torch.Generator().manual_seed(0)
    cen, ctx = torch.randint(0, V, (P,), generator=g), torch.randint(0, V, (P,), generator=g)
    neg = ((ctx[:, None] + 1 + torch.randint(0, V - 1, (P, N), generator=g)) % V).to(I32)   # never the context word
    assert not bool((neg == ctx[:, None]).any())
    loss = float(m.train_step(cen, ctx, negatives=neg)) / P
    assert abs(loss - (N + 1) * LN2) <= 1e-5         # fp32 rounding of 50 terms of ln 2
    m2 = _model(V=V, N=N)
    neg[3, 1] = ctx[3]
    loss2 = float(m2.train_step(cen, ctx, negatives=neg)) / P
    assert abs(loss2 - ((N + 1) * LN2 - LN2 / P)) <= 1e-5
    # the output rows are zero and the input rows are not
    vec = m2.table.get_rows(torch.arange(2 * V))
    assert bool(vec[0::2].abs().sum(1).gt(0).all())


def test_output_rows_start_at_zero():
    m = _model()
    rows = m.table.get_rows(torch.arange(24))
    assert not bool(rows[1::2].any()) and bool(rows[0::2].abs().sum(1).gt(0).all())
    assert torch.equal(m.vectors(), rows[0::2])
    near = m.most_similar([0, 5], 3)
    assert near.shape == (2, 3) and 0 not in near[0].tolist() and 5 not in near[1].tolist()


# ------------------------------------------------------------------------------ e. it learns
GROUPS, PER, EPOCHS = 8, 16, 4
# purity after EPOCHS epochs on the CPU with sampler seeds 0 .. 4 (measured, see the docstring below)
MEASURED_PURITY = (1.0, 1.0, 1.0, 1.0, 1.0)


def _learn(seed, dev=CPU):
    s = W2VSynth(GROUPS, PER, sentences=512, length=16, seed=0)
    m = Word2Vec(Word2VecConfig(vocab=s.vocab, dim=16, negatives=5, window=3, sample=0.0, batch_pairs=1024,
                                seed=seed), Comm(device=dev))
    m.set_counts(s.counts())
    m.attach(*s.corpus())
    losses = [m.epoch() for _ in range(EPOCHS)]
    return losses, purity(m.vectors(), PER)


@pytest.mark.parametrize("seed", [0, 3])
def test_it_learns_the_planted_groups(seed):
    """W2VSynth(8 groups x 16 words, 512 sentences of 16), d = 16, N = 5, window 3, 4 epochs of clocks of 1024 pairs.
    Purity (the share of words whose nearest cosine neighbour lies in their own group) measured on the CPU over the
    sampler seeds 0 .. 4: 1.0, 1.0, 1.0, 1.0, 1.0. The bar is 0.9 times the lowest, 0.9; chance is 15 / 127 = 0.118,
    so the bar exceeds 4 x chance = 0.472."""
    bar = 0.9 * min(MEASURED_PURITY)
    assert bar > 4 * (PER - 1) / (GROUPS * PER - 1)
    losses, pur = _learn(seed)
    print(f"seed {seed}: losses {losses}, purity {pur}")
    assert losses[-1] < losses[0] <= 6 * LN2
    assert pur >= bar


# ------------------------------------------------------------------------------ f. ranks
RV, RD, RN, RP = 40, 8, 3, 48


def _init_rows(m):
    """The same routed-space table at every world size (a table's own init is seeded per rank)."""
    t = m.table
    g = torch.Generator().manual_seed(5)
    full = torch.zeros(2 * RV, RD)
    full[t._route_keys(torch.arange(0, 2 * RV, 2))] = torch.randn(RV, RD, generator=g) * 0.3
    t.shard[: t.rows_local].copy_(full[t.base: t.base + t.rows_local])


def _w2v_world(rank, world, steps=5, dev=CPU):
    torch.set_num_threads(1)
    comm = Comm(device=dev)
    m = Word2Vec(Word2VecConfig(vocab=RV, dim=RD, negatives=RN, lr=0.1, seed=9), comm)
    _init_rows(m)
    g = torch.Generator().manual_seed(2)
    m.set_counts(torch.randint(1, 50, (RV,), generator=g))
    per = RP // world
    losses = []
    cen, ctx = (torch.randint(0, RV, (RP,), generator=g).to(dev) for _ in range(2))  # one pair list
    for step in range(steps):
        lo, hi = rank * per, (rank + 1) * per
        t = m.train_step(cen[lo:hi], ctx[lo:hi], pair_base=7 + lo, epoch=1).clone()   # the negatives coincide
        comm.all_reduce_(t)
        losses.append(float(t) / RP)
    m.drain()
    return losses


@pytest.mark.parametrize("world", [2, 4])
def test_w2v_ranks_match_one_rank(world):
    many = run_world(_w2v_world, world=world)
    one = _w2v_world(0, 1)
    print(f"world {world}: {many[0]} vs one rank {one}")
    for r in range(1, world):
        assert many[r] == many[0]  # the all-reduced loss is identical on every rank
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert one[-1] < one[0]


def _epoch_world(rank, world):
    """Rank 1 holds no sentence: it still runs every clock."""
    torch.set_num_threads(1)
    comm = Comm(device=CPU)
    s = W2VSynth(4, 8, sentences=24, length=10, seed=1)
    m = Word2Vec(Word2VecConfig(vocab=s.vocab, dim=8, negatives=2, window=2, sample=0.0, batch_pairs=64, seed=1), comm)
    m.set_counts(s.counts())
    tokens, rp = s.corpus()
    if rank == 0:
        m.attach(tokens, rp)
    else:
        m.attach(tokens[:0], rp[:1], token_base=tokens.numel())
    loss = [m.epoch(), m.epoch()]
    m.drain()
    return loss, m.pairs, m.total_pairs


def test_epoch_with_a_rank_without_sentences():
    out = run_world(_epoch_world, world=2)
    one = _epoch_world(0, 1)
    assert out[1][1] == 0 and out[0][1] == out[0][2] == out[1][2] == one[2] > 64   # several clocks
    assert out[0][0] == out[1][0] and all(math.isfinite(v) for v in out[0][0])
    assert out[0][0][1] < out[0][0][0] <= 3 * LN2


# ------------------------------------------------------------------------------ g. refusals
@pytest.mark.parametrize("kw", [dict(dim=0), dict(dim=6), dict(dim=516), dict(negatives=0), dict(negatives=65),
                                dict(window=0), dict(window=65), dict(sample=-0.1), dict(sample=1.0),
                                dict(sample=float("nan")), dict(batch_pairs=0), dict(batch_pairs=1 << 30),
                                dict(transport="onesided"), dict(storage="hash"), dict(vocab=0),
                                dict(value_dtype=torch.bfloat16), dict(pull_dtype=torch.bfloat16)])
def test_config_refusals_name_w2v(kw):
    with pytest.raises(ValueError, match="w2v"):
        Word2VecConfig(**kw)


def test_model_refusals_name_w2v(monkeypatch):
    m = _model()
    tokens, rp = torch.tensor([1, 2, 3]), torch.tensor([0, 3])
    with pytest.raises(ValueError, match="w2v.*set_counts"):
        m.attach(tokens, rp)
    with pytest.raises(ValueError, match="w2v.*set_counts"):
        m.epoch()
    with pytest.raises(ValueError, match="w2v.*set_counts"):
        m.train_step(tokens, tokens)
    with pytest.raises(ValueError, match="w2v"):
        m.set_counts(torch.ones(5, dtype=I64))                      # not V counts
    with pytest.raises(ValueError, match="w2v"):
        m.set_counts(torch.zeros(12, dtype=I64))                     # nothing to draw from
    big = torch.zeros(12, dtype=I64)
    big[0] = 1 << 40
    with pytest.raises(ValueError, match="w2v.*2\\^40"):
        m.set_counts(big)
    m.set_counts(torch.ones(12, dtype=I64))
    with pytest.raises(ValueError, match="w2v.*attach"):
        m.epoch()
    with pytest.raises(ValueError, match="w2v.*vocab"):
        m.attach(torch.tensor([1, 12]), torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="w2v.*vocab"):
        m.attach(torch.tensor([-1, 2]), torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="w2v.*ascend"):
        m.attach(tokens, torch.tensor([0, 2, 1, 3]))
    with pytest.raises(ValueError, match="w2v.*ascend"):
        m.attach(tokens, torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="w2v.*2\\^40"):
        m.attach(tokens, rp, token_base=(1 << 40) - 2)


def test_gpu_tensors_need_the_extension(monkeypatch):
    """A GPU tensor without the extension is an error, never a fall-back to the reference."""
    import minips_amd.ops as O

    def missing():
        raise RuntimeError("minips_amd._w2vk is not built")

    monkeypatch.setattr(O, "w2vk", missing)
    monkeypatch.setattr(O, "_gpu", lambda t: True)
    inv, rows = _case(8, 3)
    e, h = torch.zeros(6, 4), torch.zeros(6, 8)
    thr, alias, T, _ = ops.sgns_alias(torch.ones(4, dtype=I64))
    z = torch.zeros(3, dtype=I64)
    for call in (lambda: O.sgns_forward(inv, rows, 3, 1.0),
                 lambda: O.sgns_backward(inv, e, h, rows, 3, torch.zeros(11, 8), csr=(inv.int(), inv.int())),
                 lambda: O.sgns_lookups(z, z, thr, alias, T, 0, 0, 0, 2)):
        with pytest.raises(RuntimeError, match="_w2vk"):
            call()


def test_cpu_ops_refuse_bad_arguments():
    inv, rows = _case(8, 3)
    with pytest.raises(RuntimeError, match="sgns_forward"):
        ops.sgns_forward(inv, rows, 0, 1.0)
    with pytest.raises(RuntimeError, match="sgns_forward"):
        ops.sgns_forward(inv, rows, 65, 1.0)
    with pytest.raises(RuntimeError, match="sgns_forward"):
        ops.sgns_forward(inv, rows[:, :6], 3, 1.0)
    with pytest.raises(RuntimeError, match="sgns_forward"):
        ops.sgns_forward(inv[:-1], rows, 3, 1.0)
    e, loss, h = ops.sgns_forward(inv, rows, 3, 1.0)
    with pytest.raises(RuntimeError, match="sgns_backward"):
        ops.sgns_backward(inv, e, h, rows, 3, torch.zeros(11, 12))
    with pytest.raises(RuntimeError, match="sgns_backward"):
        ops.sgns_backward(inv, e[:, :3], h, rows, 3, torch.zeros(11, 8))
    thr, alias, T, _ = ops.sgns_alias(torch.ones(4, dtype=I64))
    z = torch.zeros(3, dtype=I64)
    with pytest.raises(RuntimeError, match="sgns_lookups"):
        ops.sgns_lookups(z, z, thr, alias, T, 0, 0, 0, 65)
    with pytest.raises(RuntimeError, match="sgns_lookups"):
        ops.sgns_lookups(z, z, thr, alias[:3], T, 0, 0, 0, 2)
    with pytest.raises(RuntimeError, match="sgns_lookups"):
        ops.sgns_lookups(z, z, thr, alias, T, 0, 0, 0, 2, negatives=torch.zeros(3, 3, dtype=I32))


# ------------------------------------------------------------------------------ h. the driver
def test_synth_is_what_it_says():
    s = W2VSynth(4, 8, sentences=2000, length=10, noise=0.2, seed=3)
    tokens, rp = s.corpus()
    assert tokens.shape == (20000,) and rp.tolist() == list(range(0, 20001, 10)) and s.vocab == 32
    own = (tokens.view(2000, 10) // 8) == s.group[:, None]
    # a token is in its sentence's block with probability 1 - noise + noise / groups = 0.85
    assert abs(float(own.double().mean()) - 0.85) < 5 * math.sqrt(0.85 * 0.15 / 20000)
    assert torch.equal(s.counts(), torch.bincount(tokens, minlength=32))
    assert torch.equal(W2VSynth(4, 8, 2000, 10, 0.2, seed=3).tokens, tokens)
    with pytest.raises(ValueError, match="W2VSynth"):
        W2VSynth(0, 8)


def test_driver_flags():
    from minips_amd.train import parse

    a = parse(["--model", "w2v", "--steps", "3", "--w2v_dim", "32", "--w2v_negatives", "7", "--w2v_window", "4",
               "--w2v_sample", "0.01", "--w2v_vocab", "512", "--w2v_sentences", "100", "--w2v_len", "12", "--batch",
               "500"])
    assert (a.model, a.w2v_dim, a.w2v_negatives, a.w2v_window, a.w2v_sample, a.w2v_vocab, a.w2v_sentences, a.w2v_len,
            a.batch) == ("w2v", 32, 7, 4, 0.01, 512, 100, 12, 500) and a.transport == "collective"
    a = parse(["--model", "w2v", "--small", "1"])
    assert (a.w2v_dim, a.w2v_negatives, a.w2v_window, a.w2v_sample, a.w2v_vocab, a.w2v_sentences, a.w2v_len) == \
        (16, 5, 5, 1e-3, 128, 512, 16)
    assert parse(["--model", "w2v", "--input", "x.libsvm"]).w2v_vocab is None
    for bad in (["--model", "w2v", "--w2v_dim", "6"], ["--model", "w2v", "--w2v_dim", "516"],
                ["--model", "w2v", "--w2v_negatives", "0"], ["--model", "w2v", "--w2v_negatives", "65"],
                ["--model", "w2v", "--w2v_window", "0"], ["--model", "w2v", "--w2v_sample", "1"],
                ["--model", "w2v", "--w2v_sample", "-1"], ["--model", "w2v", "--w2v_vocab", "100"],
                ["--model", "w2v", "--w2v_sentences", "0"], ["--model", "w2v", "--w2v_len", "0"],
                ["--model", "w2v", "--input", "x.libsvm", "--w2v_sentences", "10"],
                ["--model", "w2v", "--input", "x.libsvm", "--w2v_len", "10"],
                ["--model", "w2v", "--transport", "onesided"],
                ["--model", "w2v", "--transport", "onesided", "--consistency", "ssp"],
                ["--model", "w2v", "--transport", "onesided", "--consistency", "asp"],
                ["--model", "w2v", "--kStorageType", "Map"], ["--model", "w2v", "--value_dtype", "float64"],
                ["--model", "w2v", "--value_dtype", "bfloat16"], ["--model", "w2v", "--eval_every", "5"],
                ["--model", "fm", "--w2v_dim", "16"], ["--model", "lr", "--w2v_negatives", "5"],
                ["--model", "widedeep", "--w2v_window", "3"], ["--model", "lda", "--w2v_sample", "0.1"],
                ["--model", "gbdt", "--w2v_vocab", "64"], ["--model", "lr", "--w2v_sentences", "10"],
                ["--model", "kmeans", "--w2v_len", "8"]):
        with pytest.raises(SystemExit):
            parse(bad)


def test_driver_runs_w2v_on_the_synthetic_corpus(capsys):
    from minips_amd.train import main

    assert main(["--model", "w2v", "--small", "1", "--steps", "11", "--w2v_window", "3", "--w2v_sample", "0", "--batch",
                 "1024", "--seed", "3"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "w2v" and out["w2v_dim"] == 16 and out["w2v_pairs"] > 512 * 16
    assert [it for it, _ in out["losses"]] == [9, 10]          # the driver reports every tenth and the last epoch
    assert all(0 < lv < 6 * LN2 for _, lv in out["losses"])    # below the start loss (N + 1) ln 2
    assert out["w2v_purity"] > 4 * 15 / 127


def test_driver_runs_w2v_on_a_libsvm_file(tmp_path, capsys):
    from minips_amd.train import main

    g = torch.Generator().manual_seed(1)
    lines = []
    for s in range(60):  # two planted groups over the words 1..10 and 11..20 (libsvm ids are 1-based), file order
        base = 1 if s % 2 else 11
        lines.append("0 " + " ".join(f"{w}:1" for w in (base + torch.randint(0, 10, (8,), generator=g)).tolist()))
    path = tmp_path / "sents.libsvm"
    path.write_text("\n".join(lines) + "\n")
    assert main(["--model", "w2v", "--input", str(path), "--w2v_dim", "8", "--w2v_negatives", "3", "--w2v_window", "2",
                 "--w2v_sample", "0", "--steps", "11", "--batch", "256"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["model"] == "w2v" and out["w2v_dim"] == 8 and "w2v_purity" not in out
    # 60 sentences of 8 tokens, window <= 2: between 2 * 7 and 2 * (7 + 6) pairs a sentence
    assert 60 * 14 <= out["w2v_pairs"] <= 60 * 26
    assert all(0 < lv < 4 * LN2 for _, lv in out["losses"])    # below the start loss (N + 1) ln 2
