"""LDA Gibbs kernels on the GPU (csrc/kernels/lda.hip through minips_amd.ops): every kernel against the CPU
reference of the same rule -- integers, so torch.equal -- on every lane shape, grid size, alignment form and
member-count path, the log likelihood within one unit per token, and the model: a GPU run replayed on the CPU,
two ranks on one card, no host sync."""
import functools

import pytest
import torch

from test_lda import CASES, I16, I64, _lda_world, assert_conserved, corpus, make_case, run_ops
from test_multirank_gpu import run_world

from minips_amd import ops
from minips_amd.models.lda import LDA, LDAConfig
from minips_amd.ps.comm import Comm

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def ragged(B, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, 21, (B,), generator=g).tolist())


# the CPU tests' grid, the document of 4096 tokens at K = 1024, every lane shape (R = 1, 2, 4, 8, 16 topics per
# lane: K <= 64, 128, 256, 512, 1024), and B = 1, 5, 257 documents
GPU_CASES = {
    **CASES,
    "K1024-doc4096": dict(K=1024, lens=(4096,)),
    "K128": dict(K=128, lens=(65, 3)),
    "K200": dict(K=200, lens=(65, 3)),
    "K256": dict(K=256, lens=(65, 3)),
    "K500": dict(K=500, lens=(65, 3)),
    "K512": dict(K=512, lens=(65, 3)),
    "B1": dict(K=16, lens=(37,)),
    "B5": dict(K=16, lens=(3, 0, 20, 1, 64)),
    "B257-K16": dict(K=16, lens=ragged(257, 1), V=50),
    "B257-K256": dict(K=256, lens=ragged(257, 2), V=50),
}


@functools.lru_cache(maxsize=None)
def cpu_ref(name, init=False):
    return run_ops(make_case(**GPU_CASES[name]), init=init)


def assert_same(got, ref):
    for g, r, what in zip(got, ref, ("z_new", "dk", "delta")):
        assert g.dtype == r.dtype and g.shape == r.shape, what
        assert torch.equal(torch.nan_to_num(g.float(), nan=-7.0), torch.nan_to_num(r.float(), nan=-7.0)), what
    assert torch.equal(torch.isnan(got[2]), torch.isnan(ref[2]))


def offset_view(t, dev):
    """The same values on the device at an odd byte offset and an odd leading dimension: t = buf[:, 1:]."""
    buf = torch.zeros(t.shape[0], t.shape[1] + 1, dtype=t.dtype, device=dev)
    buf[:, 1:] = t.to(dev)
    return buf[:, 1:]


# ------------------------------------------------------------------------------ sample
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_sample_equals_the_cpu(name, dev):
    c = make_case(**GPU_CASES[name])
    assert_same(run_ops(c, dev=dev), cpu_ref(name))


@pytest.mark.parametrize("blocks", [1, 3, 300])
@pytest.mark.parametrize("name", ["K3", "K65", "K1024", "B257-K16", "B257-K256"])
def test_sample_equals_the_cpu_on_forced_grids(name, blocks, dev):
    c = make_case(**GPU_CASES[name])
    assert_same(run_ops(c, dev=dev, blocks=blocks), cpu_ref(name))


@pytest.mark.parametrize("name", ["K3", "K65", "K256", "K1024", "B257-K256", "top-of-range"])
def test_sample_equals_the_cpu_on_unaligned_rows(name, dev):
    """rows at a 4-byte offset with an odd leading dimension: the scalar loads, never a refusal."""
    c = make_case(**GPU_CASES[name])
    rows = offset_view(c["rows"], dev)
    assert rows.data_ptr() % 16 == 4 and rows.stride(0) % 2 == 1
    assert_same(run_ops(c, dev=dev, rows=rows), cpu_ref(name))
    # an odd ld alone (the base pointer aligned): K = 65 rows of 68 floats in a buffer of 69
    buf = torch.zeros(c["rows"].shape[0], c["rows"].shape[1] + 1, device=dev)
    buf[:, :-1] = c["rows"].to(dev)
    assert_same(run_ops(c, dev=dev, rows=buf[:, :-1]), cpu_ref(name))


@pytest.mark.parametrize("name", ["K2", "K65", "K1024", "big-doc-ids", "B257-K16"])
def test_initialisation_equals_the_cpu(name, dev):
    c = make_case(**GPU_CASES[name])
    assert_same(run_ops(c, dev=dev, init=True), cpu_ref(name, True))
    assert_same(run_ops(c, dev=dev, init=True, blocks=2), cpu_ref(name, True))


@pytest.mark.parametrize("K", [5, 256])
def test_out_of_range_rows_and_topics_are_skipped(K, dev):
    c = make_case(K=K, lens=(9, 70, 4))
    cap = c["rows"].shape[0]
    c["inv"][2], c["inv"][10], c["inv"][80] = -1, cap, 1 << 40
    c["z_old"][4], c["z_old"][11] = K, -3
    ref = run_ops(c)
    got = run_ops(c, dev=dev)
    assert_same(got, ref)
    for t in (2, 10, 80, 4, 11):
        assert got[0][t] == c["z_old"][t]
    ref0, got0 = run_ops(c, init=True), run_ops(c, dev=dev, init=True)
    assert_same(got0, ref0)
    assert got0[0][2] == -1 and got0[0][80] == -1


# ------------------------------------------------------------------------------ delta
HEAVY_COUNTS = [3000, 2500, 100, 2048, 2049] + [1] * 40


def delta_case(K, seed=0, counts=HEAVY_COUNTS):
    """Rows by member count. HEAVY_COUNTS: 3000 and 2500 (two rows of the chunked workgroup path, side by side, so
    chunks hold the end of one and the start of the other), 100, 2048 (the last of the wave path), 2049 (the first
    of the chunked one), then 40 rows of one member, shuffled over the tokens. Two more rows have no member."""
    g = torch.Generator().manual_seed(seed + K)
    inv = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    inv = inv[torch.randperm(inv.numel(), generator=g)]
    n = inv.numel()
    z_old = torch.randint(0, K, (n,), generator=g).to(I16)
    z_new = torch.randint(0, K, (n,), generator=g).to(I16)
    z_new[::3] = z_old[::3]  # unchanged tokens: explicit zeros
    z_old[5], z_new[9] = -1, K  # a topic outside [0, K) counts nowhere
    return inv, z_old, z_new, len(counts) + 2


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("K", [3, 70, 1024])
def test_delta_equals_the_cpu_on_every_path(K, init, blocks, dev):
    check_delta(K, init, blocks, dev, HEAVY_COUNTS)


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("counts", [[2049], [1, 2049]])
def test_delta_heavy_row_at_the_edges_of_memrow(counts, init, blocks, dev):
    """The smallest row of the chunked path as the only row (every chunk is its own, the first has no member before
    it) and as the last row after a light one (it ends at n: the last chunk has no member after it)."""
    check_delta(3, init, blocks, dev, counts)


def check_delta(K, init, blocks, dev, counts):
    inv, z_old, z_new, cap = delta_case(K, counts=counts)
    W = (K + 3) & ~3
    if init:
        z_old = None
    ref = torch.full((cap, W), float("nan"))
    ops.lda_delta(inv, z_old, z_new, K, ref)
    got = torch.full((cap, W), float("nan"), device=dev)
    ops.lda_delta(inv.to(dev), None if init else z_old.to(dev), z_new.to(dev), K, got, blocks=blocks)
    got = got.cpu()
    # rows without members still hold the NaN, rows with members are fully overwritten (pad columns: 0)
    assert bool(torch.isnan(got[cap - 2:]).all()) and not bool(torch.isnan(got[: cap - 2]).any())
    assert torch.equal(got[: cap - 2], ref[: cap - 2]) and not bool(got[: cap - 2, K:].any())
    if not init:
        assert float(got[: cap - 2, :K].sum(1).abs().max()) <= 1  # -1 and +1 per token (but the two bad topics)


# ------------------------------------------------------------------------------ loglik
@pytest.mark.parametrize("name", ["K3", "K65", "K256", "K1024", "B257-K16", "top-of-range"])
def test_loglik_is_within_one_unit_per_token_of_the_cpu(name, dev):
    c = make_case(**GPU_CASES[name])
    c["nk"] = c["nk"].clamp(min=1)
    n = c["inv"].numel()
    accs = []
    for d, rows in ((CPU, c["rows"]), (dev, c["rows"].to(dev)), (dev, offset_view(c["rows"], dev))):
        acc = torch.zeros(2, dtype=I64, device=d)
        ops.lda_loglik(c["rowptr"].to(d), c["inv"].to(d), c["z_old"].to(d), rows, c["nk"].to(d), c["alpha"],
                       c["beta"], c["Vbeta"], acc)
        accs.append(acc.cpu().tolist())
    print(f"{name}: {n} tokens, CPU {accs[0][0]}, GPU - CPU {accs[1][0] - accs[0][0]} (unaligned rows "
          f"{accs[2][0] - accs[0][0]}) units of 2^-24")
    assert accs[0][1] == accs[1][1] == accs[2][1] == n
    assert abs(accs[1][0] - accs[0][0]) <= n and abs(accs[2][0] - accs[0][0]) <= n


# ------------------------------------------------------------------------------ the model
def run_model(dev, K, batch_docs, sweeps=3):
    rp, w = corpus()
    m = LDA(LDAConfig(num_topics=K, vocab=40, batch_docs=batch_docs, seed=3), Comm(device=dev))
    m.attach(rp.to(dev), w.to(dev), 0)
    m.init()
    trace = [(m.z.cpu().clone(), m.counts().cpu().clone(), m.nk.cpu().clone())]
    for _ in range(sweeps):
        m.sweep()
        trace.append((m.z.cpu().clone(), m.counts().cpu().clone(), m.nk.cpu().clone()))
    return m, trace, w


@pytest.mark.parametrize("K,batch_docs", [(5, 7), (70, 50), (256, 1)])
def test_gpu_run_replays_on_the_cpu_bit_for_bit(K, batch_docs, dev):
    g, tg, w = run_model(dev, K, batch_docs)
    c, tc, _ = run_model(CPU, K, batch_docs)
    for (zg, rg, ng), (zc, rc, nc) in zip(tg, tc):
        assert torch.equal(zg, zc) and torch.equal(rg, rc) and torch.equal(ng, nc)
    assert_conserved(g, w, g.z.cpu())
    lg, lc = g.loglik(), c.loglik()
    print(f"K {K}: loglik GPU {lg:.9f}, CPU {lc:.9f}")
    assert abs(lg - lc) <= 2.0 ** -24
    assert torch.equal(g.top_words(3).cpu(), c.top_words(3))


def test_steady_clock_has_no_host_sync(dev):
    from minips_amd.utils.syncaudit import SyncAudit

    rp, w = corpus(D=200)
    m = LDA(LDAConfig(num_topics=16, vocab=40, batch_docs=64, seed=1), Comm(device=dev))
    m.attach(rp.to(dev), w.to(dev), 0)
    m.init()
    for _ in range(2):  # warm-up: first launches, scratch allocations
        m.sweep()
    torch.cuda.synchronize()
    with SyncAudit() as audit:
        for _ in range(3):
            audit.step_begin()
            m.sweep()  # four clocks
            audit.step_end()
    rep = audit.report()
    assert rep["steps"] == 3 and rep["syncs_per_step"] == 0, rep
    assert m.it == 5
    assert_conserved(m, w, m.z.cpu())


def _lda_two_ranks_gpu(rank, world):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = _lda_world(rank, world, dev=dev)
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_card_equal_one_rank(dev):
    many = run_world(_lda_two_ranks_gpu, world=2)
    one = _lda_world(0, 1, dev=dev)
    assert one == {**_lda_world(0, 1), "loglik": one["loglik"]}  # and the card equals the CPU
    for r in range(2):
        t0, t1 = many[r]["t0"], many[r]["t1"]
        assert many[r]["z0"] == one["z0"][t0:t1] and many[r]["z"] == one["z"][t0:t1], r
        for k in ("nk", "rows", "top"):
            assert many[r][k] == one[k], (r, k)
        assert abs(many[r]["loglik"] - one["loglik"]) <= 2.0 ** -24


def test_empty_inputs_launch_nothing(dev):
    K = 4
    e64 = torch.zeros(0, dtype=I64, device=dev)
    e16 = torch.zeros(0, dtype=I16, device=dev)
    rows = torch.zeros(3, 4, device=dev)
    nk = torch.ones(K, dtype=I64, device=dev)
    dk = torch.full((K,), 5, dtype=I64, device=dev)
    acc = torch.full((2,), 5, dtype=I64, device=dev)
    delta = torch.full((3, 4), 5.0, device=dev)
    for rowptr, gid in ((torch.zeros(1, dtype=I64, device=dev), e64),                      # B == 0
                        (torch.zeros(3, dtype=I64, device=dev), torch.zeros(2, dtype=I64, device=dev))):  # empty docs
        z, _ = ops.lda_sample(rowptr, gid, e64, e16, rows, nk, 0.1, 0.01, 0.04, 1, 1, dk=dk)
        assert z.numel() == 0
        ops.lda_sample(rowptr, gid, e64, None, rows, nk, 0.1, 0.01, 0.04, 1, 0, dk=dk)
        ops.lda_loglik(rowptr, e64, e16, rows, nk, 0.1, 0.01, 0.04, acc)
    ops.lda_delta(e64, e16, e16, K, delta)
    ops.lda_delta(e64, None, e16, K, delta, csr=(torch.zeros(0, dtype=torch.int32, device=dev),) * 2)
    torch.cuda.synchronize()
    assert bool((dk == 5).all()) and bool((acc == 5).all()) and bool((delta == 5).all())
    # a document between two empty ones
    c = make_case(K=4, lens=(0, 3, 0))
    got, ref = run_ops(c, dev=dev), run_ops(c)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
