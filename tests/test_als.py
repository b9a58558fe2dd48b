"""ALS on the sparse PS (CPU): ops.als_* against an fp64 loop, the model's objective and held-out error against an
fp64 ALS run here on the same data and start, ranks over gloo, checkpoints and refusals."""
import math

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import MFSynth
from minips_amd.models.als import ALS, ALSConfig, transpose_csr
from minips_amd.ps.comm import Comm

CPU = torch.device("cpu")
I64 = torch.int64


def systems64(rowptr, inv, a, c, rows, reg, gram0=None):
    """The rule of csrc/kernels/als.h as an fp64 loop: [(A, b, contributing lookups)] per entity."""
    cap, k = rows.shape
    out = []
    for e in range(rowptr.numel() - 1):
        A = torch.zeros(k, k, dtype=torch.float64) if gram0 is None else gram0.double().clone()
        b, n = torch.zeros(k, dtype=torch.float64), 0
        for j in range(int(rowptr[e]), int(rowptr[e + 1])):
            if 0 <= int(inv[j]) < cap:
                y = rows[int(inv[j])].double()
                A += float(a[j]) * torch.outer(y, y)
                b += float(c[j]) * y
                n += 1
        out.append((A + float(reg[e]) * torch.eye(k, dtype=torch.float64), b, n))
    return out


def case(k, counts, seed, cap_extra=5):
    """Entities with ``counts`` lookups: rows drawn from few rows (duplicates), two indices out of range, cap > the
    rows in use, reg = 0.05 n (at least 0.05), slots a permutation into a longer x_old."""
    g = torch.Generator().manual_seed(seed)
    rowptr = torch.tensor([0] + counts, dtype=I64).cumsum(0)
    n, B = int(rowptr[-1]), len(counts)
    used = max(4, n // 3)
    inv = torch.randint(0, used, (n,), generator=g)
    if n >= 3:
        inv[1], inv[n - 1] = -1, used + cap_extra
    rows = torch.randn(used + cap_extra, k, generator=g) * k ** -0.25
    a, c = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    reg = 0.05 * torch.tensor(counts, dtype=torch.float32).clamp(min=1.0)
    return dict(rowptr=rowptr, inv=inv, a=a, c=c, rows=rows, reg=reg, slot=torch.randperm(B, generator=g),
                x_old=torch.randn(B + 2, k, generator=g), k=k)


def run(cs, dev=CPU, rows=None, chunk=4096, gram0=None, blocks=0):
    """ops.als_solve on ``dev``: (x_out, delta, bad) on the CPU; the rows of no slot keep their fill, 7."""
    t = {name: v.to(dev) for name, v in cs.items() if name != "k"}
    x_out, delta = torch.full_like(t["x_old"], 7.0), torch.full_like(t["x_old"], 7.0)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    desc, multi, nmd = ops.als_chunks(cs["rowptr"], chunk)
    ops.als_solve(t["rowptr"], t["inv"], t["a"], t["c"], t["rows"] if rows is None else rows, t["reg"], t["slot"],
                  t["x_old"], x_out, delta, (desc.to(dev), multi.to(dev), nmd),
                  gram0=None if gram0 is None else gram0.to(dev), bad=bad, blocks=blocks)
    return x_out.cpu(), delta.cpu(), int(bad)


@pytest.mark.parametrize("implicit", [False, True])
def test_cpu_reference_matches_the_fp64_loop(implicit):
    cs = case(8, [5, 0, 17, 1, 9], seed=3)
    gram0 = ops.als_gram(cs["rows"]) if implicit else None
    x_out, delta, bad = run(cs, gram0=gram0)
    if implicit:
        assert torch.allclose(gram0.double(), cs["rows"].double().t() @ cs["rows"].double(), rtol=1e-5, atol=1e-5)
    for e, (A, b, n) in enumerate(systems64(cs["rowptr"], cs["inv"], cs["a"], cs["c"], cs["rows"], cs["reg"], gram0)):
        s = int(cs["slot"][e])
        if n == 0:  # the empty entity is skipped
            assert torch.equal(x_out[s], cs["x_old"][s]) and not delta[s].any()
            continue
        assert torch.allclose(x_out[s].double(), torch.linalg.solve(A, b), rtol=1e-4, atol=1e-5), e
        assert torch.equal(delta[s], x_out[s] - cs["x_old"][s])
    assert bad == 0 and bool((x_out[5:] == 7.0).all())               # rows of no slot are left alone


def test_a_failed_factorisation_is_skipped_and_counted():
    cs = case(4, [4, 4], seed=1)
    cs["a"][:4], cs["reg"][0] = -1.0, 0.0
    x_out, delta, bad = run(cs)
    s, t = int(cs["slot"][0]), int(cs["slot"][1])
    assert bad == 1 and torch.equal(x_out[s], cs["x_old"][s]) and not delta[s].any() and delta[t].any()


# ------------------------------------------------------------------------------ the model
SYN = dict(users=256, items=128, k_teacher=4, per_user=24, noise=0.1, seed=0)


def _attach(m, synth, rank=0, world=1):
    rp, cols, vals = synth.csr()
    tp, rows, tv = transpose_csr(rp, cols, vals, synth.items)
    for attach, p, c, v, n in ((m.attach_users, rp, cols, vals, synth.users),
                               (m.attach_items, tp, rows, tv, synth.items)):
        lo, hi = rank * n // world, (rank + 1) * n // world
        attach(p[lo:hi + 1] - p[lo], c[int(p[lo]):int(p[hi])], v[int(p[lo]):int(p[hi])], lo)
    return m


def _init_rows(m, std=0.1):
    """The same table at every world size (a table's own init is seeded per rank)."""
    t = m.table
    full = torch.randn(t.num_rows, t.width, generator=torch.Generator().manual_seed(5)) * std
    t.shard[: t.rows_local].copy_(full[t.base: t.base + t.rows_local].to(t.shard.device))
    return full


def als64(full, synth, cfg, sweeps):
    """ALS-WR in fp64 with torch.linalg.solve, an entity at a time, from the start ``full``."""
    W = full.double().clone()
    rp, cols, vals = synth.csr()
    tp, rows, tv = transpose_csr(rp, cols, vals, synth.items)
    eye = torch.eye(cfg.k, dtype=torch.float64)
    for _ in range(sweeps):
        for p, c, v, key0, other0 in ((rp, cols, vals, 0, cfg.users), (tp, rows, tv, cfg.users, 0)):
            for e in range(p.numel() - 1):
                lo, hi = int(p[e]), int(p[e + 1])
                if hi > lo:
                    Y = W[c[lo:hi] + other0]
                    W[key0 + e] = torch.linalg.solve(Y.t() @ Y + cfg.reg * (hi - lo) * eye, Y.t() @ v[lo:hi].double())
    return W


@pytest.mark.parametrize("implicit", [False, True])
def test_objective_never_rises_and_heldout_error_matches_fp64(implicit):
    synth = MFSynth(**SYN)
    if implicit:
        synth.vals = synth.vals.abs()
    cfg = ALSConfig(users=256, items=128, k=8, reg=0.05, implicit=implicit, alpha=4.0, batch_entities=100, seed=1)
    m = _attach(ALS(cfg, Comm(device=CPU)), synth)
    full = _init_rows(m)
    obj = [m.objective()]
    for _ in range(2 if implicit else 4):
        for side in ("users", "items"):
            m.half_sweep(side)
            obj.append(m.objective())
    m.drain()
    print("objective per half-sweep:", [round(o, 4) for o in obj])
    for before, after in zip(obj, obj[1:]):
        assert after <= before * (1 + 1e-5), obj
    assert m.bad_total == 0 and obj[-1] < obj[0]
    if not implicit:
        (u, i, r), W = synth.holdout(0), als64(full, synth, cfg, 4)
        ref = math.sqrt(float((((W[u] * W[i + cfg.users]).sum(1) - r.double()) ** 2).mean()))
        got = m.rmse(u, i, r)
        print(f"held-out rmse after 4 sweeps: model {got:.5f}, fp64 loop {ref:.5f}")
        assert got <= 1.05 * ref


def _als_world(rank, world, dev=CPU):
    torch.set_num_threads(1)
    comm = Comm(device=dev)
    synth = MFSynth(users=64, items=48, k_teacher=3, per_user=12, noise=0.1, seed=2)
    m = ALS(ALSConfig(users=64, items=48, k=8, reg=0.05, batch_entities=10), comm)
    _attach(m, synth, rank, world)
    _init_rows(m)
    out = []
    for _ in range(2):
        m.sweep()
        out.append(m.rmse(*synth.holdout(1)))
    m.drain()
    return out + [float(m.bad_total)]


@pytest.mark.parametrize("world", [2, 4])
def test_als_ranks_match_one_rank(world):
    many = run_world(_als_world, world=world)
    one = _als_world(0, 1)
    print(f"world {world}: {many[0]} vs one rank {one}")
    for r in range(1, world):
        assert many[r][:2] == many[0][:2]
    for a, b in zip(many[0], one):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], one)
    assert one[2] == 0 and one[1] < one[0] < 1.0


def test_save_restore_is_bit_exact(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    synth = MFSynth(users=64, items=48, k_teacher=3, per_user=12, seed=2)
    a = _attach(ALS(ALSConfig(users=64, items=48, k=8, batch_entities=20, seed=3), Comm(device=CPU)), synth)
    a.sweep()
    a.drain()
    Checkpointer(a.comm, str(tmp_path / "ck_")).save({0: a.table}, iteration=1, blocking=True)
    b = _attach(ALS(ALSConfig(users=64, items=48, k=8, batch_entities=20, seed=9), Comm(device=CPU)), synth)
    assert Checkpointer(b.comm, str(tmp_path / "ck_")).load({0: b.table}) == 1
    assert torch.equal(a.table.shard, b.table.shard)
    a.sweep(), b.sweep()
    a.drain(), b.drain()
    assert torch.equal(a.table.shard, b.table.shard)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=6), dict(k=132), dict(reg=0.0), dict(reg=float("nan")),
                                dict(transport="onesided"), dict(consistency="ssp"), dict(consistency="asp"),
                                dict(staleness=1), dict(storage="hash"), dict(storage="map"),
                                dict(value_dtype=torch.bfloat16), dict(pull_dtype=torch.bfloat16), dict(users=0)])
def test_config_refusals_name_als(kw):
    with pytest.raises(ValueError, match="als"):
        ALSConfig(**kw)


def test_model_and_op_refusals():
    m = ALS(ALSConfig(users=4, items=3, k=4), Comm(device=CPU))
    with pytest.raises(ValueError, match="als.*attach_users"):
        m.sweep()
    with pytest.raises(ValueError, match="als.*ascend"):
        m.attach_users(torch.tensor([0, 2, 1]), torch.tensor([0]), torch.ones(1))
    with pytest.raises(ValueError, match="als.*ids"):
        m.attach_users(torch.tensor([0, 1]), torch.tensor([3]), torch.ones(1))


def test_driver_refusals_and_runs(tmp_path, capsys):
    import json

    from minips_amd.train import main, parse

    als = (["--als_k", "6"], ["--als_k", "132"], ["--als_reg", "0"], ["--transport", "onesided"], ["--eval_every", "2"],
           ["--consistency", "ssp"], ["--kStorageType", "Map"], ["--value_dtype", "bfloat16"])
    other = (["--als_k", "8"], ["--als_reg", "0.1"], ["--als_implicit"], ["--als_alpha", "2"], ["--als_users", "9"],
             ["--als_items", "9"], ["--als_per_user", "3"])
    for argv in [["--model", "als"] + f for f in als] + [["--model", "fm"] + f for f in other]:
        with pytest.raises(SystemExit):
            parse(argv)
    rp, cols, vals = MFSynth(users=40, items=12, k_teacher=2, per_user=6, seed=1).csr()
    path = tmp_path / "ratings.libsvm"   # a line is a user: `label item:rating ...`, ids from 1
    path.write_text("".join("0 " + " ".join(f"{int(cols[j]) + 1}:{float(vals[j]):.4f}" for j in range(rp[u], rp[u + 1]))
                            + "\n" for u in range(40)))
    for argv, k in ((["--small", "1"], 8), (["--input", str(path), "--als_k", "4"], 4)):
        assert main(["--model", "als", "--steps", "3"] + argv) == 0
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["model"] == "als" and out["als_k"] == k and 0 < out["als_rmse"] < 0.5
