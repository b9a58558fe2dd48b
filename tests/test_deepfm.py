"""DeepFM on the CPU: the FM interaction term over Wide&Deep's field embeddings (csrc/kernels/deepfm.h states
the rule; ops.wd_fm_forward / ops.wd_fm_backward carry its fp32 references; WideDeepConfig(fm_term=True) runs it).
  references   against fp64 autograd of the pairwise formula sum_{f<g} <v_f, v_g> on bf16-exact inputs
  model        the default is untouched (the ops are never called, no S buffer), evaluate() leaves training
               bit-identical, gloo worlds 2 and 4 equal one rank, checkpoints interchange with Wide&Deep's
  what it buys held-out log loss on FM-teacher labels against plain Wide&Deep
  refusals     the configuration's and the driver's"""
import json
import math
import os

import pytest
import torch

from test_ps_gloo import run_world

from minips_amd import ops
from minips_amd.data.synthetic import CriteoSynth, FMSynth
from minips_amd.models.widedeep import WideDeep, WideDeepConfig
from minips_amd.ps.comm import Comm

BF = torch.bfloat16
CARDS = [50, 7, 300, 20, 5, 60, 90, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28]
HID = (64, 32, 16)


# ---- the references ---------------------------------------------------------------------------------
def _inputs(B, F, D, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.full((B, ldx), float("nan"), dtype=BF)  # columns >= F*D must not be read
    X[:, : F * D] = (torch.randn(B, F * D, generator=g) * 0.5).to(BF)
    wide = torch.randn(B, generator=g)
    dz = torch.randn(B, generator=g)
    return X, wide, dz


def _pairwise64(X, F, D):
    """fm_b = sum_{f<g} <v_f, v_g> in fp64 with autograd, from the definition (no S^2 - q identity)."""
    B = X.shape[0]
    v = X[:, : F * D].double().reshape(B, F, D).clone().requires_grad_(True)
    gram = torch.einsum("bfc,bgc->bfg", v, v)
    fm = torch.triu(gram, diagonal=1).sum((1, 2))
    return v, fm


@pytest.mark.parametrize("B,F,D,ldx", [(5, 4, 8, 40), (3, 26, 32, 896), (7, 3, 12, 36), (2, 9, 64, 600)])
def test_references_against_fp64_autograd(B, F, D, ldx):
    X, wide, dz = _inputs(B, F, D, ldx, seed=B * 100 + F)
    v, fm64 = _pairwise64(X, F, D)
    w0 = wide.clone()
    S = ops.wd_fm_forward(X, F, D, wide)
    assert S.shape == (B, D) and S.dtype == torch.float32
    a = v.detach().abs()
    # fp32 rounding: the forward's own bound (tests/test_deepfm_gpu.py), u = 2^-24
    u = 2.0 ** -24
    A = 0.5 * ((a.sum(1) ** 2).sum(1) + (a * a).sum((1, 2)))
    assert bool(((S.double() - v.detach().sum(1)).abs() <= (F + 2) * u * a.sum(1)).all())
    err = (wide.double() - (w0.double() + fm64.detach())).abs()
    assert bool((err <= (2 * F + D + 16) * u * A + u * wide.abs().double()).all()), err
    # backward with dX = 0: dz (S - v) to one bf16 rounding (2^-8 relative; the fp32 steps are far below it)
    (fm64 * dz.double()).sum().backward()
    dX = torch.zeros(B, F * D, dtype=BF)
    out = ops.wd_fm_backward(X, S, dz, dX, F, D)
    assert out is dX
    g64 = v.grad.reshape(B, F * D)
    mag = (dz.abs().double()[:, None, None] * (S.double().abs()[:, None, :] + a)).reshape(B, F * D)
    assert bool(((dX.double() - g64).abs() <= 2.0 ** -8 * g64.abs() + 8 * u * mag).all())
    # ... and onto a non-zero dX: exactly the stated expression
    g = torch.Generator().manual_seed(1)
    dX0 = torch.randn(B, F * D, generator=g).to(BF)
    dX1 = dX0.clone()
    ops.wd_fm_backward(X, S, dz, dX1, F, D)
    vf = X[:, : F * D].float().reshape(B * F, D)
    want = (dX0.view(B * F, D).float() + dz.repeat_interleave(F)[:, None] * (S.repeat_interleave(F, 0) - vf)).to(BF)
    assert torch.equal(dX1.view(B * F, D), want)


def test_one_field_has_no_interaction():
    X, wide, dz = _inputs(6, 1, 16, 24, seed=2)
    w0 = wide.clone()
    S = ops.wd_fm_forward(X, 1, 16, wide)
    assert torch.equal(wide, w0)  # fm == 0.0 exactly: S^2 - q is v^2 - v^2 per column
    assert torch.equal(S, X[:, :16].float())
    dX = torch.zeros(6, 16, dtype=BF)
    ops.wd_fm_backward(X, S, dz, dX, 1, 16)
    assert bool((dX == 0).all())


def test_perm_is_respected_and_an_out_of_range_entry_is_skipped():
    B, F, D = 4, 5, 8
    X, wide, dz = _inputs(B, F, D, 48, seed=3)
    S = ops.wd_fm_forward(X, F, D, wide)
    n = B * F
    g = torch.Generator().manual_seed(4)
    dX0 = torch.randn(n, D, generator=g).to(BF)  # row i: the gradient of lookup i
    nat = dX0.clone()
    ops.wd_fm_backward(X, S, dz, nat, F, D)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    srt = torch.empty_like(dX0)
    srt[perm.long()] = dX0  # lookup i's gradient lies in row perm[i]
    ops.wd_fm_backward(X, S, dz, srt, F, D, perm=perm)
    assert torch.equal(srt[perm.long()], nat)
    # lookups 3 and 7 point outside [0, n): rows perm[3] and perm[7] are then addressed by nobody and keep
    # their values
    bad = perm.clone()
    bad[3], bad[7] = n, -1
    srt2 = torch.empty_like(dX0)
    srt2[perm.long()] = dX0
    ops.wd_fm_backward(X, S, dz, srt2, F, D, perm=bad)
    keep = torch.ones(n, dtype=torch.bool)
    keep[[3, 7]] = False
    assert torch.equal(srt2[perm.long()][keep], nat[keep])
    assert torch.equal(srt2[perm.long()][~keep], dX0[~keep])


# ---- the model --------------------------------------------------------------------------------------
def _model(fm_term, cards=CARDS, seed=0, **kw):
    return WideDeep(WideDeepConfig(cards=cards, hidden=HID, seed=seed, fm_term=fm_term, **kw),
                    Comm(device=torch.device("cpu")))


def test_default_is_unchanged(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the FM term ran without fm_term")

    monkeypatch.setattr(ops, "wd_fm_forward", boom)
    monkeypatch.setattr(ops, "wd_fm_backward", boom)
    assert WideDeepConfig(cards=CARDS).fm_term is False
    m = _model(False)
    data = CriteoSynth(64, cards=CARDS, seed=3)
    for _ in range(5):
        assert math.isfinite(float(m.train_step(*data.next())))
    m.evaluate(data.holdout(9).next() for _ in range(2))
    m.drain()
    assert all("S" not in b for b in m._bufs.values()) and all("S" not in b for b in m._ebufs.values())
    monkeypatch.undo()
    on = _model(True)
    on.train_step(*CriteoSynth(64, cards=CARDS, seed=3).next())
    assert on._bufs[64]["S"].shape == (64, 32) and on._bufs[64]["S"].dtype == torch.float32


def _state(m):
    out = {}
    for name, t in (("emb", m.emb), ("dense", m.dense)):
        for k, v in t.shard_state()[1].items():
            out[f"{name}.{k}"] = v.detach().cpu().clone()
    return out


def _train(eval_after=(), steps=6):
    m = _model(True)
    data = CriteoSynth(64, cards=CARDS, seed=3)
    losses, evals = [], []
    for it in range(steps):
        losses.append(m.train_step(*data.next()).clone())
        if it + 1 in eval_after:
            held = data.holdout(1000)
            evals.append(m.evaluate(held.next() for _ in range(2)))
    m.drain()
    return torch.stack(losses), _state(m), evals


def test_evaluation_leaves_training_untouched():
    plain, with_eval = _train(), _train(eval_after=(2, 4))
    assert torch.equal(plain[0], with_eval[0])
    assert plain[1].keys() == with_eval[1].keys() and len(plain[1]) >= 3
    for k in plain[1]:
        assert torch.equal(plain[1][k], with_eval[1][k]), k
    assert len(with_eval[2]) == 2 and all(r["n"] == 128 and r["logloss"] > 0 for r in with_eval[2])
    # the term is in the evaluation too: another model than the plain one
    off = _model(False)
    data = CriteoSynth(64, cards=CARDS, seed=3)
    assert not torch.equal(off.train_step(*data.next()), plain[0][0])


PER_RANK = 16


def _wd_fm_run(rank, world, steps=4):
    torch.set_num_threads(1)
    m = _model(True)
    g = torch.Generator().manual_seed(5)
    full = torch.randn(m.num_rows, m.cfg.row_width, generator=g) * 0.1  # (embeddings large enough for the term)
    full[:, m.cfg.emb_dim:] = 0
    m.emb.shard.copy_(full[m.emb.base: m.emb.base + m.emb.rows_local])
    total = PER_RANK * 8
    data = CriteoSynth(total, cards=CARDS, device="cpu", seed=11)
    per = total // world
    losses = []
    for _ in range(steps):
        dense, keys, y = data.next()
        sl = slice(rank * per, (rank + 1) * per)
        t = m.train_step(dense[sl], keys[sl], y[sl]).clone()
        m.comm.all_reduce_(t)
        losses.append(float(t) / total)
    return losses


@pytest.fixture(scope="module")
def fm_one_rank():
    return _wd_fm_run(0, 1)


@pytest.mark.parametrize("world", [2, 4])
def test_several_ranks_match_one_rank(world, fm_one_rank):
    many = run_world(_wd_fm_run, world=world)
    for r in range(1, world):
        assert many[r] == many[0]  # the all-reduced loss is identical on every rank
    print(f"world {world}: {many[0]} vs one rank {fm_one_rank}")
    for a, b in zip(many[0], fm_one_rank):
        assert abs(a - b) <= 3e-3 * max(1.0, abs(b)), (many[0], fm_one_rank)


def test_checkpoints_interchange_with_wide_and_deep(tmp_path):
    from minips_amd.ps.checkpoint import Checkpointer

    data = CriteoSynth(64, cards=CARDS, seed=3)
    batches = [data.next() for _ in range(4)]

    def tables(m):
        return {0: m.emb, 1: m.dense}

    for src, dst in ((False, True), (True, False)):  # a W&D checkpoint into fm_term=True, and back
        prefix = str(tmp_path / f"ck{int(src)}") + os.sep
        a = _model(src)
        for b in batches[:2]:
            a.train_step(*b)
        a.drain()
        Checkpointer(a.comm, prefix).save(tables(a), iteration=2, blocking=True)
        b_ = _model(dst, seed=1)  # other initial values: everything must come from the checkpoint
        assert Checkpointer(b_.comm, prefix).load(tables(b_)) == 2
        sa, sb = _state(a), _state(b_)
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
        # ... and it continues as a model of its own flag trained from that state would
        ref = _model(dst, seed=1)
        Checkpointer(ref.comm, prefix).load(tables(ref))
        assert torch.equal(b_.train_step(*batches[2]), ref.train_step(*batches[2]))


# ---- what it buys -----------------------------------------------------------------------------------
def _fm_teacher_logloss(fm_term, seed=0, steps=100):
    F, card, B = 8, 32, 512
    data = FMSynth(B, fields=F, card=card, seed=seed)
    m = _model(fm_term, cards=[card] * F, seed=seed)

    def batch(gen):
        _, cols, _, y = gen.next()
        return torch.zeros(B, m.cfg.n_dense), cols.view(B, F), y

    for _ in range(steps):
        m.train_step(*batch(data))
    held = data.holdout(777 + seed)
    return m.evaluate(batch(held) for _ in range(8))["logloss"]


def test_what_the_term_buys():
    """Labels of a rank-4 FM teacher over 8 fields of 32 ids, dense input all zero, 100 steps of 512 samples,
    8 held-out batches, seed 0: Wide&Deep learns the crosses only through its MLP."""
    wd, dfm = _fm_teacher_logloss(False), _fm_teacher_logloss(True)
    print(f"held-out log loss: Wide&Deep {wd:.4f}, with the FM term {dfm:.4f} ({dfm / wd:.3f} x)")
    assert dfm < math.log(2) and dfm < 0.6 * wd


# ---- refusals ---------------------------------------------------------------------------------------
def test_config_refusals():
    with pytest.raises(ValueError, match="fm_term"):
        WideDeepConfig(cards=CARDS, fm_term=True, transport="onesided")
    with pytest.raises(ValueError, match="fm_term"):
        WideDeepConfig(cards=CARDS, fm_term=True, consistency="ssp", staleness=1)  # auto resolves to one-sided
    with pytest.raises(ValueError, match="fm_term"):
        WideDeepConfig(cards=CARDS, fm_term=True, consistency="asp", dense_transport="onesided",
                       transport="collective")
    for d in (0, 65, 128):
        with pytest.raises(ValueError, match="fm_term"):
            WideDeepConfig(cards=CARDS, fm_term=True, emb_dim=d, row_width=d + 4)
    WideDeepConfig(cards=CARDS, emb_dim=128, row_width=132)  # without the flag nothing is refused
    c = WideDeepConfig(cards=CARDS, fm_term=True, consistency="ssp", staleness=1, transport="collective",
                       wide_optimizer="ftrl", wide_l1=0.5)
    assert c.fm_term and c.transport == "collective"


def _drive(capsys, monkeypatch, *argv):
    from minips_amd import train

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert train.main(list(argv)) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_driver(capsys, monkeypatch, tmp_path):
    from minips_amd import train

    out = _drive(capsys, monkeypatch, "--model", "deepfm", "--small", "1", "--steps", "4", "--eval_every", "2",
                 "--wide_optimizer", "ftrl", "--ftrl_l1", "0.5")
    assert out["fm_term"] is True and out["model"] == "deepfm" and out["steps"] == 4
    assert [e[0] for e in out["evals"]] == [2, 4] and "wide_nnz" in out
    assert out["losses"] and all(math.isfinite(l) for _, l in out["losses"])
    plain = _drive(capsys, monkeypatch, "--small", "1", "--steps", "4")
    assert "fm_term" not in plain
    dfm = _drive(capsys, monkeypatch, "--model", "deepfm", "--small", "1", "--steps", "4")
    assert dfm["losses"] != plain["losses"]  # the term is in the step
    # checkpoints: saved by deepfm, resumed by deepfm
    prefix = str(tmp_path / "ck") + os.sep
    _drive(capsys, monkeypatch, "--model", "deepfm", "--small", "1", "--steps", "4", "--checkpoint_toggle", "1",
           "--checkpoint_file_prefix", prefix, "--checkpoint_every", "2")
    res = _drive(capsys, monkeypatch, "--model", "deepfm", "--small", "1", "--steps", "6", "--use_weight_file", "1",
                 "--checkpoint_file_prefix", prefix)
    assert 0 < res["start"] < 6 and res["fm_term"] is True  # resumed at the saved iteration
    for argv in (("--model", "deepfm", "--consistency", "ssp"), ("--model", "deepfm", "--consistency", "asp"),
                 ("--model", "deepfm", "--transport", "onesided")):
        with pytest.raises(SystemExit) as e:
            train.parse(list(argv))
        assert e.value.code == 2 and "deepfm" in capsys.readouterr().err
    a = train.parse(["--model", "deepfm", "--consistency", "ssp", "--staleness", "1", "--transport", "collective"])
    assert a.transport == "collective"
