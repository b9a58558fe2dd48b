#!/usr/bin/env python3
"""Throughput of the other BASELINE configurations on the GPU parameter server, with the same
timing discipline as bench.py (W untimed warmup steps, exactly K timed steps bracketed by
barrier + synchronize, max over ranks, whole-job value, one JSON line on rank 0).

    python tools/bench_models.py --model gpt2 --steps 10 --warmup 3
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/bench_models.py --model dlrm

models: mlp (config 2, samples/s), gpt2 (config 4, tokens/s), dlrm (config 5, samples/s),
        dlrm-10b (config 5 at its per-GPU shard: 1.25B rows x 64 bf16 per GPU, ASP), lr (config 1 on GPUs,
        samples/s), kmeans (samples/s), widedeep-ssp (config 3), widedeep (the same driver under BSP; takes
        --wide_optimizer ftrl and reports wide_nnz), deepfm (widedeep with the FM term over its embeddings,
        WideDeepConfig(fm_term=True)), dcn (widedeep with --cross_layers Deep & Cross layers over its input,
        WideDeepConfig(cross_layers=L)), ffm (the field-aware FM, --ffm_fields x 262144 features, --ffm_k),
        gbdt (a boosting round of the fixed-point histogram GBDT over --batch resident samples per rank; --gbdt_depth,
        --gbdt_bins, --gbdt_features; ms_per_step is ms per tree), lda (a sweep of the fixed-point collapsed Gibbs
        sampler over --batch resident tokens per rank; --lda_topics; ms_per_step is ms per sweep), w2v (a clock of
        word2vec skip-gram with negative sampling on --batch pairs of Zipf words; --w2v_dim, --w2v_negatives).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# 8 HIP hardware queues (the step's 6-7 streams otherwise share 4 and serialise; see
# minips_amd/__init__.py): HIP reads this when torch loads it, so before the torch import
if os.environ.get("GPU_MAX_HW_QUEUES", "4") == "4":  # unset or HIP's default (the GPU box exports 4)
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("MINIPS_HW_QUEUES", "8")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(args, comm):
    dev = comm.device
    r = comm.rank
    if args.model == "mlp":
        from minips_amd.data.synthetic import MnistSynth
        from minips_amd.models.mlp import MLP, MLPConfig

        B = args.batch or 8192
        m = MLP(MLPConfig(consistency=args.consistency, staleness=args.staleness), comm)
        data = MnistSynth(B, device=dev, seed=r)
        use_graph = bool(args.graph) and comm.world == 1 and args.consistency == "bsp"
        if use_graph:  # launch-bound model: one HIP-graph launch per step
            from minips_amd.utils.graph import GraphedStep

            step = GraphedStep(lambda x, y: m.train_step(x, y)[0], data.next(), tables=[m.table])
            return m, (lambda: step(*data.next())), B, "samples/s", \
                dict(model="MLP 784-512-512-10 (Adam, dense PS table)", seq_len=None, hip_graph=True)
        return m, (lambda: m.train_step(*data.next())[0]), B, "samples/s", \
            dict(model="MLP 784-512-512-10 (Adam, dense PS table)", seq_len=None, hip_graph=False)
    if args.model == "gpt2":
        from minips_amd.data.synthetic import TokenSynth
        from minips_amd.models.gpt2 import GPT2, GPT2Config

        B, T = args.batch or 8, args.seq
        m = GPT2(GPT2Config(consistency=args.consistency, staleness=args.staleness,
                            clip_norm=args.clip_norm or None), comm)
        data = TokenSynth(B, T, device=dev, seed=r)
        return m, (lambda: m.train_step(*data.next())), B * T, "tokens/s", \
            dict(model="GPT-2 small 124M (12L/768d/12H, vocab 50257), dense params sharded over PS ranks",
                 seq_len=T, batch_per_gpu=B, **({"clip_norm": args.clip_norm} if args.clip_norm else {}))
    if args.model in ("dlrm", "dlrm-10b"):
        from minips_amd.models.dlrm import DLRM, DLRMConfig

        B = args.batch or 16384
        if args.model == "dlrm-10b":
            # BASELINE config 5: a 10B-row table over 8 GPUs = 1.25B rows (x 16 fp32 + row-wise
            # Adagrad state = 85 GB) per GPU; weak scaling keeps the per-GPU shard fixed
            rows = args.rows_per_gpu * comm.world
            cfg = DLRMConfig(num_rows=rows, D=args.dim, consistency=args.consistency if args.consistency != "bsp"
                             else "asp", staleness=args.staleness, transport=args.transport, max_batch=B)
        else:
            cfg = DLRMConfig(num_rows=args.rows, consistency=args.consistency, staleness=args.staleness,
                             transport=args.transport, max_batch=B)
        m = DLRM(cfg, comm)
        from minips_amd.data.synthetic import DLRMSynth

        gen = DLRMSynth(B, cfg.F, cfg.num_rows, cfg.n_dense, device=dev, seed=r)

        def batch():
            return gen.next()

        state = {"cur": batch()}

        def step():  # next batch generated one step ahead: lookahead key planning
            nxt = batch()
            cur, state["cur"] = state["cur"], nxt
            return m.train_step(*cur, next_keys=nxt[1])

        return m, step, B, "samples/s", dict(model=f"DLRM {cfg.num_rows} rows x {cfg.D} {cfg.emb_dtype} "
                                                   f"(26 sparse + 13 dense), "
                                                   f"{cfg.consistency}, {cfg.transport}", seq_len=None,
                                             rows_per_gpu=cfg.num_rows // comm.world, consistency=cfg.consistency)
    if args.model == "lr":
        from minips_amd.data.synthetic import SparseLRSynth
        from minips_amd.models.lr import SparseLR, SparseLRConfig

        B = args.batch or 65536
        vdt = getattr(torch, args.value_dtype)
        ftrl = {}
        if args.sparse_optimizer == "ftrl":
            ftrl = dict(optimizer="ftrl", ftrl_alpha=args.ftrl_alpha, ftrl_beta=args.ftrl_beta, l1=args.ftrl_l1,
                        l2=args.ftrl_l2)
        m = SparseLR(SparseLRConfig(consistency=args.consistency, staleness=args.staleness, value_dtype=vdt, **ftrl),
                     comm)
        data = SparseLRSynth(B, nnz=64, device=dev, seed=r)
        extra = dict(sparse_optimizer="ftrl", ftrl=ftrl) if ftrl else {}
        return m, (lambda: m.train_step(*data.next())), B, "samples/s", \
            dict(model=f"sparse LR, 16.6M features, 64 nnz/row, {args.value_dtype} table", seq_len=None, **extra)
    if args.model == "fm":
        from minips_amd.data.synthetic import FMSynth
        from minips_amd.models.fm import FM, FMConfig

        B = args.batch or 65536
        fields, card = 64, 262144  # 16.8M features, 64 nnz/row: sparse LR's shape
        lin = {}
        if args.wide_optimizer == "ftrl":
            lin = dict(linear_optimizer="ftrl", linear_alpha=args.ftrl_alpha, linear_beta=args.ftrl_beta,
                       linear_l1=args.ftrl_l1, linear_l2=args.ftrl_l2, linear_grad_scale=args.ftrl_grad_scale)
        m = FM(FMConfig(num_dims=fields * card, k=args.fm_k, consistency=args.consistency, staleness=args.staleness,
                        **lin), comm)
        data = FMSynth(B, fields=fields, card=card, device=dev, seed=0).holdout(1000 + r)
        return m, (lambda: m.train_step(*data.next())), B, "samples/s", \
            dict(model=f"factorization machine k={args.fm_k}, {fields * card} features, {fields} nnz/row, fp32 rows "
                       f"of {args.fm_k + 4}", seq_len=None, **({"linear_optimizer": "ftrl"} if lin else {}))
    if args.model == "ffm":
        from minips_amd.data.synthetic import FFMSynth
        from minips_amd.models.ffm import FFM, FFMConfig

        B = args.batch or 16384
        fields, card = args.ffm_fields, 262144  # 26 fields: 6.8M features, 26 nnz/row (Criteo's categorical shape)
        lin = {}
        if args.wide_optimizer == "ftrl":
            lin = dict(linear_optimizer="ftrl", linear_alpha=args.ftrl_alpha, linear_beta=args.ftrl_beta,
                       linear_l1=args.ftrl_l1, linear_l2=args.ftrl_l2, linear_grad_scale=args.ftrl_grad_scale)
        m = FFM(FFMConfig(num_dims=fields * card, num_fields=fields, k=args.ffm_k, consistency=args.consistency,
                          staleness=args.staleness, **lin), comm)
        # (a rank-1 teacher and a ring of ready batches: the field-aware teacher's logits are a [B, F, F] gather,
        # data generation that is not the model's step)
        data = FFMSynth(B, fields=fields, card=card, k_teacher=1, device=dev, seed=0).holdout(1000 + r)
        ring, at = [data.next() for _ in range(4)], [0]

        def step():
            at[0] += 1
            return m.train_step(*ring[at[0] % len(ring)])

        return m, step, B, "samples/s", \
            dict(model=f"field-aware factorization machine k={args.ffm_k}, {fields} fields, {fields * card} features, "
                       f"{fields} nnz/row, fp32 rows of {fields * args.ffm_k + 4}", seq_len=None,
                 **({"linear_optimizer": "ftrl"} if lin else {}))
    if args.model == "gbdt":
        from minips_amd.data.synthetic import GBDTSynth
        from minips_amd.models.gbdt import GBDT, GBDTConfig

        # a boosting round over a resident shard of --batch samples per rank (default 4M x 32 features, 64 bins,
        # depth 6); a "step" is one tree: max_trees covers the warm-up and the timed rounds
        rows = args.batch or 1 << 22
        m = GBDT(GBDTConfig(num_features=args.gbdt_features, num_bins=args.gbdt_bins, depth=args.gbdt_depth,
                            max_trees=args.steps + args.warmup + 1), comm)
        X, y = GBDTSynth(rows, features=args.gbdt_features, device=dev, seed=0).holdout(1000 + r).next()
        m.make_cuts(X[: 1 << 20])
        m.attach(X, y)
        del X
        return m, m.boost, rows, "samples/s", \
            dict(model=f"histogram GBDT depth {args.gbdt_depth}, {args.gbdt_bins} bins, {args.gbdt_features} features, "
                       f"{rows} resident samples per rank, int64 fixed-point histograms", seq_len=None)
    if args.model == "lda":
        from minips_amd.models.lda import LDA, LDAConfig
        from tools.bench_lda import make_corpus

        # a sweep over a resident corpus of --batch tokens per rank (default 4M, documents of 128 tokens, a power
        # law over 65536 words), clocks of 8192 documents; a "step" is one sweep
        tokens = args.batch or 1 << 22
        rowptr, words = make_corpus(tokens, 128, 1 << 16, dev, seed=r)
        m = LDA(LDAConfig(num_topics=args.lda_topics, vocab=1 << 16, batch_docs=8192, seed=0), comm)
        m.attach(rowptr, words, r * (rowptr.numel() - 1))
        m.init()

        def sweep():
            m.sweep()
            return m.nk[:1].float()

        return m, sweep, words.numel(), "tokens/s", \
            dict(model=f"LDA collapsed Gibbs, {args.lda_topics} topics, 65536 words, {words.numel()} resident tokens "
                       f"per rank, clocks of 8192 documents, int64 fixed-point weights", seq_len=None)
    if args.model == "w2v":
        from minips_amd.models.word2vec import Word2Vec, Word2VecConfig
        from tools.bench_fm import draw_keys

        # a clock on --batch explicit pairs (default 65536) of Zipf(1.05) words over 2^20 words, the negatives drawn
        # from the unigram^0.75 of the same law; a ring of ready pair batches (pair generation is epoch()'s job)
        B, V = args.batch or 65536, 1 << 20
        gen = torch.Generator(device=dev).manual_seed(1000 + r)
        m = Word2Vec(Word2VecConfig(vocab=V, dim=args.w2v_dim, negatives=args.w2v_negatives, batch_pairs=B,
                                    consistency=args.consistency, staleness=args.staleness), comm)
        m.set_counts(torch.bincount(draw_keys("zipf", 1 << 24, V, 1.05, torch.Generator(device=dev).manual_seed(7),
                                              dev), minlength=V) + 1)
        ring = [(draw_keys("zipf", B, V, 1.05, gen, dev), draw_keys("zipf", B, V, 1.05, gen, dev)) for _ in range(4)]
        at = [0]

        def step():
            at[0] += 1
            return m.train_step(*ring[at[0] % len(ring)], pair_base=(at[0] * comm.world + r) * B)

        return m, step, B, "pairs/s", \
            dict(model=f"word2vec skip-gram, {args.w2v_negatives} negatives, {V} words, fp32 rows of {args.w2v_dim}, "
                       f"Zipf(1.05) words", seq_len=None)
    if args.model == "kmeans":
        from minips_amd.models.kmeans import KMeans, KMeansConfig

        B = args.batch or 65536
        cfg = KMeansConfig(K=1000, dims=128, consistency=args.consistency, staleness=args.staleness)
        m = KMeans(cfg, comm)
        g = torch.Generator(device=dev)
        g.manual_seed(r)
        return m, (lambda: m.train_step(torch.randn(B, cfg.dims, generator=g, device=dev))), B, "samples/s", \
            dict(model="mini-batch K-Means K=1000 D=128", seq_len=None)
    if args.model in ("widedeep", "widedeep-ssp", "deepfm", "dcn"):
        from minips_amd.data.synthetic import CriteoSynth
        from minips_amd.models.widedeep import WideDeep, WideDeepConfig

        B = args.batch or 16384
        bsp = args.model in ("widedeep", "deepfm", "dcn")
        fm_term = args.model == "deepfm"
        cross = args.cross_layers if args.model == "dcn" else 0
        wide = {}
        if args.wide_optimizer == "ftrl":
            wide = dict(wide_optimizer="ftrl", wide_alpha=args.ftrl_alpha, wide_beta=args.ftrl_beta,
                        wide_l1=args.ftrl_l1, wide_l2=args.ftrl_l2,
                        wide_grad_scale=args.ftrl_grad_scale or float(B * comm.world))
        cfg = WideDeepConfig(consistency="bsp" if bsp else "ssp", staleness=0 if bsp else max(1, args.staleness),
                             transport=args.transport, max_batch=B, fm_term=fm_term, cross_layers=cross, **wide)
        m = WideDeep(cfg, comm)
        if bsp:  # BSP, the look-ahead feeder below
            from minips_amd.models.feeder import LookaheadFeeder
            from minips_amd.models.layers import compute_priority

            data = CriteoSynth(B, cards=cfg.cards, device=dev, seed=1000 + r)
            if dev.type == "cuda":
                main = torch.cuda.Stream(device=dev, priority=compute_priority())
                main.wait_stream(torch.cuda.default_stream(dev))
                torch.cuda.set_stream(main)
            feeder = LookaheadFeeder(m, data, comm)
            extra = dict(wide_optimizer="ftrl", ftrl=wide) if wide else {}
            if fm_term:
                extra["fm_term"] = True
            if cross:
                extra["cross_layers"] = cross
            name = ("DeepFM (Wide&Deep + FM term)" if fm_term else
                    f"DCN (Wide&Deep + {cross} cross layers)" if cross else "Wide&Deep")
            return m, feeder.step, B, "samples/s", dict(model=f"{name} Criteo BSP (collective)", seq_len=None,
                                                 consistency="bsp", transport=args.transport, feeder="lookahead",
                                                 **extra)
        data = CriteoSynth(B, cards=cfg.cards, device=dev, seed=1000 + r)
        if args.feeder == "inline":  # the next batch generated on the compute stream at step start
            state = {"cur": data.next()}

            def step():
                nxt = data.next()
                cur, state["cur"] = state["cur"], nxt
                return m.train_step(*cur, next_keys=nxt[1])

            return m, step, B, "samples/s", dict(model=f"Wide&Deep Criteo SSP ({args.transport})", seq_len=None,
                                                 consistency=f"ssp{cfg.staleness}", transport=args.transport,
                                                 feeder="inline")
        # bench.py's driver: the step on its own stream, the next batch generated and planned on
        # the planning stream a step ahead (LookaheadFeeder), for either transport
        from minips_amd.models.feeder import LookaheadFeeder
        from minips_amd.models.layers import compute_priority

        if dev.type == "cuda":
            main = torch.cuda.Stream(device=dev, priority=compute_priority())
            main.wait_stream(torch.cuda.default_stream(dev))
            torch.cuda.set_stream(main)
        feeder = LookaheadFeeder(m, data, comm)
        return m, feeder.step, B, "samples/s", dict(model=f"Wide&Deep Criteo SSP ({args.transport})", seq_len=None,
                                             consistency=f"ssp{cfg.staleness}", transport=args.transport,
                                             feeder="lookahead")
    raise SystemExit(f"unknown model {args.model}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2", choices=["mlp", "gpt2", "dlrm", "dlrm-10b", "lr", "kmeans",
                                                         "widedeep-ssp", "widedeep", "fm", "deepfm", "dcn", "ffm",
                                                         "gbdt", "lda", "w2v"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (samples or sequences)")
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=100_000_000, help="DLRM embedding rows (whole table)")
    ap.add_argument("--rows-per-gpu", type=int, default=1_250_000_000, help="dlrm-10b: rows per GPU shard")
    ap.add_argument("--dim", type=int, default=64, help="dlrm-10b: embedding width (bf16 rows: 64 fits 288 GB)")
    ap.add_argument("--consistency", default="bsp")
    ap.add_argument("--graph", type=lambda v: v.lower() in ("1", "true", "yes"), default=None,
                    help="mlp: capture the step in a HIP graph (one rank, BSP; off by default: at batch 8192 the "
                         "step is GPU-bound, 0.364 vs 0.350 ms measured)")
    ap.add_argument("--staleness", type=int, default=0)
    ap.add_argument("--feeder", default="lookahead", choices=["lookahead", "inline"],
                    help="widedeep-ssp: next batch generated + planned a step ahead on the planning stream "
                         "(bench.py's LookaheadFeeder) or generated inline at the step start")
    ap.add_argument("--transport", default="auto", choices=["auto", "collective", "onesided"],
                    help="widedeep-ssp / dlrm: RCCL collectives or the asynchronous PS (ps/onesided.py); auto = "
                         "the model's default (DLRM SSP/ASP: onesided; widedeep-ssp: collective)")
    ap.add_argument("--value-dtype", default="float32", choices=["float32", "float64"],
                    help="lr: table precision (float64 = the reference's CreateTable<double>)")
    ap.add_argument("--clip-norm", "--clip_norm", dest="clip_norm", type=float, default=0.0,
                    help="gpt2: > 0 clips the gradient to this global l2 norm in every clock (0: off)")
    ap.add_argument("--sparse_optimizer", "--sparse-optimizer", dest="sparse_optimizer", default="add",
                    choices=["add", "ftrl"], help="lr: the table's apply (ftrl: FTRL-Proximal; the result gains nnz)")
    ap.add_argument("--ftrl_alpha", type=float, default=0.1)
    ap.add_argument("--ftrl_beta", type=float, default=1.0)
    ap.add_argument("--ftrl_l1", type=float, default=0.0)
    ap.add_argument("--ftrl_l2", type=float, default=0.0)
    ap.add_argument("--wide_optimizer", "--wide-optimizer", dest="wide_optimizer", default="adagrad",
                    choices=["adagrad", "ftrl"],
                    help="widedeep: the wide column's rule (ftrl: FTRL-Proximal with the --ftrl_* flags; the result "
                         "gains wide_nnz)")
    ap.add_argument("--ftrl_grad_scale", type=float, default=0.0, help="widedeep ftrl: 0 = batch size x world")
    ap.add_argument("--fm_k", "--fm-k", dest="fm_k", type=int, default=16, help="fm: factors per feature")
    ap.add_argument("--cross_layers", type=int, default=3, help="dcn: cross layers, 1..4")
    ap.add_argument("--ffm_k", "--ffm-k", dest="ffm_k", type=int, default=4, help="ffm: factors per partner field")
    ap.add_argument("--ffm_fields", "--ffm-fields", dest="ffm_fields", type=int, default=26, help="ffm: fields")
    ap.add_argument("--gbdt_depth", "--gbdt-depth", dest="gbdt_depth", type=int, default=6, help="gbdt: tree depth")
    ap.add_argument("--gbdt_bins", "--gbdt-bins", dest="gbdt_bins", type=int, default=64, help="gbdt: bins")
    ap.add_argument("--lda_topics", "--lda-topics", dest="lda_topics", type=int, default=256, help="lda: topics")
    ap.add_argument("--w2v_dim", "--w2v-dim", dest="w2v_dim", type=int, default=128, help="w2v: vector width")
    ap.add_argument("--w2v_negatives", "--w2v-negatives", dest="w2v_negatives", type=int, default=5,
                    help="w2v: negatives per pair")
    ap.add_argument("--gbdt_features", "--gbdt-features", dest="gbdt_features", type=int, default=32,
                    help="gbdt: features (the teacher reads 5)")
    args = ap.parse_args()
    if args.wide_optimizer == "ftrl" and args.model not in ("widedeep", "deepfm", "dcn", "fm", "ffm"):
        ap.error("--wide_optimizer ftrl: --model widedeep, deepfm, dcn, fm and ffm only")
    if args.model == "dcn" and not 1 <= args.cross_layers <= 4:
        ap.error("--model dcn: --cross_layers must be in [1, 4]")
    if args.sparse_optimizer == "ftrl" and (args.model != "lr" or args.value_dtype != "float32"):
        ap.error("--sparse_optimizer ftrl: --model lr with --value-dtype float32 only")
    if args.clip_norm and args.model != "gpt2":
        ap.error("--clip_norm: --model gpt2 only")
    if args.transport == "auto" and not args.model.startswith("dlrm"):
        args.transport = "collective"
    from minips_amd.ps.comm import init_distributed

    comm = init_distributed()
    dev = comm.device
    model, step, per_step, unit, cfg = build(args, comm)
    for _ in range(args.warmup):
        step()
    model.drain()
    torch.cuda.synchronize(dev)
    comm.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    model.drain()
    torch.cuda.synchronize(dev)
    comm.barrier()
    torch.cuda.synchronize(dev)
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    if comm.world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t)
    if args.sparse_optimizer == "ftrl":  # after the timed window: a host read (collective)
        cfg["nnz"] = model.nnz()
    if args.wide_optimizer == "ftrl" and args.model in ("fm", "ffm"):  # likewise
        cfg["linear_nnz"] = model.linear_nnz()
    elif args.wide_optimizer == "ftrl":  # likewise
        cfg["wide_nnz"] = model.wide_nnz()
    if comm.rank == 0:
        print(json.dumps({
            "metric": f"{unit.split('/')[0]}/sec (whole job) {args.model} {cfg.pop('consistency', args.consistency)}",
            "value": round(per_step * comm.world * args.steps / el, 1), "unit": unit, "n_gpus": comm.world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000 * el / args.steps, 3),
            "higher_is_better": True, "scaling": "weak",
            "dtype": ("bf16" if args.model in ("mlp", "gpt2", "dlrm", "dlrm-10b", "widedeep-ssp", "widedeep", "deepfm",
                                                 "dcn")
                      else ("fp64" if args.value_dtype == "float64" and args.model == "lr" else "fp32")),
            "data": "synthetic", "last": float(out.float().sum()) if torch.is_tensor(out) else None,
            "config": dict(cfg, parallelism=f"ps-dp{comm.world}"),
        }), flush=True)
    if comm.world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
