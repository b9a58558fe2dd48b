"""Training driver of one PS rank (one process per GPU; torchrun / minips_amd.elastic set the env).

    python -m minips_amd.train --model widedeep --steps 100 --checkpoint_toggle=1 \
        --checkpoint_file_prefix=/tmp/ck/ --checkpoint_every 20

Flags keep the reference names where the reference has them (lr_example.cpp:20-56, §5.6):
checkpoint_toggle, checkpoint_file_prefix, use_weight_file, heartbeat_interval, report_prefix,
report_interval, with_injected_straggler, kModelType (= --consistency), kStaleness, batch_size,
num_iters (= --steps), alpha (LR). Extra: --fail_rank/--fail_step fault injection, --metrics_dir,
--eval_every/--eval_batches/--eval_seed (held-out AUC and log loss of widedeep / dlrm; off by default).
--model deepfm is widedeep with the FM second-order term over its field embeddings (WideDeepConfig(fm_term=True)):
every widedeep flag applies, the final JSON gains fm_term, SSP / ASP need --transport collective.
--model dcn is widedeep with --cross_layers (default 3, 1..4) Deep & Cross layers over its whole input
(WideDeepConfig(cross_layers=L)): every widedeep flag applies, the final JSON gains cross_layers, collective only.
--model ffm is the field-aware FM (models/ffm.py): --ffm_k factors per partner field; the synthetic stream takes
--fm_fields / --fm_card, an --input file --ffm_fields F [--ffm_field_bounds a,b,...] (a key's field is its key
range); the final JSON gains ffm_fields and ffm_k, collective only.
--model gbdt is the fixed-point histogram GBDT (models/gbdt.py): --steps counts boosting rounds over a resident
shard -- --gbdt_rows synthetic samples per rank (GBDTSynth), or an --input libsvm file densified to
--gbdt_features columns (an absent feature is 0.0); --gbdt_depth / --gbdt_bins / --gbdt_lr / --gbdt_lambda,
--gbdt_model_out PATH saves the trees; the final JSON gains gbdt_trees, gbdt_depth and gbdt_bins, collective only.
--model lda is Latent Dirichlet Allocation by fixed-point collapsed Gibbs sampling (models/lda.py): --steps counts
sweeps over a resident corpus -- --lda_docs synthetic documents of --lda_doc_len tokens over all ranks (LDASynth),
or an --input libsvm file whose lines are documents (`label word:count ...`, the label is ignored);
--lda_topics / --lda_alpha / --lda_beta / --lda_vocab, --batch documents per clock; the reported loss is the
negative per-token log likelihood; the final JSON gains lda_topics, lda_tokens and lda_loglik, collective BSP only.
--model w2v is word2vec by skip-gram with negative sampling (models/word2vec.py): --steps counts epochs over a
resident corpus -- --w2v_sentences synthetic sentences of --w2v_len tokens over all ranks (W2VSynth), or an --input
libsvm file whose lines are sentences in file order (`label word:x ...`, ids minus one, values ignored);
--w2v_dim / --w2v_negatives / --w2v_window / --w2v_sample / --w2v_vocab, --batch pairs per clock; the reported loss
is the epoch's mean pair loss; the final JSON gains w2v_dim, w2v_pairs and (synthetic) w2v_purity, collective only.
On --use_weight_file the tables restore from the checkpoint and training resumes at the saved
iteration with the data stream advanced to the same position, so a restarted run ends with the
same parameters as an uninterrupted one (BSP).
The last line on rank 0 is a JSON summary (losses, final iteration, parameter checksum).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time


import torch
import torch.distributed as dist


def _flag_bool(v):
    return str(v).lower() in ("1", "true", "yes", "on")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="widedeep", choices=["widedeep", "mlp", "dlrm", "gpt2", "lr", "kmeans", "fm",
                                                             "deepfm", "dcn", "ffm", "gbdt", "lda", "w2v"])
    ap.add_argument("--steps", "--num_iters", dest="steps", type=int, default=20)
    ap.add_argument("--batch", "--batch_size", dest="batch", type=int, default=0)
    ap.add_argument("--consistency", "--kModelType", dest="consistency", default="bsp", type=str.lower)
    ap.add_argument("--staleness", "--kStaleness", dest="staleness", type=int, default=0)
    ap.add_argument("--small", type=_flag_bool, default=False, help="tiny shapes (CPU tests)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint_toggle", type=_flag_bool, default=False)
    ap.add_argument("--checkpoint_file_prefix", default="/tmp/minips_ckpt/")
    ap.add_argument("--checkpoint_text_limit", type=int, default=1 << 22,
                    help="write the reference text file (<idx>:<val>) for shards of up to this many values "
                    "(-1: every shard, streamed); the binary sidecar is always written")
    ap.add_argument("--checkpoint_every", type=int, default=100)
    ap.add_argument("--use_weight_file", type=_flag_bool, default=False)
    ap.add_argument("--heartbeat_interval", type=float, default=0.0)
    ap.add_argument("--heartbeat_dir", default="")
    ap.add_argument("--fail_rank", type=int, default=-1)
    ap.add_argument("--fail_step", type=int, default=-1)
    ap.add_argument("--fail_mode", default="exit", choices=["exit", "hang", "hang_in_step"])
    ap.add_argument("--scale_check_every", type=int, default=10,
                    help="steps between checks for a supervisor scale directive (a max all-reduce of the "
                         "directive generation the ranks saw; minips_amd.elastic scale)")
    ap.add_argument("--recovery", default="inplace", choices=["inplace", "restart"],
                    help="inplace: after a peer failure the survivors roll back in their processes and "
                         "the supervisor relaunches only the failed rank; restart: the whole rank set")
    ap.add_argument("--value_dtype", default="float32", choices=["float32", "float64"],
                    help="LR table precision; float64 = the reference's CreateTable<double> (lr_example.cpp:182)")
    ap.add_argument("--transport", default="auto", choices=["auto", "collective", "onesided"],
                    help="W&D / DLRM SSP/ASP data path: RCCL collectives, or the asynchronous PS "
                         "(one-sided row reads, inbox pushes, owner-side optimizer apply; ps/onesided.py); "
                         "auto = the model's default (DLRM SSP/ASP: onesided, otherwise collective)")
    ap.add_argument("--asp_bound", type=int, default=-1,
                    help="ASP on the one-sided transport: >= 0 bounds how far a Get may run ahead of the "
                         "owners' applies (the SSP gate); -1 (default): unbounded, the reference ASP")
    ap.add_argument("--asp_depth", type=int, default=2,
                    help="ASP on the collective transport: clocks in flight before a Get waits (pipelining)")
    ap.add_argument("--force_quit_rank", type=int, default=-1,
                    help="(LR --input) treat this rank's shard as empty: it ForceQuits, the others continue")
    ap.add_argument("--checkpoint_commit", default="eager", choices=["eager", "async"],
                    help="eager: publish a checkpoint at the next step (waits for its files); async: "
                         "publish once every rank's writer finished (training never waits for the disk)")
    ap.add_argument("--with_injected_straggler", type=_flag_bool, default=False)
    ap.add_argument("--kStorageType", default="Vector", type=str.lower, choices=["vector", "map"],
                    help="LR parameter storage: Vector (key range) or Map (GPU hash table, MapStorage)")
    ap.add_argument("--K", type=int, default=0, help="K-Means centres (0: model default)")
    ap.add_argument("--kmeans_init_mode", default="", choices=["", "random", "kmeans++", "kmeans_parallel"],
                    help="K-Means seeding from a batch of local data (reference kmeans.cpp:154-192); "
                         "empty: N(0,1) centres")
    ap.add_argument("--report_prefix", default="")
    ap.add_argument("--report_interval", type=int, default=10)
    ap.add_argument("--metrics_dir", default="")
    ap.add_argument("--timing_skip", type=int, default=0,
                    help="iterations excluded from steady_ms_per_iter (first-launch / warm-up costs)")
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--num_workers_per_node", type=int, default=1,
                    help="LR: logical workers per rank, each with its own sampler and batch_size (reference flag); "
                    "their batches of a clock go out as one fused Get/Add")
    ap.add_argument("--input", default="", help="libsvm file / directory / comma list (LR; reference --input); "
                    "local, webhdfs://nn:port/path or hdfs://nn:port/path")
    ap.add_argument("--hdfs_namenode", default="", help="read a bare --input path from this HDFS namenode")
    ap.add_argument("--hdfs_namenode_port", type=int, default=9000)
    ap.add_argument("--hdfs_http_port", type=int, default=0, help="> 0: read HDFS through WebHDFS on this port")
    ap.add_argument("--assigner_master_port", type=int, default=0,
                    help="> 0: rank 0 serves locality-aware block assignment (HDFSBlockAssigner) on this port")
    ap.add_argument("--num_dims", type=int, default=0, help="feature count (reference flag; 0: infer / default)")
    ap.add_argument("--eval_every", type=int, default=0,
                    help="> 0: every N steps and at the end, all ranks evaluate --eval_batches held-out batches "
                         "(widedeep / dlrm: exact binned AUC and log loss); 0: off, nothing changes")
    ap.add_argument("--eval_batches", type=int, default=4, help="held-out batches per rank and evaluation")
    ap.add_argument("--eval_seed", type=int, default=12345,
                    help="seed of the held-out stream (re-created at every evaluation: the same batches each time)")
    ap.add_argument("--clip_norm", type=float, default=0.0,
                    help="> 0: clip the gradient to this global l2 norm in every dense clock (gpt2 / mlp; a clock "
                         "whose gradient is not finite is skipped); 0: off, nothing changes")
    ap.add_argument("--lr_warmup", type=int, default=0, help="linear lr warmup over this many steps (gpt2 / mlp)")
    ap.add_argument("--lr_decay_steps", type=int, default=0,
                    help="> 0: cosine lr decay from the end of the warmup down to --lr_min_ratio at this step")
    ap.add_argument("--lr_min_ratio", type=float, default=0.0, help="final lr / peak lr of the cosine decay")
    ap.add_argument("--sparse_optimizer", default="add", choices=["add", "ftrl"],
                    help="LR server apply: add (the reference's w += delta) or ftrl (per-coordinate FTRL-Proximal "
                         "with L1 / L2; Vector storage, float32)")
    ap.add_argument("--ftrl_alpha", type=float, default=0.1, help="FTRL-Proximal per-coordinate rate alpha")
    ap.add_argument("--ftrl_beta", type=float, default=1.0)
    ap.add_argument("--ftrl_l1", type=float, default=0.0, help="L1 strength: weights with |z| <= l1 are exactly 0")
    ap.add_argument("--ftrl_l2", type=float, default=0.0)
    ap.add_argument("--wide_optimizer", default="adagrad", choices=["adagrad", "ftrl"],
                    help="W&D wide column: adagrad (its own row-wise accumulator) or ftrl (FTRL-Proximal with the "
                         "--ftrl_* flags beside the row-wise Adagrad embedding; collective transport)")
    ap.add_argument("--ftrl_grad_scale", type=float, default=0.0,
                    help="--wide_optimizer ftrl: factor on the pushed mean-loss gradient of the wide columns; 0 "
                         "(default): batch size x world, the summed-loss gradient")
    ap.add_argument("--fm_k", type=int, default=16, help="fm: factors per feature (k % 4 == 0, 4 <= k <= 60)")
    ap.add_argument("--cross_layers", type=int, default=None,
                    help="dcn: cross layers over the assembled input, 1..4 (default 3)")
    ap.add_argument("--fm_fields", type=int, default=0,
                    help="fm, synthetic data: fields per sample, one active feature each (0: 8 with --small, else 64)")
    ap.add_argument("--fm_card", type=int, default=0,
                    help="fm, synthetic data: ids per field (0: 32 with --small, else 262144)")
    ap.add_argument("--ffm_k", type=int, default=4,
                    help="ffm: factors per feature and partner field (k % 4 == 0, 4 <= k <= 16)")
    ap.add_argument("--ffm_fields", type=int, default=0,
                    help="ffm with --input: fields F of the file's keys (1 <= F <= 64, F * ffm_k <= 512); the "
                         "synthetic stream takes --fm_fields")
    ap.add_argument("--ffm_field_bounds", default="",
                    help="ffm with --input: F - 1 ascending key boundaries a,b,... over the loaded keys (the "
                         "file's ids minus one); default: equal key ranges")
    ap.add_argument("--gbdt_depth", type=int, default=None, help="gbdt: tree depth, 1..8 (default 6)")
    ap.add_argument("--gbdt_bins", type=int, default=None, help="gbdt: bins per feature, 2..256 (default 64)")
    ap.add_argument("--gbdt_lr", type=float, default=None, help="gbdt: shrinkage of every tree (default 0.1)")
    ap.add_argument("--gbdt_lambda", type=float, default=None, help="gbdt: L2 on the leaf values, > 0 (default 1.0)")
    ap.add_argument("--gbdt_rows", type=int, default=None,
                    help="gbdt, synthetic data: resident samples per rank (default 4096 with --small, else 1048576)")
    ap.add_argument("--gbdt_features", type=int, default=None,
                    help="gbdt: feature columns (synthetic: >= 5, default 8; with --input: required, keys beyond "
                         "it are dropped)")
    ap.add_argument("--gbdt_model_out", default="", help="gbdt: rank 0 saves the cuts and the trees here at the end")
    ap.add_argument("--lda_topics", type=int, default=None, help="lda: topics K, 2..1024 (default 16)")
    ap.add_argument("--lda_alpha", type=float, default=None, help="lda: document-topic prior, (0, 64] (default 0.1)")
    ap.add_argument("--lda_beta", type=float, default=None, help="lda: topic-word prior, (0, 64] (default 0.01)")
    ap.add_argument("--lda_vocab", type=int, default=None,
                    help="lda: vocabulary size (synthetic default: 256 with --small, else 65536; with --input: the "
                         "largest word of all shards + 1)")
    ap.add_argument("--lda_docs", type=int, default=None,
                    help="lda, synthetic data: documents over all ranks (default 256 with --small, else 65536)")
    ap.add_argument("--lda_doc_len", type=int, default=None,
                    help="lda, synthetic data: tokens per document, 1..4096 (default 48 with --small, else 128)")
    ap.add_argument("--w2v_dim", type=int, default=None, help="w2v: vector width, a multiple of 4 in [4, 512] "
                                                              "(default 16 with --small, else 128)")
    ap.add_argument("--w2v_negatives", type=int, default=None, help="w2v: negatives per pair, 1..64 (default 5)")
    ap.add_argument("--w2v_window", type=int, default=None, help="w2v: the largest window, 1..64 (default 5)")
    ap.add_argument("--w2v_sample", type=float, default=None,
                    help="w2v: subsampling threshold in [0, 1), 0 keeps every token (default 1e-3)")
    ap.add_argument("--w2v_vocab", type=int, default=None,
                    help="w2v: vocabulary size (synthetic default: 128 with --small, else 65536, a multiple of the 8 / "
                         "256 planted groups; with --input: the largest word id over all ranks + 1)")
    ap.add_argument("--w2v_sentences", type=int, default=None,
                    help="w2v, synthetic data: sentences over all ranks (default 512 with --small, else 262144)")
    ap.add_argument("--w2v_len", type=int, default=None,
                    help="w2v, synthetic data: tokens per sentence (default 16 with --small, else 32)")
    args = ap.parse_args(argv)
    if args.sparse_optimizer == "ftrl":
        if args.model != "lr":
            ap.error(f"--sparse_optimizer ftrl supports --model lr, not {args.model}")
        if args.kStorageType != "vector":
            ap.error("--sparse_optimizer ftrl needs --kStorageType Vector (no ftrl on hash tables)")
        if args.value_dtype != "float32":
            ap.error(f"--sparse_optimizer ftrl keeps float32 weights, not --value_dtype {args.value_dtype}")
        if not args.ftrl_alpha > 0 or not (args.ftrl_beta >= 0 and args.ftrl_l1 >= 0 and args.ftrl_l2 >= 0):
            ap.error("--sparse_optimizer ftrl: --ftrl_alpha > 0, --ftrl_beta, --ftrl_l1 and --ftrl_l2 >= 0")
    if args.wide_optimizer == "ftrl":
        if args.model not in ("widedeep", "deepfm", "dcn", "fm", "ffm"):
            ap.error(f"--wide_optimizer ftrl supports --model widedeep, deepfm, dcn, fm and ffm, not {args.model}")
        if not args.ftrl_alpha > 0 or not (args.ftrl_beta >= 0 and args.ftrl_l1 >= 0 and args.ftrl_l2 >= 0):
            ap.error("--wide_optimizer ftrl: --ftrl_alpha > 0, --ftrl_beta, --ftrl_l1 and --ftrl_l2 >= 0")
        if not 0 <= args.ftrl_grad_scale < float("inf"):
            ap.error("--wide_optimizer ftrl: --ftrl_grad_scale must be finite and >= 0 (0: batch size x world)")
    args.opt_flags = bool(args.clip_norm or args.lr_warmup or args.lr_decay_steps or args.lr_min_ratio)
    if args.opt_flags and args.model not in ("gpt2", "mlp"):
        ap.error(f"--clip_norm / --lr_warmup / --lr_decay_steps / --lr_min_ratio support --model gpt2 and mlp, "
                 f"not {args.model}")
    if args.clip_norm < 0 or args.lr_warmup < 0 or args.lr_decay_steps < 0 or not 0 <= args.lr_min_ratio <= 1 \
            or (args.lr_decay_steps and args.lr_decay_steps <= args.lr_warmup):
        ap.error("--clip_norm >= 0, 0 <= --lr_warmup < --lr_decay_steps (or no decay), 0 <= --lr_min_ratio <= 1")
    if args.lr_min_ratio and not args.lr_decay_steps:
        ap.error("--lr_min_ratio needs --lr_decay_steps")
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        ap.error("--eval_every must be >= 0 and --eval_batches >= 1")
    if args.eval_every > 0 and args.model not in ("widedeep", "deepfm", "dcn", "dlrm", "fm", "ffm", "gbdt"):
        ap.error(f"--eval_every: held-out evaluation supports --model widedeep, deepfm, dcn, dlrm, fm, ffm and gbdt, "
                 f"not {args.model}")
    gbdt_flags = [f"--{k}" for k in ("gbdt_depth", "gbdt_bins", "gbdt_lr", "gbdt_lambda", "gbdt_rows",
                                     "gbdt_features") if getattr(args, k) is not None]
    if args.gbdt_model_out:
        gbdt_flags.append("--gbdt_model_out")
    if args.model == "gbdt":
        args.gbdt_depth = 6 if args.gbdt_depth is None else args.gbdt_depth
        args.gbdt_bins = 64 if args.gbdt_bins is None else args.gbdt_bins
        args.gbdt_lr = 0.1 if args.gbdt_lr is None else args.gbdt_lr
        args.gbdt_lambda = 1.0 if args.gbdt_lambda is None else args.gbdt_lambda
        if not 1 <= args.gbdt_depth <= 8:
            ap.error(f"--model gbdt: --gbdt_depth {args.gbdt_depth} must be in [1, 8]")
        if not 2 <= args.gbdt_bins <= 256:
            ap.error(f"--model gbdt: --gbdt_bins {args.gbdt_bins} must be in [2, 256]")
        if not args.gbdt_lr > 0 or not args.gbdt_lambda > 0:
            ap.error("--model gbdt: --gbdt_lr and --gbdt_lambda must be > 0")
        if args.input and args.gbdt_features is None:
            ap.error("--model gbdt with --input needs --gbdt_features (the columns the file is densified to)")
        if args.input and args.gbdt_rows is not None:
            ap.error("--model gbdt: --gbdt_rows sizes the synthetic shard, not an --input file")
        args.gbdt_features = 8 if args.gbdt_features is None else args.gbdt_features
        if not 1 <= args.gbdt_features <= 4096 or (not args.input and args.gbdt_features < 5):
            ap.error(f"--model gbdt: --gbdt_features {args.gbdt_features} must be in [1, 4096] (the synthetic "
                     f"teacher reads 5)")
        args.gbdt_rows = (4096 if args.small else 1 << 20) if args.gbdt_rows is None else args.gbdt_rows
        if args.gbdt_rows < 1:
            ap.error(f"--model gbdt: --gbdt_rows {args.gbdt_rows} must be >= 1")
        if (1 << (args.gbdt_depth - 1)) * args.gbdt_features * args.gbdt_bins * 24 > 1 << 30:
            ap.error("--model gbdt: the last level's histogram [2^(depth-1), features, bins, 3] int64 is above 1 GiB")
        if args.steps > 65536:
            ap.error(f"--model gbdt: --steps {args.steps} boosting rounds, at most 65536 trees")
        if args.transport == "onesided":
            ap.error("--model gbdt needs --transport collective (no gbdt on the one-sided transport)")
        if args.consistency != "bsp":
            ap.error("--model gbdt is bulk-synchronous: every level all-reduces its histogram (--consistency bsp)")
        if args.checkpoint_toggle or args.use_weight_file:
            ap.error("--model gbdt: no table checkpoints (--gbdt_model_out saves the trees; an elastic restart of a "
                     "boosting run is out of scope)")
        if args.eval_every > 0 and args.input:
            ap.error("--model gbdt: --eval_every needs the synthetic stream (an --input file has no held-out split)")
    elif gbdt_flags:
        ap.error(f"{' / '.join(gbdt_flags)}: --model gbdt only, not {args.model}")
    lda_flags = [f"--{k}" for k in ("lda_topics", "lda_alpha", "lda_beta", "lda_vocab", "lda_docs", "lda_doc_len")
                 if getattr(args, k) is not None]
    if args.model == "lda":
        args.lda_topics = 16 if args.lda_topics is None else args.lda_topics
        args.lda_alpha = 0.1 if args.lda_alpha is None else args.lda_alpha
        args.lda_beta = 0.01 if args.lda_beta is None else args.lda_beta
        if not 2 <= args.lda_topics <= 1024:
            ap.error(f"--model lda: --lda_topics {args.lda_topics} must be in [2, 1024]")
        if not 0 < args.lda_alpha <= 64 or not 0 < args.lda_beta <= 64:
            ap.error("--model lda: --lda_alpha and --lda_beta must be in (0, 64]")
        if args.input and (args.lda_docs is not None or args.lda_doc_len is not None):
            ap.error("--model lda: --lda_docs / --lda_doc_len size the synthetic corpus, not an --input file")
        if not args.input:
            args.lda_vocab = (256 if args.small else 65536) if args.lda_vocab is None else args.lda_vocab
            args.lda_docs = (256 if args.small else 65536) if args.lda_docs is None else args.lda_docs
            args.lda_doc_len = (48 if args.small else 128) if args.lda_doc_len is None else args.lda_doc_len
            if args.lda_docs < 1 or not 1 <= args.lda_doc_len <= 4096:
                ap.error("--model lda: --lda_docs must be >= 1 and --lda_doc_len in [1, 4096]")
            if args.lda_vocab < args.lda_topics:
                ap.error(f"--model lda: --lda_vocab {args.lda_vocab} is below --lda_topics {args.lda_topics} (every "
                         f"planted topic owns a word block)")
        if args.lda_vocab is not None and not 1 <= args.lda_vocab < 1 << 31:
            ap.error(f"--model lda: --lda_vocab {args.lda_vocab} must be in [1, 2^31)")
        if args.batch < 0:
            ap.error(f"--model lda: --batch {args.batch} documents per clock must be >= 1 (0: 4096)")
        if args.transport == "onesided":
            ap.error("--model lda needs --transport collective (no lda on the one-sided transport)")
        if args.consistency != "bsp":
            ap.error("--model lda is bulk-synchronous: every clock all-reduces the topic totals (--consistency bsp; "
                     "no SSP or ASP)")
        if args.kStorageType != "vector":
            ap.error("--model lda needs --kStorageType Vector (no lda on hash tables)")
        if args.value_dtype != "float32":
            ap.error(f"--model lda keeps float32 count rows, not --value_dtype {args.value_dtype}")
        if args.eval_every > 0:
            ap.error("--model lda: no --eval_every (held-out fold-in perplexity is out of scope; the loss is the "
                     "training log likelihood)")
        if args.checkpoint_toggle or args.use_weight_file:
            ap.error("--model lda: no table checkpoints (they do not hold the topic of every token)")
    elif lda_flags:
        ap.error(f"{' / '.join(lda_flags)}: --model lda only, not {args.model}")
    w2v_flags = [f"--{k}" for k in ("w2v_dim", "w2v_negatives", "w2v_window", "w2v_sample", "w2v_vocab",
                                    "w2v_sentences", "w2v_len") if getattr(args, k) is not None]
    if args.model == "w2v":
        args.w2v_dim = (16 if args.small else 128) if args.w2v_dim is None else args.w2v_dim
        args.w2v_negatives = 5 if args.w2v_negatives is None else args.w2v_negatives
        args.w2v_window = 5 if args.w2v_window is None else args.w2v_window
        args.w2v_sample = 1e-3 if args.w2v_sample is None else args.w2v_sample
        if args.w2v_dim % 4 or not 4 <= args.w2v_dim <= 512:
            ap.error(f"--model w2v: --w2v_dim {args.w2v_dim} must be a multiple of 4 in [4, 512]")
        if not 1 <= args.w2v_negatives <= 64:
            ap.error(f"--model w2v: --w2v_negatives {args.w2v_negatives} must be in [1, 64]")
        if not 1 <= args.w2v_window <= 64:
            ap.error(f"--model w2v: --w2v_window {args.w2v_window} must be in [1, 64]")
        if not 0 <= args.w2v_sample < 1:
            ap.error(f"--model w2v: --w2v_sample {args.w2v_sample} must be in [0, 1)")
        if args.input and (args.w2v_sentences is not None or args.w2v_len is not None):
            ap.error("--model w2v: --w2v_sentences / --w2v_len size the synthetic corpus, not an --input file")
        if not args.input:
            args.w2v_vocab = (128 if args.small else 65536) if args.w2v_vocab is None else args.w2v_vocab
            args.w2v_sentences = (512 if args.small else 262144) if args.w2v_sentences is None else args.w2v_sentences
            args.w2v_len = (16 if args.small else 32) if args.w2v_len is None else args.w2v_len
            groups = 8 if args.small else 256
            if args.w2v_sentences < 1 or args.w2v_len < 1:
                ap.error("--model w2v: --w2v_sentences and --w2v_len must be >= 1")
            if args.w2v_vocab < groups or args.w2v_vocab % groups:
                ap.error(f"--model w2v: --w2v_vocab {args.w2v_vocab} must be a positive multiple of the {groups} "
                         f"planted groups of the synthetic corpus")
        if args.w2v_vocab is not None and not 1 <= args.w2v_vocab < 1 << 30:
            ap.error(f"--model w2v: --w2v_vocab {args.w2v_vocab} must be in [1, 2^30)")
        if args.batch < 0 or args.batch * (args.w2v_negatives + 2) >= 1 << 31:
            ap.error(f"--model w2v: --batch {args.batch} pairs per clock must be >= 1 (0: 65536) with batch * "
                     f"(negatives + 2) < 2^31")
        if args.transport == "onesided":
            ap.error("--model w2v needs --transport collective (no w2v on the one-sided transport, SSP / ASP "
                     "included)")
        if args.kStorageType != "vector":
            ap.error("--model w2v needs --kStorageType Vector (no w2v on hash tables)")
        if args.value_dtype != "float32":
            ap.error(f"--model w2v keeps float32 rows, not --value_dtype {args.value_dtype}")
        if args.eval_every > 0:
            ap.error("--model w2v: no --eval_every (there is no held-out split of a corpus; the loss is the epoch's "
                     "mean pair loss)")
    elif w2v_flags:
        ap.error(f"{' / '.join(w2v_flags)}: --model w2v only, not {args.model}")
    if args.model == "fm":
        if args.fm_k % 4 or not 4 <= args.fm_k <= 60:
            ap.error(f"--model fm: --fm_k {args.fm_k} must be a multiple of 4 in [4, 60]")
        if args.transport == "onesided":
            ap.error("--model fm needs --transport collective (no fm on the one-sided transport)")
        if args.kStorageType != "vector":
            ap.error("--model fm needs --kStorageType Vector (no fm on hash tables)")
        if args.value_dtype != "float32":
            ap.error(f"--model fm keeps float32 rows, not --value_dtype {args.value_dtype}")
        if args.eval_every > 0 and args.input:
            ap.error("--model fm: --eval_every needs the synthetic stream (an --input file has no held-out split)")
    if args.model == "ffm":
        fields = args.ffm_fields if args.input else (args.fm_fields or (8 if args.small else 64))
        if args.ffm_k % 4 or not 4 <= args.ffm_k <= 16:
            ap.error(f"--model ffm: --ffm_k {args.ffm_k} must be a multiple of 4 in [4, 16]")
        if args.input and not args.ffm_fields:
            ap.error("--model ffm with --input needs --ffm_fields (the fields of the file's keys)")
        if not 1 <= fields <= 64 or fields * args.ffm_k > 512:
            ap.error(f"--model ffm: {fields} fields with --ffm_k {args.ffm_k}: 1 <= fields <= 64 and fields * ffm_k "
                     f"<= 512")
        try:
            args.ffm_bounds = [int(v) for v in args.ffm_field_bounds.split(",") if v.strip()] or None
        except ValueError:
            ap.error(f"--ffm_field_bounds {args.ffm_field_bounds!r}: comma-separated integer keys")
        if args.ffm_bounds is not None and (not args.input or len(args.ffm_bounds) != fields - 1 or any(
                b <= a for a, b in zip(args.ffm_bounds, args.ffm_bounds[1:]))):
            ap.error(f"--ffm_field_bounds: --input only, --ffm_fields - 1 = {fields - 1} ascending keys")
        if args.transport == "onesided":
            ap.error("--model ffm needs --transport collective (no ffm on the one-sided transport)")
        if args.kStorageType != "vector":
            ap.error("--model ffm needs --kStorageType Vector (no ffm on hash tables)")
        if args.value_dtype != "float32":
            ap.error(f"--model ffm keeps float32 rows, not --value_dtype {args.value_dtype}")
        if args.eval_every > 0 and args.input:
            ap.error("--model ffm: --eval_every needs the synthetic stream (an --input file has no held-out split)")
    elif args.ffm_fields or args.ffm_field_bounds:
        ap.error(f"--ffm_fields / --ffm_field_bounds: --model ffm only, not {args.model}")
    if args.transport == "auto":  # SSP / ASP run on the asynchronous one-sided PS (W&D, DLRM), BSP on collectives
        args.transport = ("onesided" if args.model in ("dlrm", "widedeep", "deepfm", "dcn")
                          and args.consistency in ("ssp", "asp") else "collective")
    if args.model == "deepfm" and args.transport == "onesided":
        ap.error("--model deepfm with SSP / ASP needs --transport collective (the FM term is not built for the "
                 "one-sided transport)")
    if args.cross_layers is not None and args.model != "dcn":
        ap.error(f"--cross_layers: --model dcn only, not {args.model}")
    if args.model == "dcn":
        if args.cross_layers is None:
            args.cross_layers = 3
        if not 1 <= args.cross_layers <= 4:
            ap.error(f"--model dcn: --cross_layers {args.cross_layers} must be in [1, 4]")
        if args.transport == "onesided":
            ap.error("--model dcn with SSP / ASP needs --transport collective (the cross layers are not built for the "
                     "one-sided transport)")
    if args.wide_optimizer == "ftrl" and args.transport == "onesided":
        ap.error("--wide_optimizer ftrl with SSP / ASP needs --transport collective (the one-sided owners apply the "
                 "row-wise Adagrad only)")
    if args.eval_every > 0 and args.transport == "onesided":
        ap.error("--eval_every: held-out evaluation needs --transport collective (evaluate() is not implemented "
                 "on the onesided transport)")
    return args


def _ftrl_kw(args) -> dict:
    """SparseLRConfig fields of --sparse_optimizer ftrl (none without the flag)."""
    if args.sparse_optimizer != "ftrl":
        return {}
    return dict(optimizer="ftrl", ftrl_alpha=args.ftrl_alpha, ftrl_beta=args.ftrl_beta, l1=args.ftrl_l1,
                l2=args.ftrl_l2)


def _fm_cfg(args, comm, nd: int, B: int):
    """FMConfig of --model fm (--wide_optimizer ftrl: the linear column on FTRL with the --ftrl_* flags)."""
    from .models.fm import FMConfig

    lin = {}
    if args.wide_optimizer == "ftrl":
        lin = dict(linear_optimizer="ftrl", linear_alpha=args.ftrl_alpha, linear_beta=args.ftrl_beta,
                   linear_l1=args.ftrl_l1, linear_l2=args.ftrl_l2, linear_grad_scale=args.ftrl_grad_scale)
    return FMConfig(num_dims=nd, k=args.fm_k, lr=args.alpha, consistency=args.consistency, staleness=args.staleness,
                    seed=args.seed, **lin)


def _ffm_cfg(args, comm, nd: int, fields: int):
    """FFMConfig of --model ffm (--wide_optimizer ftrl: the linear column on FTRL with the --ftrl_* flags)."""
    from .models.ffm import FFMConfig

    lin = {}
    if args.wide_optimizer == "ftrl":
        lin = dict(linear_optimizer="ftrl", linear_alpha=args.ftrl_alpha, linear_beta=args.ftrl_beta,
                   linear_l1=args.ftrl_l1, linear_l2=args.ftrl_l2, linear_grad_scale=args.ftrl_grad_scale)
    return FFMConfig(num_dims=nd, num_fields=fields, k=args.ffm_k, field_bounds=args.ffm_bounds, lr=args.alpha,
                     consistency=args.consistency, staleness=args.staleness, seed=args.seed, **lin)


def _load_input(args, comm):
    """This rank's libsvm shard: static byte-range blocks, or blocks handed out by the locality-aware
    assigner that rank 0 serves (reference HDFSManager: node 0 runs the HDFSBlockAssigner)."""
    from ._native import runtime
    from .data.loader import LibsvmData

    url = args.input
    if args.hdfs_namenode and "://" not in url:
        auth = (f"webhdfs://{args.hdfs_namenode}:{args.hdfs_http_port}" if args.hdfs_http_port > 0
                else f"hdfs://{args.hdfs_namenode}:{args.hdfs_namenode_port}")
        url = auth + ("" if url.startswith("/") else "/") + url
    if args.assigner_master_port <= 0:
        return LibsvmData(url, comm.rank, comm.world)
    srv = None
    if comm.rank == 0:
        srv = runtime().BlockAssignerServer(args.assigner_master_port)
        srv.start()
    master = os.environ.get("MASTER_ADDR", "127.0.0.1")
    data = LibsvmData(url, comm.rank, comm.world, assigner=f"{master}:{args.assigner_master_port}",
                      host=runtime().local_host_name())
    if srv is not None:  # serve until every loader thread of every rank has exited (kExit)
        srv.wait_done(600.0)
        print(f"[rank 0] block assigner: {srv.local_served} local / {srv.remote_served} remote blocks", flush=True)
        srv.stop()
    return data


class _Resident:
    """The data stream of --model gbdt: the shard is resident in the model, a boosting round draws nothing."""

    def __init__(self, synth):
        self.synth = synth

    def next(self):
        return None

    def skip(self, k: int):
        pass

    def holdout(self, seed: int):
        return self.synth.holdout(seed)


SMALL_CARDS = [50, 7, 300, 20, 5, 60, 90, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
               28]


def _opt_kw(args) -> dict:
    """--clip_norm / --lr_* as GPT2Config / MLPConfig fields."""
    return dict(clip_norm=args.clip_norm or None, lr_warmup=args.lr_warmup, lr_decay_steps=args.lr_decay_steps,
                lr_min_ratio=args.lr_min_ratio)


def build(args, comm):
    """-> (model, tables {id: table}, make_data() -> a fresh data stream with next()/skip(), step
    fn(batch) -> loss, samples/step). A fresh stream + skip(k) repositions the data at iteration k
    (restart and in-place rollback)."""
    dev = comm.device
    r = comm.rank
    seed = args.seed * 1000 + r
    if args.model in ("widedeep", "deepfm", "dcn"):  # deepfm / dcn: the same model with the FM term / cross layers
        from .data.synthetic import CriteoSynth
        from .models.widedeep import WideDeep, WideDeepConfig

        B = args.batch or (64 if args.small else 16384)
        wide = {}
        if args.wide_optimizer == "ftrl":
            wide = dict(wide_optimizer="ftrl", wide_alpha=args.ftrl_alpha, wide_beta=args.ftrl_beta,
                        wide_l1=args.ftrl_l1, wide_l2=args.ftrl_l2,
                        wide_grad_scale=args.ftrl_grad_scale or float(B * comm.world))
        cfg = WideDeepConfig(consistency=args.consistency, staleness=args.staleness, transport=args.transport,
                             max_batch=B, fm_term=args.model == "deepfm",
                             cross_layers=args.cross_layers if args.model == "dcn" else 0,
                             **({"cards": SMALL_CARDS} if args.small else {}), **wide)
        m = WideDeep(cfg, comm)
        return m, {0: m.emb, 1: m.dense}, (lambda: CriteoSynth(B, cards=cfg.cards, device=dev, seed=seed)), \
            (lambda b: m.train_step(*b)), B
    if args.model == "mlp":
        from .data.synthetic import MnistSynth
        from .models.mlp import MLP, MLPConfig

        m = MLP(MLPConfig(consistency=args.consistency, staleness=args.staleness, **_opt_kw(args)), comm)
        B = args.batch or (64 if args.small else 8192)
        return m, {0: m.table}, (lambda: _Skippable(MnistSynth(B, device=dev, seed=seed))), \
            (lambda b: m.train_step(*b)[0]), B
    if args.model == "dlrm":
        from .models.dlrm import DLRM, DLRMConfig

        B = args.batch or (64 if args.small else 16384)
        cfg = DLRMConfig(num_rows=20000 if args.small else 100_000_000, consistency=args.consistency,
                         staleness=args.staleness, transport=args.transport, max_batch=B)
        m = DLRM(cfg, comm)
        return m, {0: m.emb, 1: m.dense}, (lambda: _Skippable(_DLRMData(B, cfg, dev, seed))), \
            (lambda b: m.train_step(*b)), B
    if args.model == "gpt2":
        from .data.synthetic import TokenSynth
        from .models.gpt2 import GPT2, GPT2Config

        kw = dict(vocab=500, n_ctx=64, d=128, n_layer=2, n_head=2) if args.small else {}
        cfg = GPT2Config(consistency=args.consistency, staleness=args.staleness, **_opt_kw(args), **kw)
        m = GPT2(cfg, comm)
        B = args.batch or (2 if args.small else 8)
        return m, {0: m.table}, (lambda: _Skippable(TokenSynth(B, cfg.n_ctx, vocab=cfg.vocab, device=dev,             \
                                                               seed=seed))),                                          \
            (lambda b: m.train_step(*b)), B * cfg.n_ctx
    if args.model == "lr" and args.input:
        # reference LR on a libsvm file (lr_example.cpp --input): this rank's shard is loaded by the
        # native block assigner / mmap reader and kept resident in HBM; batches are consecutive
        # rows from a random start (lib/batch_data_sampler.cpp), cut on the device
        from .models.lr import SparseLR, SparseLRConfig

        shard = args._shard.to(dev)
        nd = args.num_dims
        if not nd:  # every rank must size the table alike: max feature id over all shards
            t = torch.tensor([float(shard.cols.max()) + 1 if shard.cols.numel() else 1.0], device=dev)
            comm.all_reduce_(t, op=dist.ReduceOp.MAX)
            nd = int(t.item())
        m = SparseLR(SparseLRConfig(num_dims=nd, alpha=args.alpha, consistency=args.consistency,
                                    staleness=args.staleness, storage=args.kStorageType,
                                    value_dtype=getattr(torch, args.value_dtype), **_ftrl_kw(args)), comm)
        B = args.batch or 1024
        W = max(1, args.num_workers_per_node)
        return m, {0: m.table}, (lambda: _Skippable(_WorkerGroup([_Batches(shard, B, seed + _WSEED * w)
                                                                  for w in range(W)]))), \
            (lambda b: -m.train_step(*b)), B * W
    if args.model == "lr":
        from .data.synthetic import SparseLRSynth
        from .models.lr import SparseLR, SparseLRConfig

        nd = args.num_dims or (5000 if args.small else 16_609_143)
        m = SparseLR(SparseLRConfig(num_dims=nd, alpha=args.alpha, consistency=args.consistency,
                                    staleness=args.staleness, storage=args.kStorageType,
                                    value_dtype=getattr(torch, args.value_dtype), **_ftrl_kw(args)), comm)
        B = args.batch or (128 if args.small else 65536)
        W = max(1, args.num_workers_per_node)
        return m, {0: m.table}, \
            (lambda: _Skippable(_WorkerGroup([SparseLRSynth(B, num_dims=nd, nnz=16 if args.small else 64, device=dev,
                                                            seed=seed + _WSEED * w) for w in range(W)]))), \
            (lambda b: -m.train_step(*b)), B * W
    if args.model == "fm" and args.input:
        # a libsvm file through the LR loader path: the shard resident in HBM, batches cut on the device
        from .models.fm import FM

        shard = args._shard.to(dev)
        nd = args.num_dims
        if not nd:  # every rank must size the table alike: max feature id over all shards
            t = torch.tensor([float(shard.cols.max()) + 1 if shard.cols.numel() else 1.0], device=dev)
            comm.all_reduce_(t, op=dist.ReduceOp.MAX)
            nd = int(t.item())
        B = args.batch or 1024
        m = FM(_fm_cfg(args, comm, nd, B), comm)
        return m, {0: m.table, **({1: m.bias} if m.bias is not None else {})}, \
            (lambda: _Skippable(_Batches(shard, B, seed))), (lambda b: m.train_step(*b)), B
    if args.model == "fm":
        from .data.synthetic import FMSynth
        from .models.fm import FM

        fields = args.fm_fields or (8 if args.small else 64)
        card = args.fm_card or (32 if args.small else 262144)
        B = args.batch or (128 if args.small else 65536)
        m = FM(_fm_cfg(args, comm, fields * card, B), comm)
        # one teacher for every rank (seed), this rank's own sample stream
        return m, {0: m.table, **({1: m.bias} if m.bias is not None else {})}, \
            (lambda: _Skippable(FMSynth(B, fields=fields, card=card, device=dev, seed=args.seed).holdout(seed + 1))), \
            (lambda b: m.train_step(*b)), B
    if args.model == "ffm" and args.input:
        # a libsvm file through the LR loader path; a key's field comes from its key range
        from .models.ffm import FFM

        shard = args._shard.to(dev)
        nd = args.num_dims
        if not nd:  # every rank must size the table alike: max feature id over all shards
            t = torch.tensor([float(shard.cols.max()) + 1 if shard.cols.numel() else 1.0], device=dev)
            comm.all_reduce_(t, op=dist.ReduceOp.MAX)
            nd = int(t.item())
        B = args.batch or 1024
        m = FFM(_ffm_cfg(args, comm, nd, args.ffm_fields), comm)
        return m, {0: m.table, **({1: m.bias} if m.bias is not None else {})}, \
            (lambda: _Skippable(_Batches(shard, B, seed))), (lambda b: m.train_step(*b)), B
    if args.model == "ffm":
        from .data.synthetic import FFMSynth
        from .models.ffm import FFM

        fields = args.fm_fields or (8 if args.small else 64)
        card = args.fm_card or (32 if args.small else 262144)
        B = args.batch or (128 if args.small else 16384)
        m = FFM(_ffm_cfg(args, comm, fields * card, fields), comm)
        # one teacher for every rank (seed), this rank's own sample stream
        return m, {0: m.table, **({1: m.bias} if m.bias is not None else {})}, \
            (lambda: _Skippable(FFMSynth(B, fields=fields, card=card, device=dev, seed=args.seed).holdout(seed + 1))), \
            (lambda b: m.train_step(*b)), B
    if args.model == "gbdt":
        from .data.synthetic import GBDTSynth
        from .models.gbdt import GBDT, GBDTConfig

        F = args.gbdt_features
        m = GBDT(GBDTConfig(num_features=F, num_bins=args.gbdt_bins, depth=args.gbdt_depth, lr=args.gbdt_lr,
                            reg_lambda=args.gbdt_lambda, max_trees=max(args.steps, 1)), comm)
        synth = None
        if args.input:  # the libsvm shard densified once: an absent feature is 0.0, keys beyond F are dropped
            shard = args._shard.to(dev)
            X = torch.zeros(shard.n, F, dtype=torch.float32, device=dev)
            row = torch.repeat_interleave(torch.arange(shard.n, device=dev), shard.rowptr[1:] - shard.rowptr[:-1])
            ok = (shard.cols >= 0) & (shard.cols < F)
            X.index_put_((row[ok], shard.cols[ok]), shard.vals[ok], accumulate=True)
            y = shard.labels
        else:  # one teacher, this rank's own samples
            synth = GBDTSynth(args.gbdt_rows, features=F, device=dev, seed=args.seed).holdout(seed + 1)
            X, y = synth.next()
        m.make_cuts(X)
        m.attach(X, y)
        rows = X.shape[0]
        # boost() returns the loss summed over every rank's samples
        return m, {}, (lambda: _Resident(synth)), (lambda b: m.boost() / comm.world), max(rows, 1)
    if args.model == "lda":
        from .models.lda import LDA, LDAConfig

        if args.input:  # every line a document of word:count pairs (the label is ignored); this rank's lines
            shard = args._shard
            rp_f, words = shard.rowptr.long().cpu(), shard.cols.long().cpu()
            cnt = shard.vals.cpu().round().clamp(min=0).long()
            doc = torch.repeat_interleave(torch.arange(shard.n), rp_f[1:] - rp_f[:-1])
            words, doc = torch.repeat_interleave(words, cnt), torch.repeat_interleave(doc, cnt)
            rp = torch.zeros(shard.n + 1, dtype=torch.int64)
            rp[1:] = torch.cumsum(torch.bincount(doc, minlength=shard.n), 0)
            t = torch.zeros(comm.world + 1, dtype=torch.int64, device=dev)
            t[comm.rank] = shard.n
            comm.all_reduce_(t)  # the documents of the ranks before this one: the global ids
            base = int(t[: comm.rank].sum())
            vmax = torch.tensor([int(words.max()) + 1 if words.numel() else 1], dtype=torch.int64, device=dev)
            comm.all_reduce_(vmax, op=dist.ReduceOp.MAX)
            V = args.lda_vocab if args.lda_vocab is not None else int(vmax)
        else:  # one corpus for every rank (seed), this rank's even slice of its documents
            from .data.synthetic import LDASynth
            from .ps.tables import even_bounds

            synth = LDASynth(args.lda_topics, args.lda_vocab, args.lda_docs, args.lda_doc_len, seed=args.seed)
            b = even_bounds(args.lda_docs, comm.world)
            base, hi = b[comm.rank], b[comm.rank + 1]
            rp = synth.rowptr[base:hi + 1] - synth.rowptr[base]
            words = synth.words[int(synth.rowptr[base]):int(synth.rowptr[hi])]
            V = args.lda_vocab
        m = LDA(LDAConfig(num_topics=args.lda_topics, vocab=V, alpha=args.lda_alpha, beta=args.lda_beta,
                          batch_docs=args.batch or 4096, seed=args.seed), comm)
        m.attach(rp, words, base)
        m.init()

        def lda_step(_):  # a sweep; the loss (collective, read on the host) at the driver's report intervals only
            m.sweep()
            report = m.it % 10 == 0 or m.it == args.steps
            return torch.tensor([-m.loglik() if report else 0.0], device=dev)

        return m, {}, (lambda: _Resident(None)), lda_step, 1
    if args.model == "w2v":
        from .models.word2vec import Word2Vec, Word2VecConfig

        if args.input:  # every line a sentence, its words in file order (label and values ignored); this rank's lines
            shard = args._shard
            rp, words = shard.rowptr.long().cpu(), shard.cols.long().cpu()
            t = torch.zeros(comm.world + 1, dtype=torch.int64, device=dev)
            t[comm.rank] = words.numel()
            comm.all_reduce_(t)  # the tokens of the ranks before this one: the global token positions
            base = int(t[: comm.rank].sum())
            vmax = torch.tensor([int(words.max()) + 1 if words.numel() else 1], dtype=torch.int64, device=dev)
            comm.all_reduce_(vmax, op=dist.ReduceOp.MAX)
            V = args.w2v_vocab if args.w2v_vocab is not None else int(vmax)
            if words.numel() and int(words.max()) >= V:
                raise ValueError(f"w2v: the input holds the word id {int(words.max()) + 1}, --w2v_vocab is {V}")
            args._w2v_group = 0
        else:  # one corpus for every rank (seed), this rank's even slice of its sentences
            from .data.synthetic import W2VSynth
            from .ps.tables import even_bounds

            groups = 8 if args.small else 256
            V = args.w2v_vocab
            synth = W2VSynth(groups, V // groups, args.w2v_sentences, args.w2v_len, seed=args.seed)
            b = even_bounds(args.w2v_sentences, comm.world)
            lo, hi = b[comm.rank], b[comm.rank + 1]
            base = int(synth.rowptr[lo])
            rp = synth.rowptr[lo:hi + 1] - base
            words = synth.tokens[base:int(synth.rowptr[hi])]
            args._w2v_group = V // groups
        m = Word2Vec(Word2VecConfig(vocab=V, dim=args.w2v_dim, negatives=args.w2v_negatives, window=args.w2v_window,
                                    sample=args.w2v_sample, lr=args.alpha, batch_pairs=args.batch or 65536,
                                    seed=args.seed, consistency=args.consistency, staleness=args.staleness), comm)
        counts = torch.bincount(words, minlength=V).to(dev)
        comm.all_reduce_(counts)
        m.set_counts(counts)
        m.attach(words, rp, base)

        class _Epochs(_Resident):  # a restart at iteration k resumes with epoch k's draws
            def skip(self, k: int):
                m.epochs = k

        # epoch() returns the epoch's mean pair loss over all ranks (collective, read on the host once an epoch)
        return m, {0: m.table}, (lambda: _Epochs(None)), (lambda _: torch.tensor([m.epoch()], device=dev)), 1
    if args.model == "kmeans" and args.input:
        # the reference K-Means input: sparse libsvm points (kmeans.cpp reads --input); the
        # shard stays resident in HBM and batches are consecutive rows, cut on the device
        from .models.kmeans import KMeans, KMeansConfig

        shard = args._shard.to(dev)
        nd = args.num_dims
        if not nd:  # every rank must size the table alike: max feature id over all shards
            t = torch.tensor([float(shard.cols.max()) + 1 if shard.cols.numel() else 1.0], device=dev)
            comm.all_reduce_(t, op=dist.ReduceOp.MAX)
            nd = int(t.item())
        cfg = KMeansConfig(K=args.K or 8, dims=nd, consistency=args.consistency, staleness=args.staleness,
                           init_mode=args.kmeans_init_mode or "random", seed=seed)
        B = args.batch or 256
        init = None
        if args.kmeans_init_mode:
            rp, c, v, _ = shard.batch(0, max(B, cfg.K))
            init = torch.zeros(rp.numel() - 1, nd, dtype=torch.float32, device=dev)
            row = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=dev), rp[1:] - rp[:-1])
            ok = c < nd
            init.index_put_((row[ok], c[ok]), v[ok], accumulate=True)  # densify the seeding batch only
        m = KMeans(cfg, comm, init_data=init)
        return m, {0: m.table}, (lambda: _Skippable(_Batches(shard, B, seed))), \
            (lambda b: m.train_step_csr(b[0], b[1], b[2])), B
    if args.model == "kmeans":
        from .models.kmeans import KMeans, KMeansConfig

        cfg = KMeansConfig(K=args.K or (8 if args.small else 1000), dims=16 if args.small else 128,
                           consistency=args.consistency, staleness=args.staleness,
                           init_mode=args.kmeans_init_mode or "random", seed=seed)
        B = args.batch or (256 if args.small else 65536)
        # seeding reads its own batch of local data (rank 0's seeds are broadcast)
        init = _GaussData(max(B, cfg.K), cfg.dims, dev, seed + 7919).next() if args.kmeans_init_mode else None
        m = KMeans(cfg, comm, init_data=init)
        return m, {0: m.table}, (lambda: _Skippable(_GaussData(B, cfg.dims, dev, seed))), (lambda b: m.train_step(b)), B
    raise ValueError(args.model)


_WSEED = 104729


class _WorkerGroup:
    """``--num_workers_per_node`` logical workers on one GPU rank (the reference runs that many
    worker threads per process over the node's data, driver/engine.cpp:266-288, lr_example.cpp:
    203-207): each worker keeps its own sampler (own start point / seed, its own batch_size), and
    the W CSR batches of a clock are concatenated into ONE Get / Add / Clock -- one set of launches
    instead of W. Under BSP this is exactly the reference's result: all W workers read the clock-c
    parameters and the server sums their pushes (VectorStorage::SubAdd is additive); under SSP/ASP
    the workers of a rank advance together, a schedule both models admit."""

    def __init__(self, its):
        self.its = its

    def next(self):
        parts = [it.next() for it in self.its]
        if len(parts) == 1:
            return parts[0]
        rps, off = [], 0
        for i, (rp, c, _, _) in enumerate(parts):
            rps.append((rp if i == 0 else rp[1:]) + off)
            off += c.numel()
        return (torch.cat(rps), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                torch.cat([p[3] for p in parts]))


class _Skippable:
    def __init__(self, inner):
        self.inner = inner

    def next(self):
        return self.inner.next()

    def skip(self, n):
        for _ in range(n):
            self.inner.next()

    def holdout(self, seed):
        return self.inner.holdout(seed)


class _Batches:
    def __init__(self, shard, B, seed):
        self.it = shard.batches(B, seed=seed)

    def next(self):
        return next(self.it)


class _DLRMData:
    def __init__(self, B, cfg, dev, seed):
        from .data.synthetic import DLRMSynth

        self.gen = DLRMSynth(B, cfg.F, cfg.num_rows, cfg.n_dense, device=dev, seed=seed)

    def next(self):
        return self.gen.next()

    def holdout(self, seed):
        return self.gen.holdout(seed)


class _GaussData:
    def __init__(self, B, D, dev, seed):
        self.B, self.D, self.dev = B, D, dev
        self.g = torch.Generator(device=dev)
        self.g.manual_seed(seed)

    def next(self):
        return torch.randn(self.B, self.D, generator=self.g, device=self.dev)


def _is_comm_failure(e: BaseException) -> bool:
    """A collective failed because a peer died or the communicator was aborted -- by type, not by
    message: RCCL (TORCH_NCCL_ASYNC_ERROR_HANDLING=2: an aborted / timed-out communicator) and the
    c10d store raise the torch.distributed error classes (DistBackendError, DistNetworkError,
    DistStoreError); gloo's transport raises a RuntimeError tagged with its gloo source location
    ("[.../gloo/transport/tcp/pair.cc:547] Connection closed by peer"). Errors of this process's
    own code (a failed kernel, the async PS server) are not peer failures and propagate."""
    if isinstance(e, dist.DistError):
        return True
    head = str(e).split("]", 1)[0]
    return isinstance(e, RuntimeError) and head.startswith("[") and "/gloo/" in head


def _force_quit(comm, has_data: bool, rank: int):
    """Graceful degradation (reference lr_example.cpp:145-152, mailbox.cpp:159-171): a rank with
    no data leaves and the others continue among themselves. Every rank learns every rank's flag
    (one all-gather), the survivors form a sub-group (collective over the full group); a quitting
    rank returns None. Survivors get a Comm over their group: the tables are built on it, so
    they are sharded over the survivors only."""
    from .ps.comm import Comm
    from .utils import metrics

    if comm.world == 1:
        return comm
    flags = torch.empty(comm.world, dtype=torch.float32, device=comm.device)
    comm.all_gather(flags, torch.tensor([1.0 if has_data else 0.0], device=comm.device))
    survivors = [r for r, f in enumerate(flags.tolist()) if f > 0]
    if len(survivors) == comm.world:
        return comm
    if not survivors:
        raise RuntimeError("no rank has any data")
    quitters = sorted(set(range(comm.world)) - set(survivors))
    if rank == survivors[0]:
        metrics.fault_tolerance_phase(2, f"kForceQuit from ranks {quitters} (no data); {len(survivors)} ranks continue")
    group = dist.new_group(survivors)
    if not has_data:
        print(f"[rank {rank}] kForceQuit: no data, leaving the job", file=sys.stderr, flush=True)
        return None
    return Comm(group=group, device=comm.device)


class _ckpt_state:
    """Heartbeat state "ckpt" while a checkpoint is written / committed: a multi-GB shard write
    advances no step, and the supervisor gives that state its own (long) limit instead of the
    stuck-in-a-step progress timeout."""

    def __init__(self, hb):
        self.hb = hb

    def __enter__(self):
        if self.hb is not None:
            self.prev, self.hb.state = self.hb.state, "ckpt"

    def __exit__(self, *exc):
        if self.hb is not None:
            self.hb.state = self.prev


def _scale_directive(hb_dir: str, generation: int) -> dict | None:
    """A supervisor scale directive newer than ``generation`` (None: none, or a failure rollback)."""
    try:
        d = json.loads(open(os.path.join(hb_dir, "rollback.json")).read())
    except (OSError, ValueError):
        return None
    return d if d.get("kind") == "scale" and int(d.get("generation", -1)) > generation else None


def _wait_directive(hb_dir: str, generation: int, timeout: float = 300.0) -> dict:
    """Rollback directive of the supervisor (minips_amd.elastic): a newer generation with the
    rendezvous port of the re-formed group (the reference's kRollBack, mailbox.cpp:172-191)."""
    path = os.path.join(hb_dir, "rollback.json")
    t0 = time.time()
    while time.time() - t0 < timeout:
        try:
            d = json.loads(open(path).read())
            if int(d["generation"]) > generation:
                return d
        except (OSError, ValueError, KeyError):
            pass
        time.sleep(0.05)
    raise TimeoutError("no rollback directive from the supervisor")


def main(argv=None):
    args = parse(argv)
    from .ps.checkpoint import Checkpointer
    from .ps.comm import init_distributed
    from .ps.fault import FaultInjector, Heartbeat
    from .utils import metrics

    if args.metrics_dir:
        os.environ["MINIPS_METRICS_DIR"] = args.metrics_dir
    os.environ["MINIPS_ASP_DEPTH"] = str(max(0, args.asp_depth))
    if args.asp_bound >= 0:
        os.environ["MINIPS_ASP_BOUND"] = str(args.asp_bound)
    # the asynchronous tables' peers hold IPC mappings of every shard and a shared board: a lost
    # rank restarts the whole set from the checkpoint, never an in-place rollback
    inplace = args.recovery == "inplace" and bool(args.heartbeat_dir) and args.transport != "onesided"
    if inplace:  # RCCL: a dead peer aborts the communicator and raises, instead of killing us
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "2")
    comm = init_distributed()
    rank = comm.rank
    generation = int(os.environ.get("MINIPS_GENERATION", "0"))
    hb = Heartbeat(args.heartbeat_dir, rank, args.heartbeat_interval, state_fn=lambda: comm.state()) \
        if args.heartbeat_interval > 0 and args.heartbeat_dir else None
    if hb is not None:
        # what this rank can recover from: the supervisor takes the in-place branch only if EVERY
        # rank can roll back in its process (the one-sided tables cannot: peers hold IPC mappings of
        # the dead rank's shards and a shared progress board -- the whole set restarts instead)
        hb.write_caps(inplace=inplace, transport=args.transport)
    if args.model in ("lr", "kmeans", "fm", "ffm", "gbdt", "lda", "w2v") and args.input:
        from .data.loader import LibsvmData

        args._shard = _load_input(args, comm)
        sub = _force_quit(comm, args._shard.n > 0 and args.force_quit_rank != rank, rank)
        if sub is None:
            if hb:
                hb.stop()
            dist.destroy_process_group()
            return 0
        if sub is not comm:
            comm = sub
            inplace = False  # a sub-group job restarts as a whole (its ranks are a subset)
    model, tables, make_data, step_fn, per_step = build(args, comm)
    data = make_data()
    ck = Checkpointer(comm, args.checkpoint_file_prefix, text_limit=args.checkpoint_text_limit)
    start = 0
    if args.use_weight_file and not ck.exists():
        # a restart before the first committed checkpoint (or with checkpoint_toggle off): there
        # is nothing to roll back to, so the relaunched job starts over
        print(f"[rank {rank}] --use_weight_file but no committed checkpoint under "
              f"{args.checkpoint_file_prefix!r}: starting from iteration 0", file=sys.stderr, flush=True)
    elif args.use_weight_file:
        start = ck.load(tables)
        data.skip(start)
        failed = int(os.environ.get("MINIPS_FAILED_RANK", "-1"))
        metrics.fault_tolerance_phase(4 if rank == failed else 5, f"rank {rank} restored iteration {start}")
    if hb:
        hb.progress(start - 1)
    inj = FaultInjector(rank, args.fail_rank, args.fail_step, args.with_injected_straggler, args.seed,
                        mode=args.fail_mode, heartbeat=hb)
    log = metrics.get_logger()
    losses = []
    evals = []  # [iteration, auc, logloss, n] per held-out evaluation (--eval_every)
    t_eval = 0.0  # wall time spent evaluating since t_steady (excluded from steady_ms_per_iter)

    def evaluate(it_done: int):
        """All ranks: the same --eval_batches held-out batches every time (the stream is re-created:
        this rank's teacher, its own slice by seed), summed over the ranks."""
        nonlocal t_eval
        if comm.device.type == "cuda":
            torch.cuda.synchronize(comm.device)
        t0 = time.perf_counter()
        held = make_data().holdout(args.eval_seed * 1000 + rank)
        r = model.evaluate(held.next() for _ in range(args.eval_batches))
        if comm.device.type == "cuda":
            torch.cuda.synchronize(comm.device)
        dt = time.perf_counter() - t0
        t_eval += dt
        evals.append([it_done, r["auc"], r["logloss"], r["n"]])
        log.event("eval", step=it_done, auc=r["auc"], auc_slack=r["auc_slack"], logloss=r["logloss"], n=r["n"],
                  n_pos=r["n_pos"], n_nan=r["n_nan"], eval_ms=round(dt * 1e3, 3))
        if rank == 0:
            auc = "nan" if r["auc"] is None else f"{r['auc']:.5f}"
            ll = "nan" if r["logloss"] is None else f"{r['logloss']:.5f}"
            print(f"Eval iteration={it_done} auc={auc} logloss={ll} n={r['n']}", flush=True)
    report = open(args.report_prefix + f"report_{rank}", "a") if args.report_prefix else None
    t_start = time.perf_counter()
    t_steady, n_steady = None, 0

    def rollback():
        """Survivor side of an in-place recovery (reference: mailbox.cpp:172-191 kRollBack ->
        RollBackServer / RollBackWorker): drop the broken communicator, join the re-formed group
        on the supervisor's new rendezvous, restore every table from the last committed
        checkpoint and reposition the data; the relaunched rank restores the same iteration."""
        nonlocal generation, data, losses
        hb.state = "recover"
        ck.abandon()
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001 - the group is already broken
            pass
        d = _wait_directive(args.heartbeat_dir, generation)
        generation = int(d["generation"])
        os.environ["MASTER_PORT"] = str(d["port"])
        os.environ["MINIPS_GENERATION"] = str(generation)
        dist.destroy_process_group() if dist.is_initialized() else None
        init_distributed()
        comm.refresh()
        for t in tables.values():
            t.reset_after_rollback()
        if hasattr(model, "_pending_plans"):
            model._pending_plans = []  # planned on the broken communicator
        if not ck.exists():
            raise RuntimeError("in-place rollback needs a committed checkpoint")
        it0 = ck.load(tables)
        data = make_data()
        data.skip(it0)
        losses = [x for x in losses if x[0] < it0]
        evals[:] = [e for e in evals if e[0] <= it0]
        metrics.fault_tolerance_phase(5, f"rank {rank} rolled back in place to iteration {it0} "
                                         f"(failed rank {d.get('failed_rank')}, generation {generation})")
        hb.state = "run"
        hb.progress(it0 - 1)
        return it0

    def scale(it_now: int):
        """Live rescale at a step boundary (the reference's kScaleRollback): every rank of the old
        group checkpoints iteration ``it_now``, leaves the group; ranks < the new world re-form it
        in this process, rebuild their tables on the new shard ranges and restore (reshard) that
        checkpoint; the others retire. Returns the iteration to continue from, or None (retired)."""
        nonlocal generation, data, losses, model, tables, make_data, step_fn, per_step, ck
        hb.state = "recover"
        model.drain()
        with _ckpt_state(hb):
            ck.save(tables, iteration=it_now, blocking=True)
            ck.commit()
        d = _wait_directive(args.heartbeat_dir, generation)
        generation, world = int(d["generation"]), int(d["world"])
        comm.barrier()
        ps = getattr(comm, "_async_ps", None)
        if ps is not None:
            # one-sided tables: stop this owner's server thread (it holds raw pointers to the shards
            # and inboxes freed below) and drop the board; build() makes a fresh AsyncPS on the new
            # group, whose ranks (new ones included) all join its rendezvous
            ps.close()
            comm._async_ps = None
        dist.destroy_process_group()
        if rank >= world:
            metrics.fault_tolerance_phase(5, f"rank {rank} retired by the scale to {world} ranks at iteration {it_now}")
            hb.stop()
            return None
        os.environ.update(MASTER_PORT=str(d["port"]), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                          MINIPS_GENERATION=str(generation))
        model = tables = step_fn = None  # free the old shards before the new ones are allocated
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        init_distributed()
        comm.refresh()
        model, tables, make_data, step_fn, per_step = build(args, comm)
        ck = Checkpointer(comm, args.checkpoint_file_prefix, text_limit=args.checkpoint_text_limit)
        it0 = ck.load(tables)
        data = make_data()
        data.skip(it0)
        losses = [x for x in losses if x[0] < it0]
        evals[:] = [e for e in evals if e[0] <= it0]
        metrics.fault_tolerance_phase(5, f"rank {rank} rescaled in place to {world} ranks at iteration {it0} "
                                         f"(generation {generation})")
        hb.state = "run"
        hb.progress(it0 - 1)
        return it0

    it = start
    while it < args.steps:
        # (the rule depends on ``it`` only: ranks started by a scale-out resume at the same
        # iteration as the survivors and must take part in the same checks)
        if hb is not None and args.scale_check_every > 0 and it % args.scale_check_every == 0:
            # do the ranks agree that a scale directive is pending? (all of them act at THIS step)
            d = _scale_directive(args.heartbeat_dir, generation)
            flag = torch.tensor([float(d["generation"]) if d else 0.0], device=comm.device)
            comm.all_reduce_(flag, op=dist.ReduceOp.MAX)
            if float(flag) > generation:
                nxt = scale(it)
                if nxt is None:
                    return 0
                it = nxt
                t_steady = None
                continue
        try:
            if it == start + args.timing_skip and t_steady is None:
                if comm.device.type == "cuda":
                    torch.cuda.synchronize(comm.device)
                t_steady, n_steady, t_eval = time.perf_counter(), args.steps - it, 0.0
            with _ckpt_state(hb):  # checkpoint phases are not steps: their own heartbeat state
                if args.checkpoint_commit == "async":
                    ck.try_commit()  # publishes an in-flight checkpoint once every rank's files are written
                else:
                    ck.commit()  # publishes the checkpoint issued after the previous step (no-op otherwise)
            inj.step(it)
            t0 = time.perf_counter()
            with metrics.range(f"step {it}"):
                batch = data.next()
                inj.in_step(it)
                loss = step_fn(batch)
            if (it + 1) % 10 == 0 or it + 1 == args.steps:
                with comm.waiting():
                    lv = float(loss.float().sum()) / per_step
                losses.append((it, lv))
                opt = {}
                if args.opt_flags:  # (read at report intervals only: clip_stats() drains the clock)
                    tab = tables[0]
                    opt["lr"] = tab.lr_at(tab.step)
                    if tab.clip_norm is not None:
                        cs = tab.clip_stats()
                        opt.update(grad_norm=cs["norm"], clip_scale=cs["scale"])
                log.step(it, per_step, time.perf_counter() - t0, comm.stats, loss=lv, **opt)
                if rank == 0:
                    print(f"Current iteration={it + 1} on node={rank} loss={lv:.5f}"
                          + "".join(f" {k}={v:.6g}" for k, v in opt.items()), flush=True)
            if report and (it + 1) % args.report_interval == 0:
                report.write(f"{it + 1}\t{(time.perf_counter() - t_start) * 1e3:.1f}\n")
                report.flush()
            if args.checkpoint_toggle and args.checkpoint_every > 0 and (it + 1) % args.checkpoint_every == 0 \
                    and it + 1 < args.steps:
                with _ckpt_state(hb):
                    ck.save(tables, iteration=it + 1)
            if hb:
                hb.progress(it)
            it += 1
            if args.eval_every > 0 and it % args.eval_every == 0 and it < args.steps:
                evaluate(it)
        except Exception as e:  # noqa: BLE001
            if not (inplace and hb is not None and comm.world > 1 and _is_comm_failure(e)):
                raise
            print(f"[rank {rank}] collective failed at iteration {it} ({type(e).__name__}): rolling back in place",
                  file=sys.stderr, flush=True)
            it = rollback()
            t_steady = None
    model.drain()
    if comm.device.type == "cuda":
        torch.cuda.synchronize(comm.device)
    steady_ms = ((time.perf_counter() - t_steady - t_eval) * 1e3 / n_steady
                 if t_steady is not None and n_steady else None)
    if args.eval_every > 0:
        evaluate(args.steps)
    with _ckpt_state(hb):
        ck.commit()
    # parameter checksum over every table (identical on all ranks): the parameter values only
    # (hash tables also export their keys, which are not parameters)
    def _param_sum(t):
        arrays = t.shard_state()[1]
        a = arrays.get("params", arrays.get("master", arrays.get("rows")))
        if a is None:
            a = next(iter(arrays.values()))
        return float(a.double().sum())

    sums = torch.tensor([_param_sum(t) for t in tables.values()], dtype=torch.float64, device=comm.device)
    if tables:
        comm.all_reduce_(sums)
    if comm.device.type == "cuda":
        torch.cuda.synchronize(comm.device)
    if hb:
        hb.stop()
    ftrl_final = {}
    if args.model == "gbdt":  # every rank holds the same trees: the checksum is the sum of their leaves
        sums = model.leaf[: model.num_trees].double().sum().reshape(1)
        ftrl_final.update(gbdt_trees=model.num_trees, gbdt_depth=model.cfg.depth, gbdt_bins=model.cfg.num_bins)
        if args.gbdt_model_out and comm.rank == 0:
            model.save(args.gbdt_model_out)
    if args.model == "lda":  # the topic totals are replicated: their sum is the corpus's token count
        sums = model.nk.double().sum().reshape(1)
        ftrl_final.update(lda_topics=model.K, lda_tokens=int(model.nk.sum()), lda_loglik=round(model.loglik(), 6))
    if args.model == "w2v":  # vectors() is a collective Get; the purity of the planted groups is read on the host
        ftrl_final.update(w2v_dim=model.d, w2v_pairs=model.total_pairs)
        if args._w2v_group:
            from .models.word2vec import purity

            ftrl_final["w2v_purity"] = round(purity(model.vectors(), args._w2v_group), 6)
    if args.sparse_optimizer == "ftrl":  # a collective: every rank counts its shard
        ftrl_final = dict(nnz=model.nnz(), sparse_optimizer="ftrl")
    if args.wide_optimizer == "ftrl" and args.model in ("fm", "ffm"):  # likewise a collective
        ftrl_final = dict(linear_nnz=model.linear_nnz(), wide_optimizer="ftrl")
    elif args.wide_optimizer == "ftrl":  # likewise a collective
        ftrl_final = dict(wide_nnz=model.wide_nnz(), wide_optimizer="ftrl")
    if args.model == "deepfm":
        ftrl_final["fm_term"] = True
    if args.model == "dcn":
        ftrl_final["cross_layers"] = args.cross_layers
    if args.model == "ffm":
        ftrl_final.update(ffm_fields=model.cfg.num_fields, ffm_k=model.cfg.k)
    clip_final = {}
    if args.clip_norm:
        cs = tables[0].clip_stats()
        clip_final = dict(clipped_steps=cs["clipped"], skipped_steps=cs["skipped"])
    if comm.rank == 0:
        print(json.dumps(dict(model=args.model, steps=args.steps, start=start, losses=losses,
                              checksum=[round(float(x), 6) for x in sums.cpu()],
                              total_ms=round((time.perf_counter() - t_start) * 1e3, 1),
                              steady_ms_per_iter=round(steady_ms, 4) if steady_ms is not None else None,
                              world=comm.world, generation=generation,
                              **({"evals": evals} if args.eval_every > 0 else {}), **clip_final, **ftrl_final)),
              flush=True)
    if comm.world > 1:
        comm.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
