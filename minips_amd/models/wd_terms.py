"""The optional interaction terms of Wide & Deep (models/widedeep.py). ``forward`` adds a term to the wide logit behind
the input assembly, ``backward`` its gradient to the embedding gradient dX behind the dX dgrad, both over the buffers
``b`` of one batch size (WideDeep's, with what ``buffers`` returns merged in). WideDeepConfig's field ``option``
switches a term on (``what``: its name in the one-sided transport's refusal); WideDeep runs those in TERMS' order.
  name          the term's entry of the dense layout (``shape``; 64-aligned start), or None: no parameters, shape or
                init. The entries lie directly behind W1, inside layer 1's bucket, the last to go out: _bucket_done(1,
                ...) releases the later buckets before a term's gradient (written after the dX dgrad) exists.
  init          draws from the generator that has drawn every Wide & Deep parameter and the earlier terms' before, so
                switching a term on moves no existing initial value.
  reads_params  forward and backward read the pulled parameters P, and the backward adds into the gradient G:
                train_step orders both against the side-stream Adam from this flag alone.
  backward      adds to row perm[b F + f] of dX per lookup (b F + f without perm): where the dgrad wrote that row.
A new term of this family is one class here, its entry in TERMS and its WideDeepConfig field.
"""
from __future__ import annotations

import torch

from .. import ops


class FMTerm:
    """DeepFM (Guo et al., 2017): the factorization machine's second-order term over the F field embeddings the deep
    tower reads (the rule: csrc/kernels/deepfm.h). The backward adds dz (S - v) per lookup from the per-sample column
    sums S the forward kept. No parameter, table state or collective: it touches neither P nor G, so it may run before
    the step waits for the previous Adam and behind the point the next one waits for."""
    option, what, name, reads_params = "fm_term", "DeepFM term is", None, False

    def check(self, cfg):
        if not 1 <= cfg.emb_dim <= 64:
            raise ValueError(f"fm_term: emb_dim is {cfg.emb_dim}, expected 1 <= emb_dim <= 64")

    def buffers(self, model, B, train):
        return {"S": torch.empty(B, model.cfg.emb_dim, dtype=torch.float32, device=model.comm.device)}

    def forward(self, model, b, P):
        ops.wd_fm_forward(b["X"], model.cfg.F, model.cfg.emb_dim, b["wide"], b["S"])

    def backward(self, model, b, P, G, perm):
        ops.wd_fm_backward(b["X"], b["S"], b["dwide"], b["dX"], model.cfg.F, model.cfg.emb_dim, perm=perm)


class CrossTerm:
    """Deep & Cross (Wang et al., 2017): L vector-weight cross layers x_{l+1} = x_0 <x_l, w_l> + b_l + x_l over the
    whole assembled input (embeddings and dense features, d = k_in0 columns); wide += <x_L, w_c> (the rule:
    csrc/kernels/dcn.h). Parameters [w_0, b_0, ..., w_{L-1}, b_{L-1}, w_c] x align8(d), b_l = 0 at the start. The
    backward adds sum_j m_j w_j per lookup to dX and leaves per-chunk batch sums in ``part``, which the fold turns into
    the cross gradients in G. ``p`` and ``k`` are the forward's dot products and constants, kept for the backward."""
    option, what, name, reads_params = "cross_layers", "cross layers are", "cross", True

    def check(self, cfg):
        if not 1 <= cfg.emb_dim <= 64:
            raise ValueError(f"cross_layers: emb_dim is {cfg.emb_dim}, expected 1 <= emb_dim <= 64")
        d = cfg.F * cfg.emb_dim + cfg.n_dense
        if d > ops.CROSS_MAX_D:
            raise ValueError(f"cross_layers: the input has d = {d} columns, the kernels take d <= {ops.CROSS_MAX_D}")

    def shape(self, cfg, k_in0):
        return (2 * cfg.cross_layers + 1, (k_in0 + 7) // 8 * 8)

    def init(self, model, full, g):
        d = model.k_in[0]
        ops.kaiming_uniform_(model.view(full, "cross")[0::2, :d], d, g)

    def buffers(self, model, B, train):
        L, dev = model.cfg.cross_layers, model.comm.device
        bufs = dict(p=torch.empty(B, L + 1, dtype=torch.float32, device=dev),
                    k=torch.empty(L + 1, dtype=torch.float32, device=dev))
        if train:
            bufs["part"] = torch.empty(ops.wd_cross_part_shape(B, model.k_in[0], L), dtype=torch.float32, device=dev)
        return bufs

    def forward(self, model, b, P):
        ops.wd_cross_forward(b["X"], model.k_in[0], model.view(P, "cross"), model.cfg.cross_layers, b["wide"], b["p"],
                             b["k"])

    def backward(self, model, b, P, G, perm):
        cfg, d, Pc = model.cfg, model.k_in[0], model.view(P, "cross")
        ops.wd_cross_backward(b["X"], d, b["p"], b["k"], b["dwide"], Pc, cfg.cross_layers, b["dX"], cfg.F, cfg.emb_dim,
                              b["part"], perm=perm)
        ops.wd_cross_fold(b["part"], Pc, d, cfg.cross_layers, model.view(G, "cross"))


class CINTerm:
    """xDeepFM (Lian et al., 2018): a Compressed Interaction Network over the F field embeddings, X^k[h] = sum_{i, j}
    W^k[h, i, j] (X^{k-1}[i] o X^0[j]) with cin_layers = (H_1, ..., H_T) feature maps -- explicit vector-wise crosses
    of degree k + 1 -- whose sum-pooled maps enter the wide logit through w_out (the rule: csrc/kernels/cin.h).
    Parameters W^1 | ... | W^T | w_out (ops.wd_cin_layout, each part 64-aligned; the pad stays 0). The backward runs,
    per layer T .. 1, the weight gradient (per-chunk partials, folded into G) and the data backward; layer 1 adds the
    embedding gradient to dX. The buffers are the feature maps, their gradients and the partials."""
    option, what, name, reads_params = "cin_layers", "CIN layers are", "cin", True

    def check(self, cfg):
        try:
            ops.wd_cin_check(cfg.F, cfg.emb_dim, cfg.cin_layers)
        except RuntimeError as e:
            raise ValueError(f"cin_layers: {e}") from None

    def shape(self, cfg, k_in0):
        return (ops.wd_cin_layout(cfg.F, cfg.cin_layers)[1],)

    def init(self, model, full, g):
        F = model.cfg.F
        Ws, w_out = ops.wd_cin_views(model.view(full, "cin"), F, model.cfg.cin_layers)
        for W in Ws:
            ops.kaiming_uniform_(W[:, :, :F], W.shape[1] * F, g)
        ops.kaiming_uniform_(w_out, w_out.numel(), g)

    def buffers(self, model, B, train):
        cfg = model.cfg
        return {"cin": ops.wd_cin_buffers(B, cfg.F, cfg.emb_dim, cfg.cin_layers, model.comm.device, train=train)}

    def forward(self, model, b, P):
        cfg = model.cfg
        ops.wd_cin_forward(b["X"], cfg.F, cfg.emb_dim, model.view(P, "cin"), cfg.cin_layers, b["wide"], b["cin"])

    def backward(self, model, b, P, G, perm):
        cfg = model.cfg
        ops.wd_cin_backward(b["X"], cfg.F, cfg.emb_dim, model.view(P, "cin"), cfg.cin_layers, b["dwide"], b["dX"],
                            b["cin"], model.view(G, "cin"), perm=perm)


class AttnTerm:
    """AutoInt (Song et al., 2019): attn_layers interacting layers of attn_heads-head self-attention (head size
    attn_dim) with a residual over the F field embeddings; the last layer's output enters the wide logit through w_out
    (the rule: csrc/kernels/attnint.h). Parameters W^1 | ... | W^T | w_out (ops.wd_attn_layout), W^l drawn N(0, 1 /
    Din_l). The backward runs, per layer T .. 1, dE^{l-1} and the per-chunk partial weight gradients, folded into G;
    layer 1 adds the embedding gradient to dX. The buffers are every layer's output, its gradient and the partials."""
    option, what, name, reads_params = "attn_layers", "interacting layers are", "attn", True

    def check(self, cfg):
        try:
            ops.wd_attn_check(cfg.F, cfg.emb_dim, cfg.attn_cfg)
        except RuntimeError as e:
            raise ValueError(f"attn_layers: {e}") from None

    def shape(self, cfg, k_in0):
        return (ops.wd_attn_layout(cfg.F, cfg.emb_dim, cfg.attn_cfg)[1],)

    def init(self, model, full, g):
        cfg = model.cfg
        Ws, w_out = ops.wd_attn_views(model.view(full, "attn"), cfg.F, cfg.emb_dim, cfg.attn_cfg)
        for W in Ws:
            W.copy_(torch.randn(W.shape, generator=g) / W.shape[0] ** 0.5)
        ops.kaiming_uniform_(w_out, w_out.numel(), g)

    def buffers(self, model, B, train):
        cfg = model.cfg
        return {"attn": ops.wd_attn_buffers(B, cfg.F, cfg.emb_dim, cfg.attn_cfg, model.comm.device, train=train)}

    def forward(self, model, b, P):
        cfg = model.cfg
        ops.wd_attn_forward(b["X"], cfg.F, cfg.emb_dim, model.view(P, "attn"), cfg.attn_cfg, b["wide"], b["attn"])

    def backward(self, model, b, P, G, perm):
        cfg = model.cfg
        ops.wd_attn_backward(b["X"], cfg.F, cfg.emb_dim, model.view(P, "attn"), cfg.attn_cfg, b["dwide"], b["dX"],
                             b["attn"], model.view(G, "attn"), perm=perm)


# the order of the layout entries, of the initial draws, of the forward and of the backward
TERMS = (FMTerm(), CrossTerm(), CINTerm(), AttnTerm())


def enabled(cfg):
    return [t for t in TERMS if getattr(cfg, t.option)]
