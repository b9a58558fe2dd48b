"""Synthetic data generators shaped like the BASELINE configs (no datasets are downloadable).

* Criteo-shaped click logs (Wide&Deep / DLRM): 13 dense features ~ N(0,1), 26 categorical
  features with the Criteo-Kaggle cardinalities; ids are drawn log-uniformly (a Zipf(1)-like
  head: P(id <= k) = ln(k+1)/ln(card)) and scattered by a bijective multiplicative hash so the
  hot ids spread over all server shards. Labels are a noisy function of the features, so the
  loss decreases during training.
* MNIST-shaped dense batches (784 -> 10 classes), GPT-2 token batches, webspam-shaped sparse
  LR batches (16.6M feature ids, libsvm-like nnz per row).
All generation happens on the target device with a torch.Generator (deterministic per rank).
"""
from __future__ import annotations

import math

import torch

# Criteo Kaggle (display advertising challenge) per-feature cardinalities.
CRITEO_KAGGLE_CARDS = [
    1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992,
    5461306, 10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572,
]
_HASH_PRIME = 2654435761  # prime: multiplication mod card is a bijection unless card % prime == 0


class CriteoSynth:
    def __init__(self, batch: int, cards=None, n_dense: int = 13, device="cpu", seed: int = 0,
                 hot_alpha: float = 1.0):
        self.batch = batch
        self.cards = list(cards or CRITEO_KAGGLE_CARDS)
        self.F = len(self.cards)
        self.n_dense = n_dense
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.offsets = torch.tensor([0] + list(_cumsum(self.cards))[:-1], dtype=torch.int64, device=self.device)
        self.card_t = torch.tensor(self.cards, dtype=torch.int64, device=self.device)
        self.log_card = torch.log(self.card_t.to(torch.float64) + 1.0)
        self.num_rows = int(sum(self.cards))
        self.hot_alpha = hot_alpha
        self.w_dense = torch.randn(n_dense, generator=self.gen, device=self.device) / math.sqrt(n_dense)

    def holdout(self, seed: int) -> "CriteoSynth":
        """A held-out stream of the SAME labelling function: the teacher (``w_dense``, the cards) is
        this generator's, the samples are an independent stream drawn from ``seed`` (a generator
        merely constructed with another seed would draw another teacher)."""
        g = CriteoSynth(self.batch, cards=self.cards, n_dense=self.n_dense, device=self.device, seed=seed,
                        hot_alpha=self.hot_alpha)
        g.w_dense = self.w_dense.clone()
        return g

    def next(self):
        B, F = self.batch, self.F
        if self.device.type == "cuda":
            # one fused gfx950 launch (csrc/kernels/data.hip) instead of ~15 torch kernels
            from .._native import kernels

            self._init_gpu()
            self._host_step += 1
            dense = torch.empty(B, self.n_dense, device=self.device)
            keys = torch.empty(B, F, dtype=torch.int64, device=self.device)
            labels = torch.empty(B, device=self.device)
            if torch.cuda.is_current_stream_capturing():
                # a captured step draws a fresh batch on every replay: the counter advances on the
                # device (graph_prepare set it from the host count before the capture)
                self._step_dev.add_(1)
                kernels().criteo_synth(self._seed, 0, self._step_dev, self.card_t, self.offsets, self.w_dense,
                                       dense, keys, labels)
            else:
                kernels().criteo_synth(self._seed, self._host_step, None, self.card_t, self.offsets, self.w_dense,
                                       dense, keys, labels)
            return dense, keys, labels
        u = torch.rand(B, F, generator=self.gen, device=self.device, dtype=torch.float64)
        raw = torch.floor(torch.exp(u * self.log_card) - 1.0).to(torch.int64)
        raw = torch.minimum(raw, self.card_t - 1).clamp_min(0)
        ids = (raw * _HASH_PRIME) % self.card_t
        keys = ids + self.offsets
        dense = torch.randn(B, self.n_dense, generator=self.gen, device=self.device)
        logit = dense @ self.w_dense + 0.5 * ((raw[:, :4] % 2).sum(1).float() - 1.0)
        noise = torch.rand(B, generator=self.gen, device=self.device)
        labels = (torch.sigmoid(2.0 * logit) > noise).float()
        return dense, keys, labels

    def _init_gpu(self):
        if not hasattr(self, "_seed"):
            self._seed = int(torch.randint(0, 2**62, (1,), generator=self.gen, device=self.device).item())
            self._host_step = 0
            # device twin of the step counter, used inside HIP-graph captures only
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.device)

    def graph_prepare(self):
        """Before capturing a step that draws batches: the device counter = the host count."""
        if self.device.type == "cuda":
            self._init_gpu()
            self._step_dev.fill_(self._host_step)

    def graph_replayed(self, n: int = 1):
        """A captured step was replayed ``n`` times: the host count follows the device's."""
        self._host_step += n

    def skip(self, n: int):
        """Advance past ``n`` batches (resume from a checkpoint at the same data position)."""
        if self.device.type == "cuda":
            self._init_gpu()
            self._host_step += n
        else:
            for _ in range(n):
                self.next()


def _cumsum(xs):
    s = 0
    for x in xs:
        s += x
        yield s


class DLRMSynth:
    """DLRM batches (BASELINE config 5): F keys per sample uniform over the whole table, n_dense
    N(0,1) features, label = dense[:, 0] > 0. On the GPU one fused launch (csrc/kernels/data.hip
    uniform_synth, counter-based RNG) per batch; on the CPU the torch generator."""

    def __init__(self, batch: int, F: int, num_rows: int, n_dense: int = 13, device="cpu", seed: int = 0):
        self.batch, self.F, self.num_rows, self.n_dense = batch, F, int(num_rows), n_dense
        self.device = torch.device(device)
        self.seed = int(seed)
        self._step = 0
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def holdout(self, seed: int) -> "DLRMSynth":
        """A held-out stream: the labels are a fixed function of the features (no teacher state), so a
        fresh seed is an independent sample of the same task."""
        return DLRMSynth(self.batch, self.F, self.num_rows, self.n_dense, device=self.device, seed=seed)

    def next(self):
        B = self.batch
        if self.device.type == "cuda":
            from .._native import kernels

            dense = torch.empty(B, self.n_dense, device=self.device)
            keys = torch.empty(B, self.F, dtype=torch.int64, device=self.device)
            labels = torch.empty(B, device=self.device)
            kernels().uniform_synth(self.seed, self._step, self.num_rows, dense, keys, labels)
            self._step += 1
            return dense, keys, labels
        dense = torch.randn(B, self.n_dense, generator=self.gen, device=self.device)
        keys = torch.randint(0, self.num_rows, (B, self.F), generator=self.gen, device=self.device)
        return dense, keys, (dense[:, 0] > 0).float()


class MnistSynth:
    """784-dim inputs in [0,1) and 10-class labels from a fixed random linear teacher."""

    def __init__(self, batch: int, device="cpu", seed: int = 0, dim: int = 784, classes: int = 10):
        self.batch, self.dim, self.classes = batch, dim, classes
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.teacher = torch.randn(dim, classes, generator=self.gen, device=self.device)

    def next(self):
        x = torch.rand(self.batch, self.dim, generator=self.gen, device=self.device)
        y = torch.argmax(x @ self.teacher, dim=1)
        return x, y


class TokenSynth:
    """GPT-2 token batches: [B, T+1] uniform ids (inputs = [:, :-1], targets = [:, 1:])."""

    def __init__(self, batch: int, seq: int, vocab: int = 50257, device="cpu", seed: int = 0):
        self.batch, self.seq, self.vocab = batch, seq, vocab
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def next(self):
        t = torch.randint(0, self.vocab, (self.batch, self.seq + 1), generator=self.gen, device=self.device)
        return t[:, :-1].contiguous(), t[:, 1:].contiguous()


class SparseLRSynth:
    """webspam-shaped sparse LR: `num_dims` features, ~nnz ids per row, linear teacher labels."""

    def __init__(self, batch: int, num_dims: int = 16_609_143, nnz: int = 64, device="cpu", seed: int = 0):
        self.batch, self.num_dims, self.nnz = batch, num_dims, nnz
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def next(self):
        B, k = self.batch, self.nnz
        cols = torch.randint(0, self.num_dims, (B, k), generator=self.gen, device=self.device)
        vals = torch.rand(B, k, generator=self.gen, device=self.device)
        teacher = ((cols * _HASH_PRIME) % 7).float() - 3.0
        y = ((teacher * vals).sum(1) > 0).float()
        rowptr = torch.arange(0, (B + 1) * k, k, device=self.device, dtype=torch.int64)
        return rowptr, cols.reshape(-1), vals.reshape(-1), y


class FMSynth:
    """Field-structured CSR batches with a factorization-machine teacher: ``fields`` fields of ``card`` ids
    each, one active feature per field with value 1 (feature id = field * card + id), a fixed random teacher
    FM of rank ``k_teacher`` (factors ~ N(0, 1), linear weights ~ N(0, 0.3^2)), labels ~ Bernoulli(sigmoid(z*)).
    next() returns (rowptr, cols, vals, labels) like SparseLRSynth."""

    def __init__(self, batch: int, fields: int = 8, card: int = 32, k_teacher: int = 4, device="cpu", seed: int = 0):
        self.batch, self.fields, self.card, self.k_teacher = batch, fields, card, k_teacher
        self.num_dims = fields * card
        self.device = torch.device(device)
        g = torch.Generator(device="cpu")  # the teacher is the same on every device
        g.manual_seed(seed)
        self.v = torch.randn(self.num_dims, k_teacher, generator=g).to(self.device)
        self.w = (0.3 * torch.randn(self.num_dims, generator=g)).to(self.device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + 1)
        self.field_base = torch.arange(fields, dtype=torch.int64, device=self.device) * card

    def holdout(self, seed: int) -> "FMSynth":
        """A held-out stream of the SAME teacher: an independent sample stream drawn from ``seed``."""
        g = FMSynth.__new__(FMSynth)
        g.__dict__.update(self.__dict__)
        g.gen = torch.Generator(device=self.device)
        g.gen.manual_seed(seed)
        return g

    def teacher_logits(self, cols2d: torch.Tensor) -> torch.Tensor:
        v = self.v[cols2d]  # [B, F, k]
        s = v.sum(1)
        return self.w[cols2d].sum(1) + 0.5 * ((s * s).sum(1) - (v * v).sum((1, 2)))

    def next(self):
        B, F = self.batch, self.fields
        ids = torch.randint(0, self.card, (B, F), generator=self.gen, device=self.device)
        cols = ids + self.field_base
        p = torch.sigmoid(self.teacher_logits(cols))
        y = (torch.rand(B, generator=self.gen, device=self.device) < p).float()
        rowptr = torch.arange(0, (B + 1) * F, F, device=self.device, dtype=torch.int64)
        vals = torch.ones(B * F, dtype=torch.float32, device=self.device)
        return rowptr, cols.reshape(-1), vals, y


class FFMSynth(FMSynth):
    """FMSynth's batches with a field-aware teacher (the rule of csrc/kernels/ffm.h): feature u keeps one vector
    per partner field, V [num_dims, fields, k_teacher] ~ N(0, 1), w ~ N(0, 0.3^2), and
    z* = sum_f w_{c_f} + sum_{f<g} <V[c_f, g], V[c_g, f]> over the one active feature c_f = f * card + id of every
    field. next() returns (rowptr, cols, vals, labels); a key's field is key // card."""

    def __init__(self, batch: int, fields: int = 8, card: int = 32, k_teacher: int = 4, device="cpu", seed: int = 0):
        super().__init__(batch, fields, card, k_teacher, device, seed)
        g = torch.Generator(device="cpu")  # the teacher is the same on every device
        g.manual_seed(seed)
        self.v = torch.randn(self.num_dims, fields, k_teacher, generator=g).to(self.device)
        self.w = (0.3 * torch.randn(self.num_dims, generator=g)).to(self.device)
        self.upper = torch.triu(torch.ones(fields, fields, device=self.device), diagonal=1)

    def holdout(self, seed: int) -> "FFMSynth":
        g = FFMSynth.__new__(FFMSynth)
        g.__dict__.update(self.__dict__)
        g.gen = torch.Generator(device=self.device)
        g.gen.manual_seed(seed)
        return g

    def teacher_logits(self, cols2d: torch.Tensor) -> torch.Tensor:
        a = self.v[cols2d]  # [B, F, F, k]: a[b, f, g] = V[c_f, g]
        pair = (a * a.transpose(1, 2)).sum(-1)
        return self.w[cols2d].sum(1) + (pair * self.upper).sum((1, 2))


class GBDTSynth:
    """Dense batches for the gradient-boosted trees (models/gbdt.py): X [batch, features] ~ U(-1, 1) with
    features >= 5, and a teacher no linear model can follow,
    z* = 3 sign(x0) sign(x1) + 2 [x2 > 0.3] x3 - 1.5 [|x4| < 0.4], labels ~ Bernoulli(sigmoid(z*)); the other
    features are noise. next() returns (X fp32, labels fp32)."""

    def __init__(self, batch: int, features: int = 8, device="cpu", seed: int = 0):
        if features < 5:
            raise ValueError(f"GBDTSynth: the teacher reads 5 features, got features = {features}")
        self.batch, self.features = batch, features
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + 1)

    def holdout(self, seed: int) -> "GBDTSynth":
        """A held-out stream of the SAME teacher: an independent sample stream drawn from ``seed``."""
        g = GBDTSynth.__new__(GBDTSynth)
        g.__dict__.update(self.__dict__)
        g.gen = torch.Generator(device=self.device)
        g.gen.manual_seed(seed)
        return g

    @staticmethod
    def teacher_logits(X: torch.Tensor) -> torch.Tensor:
        return 3.0 * torch.sign(X[:, 0]) * torch.sign(X[:, 1]) + 2.0 * (X[:, 2] > 0.3).float() * X[:, 3] \
            - 1.5 * (X[:, 4].abs() < 0.4).float()

    def next(self):
        X = torch.rand(self.batch, self.features, generator=self.gen, device=self.device) * 2.0 - 1.0
        p = torch.sigmoid(self.teacher_logits(X))
        y = (torch.rand(self.batch, generator=self.gen, device=self.device) < p).float()
        return X, y


class LDASynth:
    """A corpus with planted topics for Latent Dirichlet Allocation (models/lda.py): topic k owns the word block
    [k * (vocab // topics), (k + 1) * (vocab // topics)) with word weights from Dirichlet(1) (disjoint blocks),
    every document mixes the topics with weights from Dirichlet(0.2) and draws ``doc_len`` tokens. corpus()
    returns (rowptr int64 [docs + 1], words int64 [docs * doc_len], planted): ``planted`` is the planted model's
    own per-token log likelihood of the corpus, mean log(sum_k theta[d, k] phi[k, w]) in nats. Generated on the
    host from ``seed`` alone; ``phi`` [topics, vocab] and ``theta`` [docs, topics] stay on the object."""

    def __init__(self, topics: int = 4, vocab: int = 64, docs: int = 256, doc_len: int = 48, seed: int = 0,
                 mix: float = 0.2):
        if topics < 1 or vocab < topics or docs < 1 or doc_len < 1:
            raise ValueError(f"LDASynth: topics {topics}, vocab {vocab}, docs {docs}, doc_len {doc_len}: every topic "
                             f"needs a word block of its own")
        self.topics, self.vocab, self.docs, self.doc_len, self.block = topics, vocab, docs, doc_len, vocab // topics
        gen = torch.Generator()
        gen.manual_seed(seed + 1)
        # Dirichlet(c) = normalised Gamma(c, 1); Gamma(1) is -log U, Gamma(c) by torch's sampler
        e = -torch.log1p(-torch.rand(topics, self.block, generator=gen, dtype=torch.float64))
        self.phi = torch.zeros(topics, vocab, dtype=torch.float64)
        for k in range(topics):
            self.phi[k, k * self.block:(k + 1) * self.block] = e[k] / e[k].sum()
        g = torch._standard_gamma(torch.full((docs, topics), float(mix), dtype=torch.float64), generator=gen)
        g = g.clamp(min=1e-300)
        self.theta = g / g.sum(1, keepdim=True)
        self.zs = torch.multinomial(self.theta, doc_len, replacement=True, generator=gen)          # [docs, doc_len]
        self.words = torch.multinomial(self.phi[self.zs.reshape(-1)], 1, generator=gen).reshape(-1)
        self.rowptr = torch.arange(docs + 1, dtype=torch.int64) * doc_len

    def planted_loglik(self) -> float:
        doc = torch.arange(self.docs).repeat_interleave(self.doc_len)
        p = (self.theta[doc] * self.phi[:, self.words].t()).sum(1)
        return float(torch.log(p).mean())

    def corpus(self):
        return self.rowptr, self.words, self.planted_loglik()

    def block_of(self, words: torch.Tensor) -> torch.Tensor:
        """The planted topic whose block holds each word (words past the last block: the last topic)."""
        return (words // self.block).clamp(max=self.topics - 1)


class W2VSynth:
    """A corpus with planted word groups for word2vec (models/word2vec.py): group k owns the word block
    [k * words_per_group, (k + 1) * words_per_group). Each of the ``sentences`` sentences of ``length`` tokens picks
    a group uniformly; each token comes uniformly from that group's block with probability 1 - ``noise``, else
    uniformly from the whole vocabulary. corpus() returns (tokens int64 [sentences * length], sent_rowptr int64
    [sentences + 1]). Generated on the host from ``seed`` alone."""

    def __init__(self, groups: int = 8, words_per_group: int = 16, sentences: int = 512, length: int = 16,
                 noise: float = 0.1, seed: int = 0):
        if groups < 1 or words_per_group < 1 or sentences < 1 or length < 1 or not 0 <= noise <= 1:
            raise ValueError(f"W2VSynth: groups {groups}, words_per_group {words_per_group}, sentences {sentences}, "
                             f"length {length}, noise {noise}")
        self.groups, self.words_per_group, self.sentences, self.length = groups, words_per_group, sentences, length
        self.vocab = groups * words_per_group
        gen = torch.Generator()
        gen.manual_seed(seed + 1)
        self.group = torch.randint(groups, (sentences,), generator=gen)
        own = self.group[:, None] * words_per_group + torch.randint(words_per_group, (sentences, length), generator=gen)
        anyw = torch.randint(self.vocab, (sentences, length), generator=gen)
        noisy = torch.rand(sentences, length, generator=gen, dtype=torch.float64) < noise
        self.tokens = torch.where(noisy, anyw, own).reshape(-1)
        self.rowptr = torch.arange(sentences + 1, dtype=torch.int64) * length

    def corpus(self):
        return self.tokens, self.rowptr

    def counts(self) -> torch.Tensor:
        return torch.bincount(self.tokens, minlength=self.vocab)
