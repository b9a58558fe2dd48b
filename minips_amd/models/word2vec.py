"""Word2vec by skip-gram with negative sampling (Mikolov et al., 2013) on the GPU parameter server: the other
textbook parameter-server workload beside the click models -- a large table of short rows keyed by a power-law
vocabulary, every pair pulling N + 2 rows and pushing their gradients.

Parameters
  sparse table  2 V fp32 rows of d floats, row-wise Adagrad: key 2 w is word w's input vector v_w (N(0, init_std)),
                key 2 w + 1 its output vector u_w (zero, word2vec's start). The table is plain: save / restore /
                N -> M resharding go through the name-generic checkpoint code.
Clock: ops.sgns_lookups (the key matrix [P, N + 2]: centre, context and N integer alias-table draws keyed by (seed,
epoch, global pair id), one launch) -> plan (with the lookup CSR) -> sparse Get -> ops.sgns_forward (one launch: e,
loss, h) -> ops.sgns_backward (every unique row's gradient written once, no atomics) -> sparse Add -> Clock. The
loss is the mean over the pairs of sum_t logistic(s_t, y_t) (e carries 1 / (P * world)). Nothing is read back: a
steady one-rank clock issues no host sync. The rule is stated in csrc/kernels/sgns.h.

``set_counts`` builds the sampler's tables on the host once per corpus (rank 0's reach every rank through one
all-reduce of a buffer that is zero elsewhere, an exact integer sum); ``attach`` keeps a rank's sentences resident;
``epoch`` builds the epoch's pairs on the device (integer subsampling and reduced windows keyed by the global token
position, so they do not depend on how the sentences are split over ranks) and runs its clocks.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .. import _native, ops
from ..ps.comm import Comm
from ..ps.tables import SparseTable

_GOLD = 0x9E3779B97F4A7C15
_KEEP_SALT = 0xD1B54A32D192ED03  # separates the token draws from the negatives' (both start at mix(seed + epoch gold))
_M64 = (1 << 64) - 1


def _s64(x: int) -> int:
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def token_base(seed: int, epoch: int) -> int:
    """The uint64 every token draw of ``epoch`` is keyed under: r = mix(token_base ^ global position)."""
    return ops.lda_mix_int(ops.lda_mix_int(seed + epoch * _GOLD) ^ _KEEP_SALT)


@dataclass
class Word2VecConfig:
    vocab: int = 1 << 16
    dim: int = 128
    negatives: int = 5
    window: int = 5
    sample: float = 1e-3
    lr: float = 0.05
    init_std: float = 0.0   # 0.0: 0.5 / dim
    eps: float = 1e-8
    batch_pairs: int = 65536
    seed: int = 0
    consistency: str = "bsp"
    staleness: int = 0
    transport: str = "collective"
    storage: str = "vector"
    value_dtype: torch.dtype = torch.float32
    pull_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        if not 1 <= self.vocab < 1 << 30:
            raise ValueError(f"w2v: vocab is {self.vocab}, expected 1 <= vocab < 2^30 (two rows per word)")
        if self.dim % 4 or not ops.SGNS_MIN_DIM <= self.dim <= ops.SGNS_MAX_DIM:
            raise ValueError(f"w2v: dim is {self.dim}, expected dim % 4 == 0 and {ops.SGNS_MIN_DIM} <= dim <= "
                             f"{ops.SGNS_MAX_DIM}")
        if not 1 <= self.negatives <= ops.SGNS_MAX_NEG:
            raise ValueError(f"w2v: negatives is {self.negatives}, expected 1 <= negatives <= {ops.SGNS_MAX_NEG}")
        if not 1 <= self.window <= 64:
            raise ValueError(f"w2v: window is {self.window}, expected 1 <= window <= 64")
        if not 0 <= self.sample < 1:  # (a NaN fails the comparison)
            raise ValueError(f"w2v: sample is {self.sample}, expected 0 <= sample < 1 (0 keeps every token)")
        if not 1 <= self.batch_pairs or self.batch_pairs * (self.negatives + 2) >= 1 << 31:
            raise ValueError(f"w2v: batch_pairs is {self.batch_pairs}, expected >= 1 and batch_pairs * (negatives + 2) "
                             f"< 2^31")
        if not 0 <= self.seed < 1 << 62:
            raise ValueError(f"w2v: seed is {self.seed}, expected 0 <= seed < 2^62")
        if not self.init_std >= 0:
            raise ValueError(f"w2v: init_std is {self.init_std}, expected >= 0 (0: 0.5 / dim)")
        if self.transport != "collective":
            raise ValueError(f"w2v: transport {self.transport!r} is not supported (the one-sided owners apply the "
                             f"row-wise Adagrad of W&D's rows only); use 'collective'")
        if self.storage.lower() != "vector":
            raise ValueError(f"w2v: storage {self.storage!r} is not supported (the rows of word w are the keys 2 w and "
                             f"2 w + 1 of a range table); use 'vector'")
        if self.value_dtype != torch.float32 or self.pull_dtype != torch.float32:
            raise ValueError(f"w2v: rows are stored and pulled in fp32, not {self.value_dtype} / {self.pull_dtype}")


class Word2Vec:
    def __init__(self, cfg: Word2VecConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        self.V, self.d, self.N = cfg.vocab, cfg.dim, cfg.negatives
        if comm.device.type == "cuda":  # a missing kernel is an error, here and not at the first clock
            try:
                _native.w2vk()
            except RuntimeError as e:
                raise ValueError(f"w2v: the model runs on {comm.device} and needs the _w2vk extension: {e}") from e
        std = cfg.init_std if cfg.init_std > 0 else 0.5 / cfg.dim
        self.table = SparseTable(comm, 2 * self.V, self.d, optimizer="rowwise_adagrad", lr=cfg.lr, eps=cfg.eps,
                                 pull_dtype=torch.float32, push_dtype=torch.float32, value_dtype=torch.float32,
                                 init_std=std, seed=cfg.seed + 1234, consistency=cfg.consistency,
                                 staleness=cfg.staleness, table_id=0)
        # the output vectors start at zero: the rows of the odd keys
        self.table.zero_rows(torch.arange(1, 2 * self.V, 2, dtype=torch.int64, device=comm.device))
        self.thr = self.alias = self.keep = None
        self.T = 0
        self.tokens = self.sid = None
        self.token_base = 0
        self.epochs = 0          # epochs run by epoch()
        self.pairs = 0           # this rank's pairs in the last epoch
        self.total_pairs = 0     # all ranks'

    # -- the sampler's tables ---------------------------------------------------------------
    def set_counts(self, counts: torch.Tensor):
        """Builds the negative sampler's alias table and the subsampling thresholds from the int64 word counts [V]
        of the whole corpus (ops.sgns_alias / ops.sgns_keep: host, Python integers, a fixed order). On several
        ranks rank 0's tables reach every rank through one all-reduce of a buffer that is zero elsewhere."""
        c = counts.detach().to("cpu", torch.int64).reshape(-1)
        if c.numel() != self.V:
            raise ValueError(f"w2v: set_counts takes {self.V} word counts, got {c.numel()}")
        if int(c.sum()) >= ops.SGNS_MAX_TOKENS:
            raise ValueError(f"w2v: the corpus holds {int(c.sum())} tokens, expected fewer than 2^40")
        thr, alias, T, _ = ops.sgns_alias(c)
        buf = torch.cat([thr, alias.long(), ops.sgns_keep(c, self.cfg.sample), torch.tensor([T], dtype=torch.int64)])
        if self.comm.world > 1 and not self.comm.emulated:
            if self.comm.rank != 0:
                buf.zero_()
            buf = buf.to(self.comm.device)
            self.comm.all_reduce_(buf)
            buf = buf.cpu()
        V, dev = self.V, self.comm.device
        self.thr, self.alias = buf[:V].contiguous().to(dev), buf[V:2 * V].to(torch.int32).to(dev)
        self.keep, self.T = buf[2 * V:3 * V].contiguous().to(dev), int(buf[3 * V])
        self.counts = c
        return self

    def _need_counts(self, what: str):
        if self.thr is None:
            raise ValueError(f"w2v: {what} before set_counts(counts): the sampler's tables do not exist")

    # -- one clock --------------------------------------------------------------------------
    def train_step(self, centres, contexts, negatives=None, pair_base: int = 0, epoch: int = 0) -> torch.Tensor:
        """One clock on explicit pairs (centres / contexts int64 [P] words): lookups, Get, forward, backward, Add,
        Clock. The negatives of pair p are the draws of the global pair pair_base + p in ``epoch`` unless the
        explicit int32 [P, N] ``negatives`` are given. Returns the summed loss of this rank's pairs (a device tensor;
        no host sync). P may be 0: the rank plans zero keys, pushes zero rows and clocks."""
        cfg, dev, N = self.cfg, self.comm.device, self.N
        P = centres.numel()
        if negatives is None:
            self._need_counts("train_step without explicit negatives")
        if P:
            thr, alias = (self.thr, self.alias) if self.thr is not None else self._no_tables()
            keys = ops.sgns_lookups(centres, contexts, thr, alias, max(self.T, 1), cfg.seed, epoch, pair_base, N,
                                    negatives).reshape(-1)
        else:
            keys = torch.empty(0, dtype=torch.int64, device=dev)
        plan = self.table.plan(keys, csr=True)
        rows, plan = self.table.get(keys, plan=plan)
        if plan.keys_n:
            e, loss, h = ops.sgns_forward(plan.inv, rows, N, 1.0 / (P * self.comm.world))
            grad_rows = (torch.empty if dev.type == "cuda" else torch.zeros)(max(plan.cap, 1), self.d,
                                                                             dtype=torch.float32, device=dev)
            ops.sgns_backward(plan.inv, e, h, rows, N, grad_rows, csr=plan.csr[:2] if plan.csr is not None else None)
            self.table.add(plan, grad_rows)
            out = loss.sum()
        else:
            if self.comm.world > 1:  # the push is a collective: a rank without pairs pushes zero rows
                self.table.add(plan, torch.zeros(max(plan.cap, 1), self.d, dtype=torch.float32, device=dev))
            out = torch.zeros((), dtype=torch.float32, device=dev)
        self.table.clock()
        return out

    def _no_tables(self):
        """Placeholders for sgns_lookups with explicit negatives before set_counts (they are not read)."""
        dev = self.comm.device
        return torch.zeros(self.V, dtype=torch.int64, device=dev), torch.zeros(self.V, dtype=torch.int32, device=dev)

    # -- data -------------------------------------------------------------------------------
    def attach(self, tokens: torch.Tensor, sent_rowptr: torch.Tensor, token_base: int = 0):
        """Keeps this rank's sentences resident: sentence i holds the words tokens[sent_rowptr[i]:sent_rowptr[i + 1]]
        and its first token has the global position token_base + sent_rowptr[i]. Collective (the word counts are
        all-reduced for the 2^40-token limit; the sampler keeps the counts set_counts was given, which may come
        from a larger corpus than the one attached)."""
        self._need_counts("attach")
        dev = self.comm.device
        rp = sent_rowptr.detach().to("cpu", torch.int64).reshape(-1)
        w = tokens.detach().to("cpu", torch.int64).reshape(-1)
        S, n = rp.numel() - 1, w.numel()
        if S < 0 or int(rp[0]) != 0 or int(rp[-1]) != n or bool((rp[1:] < rp[:-1]).any()):
            raise ValueError(f"w2v: sent_rowptr must ascend from 0 to the {n} tokens it indexes")
        if n and (int(w.min()) < 0 or int(w.max()) >= self.V):
            raise ValueError(f"w2v: words must lie in [0, vocab = {self.V}), found {int(w.min())} .. {int(w.max())}")
        if token_base < 0 or token_base + n >= ops.SGNS_MAX_TOKENS:
            raise ValueError(f"w2v: the token positions {token_base} .. {token_base + n} must lie in [0, 2^40)")
        if n * 2 * self.cfg.window >= 1 << 31:
            raise ValueError(f"w2v: {n} tokens on one rank with window {self.cfg.window}, expected tokens * 2 * window "
                             f"< 2^31 (attach fewer sentences per rank)")
        counts = torch.bincount(w, minlength=self.V).to(dev)
        if self.comm.world > 1:
            self.comm.all_reduce_(counts)
        if int(counts.sum()) >= ops.SGNS_MAX_TOKENS:
            raise ValueError(f"w2v: the corpus holds {int(counts.sum())} tokens, expected fewer than 2^40")
        self.tokens = w.to(dev)
        self.sid = torch.repeat_interleave(torch.arange(S, dtype=torch.int64), rp[1:] - rp[:-1]).to(dev)
        self.token_base = int(token_base)
        return self

    def make_pairs(self, epoch: int):
        """(centres, contexts) int64 [P] of this rank's sentences in ``epoch``, built with torch ops on the device.
        Token i (global position g) draws r = mix(token_base(seed, epoch) ^ g): it is kept iff r >> 32 <=
        keep[word] (word2vec's subsampling, ops.sgns_keep), and as a centre it has the reduced window b = 1 +
        mulhi_u64(mix(r), window). Among the kept tokens of its sentence it pairs with the up to b before and the up
        to b after it. Ordered by centre and then by offset (-b .. -1, 1 .. b). One host read (the pair count)."""
        cfg, dev = self.cfg, self.comm.device
        n, w = self.tokens.numel(), cfg.window
        if n == 0:
            z = torch.empty(0, dtype=torch.int64, device=dev)
            return z, z.clone()
        pos = torch.arange(n, dtype=torch.int64, device=dev)
        r = ops._lda_mix((pos + self.token_base) ^ _s64(token_base(cfg.seed, epoch)))
        kept = ops._lda_lsr(r, 32) <= self.keep[self.tokens]
        rank = torch.cumsum(kept, 0) - 1             # a kept token's index among the kept ones
        m = rank[-1] + 1                             # how many are kept (device)
        slot = torch.where(kept, rank, torch.full_like(rank, n))
        at = torch.zeros(n + 1, dtype=torch.int64, device=dev).scatter_(0, slot, pos)[:n]  # kept index -> token
        b = 1 + ops.mulhi_u64(ops._lda_mix(r[at]), torch.full((n,), w, dtype=torch.int64, device=dev))
        off = torch.cat([torch.arange(-w, 0, device=dev), torch.arange(1, w + 1, device=dev)])
        j = pos[:, None] + off[None, :]              # kept index of the candidate context
        ok = (pos[:, None] < m) & (j >= 0) & (j < m) & (off.abs()[None, :] <= b[:, None])
        jc = j.clamp(0, n - 1)
        ok &= self.sid[at[jc]] == self.sid[at][:, None]
        sel = torch.nonzero(ok.reshape(-1)).reshape(-1)   # the host read
        ci = torch.div(sel, 2 * w, rounding_mode="floor")
        return self.tokens[at[ci]], self.tokens[at[jc.reshape(-1)[sel]]]

    def epoch(self) -> float:
        """One pass over the attached sentences: this epoch's pairs (make_pairs), the global pair id of a rank's
        pair = the pairs of the lower ranks (one all-gather of the counts) + its index, then clocks of batch_pairs
        consecutive pairs; every rank runs the all-reduced maximum number of clocks. Returns the epoch's mean pair
        loss over all ranks (read on the host once, at the end)."""
        self._need_counts("epoch")
        if self.tokens is None:
            raise ValueError("w2v: epoch before attach(tokens, sent_rowptr)")
        cfg, dev, comm = self.cfg, self.comm.device, self.comm
        ep = self.epochs
        cen, ctx = self.make_pairs(ep)
        P = cen.numel()
        base, total, clocks = 0, P, -(-P // cfg.batch_pairs)
        if comm.world > 1 and not comm.emulated:
            cnt = torch.zeros(comm.world, dtype=torch.int64, device=dev)
            comm.all_gather(cnt, torch.tensor([P], dtype=torch.int64, device=dev))
            cnt = cnt.cpu()
            base, total = int(cnt[:comm.rank].sum()), int(cnt.sum())
            clocks = max(-(-int(c) // cfg.batch_pairs) for c in cnt)
        acc = torch.zeros((), dtype=torch.float64, device=dev)
        for c in range(clocks):
            lo, hi = min(c * cfg.batch_pairs, P), min((c + 1) * cfg.batch_pairs, P)
            acc += self.train_step(cen[lo:hi], ctx[lo:hi], pair_base=base + lo, epoch=ep).double()
        if comm.world > 1:
            acc = acc.reshape(1)
            comm.all_reduce_(acc)
        self.epochs, self.pairs, self.total_pairs = ep + 1, P, total
        return float(acc) / max(total, 1)

    # -- reports ----------------------------------------------------------------------------
    def vectors(self) -> torch.Tensor:
        """The input vectors fp32 [V, d] (collective: a Get of every even key)."""
        keys = torch.arange(0, 2 * self.V, 2, dtype=torch.int64, device=self.comm.device)
        return self.table.get_rows(keys)

    def most_similar(self, words, n: int = 10) -> torch.Tensor:
        """int64 [len(words), n]: every word's n nearest other words by the cosine of the input vectors, ties to
        the lower word id (a stable sort: the same answer on every device). Collective."""
        X = self.vectors()
        X = X / X.norm(dim=1, keepdim=True).clamp(min=1e-30)
        q = torch.as_tensor(words, dtype=torch.int64, device=X.device).reshape(-1)
        sim = X[q] @ X.t()
        sim[torch.arange(q.numel(), device=X.device), q] = -math.inf
        return torch.sort(sim, dim=1, descending=True, stable=True).indices[:, : min(n, self.V - 1)]

    def drain(self):
        self.table.drain()


def purity(vectors: torch.Tensor, words_per_group: int) -> float:
    """The share of words whose nearest cosine neighbour (ties to the lower id) lies in their own block of
    ``words_per_group`` consecutive ids (W2VSynth's groups). Chance is (words_per_group - 1) / (V - 1)."""
    X = vectors.detach().float().cpu()
    X = X / X.norm(dim=1, keepdim=True).clamp(min=1e-30)
    sim = X @ X.t()
    sim.fill_diagonal_(-math.inf)
    nn = torch.sort(sim, dim=1, descending=True, stable=True).indices[:, 0]
    me = torch.arange(X.shape[0])
    return float((nn // words_per_group == me // words_per_group).float().mean())
