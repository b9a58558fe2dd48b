"""Latent Dirichlet Allocation on the parameter-server data plane, by delayed-update collapsed Gibbs sampling
(AD-LDA) in exact fixed point: topics, count rows and totals are the same bits on the CPU and the GPU and on 1, 2
or 4 ranks.

State     the word-topic counts nwk live in a SparseTable(optimizer="add") of fp32 rows [vocab, align4(K)] (exact:
          every count is an integer below 2^24; the pad columns stay 0), sharded over the ranks. The topic totals
          nk int64 [K] are replicated. A rank's documents stay resident after ``attach``: rowptr, words, the topic
          z of every token (int16) and the documents' global ids doc_base + i.
Clock     clock c covers the global documents [c * batch_docs, (c + 1) * batch_docs); every rank takes the part
          of that range it holds (possibly none: it still plans zero keys and clocks, and may push zero rows):
          plan (with the lookup CSR) -> Get -> ops.lda_sample against the pulled snapshot and nk -> ops.lda_delta
          (every unique row's integer delta written once, no atomics) -> Add -> Clock -> ONE int64 all-reduce of
          dk, added to nk. Everything summed is an integer and the random draw of a token depends on (seed, sweep,
          global document id, position) only, so the result does not depend on how the documents are split over
          ranks. Nothing is read back: a steady one-rank clock issues no host sync.
The rule is stated in csrc/kernels/lda.h. ``init()`` runs the clocks of sweep 0 (uniform topics), ``sweep()`` one
pass of clocks, ``loglik()`` the per-token log likelihood of all ranks' documents under the current counts.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import torch
import torch.distributed as dist

from .. import ops
from ..ps.comm import Comm
from ..ps.tables import SparseTable

MAX_WORD_COUNT = 1 << 24   # fp32 rows hold every count exactly below this
MAX_DOC_ID = 1 << 51       # g * 4096 + j stays below 2^63


@dataclass
class LDAConfig:
    num_topics: int = 64
    vocab: int = 8192
    alpha: float = 0.1
    beta: float = 0.01
    batch_docs: int = 4096
    seed: int = 0
    transport: str = "collective"

    def __post_init__(self):
        K = self.num_topics
        if not ops.LDA_MIN_K <= K <= ops.LDA_MAX_K:
            raise ValueError(f"lda: num_topics is {K}, expected {ops.LDA_MIN_K} <= num_topics <= {ops.LDA_MAX_K}")
        if not 1 <= self.vocab < 1 << 31:
            raise ValueError(f"lda: vocab is {self.vocab}, expected 1 <= vocab < 2^31")
        if not 0 < self.alpha <= ops.LDA_MAX_PRIOR:
            raise ValueError(f"lda: alpha is {self.alpha}, expected 0 < alpha <= 64")
        if not 0 < self.beta <= ops.LDA_MAX_PRIOR:
            raise ValueError(f"lda: beta is {self.beta}, expected 0 < beta <= 64")
        if self.batch_docs < 1:
            raise ValueError(f"lda: batch_docs is {self.batch_docs}, expected >= 1")
        if not 0 <= self.seed < 1 << 63:
            raise ValueError(f"lda: seed is {self.seed}, expected 0 <= seed < 2^63")
        if self.transport != "collective":
            raise ValueError(f"lda: transport {self.transport!r} is not supported (the count deltas are plain adds "
                             f"and the totals an all-reduce; there is no lda on the one-sided transport); use "
                             f"'collective'")


class LDA:
    def __init__(self, cfg: LDAConfig, comm: Comm):
        self.cfg, self.comm = cfg, comm
        self.K, self.V = cfg.num_topics, cfg.vocab
        self.W = (self.K + 3) & ~3
        self.Vbeta = self.V * cfg.beta  # formed once, as a Python double
        self.table = SparseTable(comm, self.V, self.W, optimizer="add", init_std=0.0, pull_dtype=torch.float32,
                                 push_dtype=torch.float32, value_dtype=torch.float32, table_id=0)
        self.nk = torch.zeros(self.K, dtype=torch.int64, device=comm.device)
        self.it = 0          # sweeps done (0: only the initialisation, once ``initialised``)
        self.initialised = False
        self.rowptr = self.words = self.z = self.gid = None
        self.tokens = 0      # of this rank
        self._batches: list = []

    # -- data -------------------------------------------------------------------------------
    def attach(self, rowptr: torch.Tensor, words: torch.Tensor, doc_base: int = 0):
        """Keeps this rank's documents resident: document i holds the words[rowptr[i]:rowptr[i + 1]] and has the
        global id doc_base + i. Collective (the word counts and the number of documents are all-reduced)."""
        cfg, dev = self.cfg, self.comm.device
        rp = rowptr.detach().to("cpu", torch.int64).reshape(-1)
        w = words.detach().to("cpu", torch.int64).reshape(-1)
        D, n = rp.numel() - 1, w.numel()
        if D < 0 or (D >= 0 and (int(rp[0]) != 0 or int(rp[-1]) != n or bool((rp[1:] < rp[:-1]).any()))):
            raise ValueError(f"lda: rowptr must ascend from 0 to the {n} words it indexes")
        if D and int((rp[1:] - rp[:-1]).max()) > ops.LDA_MAX_DOC_LEN:
            raise ValueError(f"lda: a document holds {int((rp[1:] - rp[:-1]).max())} tokens, at most "
                             f"{ops.LDA_MAX_DOC_LEN} are allowed (split it)")
        if n and (int(w.min()) < 0 or int(w.max()) >= self.V):
            raise ValueError(f"lda: words must lie in [0, vocab = {self.V}), found {int(w.min())} .. {int(w.max())}")
        if not 0 <= doc_base or doc_base + D > MAX_DOC_ID:
            raise ValueError(f"lda: document ids {doc_base} .. {doc_base + D} must lie in [0, 2^51)")
        if n >= 1 << 31:
            raise ValueError(f"lda: {n} tokens on one rank, expected fewer than 2^31")
        counts = torch.bincount(w, minlength=self.V).to(dev)
        total = torch.tensor([doc_base + D], dtype=torch.int64, device=dev)
        if self.comm.world > 1:
            self.comm.all_reduce_(counts)
            self.comm.all_reduce_(total, op=dist.ReduceOp.MAX)
        top = int(counts.max()) if self.V else 0
        if top >= MAX_WORD_COUNT:
            raise ValueError(f"lda: a word occurs {top} times over all ranks, expected fewer than 2^24 (the fp32 "
                             f"count rows are exact below that)")
        self.rowptr, self.words = rp.to(dev), w.to(dev)
        self.z = torch.full((n,), -1, dtype=torch.int16, device=dev)
        self.gid = torch.arange(doc_base, doc_base + D, dtype=torch.int64, device=dev)
        self.doc_base, self.docs, self.tokens, self.total_docs = doc_base, D, n, int(total)
        # the clocks' slices, cut on the host once: (first doc, last doc, first token, last token, batch rowptr)
        bd = cfg.batch_docs
        self._batches = []
        for c in range(-(-self.total_docs // bd)):
            a = min(max(c * bd - doc_base, 0), D)
            b = min(max((c + 1) * bd - doc_base, 0), D)
            t0, t1 = int(rp[a]), int(rp[b])
            self._batches.append((a, b, t0, t1, (rp[a:b + 1] - t0).to(dev)))
        self.initialised = False
        self.it = 0
        return self

    # -- clocks -----------------------------------------------------------------------------
    def _clock(self, c: int, it: int, rebuild: bool = False):
        cfg, dev = self.cfg, self.comm.device
        a, b, t0, t1, rp = self._batches[c]
        keys = self.words[t0:t1]
        plan = self.table.plan(keys, csr=True)
        dk = torch.zeros(self.K, dtype=torch.int64, device=dev)
        if rebuild:  # the counts of the resident topics, from zero (load_state)
            z_old, z_new = None, self.z[t0:t1]
        else:
            rows, plan = self.table.get(keys, plan=plan)
            z_old = self.z[t0:t1] if it > 0 else None
        if plan.keys_n:
            if not rebuild:
                z_new, _ = ops.lda_sample(rp, self.gid[a:b], plan.inv, z_old, rows, self.nk, cfg.alpha, cfg.beta,
                                          self.Vbeta, cfg.seed, it, dk=dk)
            delta = (torch.empty if dev.type == "cuda" else torch.zeros)(max(plan.cap, 1), self.W,
                                                                         dtype=torch.float32, device=dev)
            ops.lda_delta(plan.inv, z_old, z_new, self.K, delta, csr=plan.csr[:2] if plan.csr is not None else None)
            self.table.add(plan, delta)
            if not rebuild:
                self.z[t0:t1].copy_(z_new)
        elif self.comm.world > 1:  # the push is a collective: a rank without tokens pushes zero rows
            self.table.add(plan, torch.zeros(max(plan.cap, 1), self.W, dtype=torch.float32, device=dev))
        self.table.clock()
        if not rebuild:
            self.comm.all_reduce_(dk)
            self.nk += dk

    def _need_docs(self, what: str):
        if self.z is None:
            raise ValueError(f"lda: {what} before attach(rowptr, words, doc_base)")

    def init(self):
        """The clocks of sweep 0: every token draws a uniform topic (the table and nk must be empty)."""
        self._need_docs("init")
        if self.initialised:
            raise ValueError("lda: init() twice: the counts already hold these documents")
        for c in range(len(self._batches)):
            self._clock(c, 0)
        self.initialised, self.it = True, 0
        return self

    def sweep(self):
        """One pass of clocks over all documents."""
        self._need_docs("sweep")
        if not self.initialised:
            raise ValueError("lda: sweep before init() (or load_state)")
        self.it += 1
        for c in range(len(self._batches)):
            self._clock(c, self.it)
        return self

    # -- reports ----------------------------------------------------------------------------
    def loglik(self) -> float:
        """The per-token log likelihood (nats) of all ranks' documents under the current counts. Collective;
        reads the result on the host."""
        self._need_docs("loglik")
        cfg, dev = self.cfg, self.comm.device
        acc = torch.zeros(2, dtype=torch.int64, device=dev)
        for a, b, t0, t1, rp in self._batches:
            keys = self.words[t0:t1]
            rows, plan = self.table.get(keys)
            if plan.keys_n:
                ops.lda_loglik(rp, plan.inv, self.z[t0:t1], rows, self.nk, cfg.alpha, cfg.beta, self.Vbeta, acc)
        self.comm.all_reduce_(acc)
        s, n = (int(v) for v in acc.cpu())
        return -(s / ops.LDA_LOGLIK_SCALE) / max(n, 1)

    def counts(self) -> torch.Tensor:
        """nwk fp32 [vocab, K] of the whole table (collective: a Get of every word)."""
        keys = torch.arange(self.V, dtype=torch.int64, device=self.comm.device)
        return self.table.get_rows(keys)[:, : self.K]

    def top_words(self, n: int = 10) -> torch.Tensor:
        """int64 [K, n]: every topic's n most frequent words, ties to the lower word id (a stable sort: the same
        answer on every device). Collective."""
        return torch.sort(self.counts().t(), dim=1, descending=True, stable=True).indices[:, : min(n, self.V)]

    def drain(self):
        self.table.drain()

    # -- state ------------------------------------------------------------------------------
    def state(self) -> dict:
        """This rank's topics with the replicated totals and the sweep counter (the table is rebuilt from z)."""
        self._need_docs("state")
        return dict(config=dataclasses.asdict(self.cfg), z=self.z.cpu().clone(), nk=self.nk.cpu().clone(), it=self.it,
                    doc_base=self.doc_base)

    def load_state(self, sd: dict):
        """Restores ``state()`` onto the attached documents: z, nk, the sweep counter, and the table's counts,
        rebuilt from z by one pass of add-only clocks. Collective."""
        self._need_docs("load_state")
        c, mine = sd["config"], dataclasses.asdict(self.cfg)
        for k in ("num_topics", "vocab", "alpha", "beta", "batch_docs", "seed"):
            if c[k] != mine[k]:
                raise ValueError(f"lda: the state was saved with {k} = {c[k]}, this model has {mine[k]}")
        if sd["z"].numel() != self.tokens or sd["doc_base"] != self.doc_base:
            raise ValueError(f"lda: the state holds {sd['z'].numel()} tokens from document {sd['doc_base']}, this "
                             f"rank {self.tokens} from {self.doc_base}")
        self.table.drain()
        self.table.shard.zero_()
        self.z.copy_(sd["z"])
        self.nk.copy_(sd["nk"])
        for ci in range(len(self._batches)):
            self._clock(ci, 0, rebuild=True)
        self.it, self.initialised = int(sd["it"]), True
        return self
