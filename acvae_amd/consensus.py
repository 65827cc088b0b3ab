"""Consensus (minimum-Bayes-risk) reranking of a clip's sampled captions, on the device.

A sampling captioner draws N captions per clip; the one to ship is the candidate that agrees most with the clip's other
candidates under CIDEr-D.  ``Consensus(vocabulary, corpus)`` holds what that needs besides the sampled words - a corpus's
(n-gram key, idf) table and the table of length penalties, built once and uploaded once per device - and
``acvae_consensus_scores`` (csrc/consensus.hip) scores the token rows where the rollout left them: the "references" of a
candidate are the other rows of the same launch.  There is no host scorer here (tests/consensus_util.py holds the
definition as a dictionary scorer).

A clip has candidates h_0 .. h_{N-1}, 2 <= N <= 16, token rows i64 [N, T], T <= 64, cleaned as the CIDEr-D reward cleans
them (``<start>`` skipped wherever it stands, cut at the first ``<end>``).  float64:
  c_i(g) the count of n-gram g (orders k = 1..4) in h_i;  v_i(g) = c_i(g) idf(g)
  norm_k(i) = sqrt(sum_g v_i(g)^2) over the order-k n-grams of h_i;  len(i) the number of BIGRAMS of h_i
  sim_k(i, j) = sum_{g in h_i} min(v_i(g), v_j(g)) v_j(g), divided by norm_k(i) norm_k(j) if both are non-zero, times
                exp(-(len i - len j)^2 / (2 sigma^2))
  consensus(i) = 10 mean_k (1 / (N - 1)) sum_{j != i} sim_k(i, j);  an empty candidate scores 0
  best = the lowest index among the maxima of the device's scores.
The idf belongs to a corpus, not to the batch: ``corpus`` maps a key (a clip) to its caption strings, df(g) is the number
of keys with g in at least one caption, D = len(corpus), idf(g) = ln D - ln max(1, df(g)), and an n-gram the corpus does
not hold has idf = ln D.  A clip's result therefore does not depend on what else is in the batch (the batch-derived df
of ``CiderD.prepare`` would make it).  ``corpus=None``: the empty table with idf = 1 for every n-gram, i.e. a clipped
term-frequency cosine.  Corpus words outside the vocabulary count in D and in df and get no device entry: no candidate
holds them.
"""
import numpy as np
import torch

from . import _lib

MAX_VOCAB = 65534
MAX_LENGTH = int(_lib._defs["ACVAE_CONSENSUS_MAX_LENGTH"])
MAX_SAMPLES = int(_lib._defs["ACVAE_CONSENSUS_MAX_SAMPLES"])
_ORDERS = 4


def check_sample_n(sample_n, who="Consensus"):
    if isinstance(sample_n, bool) or not isinstance(sample_n, (int, np.integer)) or not (2 <= sample_n <= MAX_SAMPLES):
        raise ValueError(f"{who}: reranking needs 2 <= N <= {MAX_SAMPLES} candidates per clip, got {sample_n!r}")
    return int(sample_n)


class Consensus:
    """``rerank=Consensus(vocabulary, corpus)`` for ``rollout_shared_encoder`` / ``forward_batch_shared_encoder`` /
    ``evaluate``; or ``select(seqs, sample_n)`` on any clip-major token rows."""

    def __init__(self, vocabulary, corpus=None, sigma=6.0):
        i2w = vocabulary.idx2word
        items = list(i2w.items()) if hasattr(i2w, "items") else list(enumerate(i2w))
        self.sigma = float(sigma)
        self.word2id = {}
        for idx, w in items:
            idx = int(idx)
            if not isinstance(w, str) or w == "" or w.split() != [w]:
                raise ValueError(f"Consensus: vocabulary word {w!r} (id {idx}) is empty or contains whitespace: a sentence "
                                 "built from it would not split back into the same words")
            if w in self.word2id:
                raise ValueError(f"Consensus: ids {self.word2id[w]} and {idx} share the word {w!r}")
            if idx < 0:
                raise ValueError(f"Consensus: negative token id {idx}")
            self.word2id[w] = idx
        self.V = max(self.word2id.values()) + 1 if self.word2id else 0
        if self.V > MAX_VOCAB:
            raise ValueError(f"Consensus: token ids up to {self.V - 1}; an n-gram key holds 16 bits per id (V <= {MAX_VOCAB})")
        if corpus is None:
            self.n_docs, self.log_d = 0, 1.0
            self.idf_keys, self.idf_vals = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float64)
        else:
            self.n_docs = len(corpus)
            if self.n_docs == 0:
                raise ValueError("Consensus: the corpus has no keys (corpus=None gives the table-free score)")
            self.log_d = float(np.log(float(self.n_docs)))
            self.idf_keys, self.idf_vals = self._idf_table(corpus)
        delta = np.arange(MAX_LENGTH, dtype=np.float64)          # a row of <= 64 words has <= 63 bigrams
        self.len_factor = np.exp(-(delta * delta) / (2.0 * self.sigma ** 2))
        self._dev = {}

    def _idf_table(self, corpus):
        """-> (ascending uint64 keys, float64 idf) of the corpus's in-vocabulary n-grams."""
        word2id = self.word2id
        df = {}
        for captions in corpus.values():
            seen = set()
            for cap in captions:
                ids = [word2id.get(w, -1) for w in cap.split()]
                for k in range(1, _ORDERS + 1):
                    for p in range(len(ids) - k + 1):
                        g = ids[p:p + k]
                        if min(g) >= 0:                          # an n-gram with a word outside the vocabulary: no entry
                            key = 0
                            for j, w in enumerate(g):
                                key |= (w + 1) << (16 * j)
                            seen.add(key)
            for key in seen:
                df[key] = df.get(key, 0) + 1
        keys = np.array(sorted(df), dtype=np.uint64)
        count = np.array([df[int(k)] for k in keys], dtype=np.float64)
        return keys, self.log_d - np.log(np.maximum(1.0, count))

    def _tables(self, device):
        """The device copies of the tables: uploaded on first use of a device, kept for good."""
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = (_lib.h2d(torch.from_numpy(self.idf_keys.view(np.int64)), device),
                                  _lib.h2d(torch.from_numpy(self.idf_vals), device),
                                  _lib.h2d(torch.from_numpy(self.len_factor), device))
        return t

    # ---- device work: no host synchronisation, nothing comes back
    def _run(self, seqs, sample_n, start_idx, end_idx, pick):
        sample_n = check_sample_n(sample_n)
        if seqs.dim() != 2 or seqs.shape[0] == 0 or seqs.shape[0] % sample_n != 0:
            raise ValueError(f"Consensus: token rows of shape {tuple(seqs.shape)}; clip-major rows [B * {sample_n}, T] expected")
        _lib.require_cuda(seqs)
        seqs = seqs.to(torch.long).contiguous()
        n, T = seqs.shape
        if not (1 <= T <= MAX_LENGTH):
            raise ValueError(f"Consensus: rows of {T} tokens; the kernel takes 1 .. {MAX_LENGTH}")
        B = n // sample_n
        keys, vals, len_factor = self._tables(seqs.device)
        score = torch.empty(B, sample_n, dtype=torch.float64, device=seqs.device)
        best = torch.empty(B, dtype=torch.long, device=seqs.device)
        picked = torch.empty(B, T, dtype=torch.long, device=seqs.device) if pick else None
        n_idf = int(self.idf_keys.size)
        _lib.call("acvae_consensus_scores", seqs, T, n, sample_n, T, int(start_idx), int(end_idx),
                  keys if n_idf else None, vals if n_idf else None, n_idf, float(self.log_d), len_factor,
                  int(self.len_factor.size), score, best, picked, _lib.current_stream())
        out = {"scores": score, "best": best}
        if pick:
            out["seqs"] = picked
        return out

    def scores(self, seqs, sample_n, start_idx=1, end_idx=2):
        """Token rows i64 [B * sample_n, T], clip-major -> {"scores": f64 [B, sample_n], "best": i64 [B]}, on the device."""
        return self._run(seqs, sample_n, start_idx, end_idx, False)

    def select(self, seqs, sample_n, start_idx=1, end_idx=2):
        """``scores`` and the picked rows: {"scores", "best", "seqs": i64 [B, T] = seqs[b * sample_n + best[b]]}."""
        return self._run(seqs, sample_n, start_idx, end_idx, True)
