"""CIDEr-D as the reward of self-critical sequence training, scored on the device.

The reference scores its rollouts with ``pycocoevalcap``'s ``Cider()`` (``utils/score_util.py:21-23``): the words go to the
host, become strings, and a dictionary-based scorer counts n-grams while the GPU idles.  Everything that score needs
besides the sampled words is known before the rollouts start, so ``CiderD.prepare(keys, key2refs, mode)`` builds the
reference side on the host (document frequencies, idf, the references' tf-idf weights, norms and lengths, the table of
length penalties), uploads it in one copy, and ``acvae_ciderd_scores`` / ``acvae_ciderd_reward`` (csrc/cider.hip) score the
token rows where the rollout left them.  There is no host ``compute_score`` here: the package keeps no CPU twin of device
work (tests/cider_util.py holds the definition as a dictionary scorer).

The score of one call over D documents, document d with reference strings R_d and hypothesis h_d (float64):
  tokens are str.split(); n-grams of orders k = 1..4; c_s(g) the count of n-gram g in sentence s
  df(g)   the number of documents with g in at least one reference;  idf(g) = ln D - ln max(1, df(g))
  v_s(g)  = c_s(g) idf(g);  norm_k(s) = sqrt(sum_g v_s(g)^2) over the order-k n-grams of s
  len(s)  the number of BIGRAMS of s (pycocoevalcap adds up term frequencies where len(ngram) - 1 == 1)
  sim_k(h, r) = sum_{g in h} min(v_h(g), v_r(g)) v_r(g), divided by norm_k(h) norm_k(r) if both are non-zero, times
                exp(-(len h - len r)^2 / (2 sigma^2))
  score(d) = 10 mean_k (1 / |R_d|) sum_r sim_k(h_d, r);  D = 1 gives ln D = 0 and every score 0 (kept on purpose).
Modes, after the reference's two callers:
  "batch"  compute_batch_score: the documents are the distinct keys; a row is scored by the words of the FIRST row with
           its key; the sampled and the greedy rollout share one table (two sets of rows in one launch)
  "rows"   compur_batch_score_samplen: every row is a document, a clip's references count once per row in df.

Device layout (include/acvae_hip.h): an in-vocabulary n-gram is the 64-bit key sum_j (id_j + 1) << (16 j), which is exact
for V <= 65534; one ascending (key, idf) array per batch; per reference an ascending (key, weight) slice; per document a
reference range; per row its document and the row whose words score it.  Reference words outside the vocabulary keep
their identity on the host (they count in df and in the norms) and need no device entry: no hypothesis holds them.
"""
import numpy as np
import torch

from . import _lib

MAX_VOCAB = 65534
MAX_LENGTH = int(_lib._defs["ACVAE_CIDER_MAX_LENGTH"])
_ORDERS = 4


def pack_ngram(ids):
    """The device key of an n-gram of token ids (all in [0, MAX_VOCAB))."""
    key = 0
    for j, w in enumerate(ids):
        key |= (int(w) + 1) << (16 * j)
    return key


class _Cooked:
    """One key's references: per reference the distinct n-grams (global ids), their counts, orders and device keys (0: holds
    an out-of-vocabulary word), the in-vocabulary ones first in ascending key order; concatenated over the references."""
    __slots__ = ("refs", "nref", "gid", "cnt", "order", "dkey", "seg", "ndev", "blen", "doc_gid", "dev_gid", "dev_dkey")


class CiderTables:
    """What prepare() built, as numpy arrays (`host`) and, after upload, as views of one device buffer (`dev`)."""
    FIELDS = (("idf_keys", np.uint64), ("idf_vals", np.float64), ("ref_keys", np.uint64), ("ref_w", np.float64),
              ("ref_norm", np.float64), ("len_factor", np.float64), ("ref_off", np.int32), ("ref_len", np.int32),
              ("doc_ref", np.int32), ("row_doc", np.int32), ("row_src", np.int32))

    def __init__(self, mode, n_rows, n_docs, log_d, host):
        self.mode, self.n_rows, self.n_docs, self.log_d, self.host = mode, n_rows, n_docs, log_d, host
        self.dev = None
        self.nbytes = sum((a.nbytes + 7) & ~7 for a in host.values())

    def upload(self, device):
        """One host-to-device copy through the page-locked ring; the tables become typed views of that buffer."""
        blob = np.zeros(self.nbytes, dtype=np.uint8)
        spans, off = {}, 0
        for name, dt in self.FIELDS:
            a = self.host[name]
            blob[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
            spans[name] = (off, a.nbytes, a.shape)
            off += (a.nbytes + 7) & ~7
        d = _lib.h2d(torch.from_numpy(blob), device)
        tdt = {np.uint64: torch.int64, np.float64: torch.float64, np.int32: torch.int32}
        self.dev = {name: d[spans[name][0]:spans[name][0] + spans[name][1]].view(tdt[dt]) for name, dt in self.FIELDS}
        self._blob = d
        return self

    # ---- device work: no host synchronisation, nothing comes back
    def scores(self, seqs, seqs2=None, start_idx=1, end_idx=2):
        """float64 scores [n_sets * n_rows] of the token rows `seqs` (and `seqs2`, e.g. the greedy rollout) i64 [n_rows, T]."""
        if self.dev is None:
            raise RuntimeError("CiderTables.scores: the tables are on the host only; prepare(..., device=) uploads them")
        sets = [seqs] + ([seqs2] if seqs2 is not None else [])
        _lib.require_cuda(*sets)
        sets = [s.to(torch.long).contiguous() for s in sets]
        n, T = sets[0].shape
        if n != self.n_rows or any(tuple(s.shape) != (n, T) for s in sets):
            raise ValueError(f"CiderD: prepared for {self.n_rows} rows, got token rows of shape {[tuple(s.shape) for s in sets]}")
        if T > MAX_LENGTH:
            raise ValueError(f"CiderD: rows of {T} tokens; the score kernel takes at most {MAX_LENGTH}")
        d, h = self.dev, self.host
        score = torch.empty(len(sets) * n, dtype=torch.float64, device=sets[0].device)
        _lib.call("acvae_ciderd_scores", sets[0], sets[1] if len(sets) > 1 else None, T, n, len(sets), T, int(start_idx),
                  int(end_idx), d["idf_keys"], d["idf_vals"], h["idf_keys"].size, float(self.log_d), d["ref_keys"], d["ref_w"],
                  h["ref_keys"].size, d["ref_off"], d["ref_norm"], d["ref_len"], h["ref_len"].size, d["doc_ref"],
                  h["doc_ref"].size - 1, d["row_doc"], d["row_src"], d["len_factor"], h["len_factor"].size, score,
                  _lib.current_stream())
        return score

    def reward(self, sampled_seqs, greedy_seqs=None, sample_n=1, start_idx=1, end_idx=2):
        """The SCST reward on the device.  sample_n == 1: sampled score - greedy score; sample_n >= 2: each row's score minus
        the mean of its clip's other rows (rows clip-major).  -> {"reward": f32 [n], "score": f64 [n] (the sampled rows'),
        "reward_mean": f64 [1]}."""
        if (sample_n <= 1) != (greedy_seqs is not None):
            raise ValueError("CiderD: the greedy rollout is the baseline of sample_n == 1, the clip's other rows of sample_n >= 2")
        score = self.scores(sampled_seqs, greedy_seqs, start_idx, end_idx)
        n = self.n_rows
        reward = torch.empty(n, dtype=torch.float32, device=score.device)
        mean = torch.empty(1, dtype=torch.float64, device=score.device)
        _lib.call("acvae_ciderd_reward", score, n, int(sample_n), reward, mean, _lib.current_stream())
        return {"reward": reward, "score": score[:n], "reward_mean": mean}


class CiderD:
    """``scorer=CiderD(vocabulary)`` for ScstWrapper / NScstWrapper / scst_Loss / Nscst_Loss / TrainStep.scst_step: the reward
    is computed on the device from the rollouts' token ids.  The references of a key are cooked once, the first time the
    key is seen (a key whose reference list changes is cooked again)."""

    def __init__(self, vocabulary, n=4, sigma=6.0):
        if int(n) != _ORDERS:
            raise ValueError("CiderD: the device kernel scores n-grams of orders 1..4 (n = 4)")
        i2w = vocabulary.idx2word
        items = list(i2w.items()) if hasattr(i2w, "items") else list(enumerate(i2w))
        self.n, self.sigma = int(n), float(sigma)
        self.word2id = {}
        for idx, w in items:
            idx = int(idx)
            if not isinstance(w, str) or w == "" or w.split() != [w]:
                raise ValueError(f"CiderD: vocabulary word {w!r} (id {idx}) is empty or contains whitespace: a sentence "
                                 "built from it would not split back into the same words")
            if w in self.word2id:
                raise ValueError(f"CiderD: ids {self.word2id[w]} and {idx} share the word {w!r}")
            if idx < 0:
                raise ValueError(f"CiderD: negative token id {idx}")
            self.word2id[w] = idx
        self.V = max(self.word2id.values()) + 1 if self.word2id else 0
        if self.V > MAX_VOCAB:
            raise ValueError(f"CiderD: token ids up to {self.V - 1}; an n-gram key holds 16 bits per id (V <= {MAX_VOCAB})")
        self._oov = {}            # reference words outside the vocabulary: host-only ids from V up
        self._gram = {}           # tuple of (extended) word ids -> global n-gram id
        self._cooked = {}
        self._df = np.zeros(1 << 16)   # scratch of prepare(): document frequency by n-gram id, all zero between calls
        self.last_prepare_s = 0.0

    # ---- once per key
    def _cook(self, refs):
        V, gram, oov, word2id = self.V, self._gram, self._oov, self.word2id
        c = _Cooked()
        c.refs, c.nref = refs, len(refs)
        gids, cnts, orders, dkeys, seg, ndev, blen = [], [], [], [], [], [], []
        for ref in refs:
            ids = []
            for w in ref.split():
                i = word2id.get(w)
                if i is None:
                    i = oov.get(w)
                    if i is None:
                        i = oov[w] = V + len(oov)
                ids.append(i)
            counts = {}
            for k in range(1, _ORDERS + 1):
                for p in range(len(ids) - k + 1):
                    g = tuple(ids[p:p + k])
                    counts[g] = counts.get(g, 0) + 1
            rows = []
            for g, tf in counts.items():
                gid = gram.get(g)
                if gid is None:
                    gid = gram[g] = len(gram)
                dk = pack_ngram(g) if max(g) < V else 0
                rows.append((dk == 0, dk, gid, tf, len(g) - 1))
            rows.sort()                                   # in-vocabulary n-grams first, by ascending device key
            gids += [r[2] for r in rows]
            cnts += [r[3] for r in rows]
            orders += [r[4] for r in rows]
            dkeys += [r[1] for r in rows]
            seg.append(len(rows))
            ndev.append(sum(1 for r in rows if not r[0]))
            blen.append(max(len(ids) - 1, 0))
        c.gid = np.array(gids, dtype=np.int64)
        c.cnt = np.array(cnts, dtype=np.float64)
        c.order = np.array(orders, dtype=np.int64)
        c.dkey = np.array(dkeys, dtype=np.uint64)
        c.seg = np.array(seg, dtype=np.int64)
        c.ndev = np.array(ndev, dtype=np.int64)
        c.blen = np.array(blen, dtype=np.int32)
        c.doc_gid, first = np.unique(c.gid, return_index=True)
        on_dev = c.dkey[first] != 0
        c.dev_gid, c.dev_dkey = c.doc_gid[on_dev], c.dkey[first][on_dev]
        return c

    def _cooked_of(self, key, key2refs):
        refs = tuple(key2refs[key])
        c = self._cooked.get(key)
        if c is None or c.refs != refs:
            if not refs:
                raise ValueError(f"CiderD: key {key!r} has no references")
            c = self._cooked[key] = self._cook(refs)
        return c

    # ---- once per batch
    def prepare(self, keys, key2refs, mode="batch", device=None):
        """Everything that depends on the references of this batch.  keys: one per row ("rows": the clip's key repeated for
        each of its rollouts).  With `device`, the tables are uploaded (queued on the current stream); without, they stay
        on the host (``tables.host``)."""
        import time
        t0 = time.perf_counter()
        if mode not in ("batch", "rows"):
            raise ValueError("CiderD.prepare: mode is 'batch' or 'rows'")
        keys = list(keys)
        n_rows = len(keys)
        if n_rows == 0:
            raise ValueError("CiderD.prepare: no rows")
        slot, first_row, row_doc = {}, [], np.empty(n_rows, dtype=np.int32)
        for i, k in enumerate(keys):
            s = slot.get(k)
            if s is None:
                s = slot[k] = len(slot)
                first_row.append(i)
            row_doc[i] = s
        cooked = [self._cooked_of(k, key2refs) for k in slot]
        mult = np.bincount(row_doc, minlength=len(cooked)).astype(np.float64)
        if mode == "batch":
            n_docs, weight = len(cooked), np.ones(len(cooked))
            row_src = np.asarray(first_row, dtype=np.int32)[row_doc]
        else:
            n_docs, weight = n_rows, mult
            row_src = np.arange(n_rows, dtype=np.int32)
        log_d = float(np.log(float(n_docs)))

        # df over the documents: a key's distinct n-grams count once per document that has the key.  Accumulated in a
        # scratch array over ALL n-grams ever cooked (ids are dense), which is zero between calls: no sort, no search
        if self._df.size < len(self._gram):
            self._df = np.zeros(max(2 * self._df.size, len(self._gram)))
        df = self._df
        doc_gid = np.concatenate([c.doc_gid for c in cooked])
        try:
            for c, wk in zip(cooked, weight):
                df[c.doc_gid] += wk                                   # (distinct within a key: a plain indexed add)
            df[doc_gid] = log_d - np.log(np.maximum(1.0, df[doc_gid]))      # the scratch now holds idf (one log per n-gram)
            idf_ref = df[np.concatenate([c.gid for c in cooked])]
            idf_doc = df[np.concatenate([c.dev_gid for c in cooked])]
        finally:
            df[doc_gid] = 0.0
        # the batch's (key, idf) table: the keys' own ascending tables merged, duplicates across keys dropped
        dkey = np.concatenate([c.dev_dkey for c in cooked])
        order = np.argsort(dkey)
        dkey, idf_doc = dkey[order], idf_doc[order]
        keep = np.ones(dkey.size, dtype=bool)
        keep[1:] = dkey[1:] != dkey[:-1]
        idf_keys, idf_vals = dkey[keep], idf_doc[keep]

        # the references' weights, norms and lengths
        w = np.concatenate([c.cnt for c in cooked]) * idf_ref
        seg = np.concatenate([c.seg for c in cooked])
        n_refs = seg.size
        ref_of = np.repeat(np.arange(n_refs), seg)
        ref_norm = np.sqrt(np.bincount(ref_of * _ORDERS + np.concatenate([c.order for c in cooked]), weights=w * w,
                                       minlength=n_refs * _ORDERS)).reshape(n_refs, _ORDERS)
        ndev = np.concatenate([c.ndev for c in cooked])
        start = np.cumsum(seg) - seg
        dev_mask = (np.arange(w.size) - start[ref_of]) < ndev[ref_of]       # a reference's device entries come first
        ref_off = np.zeros(n_refs + 1, dtype=np.int32)
        np.cumsum(ndev, out=ref_off[1:])
        ref_len = np.concatenate([c.blen for c in cooked])
        doc_ref = np.zeros(len(cooked) + 1, dtype=np.int32)
        np.cumsum([c.nref for c in cooked], out=doc_ref[1:])
        n_len = max(MAX_LENGTH - 1, int(ref_len.max())) + 1
        delta = np.arange(n_len, dtype=np.float64)
        host = dict(idf_keys=idf_keys, idf_vals=idf_vals, ref_keys=np.concatenate([c.dkey for c in cooked])[dev_mask],
                    ref_w=w[dev_mask], ref_norm=ref_norm, len_factor=np.exp(-(delta * delta) / (2.0 * self.sigma ** 2)),
                    ref_off=ref_off, ref_len=ref_len.astype(np.int32), doc_ref=doc_ref, row_doc=row_doc, row_src=row_src)
        host = {name: np.ascontiguousarray(host[name], dtype=dt) for name, dt in CiderTables.FIELDS}
        tables = CiderTables(mode, n_rows, n_docs, log_d, host)
        if device is not None:
            tables.upload(device)
        self.last_prepare_s = time.perf_counter() - t0
        return tables
