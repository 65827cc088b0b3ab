"""Diversity of a clip's N captions, counted on the device: Div-1, Div-2, mBLEU-1..4 and the vocabulary size (gDiv-1).

The numbers of the reference's ``utils/diverse_mutil.py:17-54`` (``eval_div_stats``) and ``utils/div_utils.py`` over N captions
per clip.  Every statistic behind them is an integer count of n-grams within one clip's token rows, so
``acvae_diversity_stats`` (csrc/diversity.hip) counts where the decode left the rows and ``Diversity`` keeps the per-clip
records on the device; ``result()`` makes the one download and evaluates the formulas in float64.  There is no host counter
here (tests/diversity_util.py holds the definitions on strings).

Rows: i64 [B * N, T], clip-major (row b * N + i), 2 <= N <= 16, 1 <= T <= 64, cleaned as ``acvae_consensus_scores`` cleans
them (cut at the first ``<end>``, ``<start>`` skipped wherever it stands); a kept id outside [0, V) is one shared
out-of-range word.  h_i the cleaned candidate i, L_i its length, c_i(g) the count of n-gram g in it, orders k = 1..4.
  per clip:       words = sum_i L_i;  distinct_k = the number of different order-k n-grams over the N candidates;
                  div_k = distinct_k / (1e-6 + words)  (words in the denominator for every k);  Div-k = mean over clips
  per candidate:  the clip's other N - 1 candidates are its references:  testlen = L_i,  guess_k = max(0, L_i - k + 1),
                  correct_k = sum_{g in h_i} min(c_i(g), max_{j != i} c_j(g)),
                  reflen = the L_j (j != i) that minimises (|L_j - L_i|, L_j)  ("closest")
  corpus:         per candidate index i, with C_k, G_k, TL, RL the sums over clips:  p = 1;  for k = 1..4:
                  p *= (C_k + 1e-15) / (G_k + 1e-9), bleu_k(i) = p ** (1 / k);  if (TL + 1e-15) / (RL + 1e-9) = ratio < 1,
                  every bleu_k(i) is multiplied by exp(1 - 1 / ratio);  mBLEU-k = mean_i bleu_k(i)
  global:         gDiv-1 = the number of different words over every caption seen.
The constants and the "closest" rule are pycocoevalcap's Bleu(4) as recalled; agreement with that package is NOT verified
(it is not available here).  Departure from the reference: no PTB tokenizer, the rows are vocabulary ids, so words and
tokens coincide.
"""
import math

import numpy as np
import torch

from . import _lib
from .consensus import MAX_LENGTH, MAX_SAMPLES, MAX_VOCAB

HEAD = int(_lib._defs["ACVAE_DIVERSITY_HEAD"])
PER = int(_lib._defs["ACVAE_DIVERSITY_PER_CANDIDATE"])
_ORDERS = 4
_SMALL, _TINY = 1e-9, 1e-15


def check_sample_n(sample_n, who="Diversity"):
    if isinstance(sample_n, bool) or not isinstance(sample_n, (int, np.integer)) or not (2 <= sample_n <= MAX_SAMPLES):
        raise ValueError(f"{who}: diversity is defined over 2 <= N <= {MAX_SAMPLES} captions per clip, got {sample_n!r}")
    return int(sample_n)


def record_ints(sample_n):
    """The int32 words of one clip's record (include/acvae_hip.h)."""
    return HEAD + PER * int(sample_n)


class Diversity:
    """``evaluate(..., diversity=Diversity(vocabulary))``, then ``result()``; or ``update(seqs, sample_n)`` on any clip-major
    token rows on the device, or ``update_payload(payload)`` on a prediction document."""

    def __init__(self, vocabulary):
        i2w = vocabulary.idx2word
        items = list(i2w.items()) if hasattr(i2w, "items") else list(enumerate(i2w))
        self.word2id = {}
        for idx, w in items:
            idx = int(idx)
            if not isinstance(w, str) or w == "" or w.split() != [w]:
                raise ValueError(f"Diversity: vocabulary word {w!r} (id {idx}) is empty or contains whitespace: a sentence "
                                 "built from it would not split back into the same words")
            if w in self.word2id:
                raise ValueError(f"Diversity: ids {self.word2id[w]} and {idx} share the word {w!r}")
            if idx < 0:
                raise ValueError(f"Diversity: negative token id {idx}")
            self.word2id[w] = idx
        self.V = max(self.word2id.values()) + 1 if self.word2id else 0
        if self.V > MAX_VOCAB:
            raise ValueError(f"Diversity: token ids up to {self.V - 1}; an n-gram key holds 16 bits per id (V <= {MAX_VOCAB})")
        for name in ("<start>", "<end>"):
            if name not in self.word2id:
                raise ValueError(f"Diversity: the vocabulary has no {name} word: the rows could not be cleaned")
        self.start_idx, self.end_idx = self.word2id["<start>"], self.word2id["<end>"]
        self.reset()

    def reset(self):
        """Forget every update: the records, the seen words and the N they shared."""
        self.sample_n = None
        self._records = []
        self._seen = None

    def check(self, sample_n, who="Diversity"):
        """The refusal of an N this object cannot take (ValueError), without touching its state."""
        sample_n = check_sample_n(sample_n, who)
        if self.sample_n is not None and sample_n != self.sample_n:
            raise ValueError(f"{who}: {sample_n} captions per clip after updates with {self.sample_n}: all updates of one "
                             "object share one N (reset() starts over)")
        return sample_n

    # ---- device work: no host synchronisation, nothing comes back
    def _launch(self, seqs, sample_n, seen):
        if seqs.dim() != 2 or seqs.shape[0] == 0 or seqs.shape[0] % sample_n != 0:
            raise ValueError(f"Diversity: token rows of shape {tuple(seqs.shape)}; clip-major rows [B * {sample_n}, T] expected")
        _lib.require_cuda(seqs)
        seqs = seqs.to(torch.long)
        if seqs.stride(1) != 1 or seqs.stride(0) < seqs.shape[1]:
            seqs = seqs.contiguous()
        n, T = seqs.shape
        if not (1 <= T <= MAX_LENGTH):
            raise ValueError(f"Diversity: rows of {T} tokens; the kernel takes 1 .. {MAX_LENGTH}")
        if seen is None:
            seen = torch.zeros(self.V + 1, dtype=torch.int32, device=seqs.device)
        elif seen.device != seqs.device:
            raise ValueError(f"Diversity: rows on {seqs.device} after updates on {seen.device}")
        record = torch.empty(n // sample_n, record_ints(sample_n), dtype=torch.int32, device=seqs.device)
        _lib.call("acvae_diversity_stats", seqs, seqs.stride(0), n, sample_n, T, self.start_idx, self.end_idx, self.V, record,
                  seen, _lib.current_stream())
        return record, seen

    def update(self, seqs, sample_n):
        """Token rows i64 [B * sample_n, T] on the device, clip-major: one launch on the current stream; the record stays
        on the device until ``result()``."""
        sample_n = self.check(sample_n)
        record, self._seen = self._launch(seqs, sample_n, self._seen)
        self.sample_n = sample_n
        self._records.append(record)

    def stats(self, seqs, sample_n):
        """The raw record of one call, on the device: {"record": i32 [B, HEAD + PER * sample_n] (include/acvae_hip.h has the
        layout), "seen": i32 [V + 1]}.  Leaves the object's state alone."""
        record, seen = self._launch(seqs, check_sample_n(sample_n), None)
        return {"record": record, "seen": seen}

    def update_payload(self, payload, device=None):
        """Score a prediction document {"predictions": [{"filename", "captions": [{"tokens"}, ...]}, ...]}, the form
        ``evaluate`` writes for N captions per clip and the reference's script reads: the tokens are mapped to ids through
        the vocabulary and the rows go through ``update``.  A word the vocabulary lacks, ``<start>`` / ``<end>`` as a word,
        clips with differing numbers of captions, one caption per clip or a caption of more than 64 words: ValueError."""
        rows, counts = [], set()
        for pred in payload["predictions"]:
            caps = pred.get("captions")
            if caps is None:
                raise ValueError(f"Diversity: clip {pred.get('filename')!r} has one caption; diversity needs at least two")
            counts.add(len(caps))
            for cap in caps:
                ids = []
                for w in cap["tokens"].split():
                    if w not in self.word2id or w in ("<start>", "<end>"):
                        raise ValueError(f"Diversity: clip {pred.get('filename')!r}: the word {w!r} is not a word of the "
                                         "vocabulary")
                    ids.append(self.word2id[w])
                if len(ids) > MAX_LENGTH:
                    raise ValueError(f"Diversity: clip {pred.get('filename')!r}: a caption of {len(ids)} words; the kernel "
                                     f"takes at most {MAX_LENGTH}")
                rows.append(ids)
        if len(counts) != 1:
            raise ValueError(f"Diversity: clips with differing numbers of captions ({sorted(counts)}); one N per object")
        sample_n = self.check(counts.pop())
        T = min(MAX_LENGTH, max(len(r) for r in rows) + 1)
        seqs = np.full((len(rows), T), self.end_idx, dtype=np.int64)
        for out, ids in zip(seqs, rows):
            out[:len(ids)] = ids
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
            device = self._seen.device if self._seen is not None else torch.device("cuda", torch.cuda.current_device())
        self.update(_lib.h2d(torch.from_numpy(seqs), device), sample_n)

    # ---- the one download, and the formulas in float64
    def result(self):
        """{"Div1", "Div2", "gDiv1", "mBLeu_1" .. "mBLeu_4" (the reference's spellings), "clips", "sample_n", "per_clip":
        {"div1", "div2"} (float64 [clips], in the order of the updates)}."""
        if not self._records:
            raise ValueError("Diversity: result() without an update")
        flat = torch.cat([r.reshape(-1) for r in self._records] + [self._seen.sum(dtype=torch.int32).reshape(1)])
        flat = flat.cpu().numpy()
        return summarize(flat[:-1].reshape(-1, record_ints(self.sample_n)), self.sample_n, int(flat[-1]))


def summarize(record, sample_n, n_seen):
    """int32 records [clips, HEAD + PER * sample_n] and the number of seen words -> the result dict."""
    record = np.asarray(record).astype(np.int64)
    clips = record.shape[0]
    div = np.empty((2, clips), dtype=np.float64)
    sums = [0.0, 0.0]
    for b in range(clips):                                      # in clip order
        for k in range(2):
            div[k, b] = float(record[b, 1 + k]) / (1e-6 + float(record[b, 0]))
            sums[k] += div[k, b]
    out = {"Div1": sums[0] / clips, "Div2": sums[1] / clips, "gDiv1": float(n_seen)}
    cand = record[:, HEAD:].reshape(clips, sample_n, PER)
    total = cand.sum(axis=0)                                    # integers: [sample_n, PER]
    guess = np.stack([np.maximum(0, cand[:, :, 0] - k).sum(axis=0) for k in range(_ORDERS)], axis=1)
    mean = [0.0] * _ORDERS
    for i in range(sample_n):
        TL, RL = float(total[i, 0]), float(total[i, 1])
        p, bleu = 1.0, []
        for k in range(_ORDERS):
            p *= (float(total[i, 2 + k]) + _TINY) / (float(guess[i, k]) + _SMALL)
            bleu.append(p ** (1.0 / (k + 1)))
        ratio = (TL + _TINY) / (RL + _SMALL)
        if ratio < 1.0:
            bp = math.exp(1.0 - 1.0 / ratio)
            bleu = [x * bp for x in bleu]
        for k in range(_ORDERS):
            mean[k] += bleu[k]
    for k in range(_ORDERS):
        out[f"mBLeu_{k + 1}"] = mean[k] / sample_n
    out.update(clips=clips, sample_n=sample_n, per_clip={"div1": div[0], "div2": div[1]})
    return out
