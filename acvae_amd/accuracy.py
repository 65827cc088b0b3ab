"""Captions scored against their references on the device: BLEU-1..4, ROUGE-L and CIDEr.

The numbers of the reference's ``BaseRunner.evaluate`` (``runners/base_runner.py:295-316``: ``Bleu(n=4)``, ``Rouge()``,
``Cider()``) and of the validation pass of its training loop (``runners/pytorch_runner_vae.py:339-388``, whose ``Cider()``
score drives the scheduler and the ``best.pth`` decision).  ``Accuracy`` keeps the token rows where the decode left them;
``result()`` uploads the references of the clips seen, launches ``acvae_accuracy_stats`` (csrc/accuracy.hip: the integers
behind BLEU and ROUGE-L) and ``acvae_ciderd_scores`` (csrc/cider.hip), makes one download and evaluates the formulas in
float64.  There is no host scorer here (tests/accuracy_util.py holds the definitions on strings).

Rows: i64 [B * N, T], clip-major (row b * N + i), 1 <= N <= 16, 1 <= T <= 64, cleaned as ``acvae_diversity_stats`` cleans them
(cut at the first ``<end>``, ``<start>`` skipped wherever it stands).  References: strings, split by ``str.split()``.  A word
matches the same word; a reference word outside the vocabulary matches nothing, and neither does a row's id outside
[0, V).  h the cleaned row, L its length, R its clip's references, c_s(g) the count of n-gram g in s, orders k = 1..4.
  per row:   testlen = L,  guess_k = max(0, L - k + 1),  correct_k = sum_{g in h} min(c_h(g), max_{r in R} c_r(g)),
             reflen = the len(r) that minimises (|len(r) - L|, len(r))  ("closest");
             lcs_p = max_r LCS(h, r);  (lcs_r, len_r) = the (LCS(h, r), len(r)) with the largest quotient (the earlier
             reference on a tie)
  BLEU:      per candidate index i, with C_k, G_k, TL, RL the sums over clips:  p = 1;  for k = 1..4:
             p *= (C_k + 1e-15) / (G_k + 1e-9), bleu_k(i) = p ** (1 / k);  if (TL + 1e-15) / (RL + 1e-9) = ratio < 1, every
             bleu_k(i) is multiplied by exp(1 - 1 / ratio)
  ROUGE-L:   per row p = lcs_p / L, r = lcs_r / len_r, score = (1 + 1.2^2) p r / (r + 1.2^2 p), 0 if p or r is 0 or L is 0;
             rouge(i) = the mean over clips
  CIDEr:     ``CiderD.prepare(keys, key2refs, mode="batch")`` over all clips seen (acvae_amd/cider.py has the definition): the
             document frequencies are those of the evaluated set, as in one ``compute_score`` call; cider(i) = the mean over
             clips of the scores of the rows i, i + N, ...
  The top-level numbers are the means over i; with N = 1 they are the plain corpus scores.
The constants and rules are pycocoevalcap's ``Bleu`` / ``Rouge`` / ``Cider`` as recalled; agreement with that package is NOT
verified (it is not available here): the formulas above are this project's statement of them.  Departure from the
reference: no PTB tokenizer.  References must be given tokenized as the vocabulary's words are; the rows are vocabulary
ids, so words and tokens coincide.  METEOR and SPICE need Java and stay outside.
"""
import math

import numpy as np
import torch

from . import _lib
from .cider import CiderD
from .consensus import MAX_LENGTH, MAX_SAMPLES, MAX_VOCAB

RECORD = int(_lib._defs["ACVAE_ACCURACY_RECORD"])
OOV = -1                                          # a reference word outside the vocabulary, in the device's word array
_ORDERS = 4
_SMALL, _TINY = 1e-9, 1e-15
_BETA2 = 1.2 * 1.2


def check_sample_n(sample_n, who="Accuracy"):
    if isinstance(sample_n, bool) or not isinstance(sample_n, (int, np.integer)) or not (1 <= sample_n <= MAX_SAMPLES):
        raise ValueError(f"{who}: 1 <= N <= {MAX_SAMPLES} captions per clip, got {sample_n!r}")
    return int(sample_n)


class Accuracy:
    """``evaluate(..., accuracy=Accuracy(vocabulary, key2refs))``, then ``result()``; or ``update(keys, seqs, sample_n)`` on
    any clip-major token rows on the device, or ``update_payload(payload)`` on a prediction document."""

    def __init__(self, vocabulary, key2refs):
        i2w = vocabulary.idx2word
        items = list(i2w.items()) if hasattr(i2w, "items") else list(enumerate(i2w))
        self.word2id = {}
        for idx, w in items:
            idx = int(idx)
            if not isinstance(w, str) or w == "" or w.split() != [w]:
                raise ValueError(f"Accuracy: vocabulary word {w!r} (id {idx}) is empty or contains whitespace: a sentence "
                                 "built from it would not split back into the same words")
            if w in self.word2id:
                raise ValueError(f"Accuracy: ids {self.word2id[w]} and {idx} share the word {w!r}")
            if idx < 0:
                raise ValueError(f"Accuracy: negative token id {idx}")
            self.word2id[w] = idx
        self.V = max(self.word2id.values()) + 1 if self.word2id else 0
        if self.V > MAX_VOCAB:
            raise ValueError(f"Accuracy: token ids up to {self.V - 1}; an n-gram key holds 16 bits per id (V <= {MAX_VOCAB})")
        for name in ("<start>", "<end>"):
            if name not in self.word2id:
                raise ValueError(f"Accuracy: the vocabulary has no {name} word: the rows could not be cleaned")
        self.start_idx, self.end_idx = self.word2id["<start>"], self.word2id["<end>"]
        self.key2refs = {}
        for key, refs in key2refs.items():
            refs = tuple(refs)
            if not refs:
                raise ValueError(f"Accuracy: key {key!r} has no references")
            for ref in refs:
                if not isinstance(ref, str) or not ref.split():
                    raise ValueError(f"Accuracy: key {key!r} has a reference without words ({ref!r})")
            self.key2refs[key] = refs
        self._cider = CiderD(vocabulary)
        self.reset()

    def reset(self):
        """Forget every update: the rows, their keys and the N and row width they shared."""
        self.sample_n = None
        self.width = None
        self._keys = []
        self._seen = set()
        self._rows = []

    def check(self, sample_n, who="Accuracy"):
        """The refusal of an N this object cannot take (ValueError), without touching its state."""
        sample_n = check_sample_n(sample_n, who)
        if self.sample_n is not None and sample_n != self.sample_n:
            raise ValueError(f"{who}: {sample_n} captions per clip after updates with {self.sample_n}: all updates of one "
                             "object share one N (reset() starts over)")
        return sample_n

    def update(self, keys, seqs, sample_n=1):
        """Token rows i64 [B * sample_n, T] on the device, clip-major, and the B clips' keys.  No launch, no copy and no
        synchronisation: the rows are kept as they are until ``result()`` (every decode of this package returns freshly
        allocated rows, never a view of a reused workspace; a caller that overwrites its rows in place hands in a clone)."""
        sample_n = self.check(sample_n)
        keys = list(keys)
        if seqs.dim() != 2 or seqs.shape[0] == 0 or seqs.shape[0] != len(keys) * sample_n:
            raise ValueError(f"Accuracy: token rows of shape {tuple(seqs.shape)} for {len(keys)} keys; clip-major rows "
                             f"[{len(keys)} * {sample_n}, T] expected")
        T = seqs.shape[1]
        if not (1 <= T <= MAX_LENGTH):
            raise ValueError(f"Accuracy: rows of {T} tokens; the kernel takes 1 .. {MAX_LENGTH}")
        if self.width is not None and T != self.width:
            raise ValueError(f"Accuracy: rows of {T} tokens after updates with rows of {self.width}: all updates of one "
                             "object share one row width (reset() starts over)")
        fresh = set()
        for k in keys:
            if k not in self.key2refs:
                raise ValueError(f"Accuracy: key {k!r} has no references")
            if k in self._seen or k in fresh:
                raise ValueError(f"Accuracy: key {k!r} seen twice: a clip is scored once")
            fresh.add(k)
        _lib.require_cuda(seqs)
        if self._rows and self._rows[0].device != seqs.device:
            raise ValueError(f"Accuracy: rows on {seqs.device} after updates on {self._rows[0].device}")
        self.sample_n, self.width = sample_n, T
        self._keys += keys
        self._seen |= fresh
        self._rows.append(seqs)

    def update_payload(self, payload, device=None):
        """Score a prediction document of ``evaluate``: {"predictions": [{"filename", "tokens"}, ...]} (one caption per clip)
        or {"predictions": [{"filename", "captions": [{"tokens"}, ...]}, ...]}.  The tokens are mapped to ids through the
        vocabulary and the rows go through ``update``.  A word the vocabulary lacks, ``<start>`` / ``<end>`` as a word, clips
        with differing numbers of captions, more than 16 of them or a caption of more than 64 words: ValueError."""
        rows, keys, counts = [], [], set()
        for pred in payload["predictions"]:
            caps = pred["captions"] if "captions" in pred else [pred]
            keys.append(pred.get("filename"))
            counts.add(len(caps))
            for cap in caps:
                ids = []
                for w in cap["tokens"].split():
                    if w not in self.word2id or w in ("<start>", "<end>"):
                        raise ValueError(f"Accuracy: clip {pred.get('filename')!r}: the word {w!r} is not a word of the "
                                         "vocabulary")
                    ids.append(self.word2id[w])
                if len(ids) > MAX_LENGTH:
                    raise ValueError(f"Accuracy: clip {pred.get('filename')!r}: a caption of {len(ids)} words; the kernel "
                                     f"takes at most {MAX_LENGTH}")
                rows.append(ids)
        if len(counts) != 1:
            raise ValueError(f"Accuracy: clips with differing numbers of captions ({sorted(counts)}); one N per object")
        sample_n = self.check(counts.pop())
        T = self.width if self.width is not None else min(MAX_LENGTH, max(len(r) for r in rows) + 1)
        if max(len(r) for r in rows) > T:
            raise ValueError(f"Accuracy: a caption of {max(len(r) for r in rows)} words after updates with rows of {T} tokens")
        seqs = np.full((len(rows), T), self.end_idx, dtype=np.int64)
        for out, ids in zip(seqs, rows):
            out[:len(ids)] = ids
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
            device = self._rows[0].device if self._rows else torch.device("cuda", torch.cuda.current_device())
        self.update(keys, _lib.h2d(torch.from_numpy(seqs), device), sample_n)

    def reference_tables(self, keys):
        """The references of ``keys`` as the kernel reads them (include/acvae_hip.h): (ref_words, ref_off, clip_ref), int32."""
        words, ref_off, clip_ref = [], [0], [0]
        for k in keys:
            for ref in self.key2refs[k]:
                words += [self.word2id.get(w, OOV) for w in ref.split()]
                ref_off.append(len(words))
            clip_ref.append(len(ref_off) - 1)
        return np.array(words, dtype=np.int32), np.array(ref_off, dtype=np.int32), np.array(clip_ref, dtype=np.int32)

    # ---- one upload, the launches, one download, and the formulas in float64
    def result(self):
        """{"Bleu_1" .. "Bleu_4", "ROUGE_L", "CIDEr" (the means over the candidate index), "clips", "sample_n", "per_index":
        {each of the six: [sample_n values]}, "per_clip": {"ROUGE_L", "CIDEr": float64 [clips, sample_n]}}, clips in the order
        of the updates."""
        if not self._rows:
            raise ValueError("Accuracy: result() without an update")
        N, T, clips = self.sample_n, self.width, len(self._keys)
        rows = [r.to(torch.long) for r in self._rows]
        seqs = (rows[0] if len(rows) == 1 else torch.cat(rows)).contiguous()
        dev = seqs.device
        tabs = self.reference_tables(self._keys)
        sizes = [t.size for t in tabs]
        flat = _lib.h2d(torch.from_numpy(np.concatenate(tabs)), dev)
        ref_words, ref_off, clip_ref = torch.split(flat, sizes)
        record = torch.empty(clips * N, RECORD, dtype=torch.int32, device=dev)
        _lib.call("acvae_accuracy_stats", seqs, seqs.stride(0), clips * N, N, T, self.start_idx, self.end_idx, self.V,
                  ref_words, sizes[0], ref_off, sizes[1] - 1, clip_ref, clips, record, _lib.current_stream())
        tables = self._cider.prepare(self._keys, self.key2refs, mode="batch", device=dev)
        by_clip = seqs.view(clips, N, T)
        cider = [tables.scores(by_clip[:, i], start_idx=self.start_idx, end_idx=self.end_idx) for i in range(N)]
        down = torch.cat([torch.stack(cider, dim=1).reshape(-1).view(torch.uint8), record.reshape(-1).view(torch.uint8)])
        down = down.cpu().numpy()
        split = clips * N * 8
        return summarize(down[split:].view(np.int32).reshape(clips * N, RECORD), down[:split].view(np.float64), N)


def summarize(record, cider, sample_n):
    """int32 records [clips * sample_n, RECORD] (clip-major) and the rows' CIDEr scores -> the result dict."""
    N = int(sample_n)
    record = np.asarray(record).astype(np.int64).reshape(-1, N, RECORD)
    cider = np.asarray(cider, dtype=np.float64).reshape(-1, N)
    clips = record.shape[0]
    total = record.sum(axis=0)                                  # integers: [N, RECORD]
    guess = np.stack([np.maximum(0, record[:, :, 0] - k).sum(axis=0) for k in range(_ORDERS)], axis=1)
    rouge = np.zeros((clips, N), dtype=np.float64)
    per_index = {f"Bleu_{k + 1}": [] for k in range(_ORDERS)}
    per_index.update(ROUGE_L=[], CIDEr=[])
    for i in range(N):
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
            per_index[f"Bleu_{k + 1}"].append(bleu[k])
        rsum = csum = 0.0
        for b in range(clips):                                  # in clip order
            L, lcs_p, lcs_r, len_r = (int(x) for x in record[b, i, [0, 6, 7, 8]])
            if L > 0 and lcs_p > 0 and lcs_r > 0 and len_r > 0:
                prec, rec = float(lcs_p) / float(L), float(lcs_r) / float(len_r)
                rouge[b, i] = ((1.0 + _BETA2) * prec * rec) / (rec + _BETA2 * prec)
            rsum += rouge[b, i]
            csum += float(cider[b, i])
        per_index["ROUGE_L"].append(rsum / clips)
        per_index["CIDEr"].append(csum / clips)
    out = {}
    for name, vals in per_index.items():
        s = 0.0
        for v in vals:
            s += v
        out[name] = s / N
    out.update(clips=clips, sample_n=N, per_index=per_index, per_clip={"ROUGE_L": rouge, "CIDEr": cider})
    return out
