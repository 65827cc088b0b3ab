"""The yardstick of the CIDEr-D tests (test_cider_cpu.py, test_cider_gpu.py; tools/bench_scst.py --scorer host times it):
a dictionary-of-tuples CIDEr-D on strings in float64, written from the definition in acvae_amd/cider.py's docstring (the
public pycocoevalcap cider_scorer with its two quirks: the sentence length is the number of bigrams, and one document
gives ln D = 0 and every score 0).  It imports nothing from acvae_amd.cider and shares no helper with it.

One call scores D documents; document d has reference strings gts[d] and one hypothesis string res[d][0]:
  df(g) = number of documents with n-gram g in at least one reference; idf(g) = ln D - ln max(1, df(g))
  v_s(g) = count_s(g) * idf(g); norm_k(s) = sqrt(sum v_s(g)^2) over the order-k n-grams of s; len(s) = bigrams of s
  sim_k(h, r) = sum_{g in h} min(v_h(g), v_r(g)) * v_r(g)  [/ (norm_k(h) norm_k(r)) if both non-zero]
                * exp(-(len h - len r)^2 / (2 sigma^2))
  score(d) = 10 * mean_k (1 / |refs|) sum_r sim_k(h_d, r)
"""
import math

import numpy as np


def ngram_counts(sentence, n=4):
    words = sentence.split()
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


def ciderd(gts, res, n=4, sigma=6.0):
    """-> (mean score, per-document scores in the order of gts' keys)."""
    docs = list(gts)
    refs = [[ngram_counts(r, n) for r in gts[d]] for d in docs]
    hyps = [ngram_counts(res[d][0], n) for d in docs]
    df = {}
    for doc in refs:
        for g in set(g for r in doc for g in r):
            df[g] = df.get(g, 0) + 1
    log_d = math.log(float(len(docs)))

    def vector(counts):
        vec = [{} for _ in range(n)]
        sq = [0.0] * n
        length = 0
        for g, tf in counts.items():
            k = len(g) - 1
            vec[k][g] = float(tf) * (log_d - math.log(max(1.0, float(df.get(g, 0)))))
            sq[k] += vec[k][g] ** 2
            if k == 1:
                length += tf
        return vec, [math.sqrt(x) for x in sq], length

    scores = []
    for hyp, doc in zip(hyps, refs):
        vh, nh, lh = vector(hyp)
        total = [0.0] * n
        for r in doc:
            vr, nr, lr = vector(r)
            penalty = math.exp(-(float(lh - lr) ** 2) / (2.0 * sigma ** 2))
            for k in range(n):
                s = 0.0
                for g, x in vh[k].items():
                    y = vr[k].get(g, 0.0)
                    s += min(x, y) * y
                if nh[k] != 0 and nr[k] != 0:
                    s /= nh[k] * nr[k]
                total[k] += s * penalty
        scores.append(float(np.mean(np.array(total))) / len(doc) * 10.0)
    scores = np.array(scores, dtype=np.float64)
    return float(scores.mean()), scores


class DictCiderD:
    """The yardstick as a scorer object: compute_score(references, hypotheses) -> (mean, per-key scores)."""

    def __init__(self, n=4, sigma=6.0):
        self.n, self.sigma = n, sigma

    def compute_score(self, references, hypotheses):
        return ciderd(references, hypotheses, self.n, self.sigma)


class Vocabulary:
    def __init__(self, words):
        self.idx2word = {i: w for i, w in enumerate(words)}


SPECIALS = ["<pad>", "<start>", "<end>", "<unk>"]


def sentence_of(row, vocab, start_idx=1, end_idx=2):
    """A token row as the reference's sentence conversion reads it: <start> skipped wherever it stands, cut at the first
    <end>, every other id (<pad> and <unk> included) its word."""
    words = []
    for w in row:
        w = int(w)
        if w == start_idx:
            continue
        if w == end_idx:
            break
        words.append(vocab.idx2word[w])
    return " ".join(words)


def row_scores(seqs, keys, key2refs, vocab, mode):
    """One float64 score per row of `seqs` by the yardstick, called as the reference's two callers call their scorer:
    "batch" - the documents are the distinct keys, each scored by the first row with that key; "rows" - every row is a
    document."""
    seqs = np.asarray(seqs)
    if mode == "rows":
        gts = {i: key2refs[k] for i, k in enumerate(keys)}
        res = {i: [sentence_of(seqs[i], vocab)] for i in range(len(keys))}
        return ciderd(gts, res)[1]
    gts, res = {}, {}
    for i, k in enumerate(keys):
        if k not in gts:
            gts[k], res[k] = key2refs[k], [sentence_of(seqs[i], vocab)]
    by_key = dict(zip(gts, ciderd(gts, res)[1]))
    return np.array([by_key[k] for k in keys], dtype=np.float64)


def bound(score):
    """1e-12 * max(1, |score|): two float64 evaluations of the definition differ only in the order of sums of at most 64
    non-negative terms (<= 64 * 2^-53 relative) and a handful of correctly rounded products, one square root and one
    division per order."""
    return 1e-12 * np.maximum(1.0, np.abs(score))
