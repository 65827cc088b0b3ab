"""The yardstick of the consensus-reranking tests (test_consensus_cpu.py, test_consensus_gpu.py; tools/bench_consensus.py
times it as the host route): a dictionary-of-tuples scorer on strings in float64, written from the definition.  It
imports nothing from acvae_amd.consensus and shares no helper with it.

A clip has candidate strings h_0 .. h_{N-1}, N >= 2; tokens are str.split(); n-grams of orders k = 1..4:
  c_i(g) = count of g in h_i;  v_i(g) = c_i(g) * idf(g), idf(g) = idf[g] if the table holds g, else log_d
  norm_k(i) = sqrt(sum_g v_i(g)^2) over the order-k n-grams of h_i;  len(i) = number of bigrams of h_i
  sim_k(i, j) = sum_{g in h_i} min(v_i(g), v_j(g)) * v_j(g)  [/ (norm_k(i) norm_k(j)) if both non-zero]
                * exp(-(len i - len j)^2 / (2 sigma^2))
  consensus(i) = 10 * mean_k (1 / (N - 1)) sum_{j != i} sim_k(i, j), j ascending;  an empty candidate scores 0
i.e. CIDEr-D of h_i with the clip's other candidates as its references.  The idf table is a corpus's:
corpus_idf(corpus) counts, per n-gram, the keys with it in at least one caption (D = number of keys,
idf = ln D - ln max(1, df)); no table and log_d = 1 weigh every n-gram 1.

The bound is cider_util.bound, 1e-12 * max(1, |score|): its derivation covers sums of at most 64 terms and a few rounded
operations per order; the extra sum over at most 15 candidates (15 * 2^-53 relative) stays far inside it.
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


def corpus_idf(corpus, n=4):
    """corpus {key: [caption strings]} -> ({n-gram tuple: idf}, log_d)."""
    df = {}
    for captions in corpus.values():
        for g in set(g for c in captions for g in ngram_counts(c, n)):
            df[g] = df.get(g, 0) + 1
    log_d = math.log(float(len(corpus)))
    return {g: log_d - math.log(max(1.0, float(c))) for g, c in df.items()}, log_d


def consensus(candidates, idf=None, log_d=1.0, n=4, sigma=6.0):
    """-> float64 [N]: the consensus score of every candidate string."""
    idf = {} if idf is None else idf
    N = len(candidates)
    assert N >= 2

    def vector(sentence):
        vec = [{} for _ in range(n)]
        sq = [0.0] * n
        length = 0
        for g, tf in ngram_counts(sentence, n).items():
            k = len(g) - 1
            vec[k][g] = float(tf) * idf.get(g, log_d)
            sq[k] += vec[k][g] ** 2
            if k == 1:
                length += tf
        return vec, [math.sqrt(x) for x in sq], length

    vectors = [vector(c) for c in candidates]
    scores = []
    for i, (vh, nh, lh) in enumerate(vectors):
        total = [0.0] * n
        for j, (vr, nr, lr) in enumerate(vectors):
            if j == i:
                continue
            penalty = math.exp(-(float(lh - lr) ** 2) / (2.0 * sigma ** 2))
            for k in range(n):
                s = 0.0
                for g, x in vh[k].items():
                    y = vr[k].get(g, 0.0)
                    s += min(x, y) * y
                if nh[k] != 0 and nr[k] != 0:
                    s /= nh[k] * nr[k]
                total[k] += s * penalty
        mean = (((total[0] + total[1]) + total[2]) + total[3]) / 4.0 if n == 4 else sum(total) / n
        scores.append(mean / (N - 1) * 10.0 if candidates[i].split() else 0.0)
    return np.array(scores, dtype=np.float64)


def clip_scores(seqs, sample_n, vocab, sentence_of, idf=None, log_d=1.0, sigma=6.0):
    """Clip-major token rows [B * sample_n, T] -> float64 [B, sample_n] by the yardstick on the rows' sentences
    (``sentence_of(row, vocab)`` turns a row into its string)."""
    seqs = np.asarray(seqs)
    B = len(seqs) // sample_n
    return np.stack([consensus([sentence_of(r, vocab) for r in seqs[b * sample_n:(b + 1) * sample_n]], idf, log_d, sigma=sigma)
                     for b in range(B)])
