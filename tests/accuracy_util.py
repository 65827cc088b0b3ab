"""The yardstick of the accuracy tests (test_accuracy_cpu.py, test_accuracy_gpu.py; tools/bench_accuracy.py times it as the
host route): BLEU-1..4, ROUGE-L and CIDEr of captions against references on strings, with dictionaries of tuples and a
quadratic LCS table, in float64, written from the definitions.  It imports nothing from acvae_amd.accuracy and shares no
helper with it.

A clip has N candidate strings and a list R of reference strings; tokens are str.split(); h a candidate, L = len(tokens of
h); n-grams of orders k = 1..4; c_s(g) = count of g in s.  The word OUT ("<out>") stands for a candidate id outside the
vocabulary: it matches no reference word, not even a reference's own "<out>" (which, like every reference word outside the
vocabulary, matches no candidate word either); a candidate n-gram that holds it matches nothing.
  per candidate:  testlen = L;  guess_k = max(0, L - k + 1);
                  correct_k = sum over the different order-k g of h of min(c_h(g), max_{r in R} c_r(g));
                  reflen = the len(r), r in R, minimising (|len(r) - L|, len(r))                       ("closest")
                  lcs_p = max_r LCS(h, r);  (lcs_r, len_r) = the (LCS(h, r), len(r)) with the largest LCS / len, compared
                  as integers lcs * len' > lcs' * len; the earlier reference on a tie
  BLEU (Bleu(4), option "closest"): per candidate index i, C_k, G_k, TL, RL summed over clips; p = 1; for k = 1..4:
                  p *= (C_k + 1e-15) / (G_k + 1e-9); bleu_k(i) = p ** (1 / k); ratio = (TL + 1e-15) / (RL + 1e-9); if
                  ratio < 1 every bleu_k(i) is multiplied by exp(1 - 1 / ratio)
  ROUGE-L (Rouge(), beta = 1.2): p = lcs_p / L, r = lcs_r / len_r; score = (1 + beta^2) p r / (r + beta^2 p), 0 if p or r
                  is 0 or L is 0;  rouge(i) = mean over clips
  CIDEr:          cider_util.ciderd over the clips, candidate i of every clip as its hypothesis; cider(i) = its mean
  The top-level numbers are the means over i.

The bound of a comparison with acvae_amd.accuracy.Accuracy.result(): 1e-12 * max(1, |x|) for BLEU and ROUGE-L (the same
integers through the same dozen float64 operations, and a mean over at most a few hundred clips), cider_util.bound for CIDEr.
"""
import math

import cider_util as CU

SMALL, TINY = 1e-9, 1e-15
BETA = 1.2
OUT = "<out>"


def ngram_counts(sentence, n=4):
    words = sentence.split()
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


def lcs(a, b):
    """The length of the longest common subsequence of two word lists, by the quadratic table.  OUT in `a` equals nothing."""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if x == y and x != OUT:
                table[i + 1][j + 1] = table[i][j] + 1
            else:
                table[i + 1][j + 1] = max(table[i][j + 1], table[i + 1][j])
    return table[len(a)][len(b)]


def longest_common_substring(a, b):
    best = 0
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if x == y and x != OUT:
                table[i + 1][j + 1] = table[i][j] + 1
                best = max(best, table[i + 1][j + 1])
    return best


def cand_stats(candidate, refs, n=4):
    """One candidate string against its clip's reference strings -> {"testlen", "reflen", "guess" [n], "correct" [n],
    "lcs_p", "lcs_r", "len_r", and for the tests' non-vacuity conditions: "clipped" (some n-gram of the candidate occurs more
    often than in any reference), per reference "lcs", "substring" (the longest common substring), "unigrams" (the clipped
    unigram count against that reference alone) and "reflens", and "most" [n]: the largest reference count of one of the
    candidate's n-grams of that order}."""
    assert len(refs) >= 1
    mine = ngram_counts(candidate, n)
    theirs = [ngram_counts(r, n) for r in refs]
    h = candidate.split()
    rl = [r.split() for r in refs]
    assert all(rl)
    correct, most_of, clipped = [0] * n, [0] * n, False
    for g, v in mine.items():
        most = 0 if OUT in g else max(t.get(g, 0) for t in theirs)
        correct[len(g) - 1] += min(v, most)
        most_of[len(g) - 1] = max(most_of[len(g) - 1], most)
        clipped = clipped or v > most
    unigrams = [sum(min(v, t.get(g, 0)) for g, v in mine.items() if len(g) == 1 and OUT not in g) for t in theirs]
    reflen = min((abs(len(r) - len(h)), len(r)) for r in rl)[1]
    each = [lcs(h, r) for r in rl]
    lcs_r, len_r = each[0], len(rl[0])
    for x, r in zip(each[1:], rl[1:]):
        if x * len_r > lcs_r * len(r):
            lcs_r, len_r = x, len(r)
    return {"testlen": len(h), "reflen": reflen, "guess": [max(0, len(h) - k + 1) for k in range(1, n + 1)],
            "correct": correct, "lcs_p": max(each), "lcs_r": lcs_r, "len_r": len_r, "clipped": clipped, "lcs": each,
            "substring": [longest_common_substring(h, r) for r in rl], "unigrams": unigrams, "most": most_of,
            "reflens": [len(r) for r in rl]}


def record_of(stats):
    """A candidate's statistics as the integers of the device record (include/acvae_hip.h)."""
    return [stats["testlen"], stats["reflen"]] + list(stats["correct"]) + [stats["lcs_p"], stats["lcs_r"], stats["len_r"]]


def rouge_l(stats):
    if stats["testlen"] == 0 or stats["lcs_p"] == 0 or stats["lcs_r"] == 0:
        return 0.0
    p = float(stats["lcs_p"]) / float(stats["testlen"])
    r = float(stats["lcs_r"]) / float(stats["len_r"])
    return ((1.0 + BETA ** 2) * p * r) / (r + BETA ** 2 * p)


def corpus_bleu(cand_stats_list, n=4):
    """One candidate index's statistics over the clips -> [bleu_1 .. bleu_n], option "closest"."""
    TL = sum(c["testlen"] for c in cand_stats_list)
    RL = sum(c["reflen"] for c in cand_stats_list)
    p, bleu = 1.0, []
    for k in range(n):
        C = sum(c["correct"][k] for c in cand_stats_list)
        G = sum(c["guess"][k] for c in cand_stats_list)
        p *= (float(C) + TINY) / (float(G) + SMALL)
        bleu.append(p ** (1.0 / (k + 1)))
    ratio = (float(TL) + TINY) / (float(RL) + SMALL)
    if ratio < 1.0:
        bleu = [b * math.exp(1.0 - 1.0 / ratio) for b in bleu]
    return bleu


def accuracy(clips, keys, key2refs, n=4, cider=True):
    """[[candidate strings of clip 0], ...] (every clip with the same N >= 1), the clips' keys and the references ->
    {"Bleu_1" .. "Bleu_4", "ROUGE_L", "CIDEr", "clips", "sample_n", "per_index", "per_clip", "stats" [clip][candidate]}."""
    N = len(clips[0])
    assert N >= 1 and all(len(c) == N for c in clips) and len(keys) == len(clips) == len(set(keys))
    stats = [[cand_stats(h, key2refs[k], n) for h in c] for c, k in zip(clips, keys)]
    per_index = {f"Bleu_{k + 1}": [] for k in range(n)}
    per_index.update(ROUGE_L=[], CIDEr=[])
    rouge = [[rouge_l(s) for s in clip] for clip in stats]
    scores = [[0.0] * N for _ in clips]
    gts = {k: list(key2refs[k]) for k in keys}
    for i in range(N):
        bleu = corpus_bleu([clip[i] for clip in stats], n)
        for k in range(n):
            per_index[f"Bleu_{k + 1}"].append(bleu[k])
        per_index["ROUGE_L"].append(sum(r[i] for r in rouge) / len(clips))
        if cider:
            each = CU.ciderd(gts, {k: [c[i]] for k, c in zip(keys, clips)})[1]
            for b in range(len(clips)):
                scores[b][i] = float(each[b])
        per_index["CIDEr"].append(sum(s[i] for s in scores) / len(clips))
    out = {name: sum(vals) / N for name, vals in per_index.items()}
    out.update(clips=len(clips), sample_n=N, per_index=per_index, per_clip={"ROUGE_L": rouge, "CIDEr": scores}, stats=stats)
    return out


def sentence_of_ids(row, V, start_idx=1, end_idx=2):
    """A token row as the kernel is to read it: cut at the first <end>, <start> skipped wherever it stands, what stands
    behind the first <end> never looked at; a kept id outside [0, V) is the word OUT, every other id the word "w<id>"."""
    words = []
    for w in row:
        w = int(w)
        if w == end_idx:
            break
        if w == start_idx:
            continue
        words.append(f"w{w}" if 0 <= w < V else OUT)
    return " ".join(words)


def clips_of_rows(seqs, sample_n, V, start_idx=1, end_idx=2):
    """Clip-major token rows [B * sample_n, T] -> [[candidate strings] per clip]."""
    rows = [sentence_of_ids(r, V, start_idx, end_idx) for r in seqs]
    return [rows[b:b + sample_n] for b in range(0, len(rows), sample_n)]


def clips_of_payload(payload):
    """A prediction document of evaluate() -> (keys, [[the clip's token strings] per clip]), either form."""
    preds = payload["predictions"]
    return [p["filename"] for p in preds], [[c["tokens"] for c in p["captions"]] if "captions" in p else [p["tokens"]]
                                            for p in preds]


def bound(x):
    return 1e-12 * max(1.0, abs(x))
