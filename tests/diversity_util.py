"""The yardstick of the diversity tests (test_diversity_cpu.py, test_diversity_gpu.py; tools/bench_diversity.py times it as
the host route): Div-n, mBLEU and gDiv-1 of N captions per clip on strings with dictionaries of tuples, in float64, written
from the definitions.  It imports nothing from acvae_amd.diversity and shares no helper with it.

A clip has candidate strings h_0 .. h_{N-1}, N >= 2; tokens are str.split(); L_i = len(tokens of h_i); n-grams of orders
k = 1..4; c_i(g) = count of g in h_i.
  per clip:       words = sum_i L_i;  distinct_k = number of different order-k n-grams over all candidates;
                  div_k = distinct_k / (1e-6 + words)   (words in the denominator for every k, as div_utils.py:11-29)
  per candidate:  references = the clip's other candidates;  testlen = L_i;  guess_k = max(0, L_i - k + 1);
                  correct_k = sum over the different order-k g of h_i of min(c_i(g), max_{j != i} c_j(g));
                  reflen = the L_j, j != i, minimising (|L_j - L_i|, L_j)                       ("closest")
  corpus (diverse_mutil.py:31-52, Bleu(4)): per candidate index i, C_k, G_k, TL, RL summed over clips; p = 1; for k = 1..4:
                  p *= (C_k + 1e-15) / (G_k + 1e-9); bleu_k(i) = p ** (1 / k); ratio = (TL + 1e-15) / (RL + 1e-9); if
                  ratio < 1 every bleu_k(i) is multiplied by exp(1 - 1 / ratio);  mBLEU-k = mean_i bleu_k(i)
  global:         gDiv-1 = number of different words over every caption.

The bound of a comparison with acvae_amd.diversity.Diversity.result(): 1e-12 * max(1, |x|).  Both sides perform a dozen
correctly rounded float64 operations (and two library calls, pow and exp) on the same integers, and a mean over at most a
few hundred clips: a few 1e-16 relative is expected.
"""
import math

SMALL, TINY = 1e-9, 1e-15


def ngram_counts(sentence, n=4):
    words = sentence.split()
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


def clip_stats(candidates, n=4):
    """Candidate strings of one clip -> {"words", "distinct" [n], "cands": [{"testlen", "reflen", "guess" [n], "correct" [n],
    "clipped": some n-gram of the candidate occurs more often than in any reference}], "repeated" [n]: an order-k n-gram
    occurs more than once in the clip}."""
    assert len(candidates) >= 2
    counts = [ngram_counts(c, n) for c in candidates]
    lens = [len(c.split()) for c in candidates]
    everything = {}
    for c in counts:
        for g, v in c.items():
            everything[g] = everything.get(g, 0) + v
    distinct = [sum(1 for g in everything if len(g) == k) for k in range(1, n + 1)]
    repeated = [any(v > 1 for g, v in everything.items() if len(g) == k) for k in range(1, n + 1)]
    cands = []
    for i, mine in enumerate(counts):
        others = [c for j, c in enumerate(counts) if j != i]
        correct, clipped = [0] * n, False
        for g, v in mine.items():
            most = max(o.get(g, 0) for o in others)
            correct[len(g) - 1] += min(v, most)
            clipped = clipped or v > most
        reflen = min((abs(l - lens[i]), l) for j, l in enumerate(lens) if j != i)[1]
        cands.append({"testlen": lens[i], "reflen": reflen, "guess": [max(0, lens[i] - k + 1) for k in range(1, n + 1)],
                      "correct": correct, "clipped": clipped})
    return {"words": sum(lens), "distinct": distinct, "cands": cands, "repeated": repeated}


def record_of(stats):
    """A clip's statistics as the integers of the device record (include/acvae_hip.h): words, distinct[4], then per
    candidate testlen, reflen, correct[4]."""
    out = [stats["words"]] + list(stats["distinct"])
    for c in stats["cands"]:
        out += [c["testlen"], c["reflen"]] + list(c["correct"])
    return out


def corpus_bleu(cand_stats, n=4):
    """One candidate's statistics over the clips -> [bleu_1 .. bleu_n], option "closest"."""
    TL = sum(c["testlen"] for c in cand_stats)
    RL = sum(c["reflen"] for c in cand_stats)
    p, bleu = 1.0, []
    for k in range(n):
        C = sum(c["correct"][k] for c in cand_stats)
        G = sum(c["guess"][k] for c in cand_stats)
        p *= (float(C) + TINY) / (float(G) + SMALL)
        bleu.append(p ** (1.0 / (k + 1)))
    ratio = (float(TL) + TINY) / (float(RL) + SMALL)
    if ratio < 1.0:
        bleu = [b * math.exp(1.0 - 1.0 / ratio) for b in bleu]
    return bleu


def diversity(clips, n=4):
    """[[candidate strings of clip 0], [of clip 1], ...], every clip with the same N >= 2 -> the reference's numbers:
    {"Div1", "Div2", "gDiv1", "mBLeu_1" .. "mBLeu_4", "clips", "sample_n", "per_clip": {"div1", "div2"}, "stats"}."""
    N = len(clips[0])
    assert N >= 2 and all(len(c) == N for c in clips)
    stats = [clip_stats(c, n) for c in clips]
    div = [[s["distinct"][k] / (1e-6 + float(s["words"])) for s in stats] for k in range(2)]
    out = {"Div1": sum(div[0]) / len(clips), "Div2": sum(div[1]) / len(clips),
           "gDiv1": float(len({w for c in clips for h in c for w in h.split()}))}
    bleus = [corpus_bleu([s["cands"][i] for s in stats], n) for i in range(N)]
    for k in range(n):
        out[f"mBLeu_{k + 1}"] = sum(b[k] for b in bleus) / N
    out.update(clips=len(clips), sample_n=N, per_clip={"div1": div[0], "div2": div[1]}, stats=stats)
    return out


def sentence_of_ids(row, V, start_idx=1, end_idx=2):
    """A token row as the kernel is to read it: cut at the first <end>, <start> skipped wherever it stands, what stands
    behind the first <end> never looked at; a kept id outside [0, V) is the one word "<out>", every other id the word
    "w<id>"."""
    words = []
    for w in row:
        w = int(w)
        if w == end_idx:
            break
        if w == start_idx:
            continue
        words.append(f"w{w}" if 0 <= w < V else "<out>")
    return " ".join(words)


def clips_of_rows(seqs, sample_n, V, start_idx=1, end_idx=2):
    """Clip-major token rows [B * sample_n, T] -> [[candidate strings] per clip]."""
    rows = [sentence_of_ids(r, V, start_idx, end_idx) for r in seqs]
    return [rows[b:b + sample_n] for b in range(0, len(rows), sample_n)]


def clips_of_payload(payload):
    """A prediction document of evaluate()'s N-captions form -> [[the clip's token strings] per clip]."""
    return [[c["tokens"] for c in p["captions"]] for p in payload["predictions"]]


def bound(x):
    return 1e-12 * max(1.0, abs(x))
