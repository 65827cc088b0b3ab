"""Constrained decoding (include/acvae_hip.h, acvae_constrain_logits) in numpy: the definition as a twin of the kernel, and
a slow brute-force ban set to hold the twin against.

At step t a row's history is h = hist[:t], the words it has emitted so far (<start> is not part of it):
  theta  for every DISTINCT word w of h: x[w] <- x[w] / theta if x[w] > 0, else x[w] * theta, in fp32, once per word;
  n      n >= 1, t >= n - 1: for every i in [n - 1, t) with h[i-n+1 .. i) == h[t-n+1 .. t), ban h[i];
  m      ban end_idx at steps t < m;
  suppress  ban these ids at every step.
A ban writes -inf; the penalty comes first and a ban wins.  A history word outside [0, V) is skipped."""
import numpy as np


def ngram_bans(hist, t, n, V=None):
    """The words the n-gram rule bans at step t, straight from the definition's index form."""
    h = [int(w) for w in hist[:t]]
    out = set()
    if n >= 1 and t >= n - 1:
        for i in range(n - 1, t):
            if h[i - n + 1:i] == h[t - n + 1:t]:
                out.add(h[i])
    return {w for w in out if V is None or 0 <= w < V}


def ban_set(hist, t, end_idx, n, m, suppress, V):
    out = ngram_bans(hist, t, n, V)
    if t < m:
        out.add(int(end_idx))
    out.update(int(w) for w in suppress)
    return out


def constrain_row(x_f32, hist, t, end_idx, theta, n, m, suppress):
    """-> the constrained copy of the fp32 row x (the kernel's twin; every operation is an fp32 numpy operation)."""
    x = np.array(x_f32, dtype=np.float32, copy=True)
    V = x.size
    th = np.float32(theta)
    if th != np.float32(1.0):
        with np.errstate(all="ignore"):
            for w in sorted({int(w) for w in hist[:t] if 0 <= int(w) < V}):
                x[w] = x[w] / th if x[w] > 0 else x[w] * th
    for w in ban_set(hist, t, end_idx, n, m, suppress, V):
        x[w] = -np.inf
    return x


def banned_set(hist, t, n, V):
    """Brute force, by the rule's purpose: w is banned iff the caption h + [w] would hold its last n-gram twice - every
    n-gram of the extended caption is built and the last one looked up among the earlier ones."""
    h = [int(w) for w in hist[:t]]
    out = set()
    if n < 1:
        return out
    for w in range(V):
        ext = h + [w]
        grams = [tuple(ext[i:i + n]) for i in range(len(ext) - n + 1)]
        if grams and grams[-1] in grams[:-1]:
            out.add(w)
    return out


def repeats_ngram(words, n):
    """Does the word list hold an n-gram twice?"""
    grams = [tuple(words[i:i + n]) for i in range(len(words) - n + 1)]
    return len(grams) != len(set(grams))
