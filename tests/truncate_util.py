"""The definition of top-k / nucleus (top-p) truncation in float64 (include/acvae_hip.h, acvae_sample_next_word_truncated),
and the interval of kept counts an fp32 kernel may report for a row.

Per row of V logits x: the words are ordered by x descending, equal values by lower index (``topk_ref``'s order in
tests/test_decode_kernels_gpu.py); pi is the distribution the method samples from, softmax(x / temp) for MULTINOMIAL and
softmax(x) for GUMBEL (temp divides every Gumbel score alike); ``top_k`` keeps the first min(k, V) words of the order,
``top_p`` keeps the word at rank r iff the mass of the ranks before it is < p (rank 0 always), both keep the shorter
prefix."""
import numpy as np

GUMBEL, MULTINOMIAL = 1, 2
EPS32 = 2.0 ** -24                       # unit roundoff of fp32
THREADS = 256                            # the kernel's workgroup


def stable_order(x):
    """Indices of x by value descending, ties to the lower index: a stable sort on (-x, index)."""
    x = np.asarray(x)
    return np.lexsort((np.arange(x.size), -x.astype(np.float64)))


def mass_tol(V):
    """Bound on |kernel's (mass before a rank) / Z  -  the exact ratio| for a row of V words, derived from the sums
    sample_trunc_rows_kernel performs (csrc/losses.hip).

    Numerator and denominator are sums of the same non-negative terms e_c = expf((x_c - m) / temp) - a subset and all of
    them - added in one fixed order: a thread adds its ceil(V / 256) words in sequence, six butterfly levels add the 64
    lanes of a wavefront, the four wavefront partials are added in sequence (block_sum's order).  With N the exact
    numerator, Z the exact denominator and pi_c = e_c / Z, each computed sum S~ of exact value S satisfies
    |S~ - S| <= S * (A + X) * 2^-24 + G_S, where
      * A = ceil(V / 256) + 8: the additions - every partial sum is of non-negative terms, so each level a term passes
        through adds at most 2^-24 relative (lse_bound's count);
      * X = 4: expf, within 2 ulp of its argument's exponential (lse_bound's count);
      * G_S = 2 * 2^-24 * sum_{c in S} e_c a_c, a_c = (m - x_c) / temp: the argument - x_c - m and the division by temp
        are rounded, each within 2^-24 relative, which moves e_c by a_c * 2^-24 relative each.
    The ratio's absolute error is then at most (N / Z) * 2 (A + X) * 2^-24 + (G_N + (N / Z) G_Z) / Z
    <= 2 (12 + ceil(V / 256)) * 2^-24 + 4 * 2^-24 * sum_c pi_c a_c over the whole row, and sum_c pi_c a_c =
    H(pi) - log(sum_c e_c) <= H(pi) <= log V because the largest term is 1.  The kernel compares the numerator with
    fl(p * Z), one more rounding.  In all (2 * (12 + ceil(V / 256) + 2 log V) + 1) * 2^-24, doubled for headroom as
    lse_bound is: 1.2e-5 at V = 5000.  (Without the argument's term, i.e. for a sum of exactly known terms, this is
    4 * (12 + ceil(V / 256)) * 2^-24 = 7.6e-6.)"""
    return 2.0 * (2.0 * (12 + -(-V // THREADS) + 2.0 * np.log(max(V, 2))) + 1.0) * EPS32


def distribution(x, method, temp):
    """pi in float64 from the fp32 logits and the fp32 temperature the kernel is given."""
    te = 1.0 if method == GUMBEL else float(np.float32(temp))
    a = np.asarray(x).astype(np.float64) / te
    e = np.exp(a - a.max())
    return e / e.sum()


def mass_before(x, method, temp, order=None):
    """before[r] = mass of the ranks in front of rank r, float64 (before[0] = 0); -> (order, before)."""
    order = stable_order(x) if order is None else order
    pi = distribution(x, method, temp)[order]
    before = np.concatenate(([0.0], np.cumsum(pi)[:-1]))
    return order, before


def kept_count(before, k, q):
    """Size of the kept prefix when the nucleus cut is taken at q (q >= 1: no nucleus cut) and top-k at k (0: off)."""
    V = before.size
    n = V if q >= 1.0 else max(1, int(np.searchsorted(before, q, side="left")))     # ranks with before < q; rank 0 always
    return min(n, k) if k > 0 else n


def admissible(x, method, temp, k, p, tol=None, order=None):
    """-> (lo, hi, order): the kept counts an fp32 kernel may report for the row: the count with the nucleus cut taken at
    p - tol and at p + tol (tol = mass_tol(V) by default; p as the fp32 number the kernel is given; exactly 1.0 = off:
    no tolerance applies), both intersected with top-k."""
    x = np.asarray(x)
    order, before = mass_before(x, method, temp, order)
    p = float(np.float32(p))
    if p >= 1.0:
        n = kept_count(before, k, 1.0)
        return n, n, order
    tol = mass_tol(x.size) if tol is None else tol
    return kept_count(before, k, p - tol), kept_count(before, k, min(p + tol, np.nextafter(1.0, 0.0))), order


def brute_force_kept(x, method, temp, k, p):
    """The definition as a loop over the sorted words (plain Python floats): exact where the masses are dyadic."""
    x = [float(v) for v in np.asarray(x)]
    te = 1.0 if method == GUMBEL else float(np.float32(temp))
    words = sorted(range(len(x)), key=lambda i: (-x[i], i))
    m = max(x)
    e = [float(np.exp((v - m) / te)) for v in x]
    z = sum(e[i] for i in words)
    kept, before = [], 0.0
    for r, i in enumerate(words):
        if k > 0 and r >= k:
            break
        if r > 0 and p < 1.0 and not before / z < p:
            break
        kept.append(i)
        before += e[i]
    return kept
