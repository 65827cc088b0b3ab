"""The resampler's definition as a float64 twin, the test inputs and the bound (tests only; the product keeps no CPU twin of
its kernel).  Written from the formula, independently of ``Resample.tables()``:

  rates orig -> new, g = gcd, U = new / g, D = orig / g, c = rolloff min(1, U / D), Z zero crossings;
  g(tau) = c sinc(c tau) I0(beta sqrt(1 - (c tau / Z)^2)) / I0(beta) for |c tau| < Z, else 0;
  y[m] = sum_n x[n] g((m D - n U) / U), x zero outside [0, L);  L_out = ceil(L U / D).

  * ``kernel_fn``: g at integer numerators ``m D - n U``;
  * ``twin64``: y and A[m] = sum_n |x[n]| |g(m D / U - n)| in float64, one phase of the output at a time;
  * ``twin_f32``: a float32 matmul evaluation over the product's compacted bank, which stands in for the kernel where there
    is no GPU.

Bound, from the project's ``chain_tol`` (tests/test_kernels_gpu.py): with K = 2 ceil(Z / c) + 2, the taps an output can
touch, every valid output satisfies |y - y_64| <= chain_tol(K) A[m].  No cell is left out; where every input in an output's
support is zero, A = 0 and the output must be exactly zero.
"""
import math

import numpy as np

from frontend_util import chain_tol, clip

BEST = dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492)
FAST = dict(zeros=16, rolloff=0.85, beta=8.555504641634386)


def ratio(orig, new):
    g = math.gcd(orig, new)
    return new // g, orig // g                                   # U, D


def kernel_fn(num, U, D, zeros, rolloff, beta):
    """g((num) / U) for an integer array ``num`` = m D - n U."""
    c = rolloff * min(1.0, U / D)
    u = c * np.asarray(num, dtype=np.int64).astype(np.float64) / U
    out = np.zeros(u.shape)
    ok = np.abs(u) < zeros
    uo = u[ok]
    out[ok] = c * np.sinc(uo) * np.i0(beta * np.sqrt(1.0 - (uo / zeros) ** 2)) / np.i0(beta)
    return out


def out_len(L, U, D):
    return -((-int(L) * U) // D)


def taps(U, D, zeros, rolloff):
    return 2 * int(math.ceil(zeros / (rolloff * min(1.0, U / D)))) + 2


def twin64(x, U, D, zeros, rolloff, beta):
    """-> (y [L_out], A [L_out]) in float64.  Phase i = m mod U at a time: m = j U + i reads x[j D + q_i - h + t] for
    t = 0 .. 2 h, q_i = floor(i D / U), h = ceil(Z / c) + 1 (the support is |m D / U - n| < Z / c)."""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    Lo = out_len(L, U, D)
    h = int(math.ceil(zeros / (rolloff * min(1.0, U / D)))) + 1
    J = -(-Lo // U)
    xp = np.zeros(h + (J + 1) * D + h + 1)
    xp[h:h + L] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * h + 1)
    ax = np.lib.stride_tricks.sliding_window_view(np.abs(xp), 2 * h + 1)
    y, A = np.zeros(J * U), np.zeros(J * U)
    t = np.arange(2 * h + 1, dtype=np.int64)
    for i in range(U):
        q = (i * D) // U
        g = kernel_fn(i * D - (q - h + t) * U, U, D, zeros, rolloff, beta)       # n - j D = q - h + t
        rows = slice(q, q + J * D, D)                                            # xp index of n = j D + q - h
        y[i::U] = win[rows] @ g
        A[i::U] = ax[rows] @ np.abs(g)
    return y[:Lo], A[:Lo]


def group(U):
    """Blocks the product groups into one for a small U (U' = s U >= 32)."""
    return 1 if U >= 32 else -(-32 // U)


def cases(BT):
    """name -> (orig, new, filter settings, [(L, silent or None)]).  Per rate pair a ragged batch: 1 sample, D - 1 samples
    (where that is >= 1), exactly BT D' (the workgroup's block tile edge) and (2 BT + 3) D' + 1 (more than two tiles, a
    multiple of nothing), D' = s D the kernel's block.  One batch has an all-zero stretch longer than the filter's support,
    at a clip's start and in a clip's middle."""
    out = {}
    for name, orig, new, kw in (("44100_32000", 44100, 32000, BEST), ("48000_32000", 48000, 32000, BEST),
                                ("32000_16000", 32000, 16000, BEST), ("22050_32000", 22050, 32000, BEST),
                                ("8000_16000", 8000, 16000, BEST), ("44100_16000", 44100, 16000, BEST),
                                ("44100_16000_fast", 44100, 16000, FAST)):
        U, D = ratio(orig, new)
        Dk = group(U) * D
        lens = [1] + ([D - 1] if D - 1 >= 1 else []) + [BT * Dk, (2 * BT + 3) * Dk + 1]
        out[name] = (orig, new, kw, [(L, None) for L in lens])
    U, D = ratio(44100, 32000)
    K = taps(U, D, BEST["zeros"], BEST["rolloff"])
    out["44100_32000_silence"] = (44100, 32000, BEST, [(9 * D + 5, (0, 3 * K)), (11 * D + 3, (2 * D + 7, 2 * D + 7 + 3 * K))])
    return out


_REF = {}


def reference(name, BT):
    """The case's inputs and float64 reference, computed once and shared: dict(orig, new, kw, U, D, waves fp32 [N, Lmax],
    lens, y [list of [L_out]], A [list of [L_out]], K)."""
    key = (name, BT)
    if key not in _REF:
        orig, new, kw, clips = cases(BT)[name]
        U, D = ratio(orig, new)
        lens = np.array([L for L, _ in clips], dtype=np.int64)
        waves = np.zeros((len(clips), int(lens.max())), dtype=np.float32)
        for i, (L, silent) in enumerate(clips):
            waves[i, :L] = clip(L, orig, 2000 + 13 * i + len(name), silent)
        ys, As = zip(*(twin64(waves[i, :L], U, D, **kw) for i, L in enumerate(lens)))
        for a in (waves, lens, *ys, *As):
            a.setflags(write=False)
        _REF[key] = dict(orig=orig, new=new, kw=kw, U=U, D=D, waves=waves, lens=lens, y=list(ys), A=list(As),
                         K=taps(U, D, kw["zeros"], kw["rolloff"]))
    return _REF[key]


def twin_f32(x, rs):
    """float32 matmul evaluation of one clip over the product's compacted bank (``rs`` a ``Resample``), tile by tile and
    K-step by K-step as the kernel walks it -> y fp32 [L_out]."""
    x = np.asarray(x, dtype=np.float32)
    bank, index = rs.kernel_tables()
    Uk, Dk, W = rs.kernel_up, rs.kernel_down, rs.half_width
    Lo = int(rs.out_len(len(x)))
    J = -(-Lo // Uk)
    span = int(index[:, 0].max()) + bank.shape[1] * 32
    xp = np.zeros(W + J * Dk + span, dtype=np.float32)
    xp[W:W + len(x)] = x
    y = np.zeros((J, bank.shape[0] * 32), dtype=np.float32)
    for t in range(bank.shape[0]):
        first, n = int(index[t, 0]), int(index[t, 1])
        X = np.lib.stride_tricks.sliding_window_view(xp, n * 32)[first:first + J * Dk:Dk]     # x[j D' + first + q - W]
        y[:, 32 * t:32 * t + 32] = X @ bank[t, :n].transpose(0, 2, 1).reshape(n * 32, 32)
    return y[:, :Uk].reshape(-1)[:Lo]


def check_case(ref, out):
    """The bound on one case; ``out`` [N, >= max L_out] (numpy fp32).  Prints and returns the worst |d| / (chain_tol(K) A)
    over all valid outputs after asserting it; outputs with A = 0 must be exactly zero."""
    tol = chain_tol(ref["K"])
    worst, cells, silent = 0.0, 0, 0
    for i, L in enumerate(ref["lens"]):
        y, A = ref["y"][i], ref["A"][i]
        Lo = out_len(L, ref["U"], ref["D"])
        assert len(y) == Lo
        got = np.asarray(out[i, :Lo], dtype=np.float64)
        assert np.isfinite(got).all(), f"clip {i}: outputs left unwritten or not finite"
        zero = A == 0.0
        assert not got[zero].any(), f"clip {i}: a non-zero output over all-zero input"
        if (~zero).any():
            worst = max(worst, float((np.abs(got - y)[~zero] / (tol * A[~zero])).max()))
        cells, silent = cells + Lo, silent + int(zero.sum())
    print("resample bound: worst %.4f x bound over %d outputs (%d with A = 0), K = %d" % (worst, cells, silent, ref["K"]))
    assert worst <= 1.0, f"worst {worst:.3f} x the bound"
    return worst, cells, silent
