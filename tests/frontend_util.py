"""The log-mel front end's definition as a float64 twin, the test inputs and the bounds (tests only; the product keeps no
CPU twin of its kernel).

  * ``power_ref``: the STFT through ``torch.stft`` (periodic Hann, center=True, reflect) in float64 - an independent witness;
  * ``mel_matrix``: the mel weights written from the formula (Slaney scale, Slaney norm), independently of ``LogMel.tables()``;
  * ``twin_f32``: a float32 matmul evaluation of the same DFT, which stands in for the kernel where there is no GPU.

Bounds, from the project's ``chain_tol`` (tests/test_kernels_gpu.py): with tau = chain_tol(n_fft) and Pbar the mean of the
reference power over a clip's valid frames and bins,
  spectrogram  |dP| <= 3 tau (P + Pbar)           (|d re| <= tau max(|re|, r), r^2 = Pbar / 2, dP <= 2(|re||d re| + |im||d im|))
  log-mel      rho = 3 tau (1 + Pbar sum_f W[f, m] / M), M the reference mel power;
               M >= amin and rho <= 0.1:  |d dB| <= 4.343 rho + 1e-5 |ref dB| + 1e-5
               M <  amin:                 within 1e-4 of 10 log10(amin) - offset
               rho > 0.1:                 left out, and counted against a cap (0 without silence, 2 % with).
"""
import math

import numpy as np
import torch


def chain_tol(K):
    """tests/test_kernels_gpu.py:43-46."""
    return max(1e-5, 6 * 2.0 ** -24 * math.sqrt(K))


def mel_of(f):
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def hz_of(m):
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def mel_matrix(sr, n_fft, n_mels, fmin, fmax):
    lo, hi = mel_of(fmin), mel_of(fmax)
    p = [hz_of(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    W = np.zeros((n_fft // 2 + 1, n_mels))
    for f in range(n_fft // 2 + 1):
        b = f * sr / n_fft
        for m in range(n_mels):
            v = min((b - p[m]) / (p[m + 1] - p[m]), (p[m + 2] - b) / (p[m + 2] - p[m + 1]))
            W[f, m] = max(0.0, v) * 2.0 / (p[m + 2] - p[m])
    return W


def basis_formula(n_fft):
    """[2, n, n/2 + 1] float64: w[k] cos(2 pi k f / n), -w[k] sin(2 pi k f / n), angle reduced modulo one turn."""
    k = np.arange(n_fft, dtype=np.int64)[:, None]
    f = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * f) % n_fft).astype(np.float64) / n_fft
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft))[:, None]
    return np.stack([w * np.cos(ang), -(w * np.sin(ang))])


def power_ref(x, n_fft, hop):
    """float64 power spectrogram [T, n/2 + 1] of one clip (1-D float array)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    s = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                   center=True, pad_mode="reflect", return_complex=True)
    return (s.real ** 2 + s.imag ** 2).T.contiguous().numpy()


def db_ref(P, W, amin, ref):
    M = P @ W
    return 10.0 * np.log10(np.maximum(M, amin)) - 10.0 * math.log10(max(amin, ref)), M


def twin_f32(x, n_fft, hop, W, amin, ref):
    """float32 matmul evaluation: (power [T, nb], dB [T, n_mels]), both float32."""
    x = np.asarray(x, dtype=np.float32)
    T = 1 + len(x) // hop
    xp = np.pad(x, n_fft // 2, mode="reflect")
    frames = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]).astype(np.float32)
    b = basis_formula(n_fft).astype(np.float32)
    re, im = frames @ b[0], frames @ b[1]
    P = (re * re + im * im).astype(np.float32)
    M = P @ W.astype(np.float32)
    off = np.float32(10.0 * math.log10(max(amin, ref)))
    return P, (np.float32(10.0) * np.log10(np.maximum(M, np.float32(amin))) - off).astype(np.float32)


def spec_ratio(got, P, n_fft):
    """worst |dP| / (3 tau (P + Pbar)) over one clip's valid frames."""
    tol = 3.0 * chain_tol(n_fft) * (P + P.mean())
    return float((np.abs(np.asarray(got, dtype=np.float64) - P) / tol).max())


def db_check(got, P, W, n_fft, amin, ref):
    """-> (worst ratio over the checked cells, worst |d| over the cells below amin, cells left out, cells) for one clip.
    The bound's "1e-5 |ref|" term is read as 1e-5 times the magnitude of the reference dB value of the cell (``want``
    below: the rounding of a float32 result of that size), not of the ``ref`` parameter of the dB offset.  This is a reading
    of the bound as it was stated; with ref = 1.0, as every case here has it, the other reading would add a constant 1e-5
    where this one adds at most 1e-3 (|dB| <= 100 with amin = 1e-10)."""
    got = np.asarray(got, dtype=np.float64)
    want, M = db_ref(P, W, amin, ref)
    rho = 3.0 * chain_tol(n_fft) * (1.0 + P.mean() * W.sum(axis=0)[None, :] / np.maximum(M, 1e-300))
    floor = M < amin
    checked = ~floor & (rho <= 0.1)
    left_out = ~floor & (rho > 0.1)
    worst = 0.0
    if checked.any():
        tol = 4.343 * rho + 1e-5 * np.abs(want) + 1e-5
        worst = float((np.abs(got - want) / tol)[checked].max())
    worst_floor = float(np.abs(got - want)[floor].max()) if floor.any() else 0.0
    return worst, worst_floor, int(left_out.sum()), got.size


def clip(L, sr, seed, silent=None):
    """0.1 randn + 0.05 sin(2 pi 440 t) + 0.05 sin(2 pi 3001.5 t), rounded to fp32; ``silent`` = (start, end) exact zeros."""
    g = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64) / sr
    x = 0.1 * g.standard_normal(L) + 0.05 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * np.sin(2 * np.pi * 3001.5 * t)
    x = x.astype(np.float32)
    if silent is not None:
        x[silent[0]:silent[1]] = 0.0
    return x


def cases(FT):
    """name -> (LogMel keyword arguments, [(L, silent or None)], cap on the share of cells left out).  The smallest shapes
    that can still go wrong: the minimum length (T = 2), a length that is no multiple of anything, T exactly on the frame
    tile's edge, more than two tiles; a silent stretch at a clip's start and in a clip's middle; a hop that is no multiple
    of 4 and does not divide n_fft with n_mels no multiple of 32 and fmin = 0; hop = n_fft = 2048."""
    out = {}
    for name, kw in (("panns_32k", dict(sample_rate=32000, n_fft=1024, hop_length=320, n_mels=64, fmin=50.0, fmax=14000.0)),
                     ("panns_16k", dict(sample_rate=16000, n_fft=512, hop_length=160, n_mels=64, fmin=50.0, fmax=8000.0))):
        n, h = kw["n_fft"], kw["hop_length"]
        out[name + "_ragged"] = (kw, [(n // 2 + 1, None), (37 * h + 17, None), ((FT - 1) * h, None),
                                      ((2 * FT + 3) * h + 1, None)], 0.0)
        out[name + "_silence"] = (kw, [(40 * h + 5, (0, 9 * h)), (31 * h + 3, (12 * h + 7, 19 * h))], 0.02)
    out["n256_hop100"] = (dict(sample_rate=8000, n_fft=256, hop_length=100, n_mels=40, fmin=0.0),
                          [(129, None), (53 * 100 + 37, None), (70 * 100, None)], 0.0)
    out["n2048_hop2048"] = (dict(sample_rate=32000, n_fft=2048, hop_length=2048, n_mels=64, fmin=50.0),
                            [(2 * 2048 + 777, None)], 0.0)
    return out


_REF = {}


def reference(name, FT):
    """The case's inputs and float64 reference, computed once and shared: dict(kw, waves fp32 [N, Lmax], lens, W, P [list of
    [T_n, nb]], cap)."""
    key = (name, FT)
    if key not in _REF:
        kw, clips, cap = cases(FT)[name]
        sr = kw["sample_rate"]
        lens = np.array([L for L, _ in clips], dtype=np.int64)
        waves = np.zeros((len(clips), int(lens.max())), dtype=np.float32)
        for i, (L, silent) in enumerate(clips):
            waves[i, :L] = clip(L, sr, 1000 + 17 * i + len(name), silent)
        fmax = kw.get("fmax") or sr / 2.0
        W = mel_matrix(sr, kw["n_fft"], kw["n_mels"], kw["fmin"], fmax)
        P = [power_ref(waves[i, :L], kw["n_fft"], kw["hop_length"]) for i, L in enumerate(lens)]
        for a in (waves, lens, W, *P):
            a.setflags(write=False)
        _REF[key] = dict(kw=kw, waves=waves, lens=lens, W=W, P=P, cap=cap)
    return _REF[key]


def check_case(ref, spec, feats, amin=1e-10, refv=1.0):
    """Both bounds and the cap on one case; ``spec`` [N, T, nb] or None, ``feats`` [N, T, n_mels] (numpy).  Returns the figures
    (worst spectrogram ratio, worst dB ratio, worst floor error, left out, cells) after asserting them."""
    kw = ref["kw"]
    n, h = kw["n_fft"], kw["hop_length"]
    ws = wd = wf = 0.0
    out_cells = cells = 0
    for i, L in enumerate(ref["lens"]):
        Tn = 1 + int(L) // h
        P = ref["P"][i]
        assert P.shape[0] == Tn
        if spec is not None:
            ws = max(ws, spec_ratio(spec[i, :Tn], P, n))
        a, b, c, d = db_check(feats[i, :Tn], P, ref["W"], n, amin, refv)
        wd, wf, out_cells, cells = max(wd, a), max(wf, b), out_cells + c, cells + d
    figures = (ws, wd, wf, out_cells, cells)
    print("frontend bounds: spec %.4f x bound, dB %.4f x bound, floor |d| %.2e, left out %d of %d" % figures)
    assert ws <= 1.0, f"spectrogram: worst {ws:.3f} x the bound"
    assert wd <= 1.0, f"log-mel: worst {wd:.3f} x the bound"
    assert wf <= 1e-4, f"log-mel below amin: {wf:.3e} from the floor"
    assert out_cells <= ref["cap"] * cells, f"{out_cells} of {cells} cells left out, cap {ref['cap']:.0%}"
    return figures
