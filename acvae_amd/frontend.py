"""Log-mel front end: waveforms -> the ``[T, n_mels]`` features every encoder of the package starts from.

The three encoders (``Cnn10``, ``Cnn14_16k``, ``ResNet38``) are PANNs networks, and PANNs checkpoints are only meaningful
behind the PANNs front end (``models/encoder.py:877-885``: torchlibrosa's ``Spectrogram`` then ``LogmelFilterBank``).  The
definition, restated from torchlibrosa / librosa, for one clip ``x`` of ``L`` samples, ``n = n_fft``, ``h = hop_length``:

  * reflect-pad ``n/2`` samples on both sides of the clip's own length (``i < 0 -> -i``, ``i >= L -> 2(L-1) - i``; needs
    ``L >= n/2 + 1``); ``T = 1 + L // h`` frames, frame ``t`` = padded samples ``t*h .. t*h + n - 1``;
  * periodic Hann window ``w[k] = 0.5 - 0.5 cos(2 pi k / n)``; power ``P[t, f] = re^2 + im^2`` of the windowed DFT,
    ``f = 0 .. n/2``;
  * mel weights ``W[n/2 + 1, n_mels]`` with librosa's defaults (Slaney scale, Slaney norm);
  * ``out[t, m] = 10 log10(max(sum_f P[t, f] W[f, m], amin)) - 10 log10(max(amin, ref))``.

The split is the package's usual one (``acvae_amd.augment``): the tables are made on the host, in float64, rounded once to
fp32 and uploaded once per device; the arithmetic is one HIP kernel (``acvae_logmel_fwd``, include/acvae_hip.h) on the
current stream.  There is no CPU code path, and no gradient flows through the front end.

Audio at another rate (Clotho is 44.1 kHz, AudioCaps and field recordings 44.1 or 48 kHz) is resampled on the device in
front of it: ``Resample`` (``acvae_resample_fwd``), and ``Resampled(resample, logmel)`` / ``LogMel.at_input_rate(rate)``
for the pair.  The definition, for rates ``orig -> new`` with ``g = gcd``, ``U = new / g``, ``D = orig / g``, ``Z`` zero
crossings and ``c = rolloff * min(1, U / D)``:

  * kernel function, ``tau`` in input samples: ``g(tau) = c sinc(c tau) I0(beta sqrt(1 - (c tau / Z)^2)) / I0(beta)`` for
    ``|c tau| < Z`` and 0 otherwise, ``sinc(u) = sin(pi u) / (pi u)``;
  * output ``y[m] = sum_n x[n] g(m D / U - n)``, the argument formed exactly as ``(m D - n U) / U`` from integers, ``x`` zero
    outside ``[0, L)``; ``L_out = ceil(L U / D)``; the columns of an output row behind ``L_out`` are zeros;
  * ``kaiser_best``: ``Z = 64, rolloff = 0.9475937167399596, beta = 14.769656459379492``; ``kaiser_fast``: ``Z = 16,
    rolloff = 0.85, beta = 8.555504641634386`` (the settings librosa / resampy publish under these names).

This is the closed form: resampy's interpolated table and soxr are not reproduced bit for bit.  Not supported: clips of
different rates in one batch, a gradient through the resampler, and the resampler fused into the log-mel kernel's gather.

Training-time augmentation of such batches: ``Augmented(frontend, augment)`` / ``fe.augmented(augment)``, a front end for
the training calls that draws the config's ``augments`` per batch and applies them on the device
(``acvae_amd.augment.apply_plans``).  ``frontend=`` together with ``augment=`` stays refused.
"""
import math
import wave as _wave

import numpy as np
import torch

from . import _lib

FRAME_TILE = int(_lib._defs["ACVAE_LOGMEL_FRAME_TILE"])
N_FFTS = (256, 512, 1024, 2048)
_CHUNK, _BK = 64, 32                     # frequencies per chunk and k per K-step of the kernel's basis layout
BLOCK_TILE = int(_lib._defs["ACVAE_RESAMPLE_BLOCK_TILE"])
MAX_RATIO = int(_lib._defs["ACVAE_RESAMPLE_MAX_RATIO"])
MAX_TAPS = int(_lib._defs["ACVAE_RESAMPLE_MAX_TAPS"])
_PT = 32                                 # phases per tile of the resampler's filter bank


def hz_to_mel(f):
    """Slaney scale: 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 from 1000 Hz up."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-300) / 1000.0) / math.log(6.4))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(math.log(6.4) / 27.0 * (m - 15.0)))


class LogMel:
    """``LogMel(sample_rate, n_fft, hop_length, n_mels=64, fmin=50.0, fmax=None, ref=1.0, amin=1e-10, top_db=None)``;
    ``LogMel.panns_32k()`` / ``LogMel.panns_16k()`` are the two PANNs settings.  ``fmax=None`` is ``sample_rate / 2``.
    Limits (the kernel's): ``n_fft`` in {256, 512, 1024, 2048}, ``1 <= hop_length <= n_fft``, ``n_mels`` a multiple of 4 in
    [4, 128], every clip at least ``n_fft/2 + 1`` samples.  ``top_db`` other than None raises ValueError (PANNs uses None;
    anything else needs the batch's global maximum)."""

    def __init__(self, sample_rate, n_fft, hop_length, n_mels=64, fmin=50.0, fmax=None, ref=1.0, amin=1e-10, top_db=None):
        if top_db is not None:
            raise ValueError("top_db is not supported (PANNs uses None; clipping needs the global maximum)")
        if n_fft not in N_FFTS:
            raise ValueError(f"n_fft={n_fft}: the kernel takes {N_FFTS}")
        if not 1 <= int(hop_length) <= n_fft or int(hop_length) != hop_length:
            raise ValueError(f"hop_length={hop_length}: must be an integer in [1, n_fft]")
        if int(n_mels) != n_mels or n_mels % 4 != 0 or not 4 <= n_mels <= 128:
            raise ValueError(f"n_mels={n_mels}: the kernel takes multiples of 4 in [4, 128]")
        fmax = sample_rate / 2.0 if fmax is None else float(fmax)
        if sample_rate <= 0 or not 0 <= fmin < fmax <= sample_rate / 2.0:
            raise ValueError(f"need 0 <= fmin < fmax <= sample_rate / 2, got fmin={fmin}, fmax={fmax}, sample_rate={sample_rate}")
        if not (amin > 0 and math.isfinite(amin)) or not math.isfinite(ref):
            raise ValueError(f"need a finite amin > 0 and a finite ref, got amin={amin}, ref={ref}")
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = int(sample_rate), int(n_fft), int(hop_length), int(n_mels)
        self.fmin, self.fmax, self.ref, self.amin = float(fmin), fmax, float(ref), float(amin)
        self.n_bins = self.n_fft // 2 + 1
        self.db_offset = 10.0 * math.log10(max(self.amin, self.ref))
        self._device_tables = {}

    @classmethod
    def panns_32k(cls):
        return cls(32000, 1024, 320, n_mels=64, fmin=50.0, fmax=14000.0)

    @classmethod
    def panns_16k(cls):
        """The ``Cnn14_16k`` family."""
        return cls(16000, 512, 160, n_mels=64, fmin=50.0, fmax=8000.0)

    def at_input_rate(self, rate, **resample_args):
        """The front end for audio at ``rate``: ``self`` at the front end's own rate, otherwise ``Resampled(Resample(rate,
        sample_rate, **resample_args), self)`` (``kaiser_best`` unless told otherwise)."""
        if rate == self.sample_rate:
            return self
        return Resampled(Resample(rate, self.sample_rate, **resample_args), self)

    def augmented(self, augment):
        """``Augmented(self, augment)``: this front end with the training-time augmentation behind it."""
        return Augmented(self, augment)

    def n_frames(self, L):
        """Frames of a clip (or an array of clips) of ``L`` samples: ``1 + L // hop_length``."""
        return 1 + np.asarray(L, dtype=np.int64) // self.hop_length

    def to_float(self, wave):
        """int16 PCM -> the fp32 samples the kernel's int16 route sees (``/ 32768``, exact); fp32 passes through."""
        wave = torch.as_tensor(wave)
        return wave.to(torch.float32) / 32768.0 if wave.dtype == torch.int16 else wave

    # ------------------------------------------------------------------ tables (the only definitions in the product)
    def tables(self):
        """Host float64 ``(basis [2, n_fft, n_bins], melw [n_bins, n_mels])``: ``basis[0, k, f] = w[k] cos(2 pi k f / n)``
        and ``basis[1, k, f] = -w[k] sin(2 pi k f / n)`` (the angle reduced as ``2 pi ((k f) mod n) / n``, so every entry is
        correctly rounded float64), and the mel weights."""
        n = self.n_fft
        k = np.arange(n, dtype=np.int64)[:, None]
        f = np.arange(self.n_bins, dtype=np.int64)[None, :]
        ang = 2.0 * np.pi * ((k * f) % n).astype(np.float64) / n
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)
        basis = np.stack([w[:, None] * np.cos(ang), -(w[:, None] * np.sin(ang))])
        pts = mel_to_hz(np.linspace(hz_to_mel(self.fmin), hz_to_mel(self.fmax), self.n_mels + 2))
        bins = np.arange(self.n_bins, dtype=np.float64) * self.sample_rate / n
        lower = (bins[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None, :]
        upper = (pts[None, 2:] - bins[:, None]) / (pts[2:] - pts[1:-1])[None, :]
        melw = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[None, :]
        return basis, melw

    def kernel_tables(self):
        """The fp32 tables in the kernel's layout (include/acvae_hip.h): basis ``[n/128 chunks][n/32 K-steps][128][32]`` -
        column c < 64 of chunk q the real part of bin 64 q + c, column 64 + c its imaginary part, column 64 of chunk 0 the real
        part of the Nyquist bin - and melw ``[n_bins, n_mels]``."""
        basis, melw = self.tables()
        n, half = self.n_fft, self.n_fft // 2
        cols = np.concatenate([basis[0, :, :half].reshape(n, half // _CHUNK, 1, _CHUNK),
                               basis[1, :, :half].reshape(n, half // _CHUNK, 1, _CHUNK)], axis=2)      # [k, q, re|im, c]
        cols[:, 0, 1, 0] = basis[0, :, half]
        packed = cols.reshape(n // _BK, _BK, half // _CHUNK, 2 * _CHUNK).transpose(2, 0, 3, 1)         # [q, ks, col, kk]
        return np.ascontiguousarray(packed, dtype=np.float32).reshape(-1), np.ascontiguousarray(melw, dtype=np.float32)

    def _tables_on(self, dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        t = self._device_tables.get(key)
        if t is None:
            basis, melw = self.kernel_tables()
            t = self._device_tables[key] = (torch.from_numpy(basis).to(dev), torch.from_numpy(melw).to(dev))
        return t

    # ------------------------------------------------------------------ the device half
    def check(self, waves, wave_lens):
        """Validate a batch on the host (ValueError, before any launch) -> (waves as a tensor, lens int64 [N])."""
        if isinstance(waves, np.ndarray):
            waves = torch.from_numpy(waves)
        if not isinstance(waves, torch.Tensor) or waves.dim() != 2:
            raise ValueError("waves must be a [N, Lmax] tensor")
        if waves.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"waves must be float32 or int16 PCM, got {waves.dtype}")
        lens = np.asarray(wave_lens).reshape(-1)
        if not np.issubdtype(lens.dtype, np.integer):
            if not np.all(lens == np.floor(lens)):
                raise ValueError("wave_lens must be whole numbers of samples")
        lens = lens.astype(np.int64)
        N, Lmax = waves.shape
        if N == 0 or len(lens) != N:
            raise ValueError(f"{len(lens)} lengths for a batch of {N} clips")
        if lens.min() < self.n_bins:
            raise ValueError(f"clip {int(lens.argmin())}: {int(lens.min())} samples, reflect padding needs at least "
                             f"n_fft/2 + 1 = {self.n_bins}")
        if lens.max() > Lmax:
            raise ValueError(f"clip {int(lens.argmax())}: length {int(lens.max())} beyond the batch's {Lmax} samples")
        if Lmax > 1 << 30:
            raise ValueError(f"clips of {Lmax} samples: the kernel indexes a clip with 32-bit integers")
        T = 1 + int(lens.max()) // self.hop_length
        if N * T * self.n_bins >= 1 << 31:
            raise ValueError(f"batch of {N} x {T} frames x {self.n_bins} bins: the kernel indexes the batch with 32-bit integers")
        return waves, lens

    def __call__(self, waves, wave_lens, spectrogram=False, device=None):
        """``waves`` [N, Lmax] fp32 or int16 PCM, on the device or on the host (then uploaded, to ``device`` or the current
        GPU); ``wave_lens`` the N sample counts (host).  -> ``(feats f32 [N, Tmax, n_mels] on the device, feat_lens np.int64
        [N])`` with ``Tmax = 1 + max(wave_lens) // hop_length``; rows behind a clip's own frames are zeros.
        ``spectrogram=True``: ``(feats, feat_lens, power f32 [N, Tmax, n_bins])``."""
        waves, lens = self.check(waves, wave_lens)
        if not waves.is_cuda:
            if device is None:
                if not torch.cuda.is_available():
                    raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
                device = torch.device("cuda", torch.cuda.current_device())
            waves = _lib.h2d(waves, device)
        waves = waves.contiguous()
        dev = waves.device
        N, Lmax = waves.shape
        T = 1 + int(lens.max()) // self.hop_length
        basis, melw = self._tables_on(dev)
        lens_d = _lib.h2d(lens.astype(np.int32), dev)
        with torch.no_grad():
            feats = torch.empty(N, T, self.n_mels, device=dev)
            spec = torch.empty(N, T, self.n_bins, device=dev) if spectrogram else None
        _lib.call("acvae_logmel_fwd", waves, int(waves.dtype == torch.int16), Lmax, lens_d, basis, melw, feats, spec, N, T,
                  self.n_fft, self.hop_length, self.n_mels, self.amin, self.db_offset, _lib.current_stream())
        feat_lens = self.n_frames(lens)
        return (feats, feat_lens, spec) if spectrogram else (feats, feat_lens)


def _batch(waves, wave_lens):
    """The checks every front end makes of a batch's form -> (waves as a tensor, lens int64 [N])."""
    if isinstance(waves, np.ndarray):
        waves = torch.from_numpy(waves)
    if not isinstance(waves, torch.Tensor) or waves.dim() != 2:
        raise ValueError("waves must be a [N, Lmax] tensor")
    if waves.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"waves must be float32 or int16 PCM, got {waves.dtype}")
    lens = np.asarray(wave_lens).reshape(-1)
    if not np.issubdtype(lens.dtype, np.integer):
        if not np.all(lens == np.floor(lens)):
            raise ValueError("wave_lens must be whole numbers of samples")
    lens = lens.astype(np.int64)
    N, Lmax = waves.shape
    if N == 0 or len(lens) != N:
        raise ValueError(f"{len(lens)} lengths for a batch of {N} clips")
    if lens.max() > Lmax:
        raise ValueError(f"clip {int(lens.argmax())}: length {int(lens.max())} beyond the batch's {Lmax} samples")
    if Lmax > 1 << 30:
        raise ValueError(f"clips of {Lmax} samples: the kernel indexes a clip with 32-bit integers")
    return waves, lens


class Resample:
    """``Resample(orig_rate, new_rate, zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492)``: band-limited
    sample-rate conversion by the module docstring's definition; ``Resample.kaiser_best(o, n)`` (the defaults) and
    ``Resample.kaiser_fast(o, n)`` are the two published settings.  Limits (the kernel's): after the grouping of blocks for a
    small ``U`` (``kernel_up = s U >= 32``, ``kernel_down = s D``) both at most 1024, at most 2048 taps per output, and
    ``orig_rate != new_rate``."""
    BEST = dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492)
    FAST = dict(zeros=16, rolloff=0.85, beta=8.555504641634386)

    def __init__(self, orig_rate, new_rate, zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492):
        for name, r in (("orig_rate", orig_rate), ("new_rate", new_rate)):
            if isinstance(r, bool) or int(r) != r or r < 1:
                raise ValueError(f"{name}={r}: rates are positive whole numbers of Hz")
        if int(orig_rate) == int(new_rate):
            raise ValueError(f"orig_rate = new_rate = {int(new_rate)}: nothing to resample")
        if isinstance(zeros, bool) or int(zeros) != zeros or zeros < 1:
            raise ValueError(f"zeros={zeros}: must be a whole number >= 1")
        if not 0.0 < rolloff <= 1.0:
            raise ValueError(f"rolloff={rolloff}: must lie in (0, 1]")
        if not (beta >= 0.0 and math.isfinite(beta)):
            raise ValueError(f"beta={beta}: must be finite and >= 0")
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.zeros, self.rolloff, self.beta = int(zeros), float(rolloff), float(beta)
        g = math.gcd(self.orig_rate, self.new_rate)
        self.up, self.down = self.new_rate // g, self.orig_rate // g
        self.cutoff = self.rolloff * min(1.0, self.up / self.down)                       # c
        self.half_width = int(math.ceil(self.zeros / self.cutoff)) + 1                   # W
        self.group = 1 if self.up >= _PT else -(-_PT // self.up)                         # s: blocks per kernel block
        self.kernel_up, self.kernel_down = self.group * self.up, self.group * self.down  # U', D'
        if max(self.kernel_up, self.kernel_down) > MAX_RATIO:
            raise ValueError(f"{self.orig_rate} -> {self.new_rate} Hz is {self.down} -> {self.up} in lowest terms: the kernel "
                             f"takes ratios up to {MAX_RATIO}")
        if 2 * self.half_width > MAX_TAPS:
            raise ValueError(f"{2 * self.half_width} taps per output (zeros / (rolloff min(1, U / D)) = "
                             f"{self.zeros / self.cutoff:.1f}): the kernel takes up to {MAX_TAPS}")
        self.n_rows = 2 * self.half_width + self.kernel_down                             # rows k of H
        self._device_tables = {}
        self._kernel_tables = None

    @classmethod
    def kaiser_best(cls, orig_rate, new_rate):
        return cls(orig_rate, new_rate, **cls.BEST)

    @classmethod
    def kaiser_fast(cls, orig_rate, new_rate):
        return cls(orig_rate, new_rate, **cls.FAST)

    def out_len(self, L):
        """Output samples of a clip (or an array of clips) of ``L`` samples: ``ceil(L U / D)`` in exact integers."""
        return (np.asarray(L, dtype=np.int64) * self.up + self.down - 1) // self.down

    # ------------------------------------------------------------------ tables (the only definition in the product)
    def tables(self):
        """Host float64 ``H [2 W + D', U']``: ``H[k, i] = g(i D' / U' - (k - W))``, the kernel's view (block ``j``, phase
        ``i < U'``: ``y[j U' + i] = sum_k x[j D' + k - W] H[k, i]``).  The argument of every entry is the integer
        ``i D' - (k - W) U'`` with the common factor ``s`` taken out, over ``U``."""
        i = np.arange(self.kernel_up, dtype=np.int64)[None, :]
        k = np.arange(self.n_rows, dtype=np.int64)[:, None] - self.half_width
        num = (i * self.kernel_down - k * self.kernel_up) // self.group                  # exact: both terms carry s
        u = self.cutoff * num.astype(np.float64) / self.up                               # c tau
        inside = np.abs(u) < self.zeros
        r = np.where(inside, u / self.zeros, 0.0)
        win = np.i0(self.beta * np.sqrt(1.0 - r * r)) / np.i0(self.beta)
        return np.where(inside, self.cutoff * np.sinc(u) * win, 0.0)

    def kernel_tables(self):
        """The fp32 table in the kernel's layout (include/acvae_hip.h) and its index: ``bank [phase tiles][K-steps][32 phases]
        [32 k]``, entry ``(t, s, p, q) = H[first_k(t) + 32 s + q, 32 t + p]`` with zeros for phases ``>= U'``, rows outside
        ``H`` and K-steps behind the tile's own; ``index`` int32 ``[phase tiles, 2]``: ``first_k``, the first row of ``H`` with
        a non-zero tap in the tile, and the tile's number of K-steps (enough for its last such row).  Every tile has the
        K-steps of the widest one (``bank.shape[1]``, the kernel's ``ksteps``)."""
        if self._kernel_tables is None:
            H = self.tables()
            nt = -(-self.kernel_up // _PT)
            Hp = np.zeros((self.n_rows, nt * _PT))
            Hp[:, :self.kernel_up] = H
            index = np.zeros((nt, 2), dtype=np.int32)
            for t in range(nt):
                rows = np.nonzero(Hp[:, t * _PT:(t + 1) * _PT].any(axis=1))[0]
                index[t] = rows[0], -(-(rows[-1] - rows[0] + 1) // _BK)
            ks = int(index[:, 1].max())
            bank = np.zeros((nt, ks, _PT, _BK), dtype=np.float32)
            for t in range(nt):
                first, n = int(index[t, 0]), int(index[t, 1])
                band = np.zeros((n * _BK, _PT))
                stop = min(self.n_rows, first + n * _BK)
                band[:stop - first] = Hp[first:stop, t * _PT:(t + 1) * _PT]
                bank[t, :n] = band.reshape(n, _BK, _PT).transpose(0, 2, 1)
            self._kernel_tables = (bank, index)
        return self._kernel_tables

    def _tables_on(self, dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        t = self._device_tables.get(key)
        if t is None:
            bank, index = self.kernel_tables()
            t = self._device_tables[key] = (torch.from_numpy(bank).to(dev), torch.from_numpy(index).to(dev))
        return t

    # ------------------------------------------------------------------ the device half
    def check(self, waves, wave_lens):
        """Validate a batch on the host (ValueError, before any launch) -> (waves as a tensor, lens int64 [N])."""
        waves, lens = _batch(waves, wave_lens)
        if lens.min() < 1:
            raise ValueError(f"clip {int(lens.argmin())}: {int(lens.min())} samples")
        if len(lens) * int(self.out_len(lens.max())) >= 1 << 31:
            raise ValueError(f"batch of {len(lens)} x {int(self.out_len(lens.max()))} output samples: the kernel indexes the "
                             "batch with 32-bit integers")
        return waves, lens

    def __call__(self, waves, wave_lens, device=None):
        """``waves`` [N, Lmax] fp32 or int16 PCM at ``orig_rate``, on the device or on the host (then uploaded, to ``device`` or
        the current GPU); ``wave_lens`` the N sample counts (host).  -> ``(out f32 [N, max L_out] on the device at ``new_rate``,
        out_lens np.int64 [N])``; the columns behind a clip's own ``L_out`` are zeros."""
        waves, lens = self.check(waves, wave_lens)
        if not waves.is_cuda:
            if device is None:
                if not torch.cuda.is_available():
                    raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
                device = torch.device("cuda", torch.cuda.current_device())
            waves = _lib.h2d(waves, device)
        waves = waves.contiguous()
        dev = waves.device
        N, Lmax = waves.shape
        out_lens = self.out_len(lens)
        bank, index = self._tables_on(dev)
        lens_d = _lib.h2d(lens.astype(np.int32), dev)
        with torch.no_grad():
            out = torch.empty(N, int(out_lens.max()), device=dev)
        _lib.call("acvae_resample_fwd", waves, int(waves.dtype == torch.int16), Lmax, lens_d, bank, index, out, out.shape[1], N,
                  self.kernel_up, self.kernel_down, self.half_width, bank.shape[1], _lib.current_stream())
        return out, out_lens


class Resampled:
    """``Resampled(resample, logmel)``: audio at ``resample.orig_rate`` -> features, a front end wherever ``frontend=`` takes
    a ``LogMel``: both kernels on the current stream, the resampled batch the one tensor between them."""
    to_float = LogMel.to_float

    def __init__(self, resample, logmel):
        if resample.new_rate != logmel.sample_rate:
            raise ValueError(f"the resampler ends at {resample.new_rate} Hz, the log-mel front end starts from "
                             f"{logmel.sample_rate} Hz")
        self.resample, self.logmel = resample, logmel
        self.sample_rate = resample.orig_rate

    augmented = LogMel.augmented

    def n_frames(self, L):
        """Frames of a clip (or an array of clips) of ``L`` samples at the input rate."""
        return self.logmel.n_frames(self.resample.out_len(L))

    def check(self, waves, wave_lens):
        """Validate a batch for both halves on the host (ValueError, before any launch)."""
        waves, lens = self.resample.check(waves, wave_lens)
        short = self.resample.out_len(lens)
        if short.min() < self.logmel.n_bins:
            raise ValueError(f"clip {int(short.argmin())}: {int(lens[short.argmin()])} samples are {int(short.min())} at "
                             f"{self.logmel.sample_rate} Hz, reflect padding needs at least n_fft/2 + 1 = {self.logmel.n_bins}")
        T = 1 + int(short.max()) // self.logmel.hop_length
        if len(lens) * T * self.logmel.n_bins >= 1 << 31:
            raise ValueError(f"batch of {len(lens)} x {T} frames x {self.logmel.n_bins} bins: the kernel indexes the batch with "
                             "32-bit integers")
        return waves, lens

    def __call__(self, waves, wave_lens, spectrogram=False, device=None):
        """As ``LogMel.__call__``, from waveforms at the resampler's input rate."""
        waves, lens = self.check(waves, wave_lens)
        mid, mid_lens = self.resample(waves, lens, device=device)
        return self.logmel(mid, mid_lens, spectrogram=spectrogram)


class Augmented:
    """``Augmented(frontend, augment)``: waveforms -> features with the training-time augmentation of ``augment``
    (``acvae_amd.augment.Augment``, e.g. ``parse_augments(config["augments"])``) applied, a front end wherever ``frontend=``
    goes in training (``TrainStep.step`` / ``forward_loss``, ``forward_batch(mode="train")``).  The inner front end runs,
    the host draws ``augment.draw_shape(L_n, F)`` for the clips in batch order while the GPU works (every draw depends on
    the clip's shape alone, and ``L_n`` is known from the sample count), and ``apply_plans`` crops, rolls and masks on the
    same stream.  The lengths returned are those after the crop; ``last_plans`` keeps the plans of the latest batch.
    The draws are the reference's, made per batch at step time instead of per item in loader workers.  Evaluation never
    augments: the evaluation calls refuse an ``Augmented``."""

    def __init__(self, frontend, augment):
        if isinstance(frontend, Augmented):
            raise ValueError("the front end is already augmented")
        if not hasattr(augment, "draw_shape"):
            raise ValueError(f"augment must be an acvae_amd.augment.Augment, got {type(augment).__name__}")
        self.frontend, self.augment = frontend, augment
        self.sample_rate = frontend.sample_rate
        self.last_plans = None

    def check(self, waves, wave_lens):
        return self.frontend.check(waves, wave_lens)

    def to_float(self, wave):
        return self.frontend.to_float(wave)

    def __call__(self, waves, wave_lens, spectrogram=False, device=None):
        """As ``LogMel.__call__``; ``feat_lens`` are the clips' lengths after the crop and the batch is as long as the
        longest of them.  ``spectrogram=True`` raises ValueError: the power spectrogram is not augmented."""
        if spectrogram:
            raise ValueError("an Augmented front end returns no spectrogram (the augmentation acts on the features)")
        from . import augment as _augment
        feats, lens = self.frontend(waves, wave_lens, device=device)
        F = feats.shape[2]
        self.last_plans = plans = [self.augment.draw_shape(int(L), F) for L in lens]
        return _augment.apply_plans(feats, lens, plans)


def read_wav_any(path):
    """A 16-bit PCM ``.wav`` file at whatever rate -> ``(int16 tensor [L], rate)``, channels averaged as ``read_wav`` does;
    ``LogMel.at_input_rate(rate)`` is the front end for it."""
    with _wave.open(str(path), "rb") as fh:
        rate, width, ch, frames = fh.getframerate(), fh.getsampwidth(), fh.getnchannels(), fh.getnframes()
        if width != 2:
            raise ValueError(f"{path}: {8 * width}-bit samples, only 16-bit PCM is read")
        data = np.frombuffer(fh.readframes(frames), dtype="<i2").reshape(-1, ch)
    if ch == 1:
        return torch.from_numpy(data[:, 0].astype(np.int16)), rate
    total = data.astype(np.int32).sum(axis=1)
    return torch.from_numpy(((2 * total + ch) // (2 * ch)).astype(np.int16)), rate


def read_wav(path, sample_rate):
    """A 16-bit PCM ``.wav`` file -> int16 tensor [L] (stdlib ``wave``).  Channels are averaged in int32 and rounded (half
    up).  A file at another rate raises ValueError: there is no resampling here."""
    with _wave.open(str(path), "rb") as fh:
        rate, width, ch, frames = fh.getframerate(), fh.getsampwidth(), fh.getnchannels(), fh.getnframes()
        if width != 2:
            raise ValueError(f"{path}: {8 * width}-bit samples, only 16-bit PCM is read")
        if rate != int(sample_rate):
            raise ValueError(f"{path}: sample rate {rate}, expected {int(sample_rate)} (no resampling here)")
        data = np.frombuffer(fh.readframes(frames), dtype="<i2").reshape(-1, ch)
    if ch == 1:
        return torch.from_numpy(data[:, 0].astype(np.int16))
    total = data.astype(np.int32).sum(axis=1)
    return torch.from_numpy(((2 * total + ch) // (2 * ch)).astype(np.int16))


def refuse_augment(augment):
    if augment is not None:
        raise ValueError("frontend= together with augment=: the augment records are drawn per frame on host features; "
                         "to augment a batch of waveforms hand the step frontend=fe.augmented(...) instead")


def refuse_augmented(frontend, where):
    if isinstance(frontend, Augmented):
        raise ValueError(f"{where}: evaluation never augments, hand it the plain front end (frontend.frontend)")
