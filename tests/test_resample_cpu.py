"""CPU: the resampler's host half (acvae_amd/frontend.py: Resample, Resampled, read_wav_any) - the tables against the
float64 twin (tests/resample_util.py) and against scipy's polyphase filter, the compacted layout, output lengths, tones
through the pass band and the stop band, every ValueError path - the fairness of the GPU test's inputs (the float32 matmul
twin meets the bound on every GPU case), the C entry's argument checks and the kernel's register record."""
import ctypes
import math
import wave

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import resample_util as R
from acvae_amd import _lib
from acvae_amd import frontend as F

BT = int(_lib._defs["ACVAE_RESAMPLE_BLOCK_TILE"])
CASES = sorted(R.cases(BT))
PAIRS = [(44100, 32000, R.BEST), (48000, 32000, R.BEST), (32000, 16000, R.BEST), (22050, 32000, R.BEST),
         (8000, 16000, R.BEST), (44100, 16000, R.BEST), (44100, 16000, R.FAST)]
IDS = ["44100_32000", "48000_32000", "32000_16000", "22050_32000", "8000_16000", "44100_16000", "44100_16000_fast"]


def test_presets_and_derived_sizes():
    a, b = F.Resample.kaiser_best(44100, 32000), F.Resample.kaiser_fast(44100, 16000)
    assert (a.zeros, a.rolloff, a.beta) == (64, 0.9475937167399596, 14.769656459379492)
    assert (b.zeros, b.rolloff, b.beta) == (16, 0.85, 8.555504641634386)
    assert (a.up, a.down, a.group, a.kernel_up, a.kernel_down) == (320, 441, 1, 320, 441)
    assert F.Resample(44100, 32000).beta == a.beta and F.Resample(44100, 32000).zeros == 64
    for orig, new, U, D, s in ((48000, 32000, 2, 3, 16), (32000, 16000, 1, 2, 32), (8000, 16000, 2, 1, 16)):
        r = F.Resample(orig, new)
        assert (r.up, r.down, r.group, r.kernel_up, r.kernel_down) == (U, D, s, s * U, s * D) and s == R.group(U)
    assert a.half_width == math.ceil(64 / (a.rolloff * 320 / 441)) + 1 and 2 * a.half_width == R.taps(320, 441, 64, a.rolloff)
    assert F.Resample(22050, 32000).cutoff == a.rolloff


@pytest.mark.parametrize("orig,new,kw", PAIRS, ids=IDS)
def test_tables_against_the_twin(orig, new, kw):
    rs = F.Resample(orig, new, **kw)
    H = rs.tables()
    U, D = R.ratio(orig, new)
    Uk, Dk, W = rs.kernel_up, rs.kernel_down, rs.half_width
    assert H.dtype == np.float64 and H.shape == (2 * W + Dk, Uk)
    k = np.arange(H.shape[0], dtype=np.int64)[:, None] - W
    i = np.arange(Uk, dtype=np.int64)[None, :]
    # output m = i of block 0 reads input n = k: the numerator m D - n U in lowest terms
    num = i * D - k * U if rs.group == 1 else (i * Dk - k * Uk) // rs.group
    want = R.kernel_fn(num, U, D, **kw)
    assert np.abs(H - want).max() <= 1e-15 * np.abs(want).max()
    assert H.max() == pytest.approx(rs.cutoff, rel=1e-12), "g(0) = c sits in phase 0"
    assert not H[0].any() and not H[-1].any(), "the rows of H reach past the support of every phase on both sides"


@pytest.mark.parametrize("orig,new,kw", PAIRS, ids=IDS)
def test_kernel_layout_of_the_bank(orig, new, kw):
    """[phase tile][K-step][32 phases][32 k] from the tile's first k on: un-compacted it is tables() rounded to fp32, and
    what it leaves out is zero in tables()."""
    rs = F.Resample(orig, new, **kw)
    H = rs.tables()
    bank, index = rs.kernel_tables()
    nt = -(-rs.kernel_up // 32)
    assert bank.dtype == np.float32 and index.dtype == np.int32
    assert bank.shape == (nt, int(index[:, 1].max()), 32, 32) and index.shape == (nt, 2)
    assert bank.flags["C_CONTIGUOUS"] and 1 <= bank.shape[1] <= int(_lib._defs["ACVAE_RESAMPLE_MAX_KSTEPS"])
    full = np.zeros((H.shape[0] + bank.shape[1] * 32, nt * 32), dtype=np.float32)
    stored = np.zeros(full.shape, dtype=bool)
    for t in range(nt):
        first, n = int(index[t, 0]), int(index[t, 1])
        assert 0 <= first < H.shape[0] and 1 <= n <= bank.shape[1]
        assert not bank[t, n:].any(), "K-steps behind the tile's own are zeros"
        full[first:first + n * 32, 32 * t:32 * t + 32] = bank[t, :n].transpose(0, 2, 1).reshape(n * 32, 32)
        stored[first:first + n * 32, 32 * t:32 * t + 32] = True
    assert not full[H.shape[0]:].any() and not full[:, rs.kernel_up:].any(), "rows outside H and phases >= U' are zeros"
    assert np.array_equal(full[:H.shape[0], :rs.kernel_up], H.astype(np.float32))
    assert not H[~stored[:H.shape[0], :rs.kernel_up]].any(), "a non-zero tap outside the stored band"
    if (orig, new) == (44100, 32000):
        assert bank.shape[1] * 32 < 0.45 * H.shape[0], "the band of a phase tile is well under half of H's rows"
    assert rs.kernel_tables()[0] is bank, "made once"


def test_out_len_is_the_exact_ceiling():
    for orig, new in ((44100, 32000), (48000, 32000), (32000, 16000), (22050, 32000), (8000, 16000)):
        rs = F.Resample(orig, new)
        U, D = R.ratio(orig, new)
        Ls = sorted({max(1, q * D + d) for q in (0, 1, 2, 7, 64, 10 ** 6) for d in (-1, 0, 1)})
        got = rs.out_len(np.array(Ls))
        assert got.dtype == np.int64
        for L, g in zip(Ls, got):
            assert g == -((-L * U) // D) == R.out_len(L, U, D) and (g - 1) * D < L * U <= g * D
        assert rs.out_len(Ls[3]) == got[3]
    assert F.Resample(44100, 32000).out_len(441000) == 320000 and F.Resample(48000, 32000).out_len(2 ** 30) == 715827883


@pytest.mark.parametrize("name", CASES)
def test_scipy_agrees_with_the_direct_sum(name):
    """An independent witness of the twin: scipy's polyphase filter with h[j] = g(j / U) on the upsampled grid (scipy
    multiplies a given filter by `up`, hence the / U)."""
    signal = pytest.importorskip("scipy.signal")
    ref = R.reference(name, BT)
    U, D, kw = ref["U"], ref["D"], ref["kw"]
    half = int(math.ceil(kw["zeros"] / (kw["rolloff"] * min(1.0, U / D)))) * U + U
    h = R.kernel_fn(np.arange(-half, half + 1), U, D, **kw)
    for i, L in enumerate(ref["lens"]):
        y = signal.resample_poly(ref["waves"][i, :L].astype(np.float64), U, D, window=h / U)
        assert len(y) == len(ref["y"][i])
        assert np.abs(y - ref["y"][i]).max() <= 1e-14 * max(1.0, np.abs(ref["y"][i]).max())


@pytest.mark.parametrize("name", CASES)
def test_float32_twin_meets_the_bound_on_every_gpu_case(name):
    """The inputs of tests/test_resample_gpu.py are fair: a float32 matmul evaluation over the compacted bank sits well
    inside the bound on every one of them."""
    ref = R.reference(name, BT)
    rs = F.Resample(ref["orig"], ref["new"], **ref["kw"])
    assert 2 * rs.half_width == ref["K"]
    lo = rs.out_len(ref["lens"])
    out = np.zeros((len(lo), int(lo.max())), dtype=np.float32)
    for i, L in enumerate(ref["lens"]):
        out[i, :lo[i]] = R.twin_f32(ref["waves"][i, :L], rs)
    worst, cells, silent = R.check_case(ref, out)
    assert worst <= 0.5, "the twin should sit far inside the bound"
    assert (silent > 0) == ("silence" in name), "only the silent stretches give outputs with A = 0"


def _tone(rs, f, L=44100):
    x = np.sin(2 * np.pi * f * np.arange(L) / rs.orig_rate)
    H = rs.tables()
    Uk, Dk, W = rs.kernel_up, rs.kernel_down, rs.half_width
    J = int(rs.out_len(L)) // Uk
    xp = np.concatenate([np.zeros(W), x, np.zeros(H.shape[0] + Dk)])
    X = np.lib.stride_tricks.sliding_window_view(xp, H.shape[0])[:J * Dk:Dk]
    y = (X @ H).reshape(-1)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    rms_in = np.sqrt(np.mean(x[len(x) // 4:3 * len(x) // 4] ** 2))
    return np.sqrt(np.mean(y[mid] ** 2)) / rms_in


def test_tones_through_the_product_tables():
    """44.1 -> 32 kHz through Resample.tables() in float64: the pass band has unit gain, 17 kHz (above the new Nyquist
    frequency) is gone."""
    rs = F.Resample.kaiser_best(44100, 32000)
    g1, g14, g17 = _tone(rs, 1000.0), _tone(rs, 14000.0), _tone(rs, 17000.0)
    print(f"tone gains 44.1 -> 32 kHz: 1 kHz {g1:.6f}, 14 kHz {g14:.6f}, 17 kHz {g17:.3e}")
    assert abs(g1 - 1.0) <= 1e-3
    assert abs(g14 - 1.0) <= 1e-3
    assert g17 < 1e-6


def test_bad_settings_raise():
    for args, kw in (((32000, 32000), {}), ((44100.5, 32000), {}), ((44100, 0), {}), ((-8000, 16000), {}),
                     ((44100, 32000), dict(zeros=0)), ((44100, 32000), dict(zeros=2.5)), ((44100, 32000), dict(rolloff=0.0)),
                     ((44100, 32000), dict(rolloff=1.01)), ((44100, 32000), dict(beta=float("nan"))),
                     ((44100, 32001), {}),                                   # lowest terms beyond the kernel's ratios
                     ((48000, 1000), {}),                                    # U = 1: 32 blocks of D = 48 in one
                     ((32000, 16000), dict(zeros=600))):                     # 2 (600 / 0.47 + 1) taps per output
        with pytest.raises(ValueError):
            F.Resample(*args, **kw)
    F.Resample(44100, 32000, rolloff=1.0)
    with pytest.raises(ValueError, match="32000"):
        F.Resampled(F.Resample(44100, 32000), F.LogMel.panns_16k())
    with pytest.raises(ValueError):
        F.LogMel.panns_16k().at_input_rate(44100.5)


def test_bad_batches_raise_before_any_launch():
    rs = F.Resample(44100, 32000)
    for waves, lens in ((torch.zeros(2, 2000), [2001, 600]),            # longer than the batch's stride
                        (torch.zeros(2, 2000), [2000]),                 # one length for two clips
                        (torch.zeros(2, 2000), [2000, 0]),              # an empty clip
                        (torch.zeros(2000), [2000]),                    # not [N, Lmax]
                        (torch.zeros(2, 2000, dtype=torch.float64), [2000, 600]),
                        (torch.zeros(2, 2000, dtype=torch.int32), [2000, 600]),
                        (torch.zeros(2, 2000), [2000.5, 600])):
        with pytest.raises(ValueError):
            rs(waves, lens)
        with pytest.raises(ValueError):
            F.Resampled(rs, F.LogMel.panns_32k())(waves, lens)
    # 706 samples at 44.1 kHz are 513 at 32 kHz, the least the log-mel's reflect padding takes; 705 are 512
    both = F.LogMel.panns_32k().at_input_rate(44100)
    assert rs.out_len(706) == 513 and rs.out_len(705) == 512
    both.check(torch.zeros(2, 2000), [2000, 706])
    with pytest.raises(ValueError, match="reflect"):
        both(torch.zeros(2, 2000), [2000, 705])


def test_host_tensor_without_a_gpu_is_refused(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.Resample(44100, 32000)(torch.zeros(1, 4000), [4000])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.LogMel.panns_16k().at_input_rate(22050)(torch.zeros(1, 4000), [4000])


def test_at_input_rate_and_resampled():
    fe = F.LogMel.panns_32k()
    assert fe.at_input_rate(32000) is fe and F.LogMel.panns_16k().at_input_rate(16000.0).sample_rate == 16000
    both = fe.at_input_rate(44100)
    assert isinstance(both, F.Resampled) and both.logmel is fe and both.sample_rate == 44100
    assert (both.resample.orig_rate, both.resample.new_rate, both.resample.zeros) == (44100, 32000, 64)
    assert fe.at_input_rate(44100, **F.Resample.FAST).resample.zeros == 16
    assert list(both.n_frames(np.array([441000, 706]))) == [1001, 2]
    pcm = torch.tensor([16384, -32768], dtype=torch.int16)
    assert torch.equal(both.to_float(pcm), torch.tensor([0.5, -1.0])) and both.to_float(pcm.float()).dtype == torch.float32
    with pytest.raises(ValueError, match="augment"):       # frontend= with augment= stays refused, whatever the front end
        from acvae_amd import batch as B
        from acvae_amd.augment import AugmentParams
        B.forward_batch(torch.nn.Linear(2, 2), [torch.zeros(1, 4000), torch.zeros(1, 5), ["a"], np.array([4000]), np.array([5])],
                        "train", augment=[AugmentParams(length=26)], frontend=both)


def _write_wav(path, data, rate, width=2):
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(1 if data.ndim == 1 else data.shape[1])
        fh.setsampwidth(width)
        fh.setframerate(rate)
        fh.writeframes(data.astype("<i2" if width == 2 else "u1").tobytes())


def test_read_wav_any_round_trip(tmp_path):
    g = np.random.default_rng(5)
    mono = g.integers(-32768, 32768, size=777).astype(np.int16)
    mono[:2] = (-32768, 32767)
    _write_wav(tmp_path / "m.wav", mono, 44100)
    got, rate = F.read_wav_any(tmp_path / "m.wav")
    assert rate == 44100 and got.dtype == torch.int16 and np.array_equal(got.numpy(), mono)
    assert torch.equal(got, F.read_wav(tmp_path / "m.wav", 44100)), "the same samples as read_wav at the file's own rate"
    with pytest.raises(ValueError, match="no resampling here"):          # read_wav keeps its refusal
        F.read_wav(tmp_path / "m.wav", 32000)
    stereo = g.integers(-32768, 32768, size=(500, 2)).astype(np.int16)
    stereo[:3] = ((32767, 32767), (-32768, -32768), (-3, 0))
    _write_wav(tmp_path / "s.wav", stereo, 48000)
    got, rate = F.read_wav_any(tmp_path / "s.wav")
    want = (stereo.astype(np.int32).sum(axis=1) + 1) // 2               # averaged in int32, half rounds up
    assert rate == 48000 and got.dtype == torch.int16 and np.array_equal(got.numpy().astype(np.int32), want)
    _write_wav(tmp_path / "b.wav", np.zeros(10, dtype=np.uint8), 16000, width=1)
    with pytest.raises(ValueError, match="16-bit"):
        F.read_wav_any(tmp_path / "b.wav")


def test_entry_refuses_bad_arguments_without_a_gpu():
    ge.build()
    fn = _lib.lib().acvae_resample_fwd
    assert _lib.lib().acvae_abi_version() == 3, "an added entry: the ABI version stays"
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    good = dict(wave=p, i16=0, stride=4000, lens=p, bank=p, index=p, out=p, out_stride=3000, N=1, U=320, D=441, W=95,
                ksteps=8, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fn(*a.values())

    for kw in (dict(wave=None), dict(lens=None), dict(bank=None), dict(index=None), dict(out=None), dict(i16=2), dict(N=0),
               dict(U=0), dict(U=1025), dict(D=0), dict(D=1025), dict(U=1, D=1), dict(U=441), dict(W=0), dict(W=1025),
               dict(ksteps=0), dict(ksteps=99), dict(stride=0), dict(stride=(1 << 30) + 1), dict(out_stride=0),
               dict(out_stride=1 << 31), dict(N=1 << 20, out_stride=2048)):
        assert call(**kw) == -1, kw
    assert call(bank=p + 4) == -2


def test_kernel_keeps_everything_in_registers():
    from acvae_amd import build as b
    ge.build()
    hits = {n: u for n, u in b.resource_usage().items() if "resample_kernel" in n}
    assert len(hits) == 2, "one instance per sample type (fp32, int16)"
    for n, u in hits.items():
        assert u.get("scratch", -1) == 0, f"{n}: {u.get('scratch')} bytes per lane of scratch"
        assert u.get("vgprs", 999) <= 128, (n, u)
        assert u.get("occupancy", 0) >= 2, (n, u)      # at least two workgroups of four wavefronts per CU
