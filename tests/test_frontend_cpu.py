"""CPU: the log-mel front end's host half (acvae_amd/frontend.py) - scale anchors, the tables against the float64 twin
(tests/frontend_util.py), frame counts, every ValueError path, read_wav - the fairness of the GPU test's inputs (the
float32 matmul twin meets both bounds and both caps on every GPU case), the C entry's argument checks and the kernel's
register record."""
import ctypes
import wave

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import frontend_util as U
from acvae_amd import _lib
from acvae_amd import frontend as F

FT = int(_lib._defs["ACVAE_LOGMEL_FRAME_TILE"])


def test_slaney_scale_anchors():
    assert float(F.hz_to_mel(1000.0)) == 15.0
    assert abs(float(F.hz_to_mel(6400.0)) - 42.0) < 1e-12
    assert abs(float(F.mel_to_hz(42.0)) - 6400.0) < 1e-9 and float(F.mel_to_hz(15.0)) == 1000.0
    assert U.mel_of(1000.0) == 15.0 and abs(U.mel_of(6400.0) - 42.0) < 1e-12


@pytest.mark.parametrize("fe", [F.LogMel.panns_32k(), F.LogMel.panns_16k(),
                                F.LogMel(8000, 256, 100, n_mels=40, fmin=0.0)], ids=["32k", "16k", "8k"])
def test_tables_against_the_twin(fe):
    basis, melw = fe.tables()
    W = U.mel_matrix(fe.sample_rate, fe.n_fft, fe.n_mels, fe.fmin, fe.fmax)
    assert melw.shape == W.shape == (fe.n_bins, fe.n_mels) and melw.dtype == np.float64
    assert np.abs(melw - W).max() <= 1e-12
    assert (melw.sum(axis=0) > 0).all(), "an empty mel filter"
    assert not melw[-1].any(), "fmax <= sr/2: the Nyquist bin carries no weight"
    want = U.basis_formula(fe.n_fft)
    assert basis.dtype == np.float64 and np.array_equal(basis, want)
    k, f = np.arange(fe.n_fft)[:, None], np.arange(fe.n_bins)[None, :]
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / fe.n_fft)
    assert np.abs(basis[0] - w * np.cos(2 * np.pi * k * f / fe.n_fft)).max() < 1e-11     # the unreduced angle agrees
    assert np.abs(basis[1] + w * np.sin(2 * np.pi * k * f / fe.n_fft)).max() < 1e-11


def test_kernel_layout_of_the_basis():
    """[chunk][K-step][128 columns][32 k]: re of bin 64 q + c in column c, im in column 64 + c, the Nyquist bin's real part in
    the (identically zero) imaginary column of bin 0."""
    fe = F.LogMel.panns_16k()
    basis, melw = fe.tables()
    packed, melw32 = fe.kernel_tables()
    n = fe.n_fft
    packed = packed.reshape(n // 128, n // 32, 128, 32)
    assert packed.dtype == np.float32 and packed.size == n * n
    for q, ks, c, kk in [(0, 0, 0, 0), (1, 3, 5, 7), (3, 15, 63, 31), (2, 9, 64, 1), (0, 4, 65, 30), (3, 1, 127, 2)]:
        part, f = (0, 64 * q + c) if c < 64 else (1, 64 * q + c - 64)
        assert packed[q, ks, c, kk] == np.float32(basis[part, 32 * ks + kk, f])
    assert np.array_equal(packed[0, :, 64, :].reshape(-1), basis[0, :, n // 2].astype(np.float32))
    assert np.array_equal(melw32, melw.astype(np.float32))


def test_n_frames():
    fe = F.LogMel.panns_32k()
    assert fe.n_frames(513) == 2 and fe.n_frames(320000) == 1001 and fe.n_frames(319) == 1
    assert list(fe.n_frames(np.array([640, 959, 960]))) == [3, 3, 4]
    assert F.LogMel.panns_16k().n_frames(160000) == 1001


def test_presets():
    a, b = F.LogMel.panns_32k(), F.LogMel.panns_16k()
    assert (a.sample_rate, a.n_fft, a.hop_length, a.n_mels, a.fmin, a.fmax, a.ref, a.amin) == \
        (32000, 1024, 320, 64, 50.0, 14000.0, 1.0, 1e-10)
    assert (b.sample_rate, b.n_fft, b.hop_length, b.n_mels, b.fmin, b.fmax, b.ref, b.amin) == \
        (16000, 512, 160, 64, 50.0, 8000.0, 1.0, 1e-10)
    assert a.db_offset == 0.0


def test_bad_settings_raise():
    for kw in (dict(n_fft=1000), dict(n_fft=128), dict(n_fft=4096), dict(hop_length=0), dict(hop_length=1025),
               dict(n_mels=0), dict(n_mels=66), dict(n_mels=132), dict(top_db=80.0), dict(fmin=9000.0, fmax=8000.0),
               dict(fmax=20000.0), dict(amin=0.0)):
        args = dict(sample_rate=32000, n_fft=1024, hop_length=320)
        args.update(kw)
        with pytest.raises(ValueError):
            F.LogMel(**args)


def test_bad_batches_raise_before_any_launch():
    fe = F.LogMel.panns_32k()
    ok = torch.zeros(2, 2000)
    for waves, lens in ((torch.zeros(2, 2000), [2000, 512]),            # short clip: reflect needs n_fft/2 + 1
                        (torch.zeros(2, 2000), [2001, 600]),            # longer than the batch
                        (torch.zeros(2, 2000), [2000]),                 # one length for two clips
                        (torch.zeros(2000), [2000]),                    # not [N, Lmax]
                        (torch.zeros(2, 2000, dtype=torch.float64), [2000, 600]),
                        (torch.zeros(2, 2000, dtype=torch.int32), [2000, 600]),
                        (ok, [2000.5, 600])):
        with pytest.raises(ValueError):
            fe(waves, lens)


def test_host_tensor_without_a_gpu_is_refused(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.LogMel.panns_16k()(torch.zeros(1, 4000), [4000])


def test_frontend_with_augment_raises():
    from acvae_amd import batch as B
    from acvae_amd.augment import AugmentParams
    from acvae_amd.trainer import TrainStep
    fe = F.LogMel.panns_16k()
    model = torch.nn.Linear(2, 2)
    rec = [AugmentParams(length=26)]
    waves, caps = torch.zeros(1, 4000), torch.zeros(1, 5)
    with pytest.raises(ValueError, match="augment"):
        B.forward_batch(model, [waves, caps, ["a"], np.array([4000]), np.array([5])], "train", augment=rec, frontend=fe)
    with pytest.raises(ValueError, match="augment"):       # the batch's own AugmentParams column
        B.forward_batch(model, [waves, caps, ["a"], tuple(rec), np.array([4000]), np.array([5])], "train", frontend=fe)
    # a TrainStep needs a GPU to construct; step() refuses before it touches any of its state, so a bare instance will do
    # (an AttributeError here means that something was moved above the check)
    with pytest.raises(ValueError, match="augment"):
        TrainStep.step(object.__new__(TrainStep), waves, [4000], caps, [5], augment=rec, frontend=fe)


def _write_wav(path, data, rate, width=2):
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(1 if data.ndim == 1 else data.shape[1])
        fh.setsampwidth(width)
        fh.setframerate(rate)
        fh.writeframes(data.astype("<i2" if width == 2 else "u1").tobytes())


def test_read_wav_round_trip(tmp_path):
    g = np.random.default_rng(3)
    mono = g.integers(-32768, 32768, size=777).astype(np.int16)
    mono[:2] = (-32768, 32767)
    _write_wav(tmp_path / "m.wav", mono, 16000)
    got = F.read_wav(tmp_path / "m.wav", 16000)
    assert got.dtype == torch.int16 and np.array_equal(got.numpy(), mono)
    stereo = g.integers(-32768, 32768, size=(500, 2)).astype(np.int16)
    stereo[:3] = ((32767, 32767), (-32768, -32768), (-3, 0))
    _write_wav(tmp_path / "s.wav", stereo, 32000)
    got = F.read_wav(tmp_path / "s.wav", 32000)
    want = (stereo.astype(np.int32).sum(axis=1) + 1) // 2           # averaged in int32, half rounds up
    assert got.dtype == torch.int16 and np.array_equal(got.numpy().astype(np.int32), want)
    with pytest.raises(ValueError, match="rate"):
        F.read_wav(tmp_path / "m.wav", 32000)
    _write_wav(tmp_path / "b.wav", np.zeros(10, dtype=np.uint8), 16000, width=1)
    with pytest.raises(ValueError, match="16-bit"):
        F.read_wav(tmp_path / "b.wav", 16000)
    fe = F.LogMel.panns_16k()
    assert torch.equal(fe.to_float(torch.from_numpy(mono)), torch.from_numpy(mono.astype(np.float32) / 32768.0))


@pytest.mark.parametrize("name", sorted(U.cases(FT)))
def test_float32_twin_meets_the_bounds_on_every_gpu_case(name):
    """The inputs of tests/test_frontend_gpu.py are fair: a float32 matmul evaluation of the definition sits well inside both
    bounds and both caps on every one of them."""
    ref = U.reference(name, FT)
    kw = ref["kw"]
    T = 1 + int(ref["lens"].max()) // kw["hop_length"]
    spec = np.zeros((len(ref["lens"]), T, kw["n_fft"] // 2 + 1), dtype=np.float32)
    feats = np.zeros((len(ref["lens"]), T, kw["n_mels"]), dtype=np.float32)
    for i, L in enumerate(ref["lens"]):
        P, db = U.twin_f32(ref["waves"][i, :L], kw["n_fft"], kw["hop_length"], ref["W"], 1e-10, 1.0)
        spec[i, :len(P)], feats[i, :len(P)] = P, db
    ws, wd, _, left_out, _ = U.check_case(ref, spec, feats)
    assert ws <= 0.5 and wd <= 0.5, "the twin should sit far inside the bounds"
    if "silence" in name:
        assert left_out > 0, "the silent stretch should produce cells the bound cannot judge"


def test_entry_refuses_bad_arguments_without_a_gpu():
    ge.build()
    fn = _lib.lib().acvae_logmel_fwd
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    good = dict(wave=p, i16=0, stride=4000, lens=p, basis=p, melw=p, out=p, spec=None, N=1, T=26, n_fft=512, hop=160,
                n_mels=64, amin=1e-10, off=0.0, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fn(*a.values())

    for kw in (dict(wave=None), dict(lens=None), dict(basis=None), dict(melw=None), dict(out=None), dict(i16=2), dict(N=0),
               dict(T=0), dict(n_fft=500), dict(n_fft=128), dict(n_fft=4096), dict(hop=0), dict(hop=513), dict(n_mels=0),
               dict(n_mels=62), dict(n_mels=132), dict(amin=0.0), dict(stride=256), dict(T=27), dict(stride=(1 << 30) + 1),
               dict(N=1 << 20, T=26)):
        assert call(**kw) == -1, kw
    assert call(basis=p + 4) == -2


def test_kernel_keeps_everything_in_registers():
    from acvae_amd import build as b
    ge.build()
    hits = {n: u for n, u in b.resource_usage().items() if "logmel_kernel" in n}
    assert len(hits) == 2, "one instance per sample type (fp32, int16)"
    for n, u in hits.items():
        assert u.get("scratch", -1) == 0, f"{n}: {u.get('scratch')} bytes per lane of scratch"
        assert u.get("vgprs", 999) <= 256, (n, u)
        assert u.get("occupancy", 0) >= 2, (n, u)      # two workgroups of four wavefronts per CU


class _StubFrontend:
    """Stands in for LogMel on the host: 'features' = the waveform folded into 4 columns, 'frames' = samples // 4."""
    to_float = F.LogMel.to_float

    def __init__(self):
        self.seen = []

    def __call__(self, waves, lens, device=None):
        self.seen.append((waves.dtype, tuple(waves.shape), list(np.asarray(lens))))
        self.first = float(waves.reshape(-1)[0])
        n = waves.shape[1] // 4 * 4
        return waves[:, :n].reshape(waves.shape[0], -1, 4).clone(), np.asarray(lens) // 4


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, feats, feat_lens, *rest, **kw):
        self.calls.append((tuple(feats.shape), list(feat_lens)))
        n = feats.shape[0]
        if rest:                                                   # training forward: (caps, cap_lens)
            return {"logits": torch.zeros(n, int(max(rest[1])) - 1, 5)}
        return {"seqs": torch.full((n, 3), 2, dtype=torch.long)}


def test_wiring_hands_waveforms_to_the_frontend_and_features_to_the_model():
    """The host logic of frontend= in forward_batch and evaluate, with stand-ins for the two device halves: the waveform and
    sample-count slots are replaced by features and frame counts before the model runs, in all three modes, and evaluate
    turns int16 items into the samples they stand for before collate_fn pads them into float32."""
    from acvae_amd import batch as B
    from acvae_amd import evaluate as EV
    waves, lens = torch.arange(24.0).reshape(2, 12), np.array([12, 8])
    for mode in ("eval", "validation"):
        fe, model = _StubFrontend(), _StubModel()
        batch = [["a", "b"], waves.clone(), lens.copy()]
        B.forward_batch(model, batch, mode, frontend=fe, method="greedy", beam_size=1)
        assert fe.seen == [(torch.float32, (2, 12), [12, 8])] and model.calls == [((2, 3, 4), [3, 2])]
        assert tuple(batch[1].shape) == (2, 3, 4) and list(batch[-1]) == [3, 2]
    fe, model = _StubFrontend(), _StubModel()
    caps, cl = torch.ones(2, 4), np.array([4, 3])
    out = B.forward_batch(model, [waves.clone(), caps, ["a", "b"], lens.copy(), cl], "train", frontend=fe)
    assert model.calls == [((2, 3, 4), [3, 2])] and out["packed_logits"].shape == (5, 5)
    # without frontend= nothing is touched
    model = _StubModel()
    B.forward_batch(model, [["a", "b"], waves.clone(), lens.copy()], "eval", method="greedy", beam_size=1)
    assert model.calls == [((2, 12), [12, 8])]

    voc = EV.Vocabulary()
    for w in ("<pad>", "<start>", "<end>", "<unk>"):
        voc.add_word(w)
    fe, model = _StubFrontend(), _StubModel()
    pcm = [("x", torch.tensor([16384, -32768, 0, 8192, 1, 2, 3, 4], dtype=torch.int16)), ("y", torch.zeros(12, dtype=torch.int16))]
    got = EV.evaluate(model, pcm, voc, batch_size=2, frontend=fe)
    assert [p["filename"] for p in got["predictions"]] == ["x", "y"]
    assert fe.seen == [(torch.float32, (2, 12), [8, 12])] and model.calls == [((2, 3, 4), [2, 3])]
    assert fe.first == 0.5, "int16 PCM must reach the front end as the samples it stands for (16384 / 32768)"
