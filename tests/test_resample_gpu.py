"""GPU: the resampler (acvae_resample_fwd, acvae_amd/frontend.py: Resample, Resampled) against its float64 definition
(tests/resample_util.py) at the smallest shapes that can still go wrong, and its wiring in front of the log-mel front end
into evaluate and TrainStep.step.  Every case prints its worst ratio to the bound before asserting it."""
import random

import numpy as np
import pytest
import torch

import frontend_util as U
import resample_util as R
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from acvae_amd import frontend as F

pytestmark = pytest.mark.gpu
BT = int(_lib._defs["ACVAE_RESAMPLE_BLOCK_TILE"])
GUARD = 4096
SENTINEL = 12345.0
CASES = sorted(R.cases(BT))
EXTRA = 37                                # columns of `out` behind the longest clip's outputs


def guarded(shape):
    """A NaN-filled tensor of `shape` inside a buffer with sentinel guard regions before and after it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    body = buf[GUARD:GUARD + n]
    body.fill_(float("nan"))
    return buf, body.view(shape)


def guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def run(rs, waves, lens, extra=EXTRA):
    """Through the C ABI: waves [N, Lmax] (torch fp32 / int16, host) -> out [N, max L_out + extra] as numpy, guards checked."""
    N, Lmax = waves.shape
    stride = int(rs.out_len(max(lens))) + extra
    wd = waves.cuda()
    ld = torch.as_tensor(np.asarray(lens, dtype=np.int32)).cuda()
    bank, index = rs._tables_on(wd.device)
    obuf, out = guarded((N, stride))
    _lib.call("acvae_resample_fwd", wd, int(waves.dtype == torch.int16), Lmax, ld, bank, index, out, stride, N,
              rs.kernel_up, rs.kernel_down, rs.half_width, bank.shape[1], _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_untouched(obuf), "out: written outside [N, out_stride]"
    return out.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_definition(name):
    ref = R.reference(name, BT)
    rs = F.Resample(ref["orig"], ref["new"], **ref["kw"])
    waves, lens = torch.from_numpy(ref["waves"].copy()), ref["lens"]
    out = run(rs, waves, lens)
    assert out.shape[1] == int(rs.out_len(lens.max())) + EXTRA
    for i, L in enumerate(lens):                      # behind L_out: exactly zero, up to out_stride; before it: all written
        Lo = int(rs.out_len(L))
        assert Lo == R.out_len(L, ref["U"], ref["D"])
        assert not out[i, Lo:].any() and np.isfinite(out[i, Lo:]).all(), f"clip {i}: the row's tail is not zeros"
        assert np.isfinite(out[i, :Lo]).all(), f"clip {i}: outputs left unwritten"
    R.check_case(ref, out)
    out2 = run(rs, waves, lens)
    assert out.tobytes() == out2.tobytes(), "two runs differ"


@pytest.mark.parametrize("name", ["44100_32000", "48000_32000", "8000_16000"])
def test_int16_input_is_bit_equal_to_the_scaled_fp32_input(name):
    ref = R.reference(name, BT)
    rs = F.Resample(ref["orig"], ref["new"], **ref["kw"])
    pcm = torch.from_numpy(np.clip(np.rint(ref["waves"] * 32768.0), -32768, 32767).astype(np.int16))
    assert int(pcm.abs().max()) > 8000
    a = run(rs, pcm, ref["lens"])
    b = run(rs, pcm.float() / 32768.0, ref["lens"])
    assert a.tobytes() == b.tobytes()


def test_a_stride_shorter_than_the_outputs_drops_the_rest():
    """out_stride below a clip's L_out (the caller keeps fewer outputs): the kept ones are unchanged, nothing lands behind."""
    ref = R.reference("48000_32000", BT)
    rs = F.Resample(ref["orig"], ref["new"], **ref["kw"])
    waves = torch.from_numpy(ref["waves"].copy())
    full = run(rs, waves, ref["lens"])
    cut = run(rs, waves, ref["lens"], extra=-1001)
    assert cut.tobytes() == full[:, :cut.shape[1]].tobytes()


def test_resample_call_host_and_device_tensors():
    ref = R.reference("44100_16000_fast", BT)
    rs = F.Resample.kaiser_fast(44100, 16000)
    waves, lens = torch.from_numpy(ref["waves"].copy()), ref["lens"]
    want = run(rs, waves, lens, extra=0)
    tables = rs._device_tables[torch.cuda.current_device()]
    out_h, ol_h = rs(waves, lens)
    out_d, ol_d = rs(waves.cuda(), list(lens))
    assert out_h.is_cuda and out_h.dtype == torch.float32 and ol_h.dtype == np.int64
    assert list(ol_h) == list(ol_d) == [R.out_len(L, ref["U"], ref["D"]) for L in lens]
    assert tuple(out_h.shape) == (len(lens), max(ol_h))
    assert torch.equal(out_h, out_d) and out_h.cpu().numpy().tobytes() == want.tobytes()
    assert len(rs._device_tables) == 1 and rs._device_tables[torch.cuda.current_device()] is tables, "tables uploaded again"
    pcm = torch.from_numpy(np.clip(np.rint(ref["waves"] * 32768.0), -32768, 32767).astype(np.int16))
    assert torch.equal(rs(pcm, lens)[0], rs((pcm.float() / 32768.0).cuda(), lens)[0])
    with pytest.raises(ValueError):
        rs(waves.cuda(), [int(lens[0])] * (len(lens) - 1) + [waves.shape[1] + 1])


# ---------------------------------------------------------------------------------- end to end on a tiny model
V, E = 40, 64
RATE = 22050
WAVE_LENS = [20953, 17640, 14113]         # at 22.05 kHz: 15204 (95 x 160 + 4), 12800 (80 x 160), 10241 (64 x 160 + 1) samples at 16 kHz


def tiny_waves():
    return [torch.from_numpy(U.clip(L, RATE, 70 + i)) for i, L in enumerate(WAVE_LENS)]


def padded(waves):
    out = torch.zeros(len(waves), max(len(w) for w in waves))
    for i, w in enumerate(waves):
        out[i, :len(w)] = w
    return out, np.array([len(w) for w in waves])


def tiny_model():
    import acvae_oracle as O
    from test_model_gpu import build_model
    return build_model(V, E, O.closed_form_state(O.state_shapes(V, E, E, None, E, 512)))


def vocab():
    v = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(V - 4)]:
        v.add_word(w)
    return v


def test_resampled_is_the_two_front_ends_called_by_hand():
    fe = F.LogMel.panns_16k()
    both = fe.at_input_rate(RATE)
    assert isinstance(both, F.Resampled) and both.logmel is fe
    waves, lens = padded(tiny_waves())
    mid, ml = both.resample(waves, lens)
    assert list(ml) == [15204, 12800, 10241]
    want, wl = fe(mid, ml)
    got, gl = both(waves, lens)
    assert list(gl) == list(wl) == list(both.n_frames(lens)) and torch.equal(got, want)
    g2, _, spec = both(waves.cuda(), lens, spectrogram=True)
    assert torch.equal(g2, want) and torch.equal(spec, fe(mid, ml, spectrogram=True)[2])
    pcm = torch.from_numpy(np.rint(waves.numpy() * 32768.0).astype(np.int16))
    assert torch.equal(both(pcm, lens)[0], both(both.to_float(pcm), lens)[0])
    with pytest.raises(ValueError, match="reflect"):          # 352 samples are 256 at 16 kHz, one short of n_fft/2 + 1; 353 are 257
        both(waves[:, :400], [400, 400, 352])
    both(waves[:, :400], [400, 400, 353])


@pytest.mark.parametrize("method,beam", [("greedy", 1), ("beam", 3)])
def test_evaluate_on_other_rate_waveforms_matches_evaluate_on_their_features(method, beam):
    both, model, voc = F.LogMel.panns_16k().at_input_rate(RATE), tiny_model(), vocab()
    wav_items = [(f"clip{i}", w) for i, w in enumerate(tiny_waves())]
    feat_items = [(k, both(w[None], [len(w)])[0][0].cpu()) for k, w in wav_items]
    torch.manual_seed(4)
    want = EV.evaluate(model, feat_items, voc, method=method, beam_size=beam, max_length=8, batch_size=2)
    torch.manual_seed(4)
    got = EV.evaluate(model, wav_items, voc, method=method, beam_size=beam, max_length=8, batch_size=2, frontend=both)
    assert got == want and len(got["predictions"]) == 3


def test_train_step_on_other_rate_waveforms_is_bit_equal_to_the_step_on_their_features():
    import acvae_oracle as O
    from acvae_amd.trainer import TrainStep
    fe = F.LogMel.panns_16k()
    both = F.Resampled(F.Resample(RATE, 16000), fe)
    waves, lens = padded(tiny_waves())
    pcm = torch.from_numpy(np.rint(waves.numpy() * 32768.0).astype(np.int16))
    _, caps, _, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    steps = []
    for _ in range(4):
        m = tiny_model().train()
        m.encoder.p_block = m.encoder.p_fc = 0.0
        steps.append(TrainStep(m, V))
    t1, t2, t3, t4 = steps
    torch.manual_seed(3); random.seed(3)
    p1 = t1.step(waves.clone(), lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=both)
    mid, ml = both.resample(waves, lens)
    feats, fl = fe(mid, ml)
    torch.manual_seed(3); random.seed(3)
    p2 = t2.step(feats, fl, caps, cl, 1.0, 0, 0.5)
    t1.synchronize(); t2.synchronize()
    assert float(p1["loss"]) == float(p2["loss"]) and float(p1["grad_norm"]) == float(p2["grad_norm"])
    assert torch.equal(t1.flat_p, t2.flat_p), "parameters after one step differ"
    # the int16 route: prefetch() keeps pageable PCM as PCM, and the step on it is the step on the features of that PCM
    up = t3.prefetch(pcm)
    assert up.is_cuda and up.dtype == torch.int16
    torch.manual_seed(3); random.seed(3)
    p3 = t3.step(up, lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=both)
    feats16, fl16 = fe(*both.resample(both.to_float(pcm), lens))
    torch.manual_seed(3); random.seed(3)
    p4 = t4.step(feats16, fl16, caps, cl, 1.0, 0, 0.5)
    t3.synchronize(); t4.synchronize()
    assert float(p3["loss"]) == float(p4["loss"]) and float(p3["grad_norm"]) == float(p4["grad_norm"])
    assert torch.equal(t3.flat_p, t4.flat_p), "parameters after one step from int16 PCM differ"
    with pytest.raises(ValueError, match="augment"):
        t1.step(waves, lens.copy(), caps, cl, augment=[None] * 3, frontend=both)
