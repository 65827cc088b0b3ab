"""GPU: the log-mel front end (acvae_logmel_fwd, acvae_amd/frontend.py) against its float64 definition
(tests/frontend_util.py) at the smallest shapes that can still go wrong, and its wiring into forward_batch, evaluate and
TrainStep.step.  Every case prints its worst ratio to the bounds before asserting it."""
import random

import numpy as np
import pytest
import torch

import frontend_util as U
from acvae_amd import _lib
from acvae_amd import batch as B
from acvae_amd import evaluate as EV
from acvae_amd import frontend as F

pytestmark = pytest.mark.gpu
FT = int(_lib._defs["ACVAE_LOGMEL_FRAME_TILE"])
GUARD = 4096
SENTINEL = 12345.0
CASES = sorted(U.cases(FT))


def guarded(shape):
    """A NaN-filled tensor of `shape` inside a buffer with sentinel guard regions before and after it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    body = buf[GUARD:GUARD + n]
    body.fill_(float("nan"))
    return buf, body.view(shape)


def guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def run(fe, waves, lens, with_spec=True, melw=None):
    """Through the C ABI: waves [N, Lmax] (torch fp32 / int16, host) -> (out, spec or None) as numpy, guards checked.
    ``melw``: mel weights [nb, n_mels] (numpy) in place of the front end's own."""
    N, Lmax = waves.shape
    T = 1 + int(max(lens)) // fe.hop_length
    wd = waves.cuda()
    ld = torch.as_tensor(np.asarray(lens, dtype=np.int32)).cuda()
    basis, own = fe._tables_on(wd.device)
    melw = own if melw is None else torch.from_numpy(np.ascontiguousarray(melw, dtype=np.float32)).cuda()
    obuf, out = guarded((N, T, fe.n_mels))
    sbuf, spec = guarded((N, T, fe.n_bins)) if with_spec else (None, None)
    _lib.call("acvae_logmel_fwd", wd, int(waves.dtype == torch.int16), Lmax, ld, basis, melw, out, spec, N, T, fe.n_fft,
              fe.hop_length, fe.n_mels, fe.amin, fe.db_offset, _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_untouched(obuf), "out: written outside [N, T, n_mels]"
    assert sbuf is None or guards_untouched(sbuf), "spec: written outside [N, T, nb]"
    return out.cpu().numpy(), None if spec is None else spec.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_definition(name):
    ref = U.reference(name, FT)
    fe = F.LogMel(**ref["kw"])
    waves, lens = torch.from_numpy(ref["waves"].copy()), ref["lens"]
    out, spec = run(fe, waves, lens)
    for i, L in enumerate(lens):                      # padding rows: exactly zero; valid rows: all written
        Tn = 1 + int(L) // fe.hop_length
        assert not out[i, Tn:].any() and not spec[i, Tn:].any(), f"clip {i}: padding rows are not zeros"
        assert np.isfinite(out[i, :Tn]).all() and np.isfinite(spec[i, :Tn]).all(), f"clip {i}: rows left unwritten"
    U.check_case(ref, spec, out)
    out2, spec2 = run(fe, waves, lens)
    assert out.tobytes() == out2.tobytes() and spec.tobytes() == spec2.tobytes(), "two runs differ"
    out3, _ = run(fe, waves, lens, with_spec=False)
    assert out.tobytes() == out3.tobytes(), "spec = NULL changes out"


@pytest.mark.parametrize("name", ["n256_hop100", "panns_16k_ragged"])
def test_mel_weights_on_the_nyquist_bin_reach_the_mel_sum(name):
    """LogMel keeps fmax <= sr/2, so its own weights on the Nyquist bin are zero and the kernel's Nyquist term (which travels
    apart from the other bins) adds nothing.  A caller of the C ABI may hand in any weights: with a last row as heavy as the
    heaviest of the others, the same bounds hold against the float64 mel sum over all n/2 + 1 bins."""
    ref = dict(U.reference(name, FT))
    fe = F.LogMel(**ref["kw"])
    W = ref["W"].copy()
    W[-1] = W.max() * np.linspace(0.25, 1.0, W.shape[1])
    ref["W"] = W
    waves = torch.from_numpy(ref["waves"].copy())
    out, spec = run(fe, waves, ref["lens"], melw=W)
    U.check_case(ref, spec, out)
    plain, _ = run(fe, waves, ref["lens"])
    assert not np.array_equal(out, plain), "the Nyquist row of the weights changed nothing"


@pytest.mark.parametrize("name", ["panns_16k_ragged", "n256_hop100"])
def test_int16_input_is_bit_equal_to_the_scaled_fp32_input(name):
    ref = U.reference(name, FT)
    fe = F.LogMel(**ref["kw"])
    pcm = torch.from_numpy(np.clip(np.rint(ref["waves"] * 32768.0), -32768, 32767).astype(np.int16))
    assert int(pcm.abs().max()) > 8000
    a, sa = run(fe, pcm, ref["lens"])
    b, sb = run(fe, pcm.float() / 32768.0, ref["lens"])
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()


def test_logmel_call_host_and_device_tensors():
    ref = U.reference("panns_16k_ragged", FT)
    fe = F.LogMel.panns_16k()
    waves, lens = torch.from_numpy(ref["waves"].copy()), ref["lens"]
    want, want_spec = run(fe, waves, lens)
    tables = fe._device_tables[torch.cuda.current_device()]
    feats_h, fl_h = fe(waves, lens)
    feats_d, fl_d, spec_d = fe(waves.cuda(), list(lens), spectrogram=True)
    assert feats_h.is_cuda and feats_h.dtype == torch.float32 and fl_h.dtype == np.int64
    assert list(fl_h) == list(fl_d) == [1 + int(L) // 160 for L in lens]
    assert torch.equal(feats_h, feats_d) and feats_h.cpu().numpy().tobytes() == want.tobytes()
    assert spec_d.cpu().numpy().tobytes() == want_spec.tobytes()
    assert len(fe._device_tables) == 1 and fe._device_tables[torch.cuda.current_device()] is tables, "tables uploaded again"
    pcm = torch.from_numpy(np.clip(np.rint(ref["waves"] * 32768.0), -32768, 32767).astype(np.int16))
    assert torch.equal(fe(pcm, lens)[0], fe(fe.to_float(pcm).cuda(), lens)[0])
    with pytest.raises(ValueError):
        fe(waves.cuda(), [int(lens[0])] * 3 + [100])


# ---------------------------------------------------------------------------------- end to end on a tiny model
V, E = 40, 64
WAVE_LENS = [95 * 160 + 3, 80 * 160, 64 * 160 + 1]


def tiny_waves():
    return [torch.from_numpy(U.clip(L, 16000, 50 + i)) for i, L in enumerate(WAVE_LENS)]


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


def test_forward_batch_with_frontend_matches_the_model_on_its_features():
    import acvae_oracle as O
    fe, model = F.LogMel.panns_16k(), tiny_model()
    waves, lens = padded(tiny_waves())
    keys = [f"c{i}" for i in range(len(lens))]
    for mode in ("eval", "validation"):
        model.eval()
        torch.manual_seed(7); random.seed(7)
        feats, fl = fe(waves, lens)
        with torch.no_grad():
            want = model(feats, fl.copy(), method="greedy", max_length=8)
        torch.manual_seed(7); random.seed(7)
        batch = [keys, waves.clone(), lens.copy()]
        with torch.no_grad():
            got = B.forward_batch(model, batch, mode, frontend=fe, method="greedy", beam_size=1, max_length=8)
        assert torch.equal(got["seqs"], want["seqs"]), mode
        assert torch.equal(batch[1], feats) and len(batch[-1]) == len(lens), "batch slots not replaced"
    _, caps, _, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    model.train()
    model.encoder.p_block = model.encoder.p_fc = 0.0
    torch.manual_seed(9); random.seed(9)
    want = model(feats, fe.n_frames(lens), caps, cl, ss_ratio=1.0, dis_ratio=0)["logits"].detach()
    torch.manual_seed(9); random.seed(9)
    got = B.forward_batch(model, [waves.clone(), caps, keys, lens.copy(), cl], "train", frontend=fe, ss_ratio=1.0, dis_ratio=0)
    assert torch.equal(got["logits"].detach(), want)


@pytest.mark.parametrize("method,beam", [("greedy", 1), ("beam", 3)])
def test_evaluate_on_waveforms_matches_evaluate_on_their_features(method, beam):
    fe, model, voc = F.LogMel.panns_16k(), tiny_model(), vocab()
    waves = tiny_waves()
    wav_items = [(f"clip{i}", w) for i, w in enumerate(waves)]
    feat_items = [(k, fe(w[None], [len(w)])[0][0].cpu()) for k, w in wav_items]
    torch.manual_seed(4)
    want = EV.evaluate(model, feat_items, voc, method=method, beam_size=beam, max_length=8, batch_size=2)
    torch.manual_seed(4)
    got = EV.evaluate(model, wav_items, voc, method=method, beam_size=beam, max_length=8, batch_size=2, frontend=fe)
    assert got == want and len(got["predictions"]) == 3
    pcm_items = [(k, torch.from_numpy(np.rint(w.numpy() * 32768.0).astype(np.int16))) for k, w in wav_items]
    torch.manual_seed(4)
    a = EV.evaluate(model, pcm_items, voc, method=method, beam_size=beam, max_length=8, frontend=fe)
    torch.manual_seed(4)
    b = EV.evaluate(model, [(k, fe.to_float(w)) for k, w in pcm_items], voc, method=method, beam_size=beam, max_length=8,
                    frontend=fe)
    assert a == b


def test_ensemble_evaluate_on_waveforms():
    from acvae_amd.ensemble import ensemble_evaluate
    fe, models, voc = F.LogMel.panns_16k(), [tiny_model()], vocab()
    wav_items = [(f"clip{i}", w) for i, w in enumerate(tiny_waves())]
    feat_items = [(k, fe(w[None], [len(w)])[0][0].cpu()) for k, w in wav_items]
    torch.manual_seed(6)
    want = ensemble_evaluate(models, feat_items, voc, method="greedy", max_length=8, batch_size=2)
    torch.manual_seed(6)
    got = ensemble_evaluate(models, wav_items, voc, method="greedy", max_length=8, batch_size=2, frontend=fe)
    assert got == want


def test_train_step_on_waveforms_is_bit_equal_to_the_step_on_their_features():
    import acvae_oracle as O
    from acvae_amd.trainer import TrainStep
    fe = F.LogMel.panns_16k()
    waves, lens = padded(tiny_waves())
    _, caps, _, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    steps = []
    for _ in range(2):
        m = tiny_model().train()
        m.encoder.p_block = m.encoder.p_fc = 0.0
        steps.append((m, TrainStep(m, V)))
    (m1, t1), (m2, t2) = steps
    torch.manual_seed(3); random.seed(3)
    p1 = t1.step(waves.clone(), lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=fe)
    feats, fl = fe(waves, lens)
    torch.manual_seed(3); random.seed(3)
    p2 = t2.step(feats, fl, caps, cl, 1.0, 0, 0.5)
    t1.synchronize(); t2.synchronize()
    assert float(p1["loss"]) == float(p2["loss"]) and float(p1["grad_norm"]) == float(p2["grad_norm"])
    assert torch.equal(t1.flat_p, t2.flat_p), "parameters after one step differ"
    with pytest.raises(ValueError, match="augment"):
        t1.step(waves, lens.copy(), caps, cl, augment=[None] * 3, frontend=fe)


def test_prefetch_keeps_pageable_int16_waveforms_as_pcm():
    """prefetch() of a pageable int16 batch (what read_wav plus padding gives) followed by step(frontend=) is the step on the
    host int16 batch bit for bit: the PCM must not be cast to fp32 on the way (the kernel's 1/32768 scale would be lost)."""
    import acvae_oracle as O
    from acvae_amd.trainer import TrainStep
    fe = F.LogMel.panns_16k()
    waves, lens = padded(tiny_waves())
    pcm = torch.from_numpy(np.rint(waves.numpy() * 32768.0).astype(np.int16))
    assert not pcm.is_pinned()
    _, caps, _, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    steps = []
    for _ in range(2):
        m = tiny_model().train()
        m.encoder.p_block = m.encoder.p_fc = 0.0
        steps.append(TrainStep(m, V))
    t1, t2 = steps
    up = t1.prefetch(pcm)
    assert up.is_cuda and up.dtype == torch.int16
    torch.manual_seed(3); random.seed(3)
    p1 = t1.step(up, lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=fe)
    torch.manual_seed(3); random.seed(3)
    p2 = t2.step(pcm.clone(), lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=fe)
    t1.synchronize(); t2.synchronize()
    assert float(p1["loss"]) == float(p2["loss"]) and torch.equal(t1.flat_p, t2.flat_p)
    assert torch.equal(fe(up, lens)[0], fe(fe.to_float(pcm), lens)[0])
