"""GPU parity of the whole hot path (Hybrid_VAEModel forward -> CE + KL + MSE loss -> backward) against the
golden vectors generated from the reference (g6/g6b/g6c/g7/g8) and against the oracle's autograd for
every parameter gradient.  Token ids exact; loss |d| <= 1e-4 (north_star); tensors rtol 1e-4/atol 1e-5
where the summation order differs (hoisted attention, MFMA accumulation)."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
from acvae_amd.encoder import Cnn10, Cnn14_16k
from acvae_amd.train_util import LabelSmoothingLoss, MSELoss, Normal_kl_loss
from acvae_amd.vae_model import Hybrid_VAEModel
from conftest import load_golden, unpack_masks
from parity_util import close, grads_match_oracle

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def build_model(V, E, state=None, encoder="Cnn10", dec_dropout=0.0, proj_embed=0):
    enc = Cnn10(64, 512) if encoder == "Cnn10" else Cnn14_16k(64, 2048)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=dec_dropout,
                                    num_layers=1, rnn_type="GRU", attn_size=E)
    if proj_embed:                                  # runners/pytorch_runner_vae.py:51-56
        dec.load_word_embeddings(np.zeros((V, proj_embed), dtype=np.float32), tune=True, projection=True)
    m = Hybrid_VAEModel(enc, dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E, "dropout": 0.0},
                        prior_model="PriorRNN", prior_args={"hidden_size": E, "dropout": 0.0})
    if state is not None:
        m.load_state_dict({k: v.clone() for k, v in state.items()})
    return m.cuda()


def hip_loss(out, caps, cap_lens, V, smoothing=0.1, kl_weight=0.5, alpha=1.0):
    """runners/pytorch_runner_vae.py:315-318 with the HIP loss modules."""
    lens1 = np.asarray(cap_lens) - 1
    ce = LabelSmoothingLoss(V, smoothing).masked(out["logits"], caps[:, 1:].to(torch.long), lens1)
    kl = Normal_kl_loss()(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"])
    mse = MSELoss()(out["q_means_utt"], out["p_means_utt"])
    return ce + kl_weight * kl + alpha * mse, ce, kl, mse


def close_enc_grad(a, b, what=""):
    """Encoder gradients: tight unless a ReLU-boundary flip sits upstream (tests/test_encoder_gpu.py explains): one mask
    bit that differs between the MFMA and the CPU summation order moves every encoder gradient below it by up to ~1 %.
    Median error <= 0.2 % of max and relative L2 <= 2 %."""
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    mx = max(float(b.abs().max()), 1e-6)
    l2 = float(err.pow(2).sum().sqrt() / max(float(b.pow(2).sum().sqrt()), 1e-12))
    assert float(err.median()) <= 2e-3 * mx and l2 <= 2e-2, \
        f"{what}: median {float(err.median()):.2e} max {float(err.max()):.2e} (ref max {mx:.2e}) rel-L2 {l2:.2e}"


def close_grad_of(name, a, ref, what):
    if name.startswith("encoder."):
        close_enc_grad(a, ref, what)
    else:
        close(a, ref, 2e-3, 2e-4 * max(float(ref.abs().max()), 1e-3), what=what)


def run_case(name, tensors, full_grads, encoder="Cnn10", gn_tol=1e-3):
    g = load_golden(name)
    B, Tt, V, E, L = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    dec_p = float(g["dec_dropout"]) if "dec_dropout" in g else 0.0
    proj = int(g["proj_embed"]) if "proj_embed" in g else 0
    dec_keep = T(g["noise_dec_keep"]) if "noise_dec_keep" in g else None
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512 if encoder == "Cnn10" else 2048, encoder=encoder,
                                               proj_embed=proj or None))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, Tt, V, L, seed=seed, ragged=bool(int(g["ragged"])))
    dis = float(g["dis_ratio"])
    if "noise_eps_q" in g:
        masks = unpack_masks(g); eps_q = T(g["noise_eps_q"]); eps_p = T(g["noise_eps_p"])
        ores = None
    else:
        masks = eps_q = eps_p = None
    # With replayed noise nobody draws randn, so the generator position at each torch.rand(1) (dis_ratio) differs
    # from the reference's; recompute the reference's decisions and feed them to both oracle and HIP runs.
    flags = None
    if dis != 0 and masks is not None:
        flags = []
        torch.manual_seed(seed)
        for m_ in masks:
            torch.empty(m_.shape, dtype=torch.bool).bernoulli_(0.5)
        torch.randn(eps_q.shape)
        for t in range(eps_p.shape[0]):
            torch.randn(eps_p.shape[1:]); flags.append(bool(torch.rand(1) <= dis))
    orig_rand = torch.rand

    def patched(run):
        if flags is None:
            return run()
        it = iter(flags)
        torch.rand = lambda *a, **k: torch.tensor([0.0 if next(it) else 2.0])
        try:
            return run()
        finally:
            torch.rand = orig_rand

    # oracle run (CPU): supplies the noise when the fixture stores only a seed, and all gradients
    ostate = {k: v.clone() for k, v in state.items()}
    rec = {}
    torch.manual_seed(seed); random.seed(seed)
    noise = None if masks is None else dict(dropout=list(masks), eps_q=eps_q, eps_p=eps_p, dec_keep=dec_keep)
    ores = patched(lambda: O.OracleTrainer(ostate, V, dec_dropout=dec_p).step(feats, feat_lens.copy(), caps, cap_lens, 1.0,
                                                                            dis, noise=noise, record=rec,
                                                                            apply_update=False))
    if masks is None:
        masks, eps_q, eps_p = rec["dropout"], rec["eps_q"], rec["eps_p"]
    model = build_model(V, E, state, encoder, dec_dropout=dec_p, proj_embed=proj)
    model.train()
    model.encoder.dropout_masks = masks
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=eps_q, eps_p=eps_p, dec_keep=dec_keep)
    random.seed(seed)
    out = patched(lambda: model(feats.cuda(), feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=dis))
    loss, ce, kl, mse = hip_loss(out, caps, cap_lens, V)
    for k, v in (("loss", loss), ("ce", ce), ("kl", kl), ("mse", mse)):
        v = v.detach()
        assert abs(float(v) - float(g[k])) <= 1e-4 * max(1.0, abs(float(g[k]))), (k, float(v), float(g[k]))
    if tensors:
        assert np.array_equal(out["seqs"].cpu().numpy(), g["out_seqs"])
        for k in ("logits", "outputs", "attn_weights", "p_means", "p_logs", "p_z", "q_means", "q_logs", "q_z",
                  "q_means_utt", "p_means_utt", "sampled_logprobs"):
            close(out[k], g["out_" + k], 1e-4, 2e-5, what=k)
    loss.backward()
    named = dict(model.named_parameters())
    # the global norm is dominated by the encoder gradients: one ReLU-boundary flip (close_enc_grad) moves it by a few 1e-4
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None))
    assert abs(float(gn) - float(g["grad_norm"])) <= gn_tol * float(g["grad_norm"]), (float(gn), float(g["grad_norm"]))
    matched = None
    if full_grads:
        def under(force):
            st2 = {k: v.clone() for k, v in state.items()}
            n2 = dict(dropout=[m.clone() for m in masks], eps_q=eps_q, eps_p=eps_p, relu_force=force, dec_keep=dec_keep)
            random.seed(seed)
            return patched(lambda: O.OracleTrainer(st2, V, dec_dropout=dec_p).step(feats, feat_lens.copy(), caps, cap_lens, 1.0, dis, noise=n2,
                                                                apply_update=False))["grads"]
        matched = grads_match_oracle(model, named, ores["grads"], rec, under)
    if tensors:
        for k in [k for k in g if k.startswith("grad_") and k != "grad_norm"]:
            if matched is not None and matched is not ores["grads"] and k[5:].startswith("encoder."):
                continue      # a rounding-ambiguous ReLU bit fell the other way than in the reference run: checked above
            close_grad_of(k[5:], named[k[5:]].grad, T(g[k]), k)


def test_g6_train_step_golden():
    run_case("g6_train_step", tensors=True, full_grads=True)


def test_g16_train_step_with_projected_pretrained_embeddings_golden():
    """decoder.load_word_embeddings(vectors [V,24], tune=True, projection=True) (models/decoder.py:50-64, runner :51-56):
    word_embeddings = Sequential(Embedding(V,24), Linear(24,E)); same state-dict keys as the reference, outputs, loss and
    all gradients (incl. the three of the Sequential) against the reference's own training step (golden g16); and one
    TrainStep moves those parameters."""
    run_case("g16_train_step_projemb", tensors=True, full_grads=True)
    from acvae_amd.trainer import TrainStep
    g = load_golden("g16_train_step_projemb")
    B, Tt, V, E, L = (int(x) for x in g["dims"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512, proj_embed=24))
    model = build_model(V, E, state, proj_embed=24).train()
    assert list(model.state_dict().keys()) == list(state.keys())
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, Tt, V, L, seed=int(g["seed"]), ragged=True)
    ts = TrainStep(model, V)
    before = {k: v.clone() for k, v in model.state_dict().items() if "word_embeddings" in k}
    torch.manual_seed(1); random.seed(1)
    parts = ts.step(feats.cuda(), feat_lens.copy(), caps, cap_lens, 1.0, 0, 0.5)
    torch.cuda.synchronize()
    assert torch.isfinite(parts["loss"])
    for k, v in before.items():
        assert not torch.equal(v, model.state_dict()[k]), k


def test_g15_train_step_with_decoder_embedding_dropout_golden():
    """VAERNNBahdanauAttnDecoder(dropout=0.3): nn.Dropout on the word embedding (models/decoder.py:33,184) inside the
    fused decode loop, forward and backward, against the reference's own training step (golden g15: outputs, loss,
    gradients) with the masks that run drew; and the host's own draws follow the reference's generator order."""
    run_case("g15_train_step_decdrop", tensors=True, full_grads=True)
    g = load_golden("g15_train_step_decdrop")
    B, Tt, V, E, L = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, Tt, V, L, seed=seed, ragged=True)
    model = build_model(V, E, state, dec_dropout=0.3).train()
    masks = unpack_masks(g)
    model.encoder.dropout_masks = masks
    torch.manual_seed(seed); random.seed(seed)
    for m_ in masks:                                  # the reference drew its encoder dropout masks first
        torch.empty(m_.shape, dtype=torch.bool).bernoulli_(0.5)
    with torch.no_grad():
        out = model(feats.cuda(), feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0)
    close(out["logits"], g["out_logits"], 1e-4, 2e-5, what="logits with self-drawn masks")


def test_g6b_train_step_prior_z_golden():
    run_case("g6b_train_step_dis", tensors=True, full_grads=True)


def test_g6c_train_step_e512_golden():
    run_case("g6c_train_step_e512", tensors=False, full_grads=True)


def test_g13_train_step_cnn14_with_ln_golden():
    """N4: Cnn14_16k encoder + the ln 2048 -> E projection through the whole training step (loss triplet and gradient
    norm pinned by the reference; blocks 5/6 normalise over 16 / 8 values at this size, hence the looser norm bound)."""
    run_case("g13_train_step_cnn14", tensors=False, full_grads=False, encoder="Cnn14_16k", gn_tol=2e-3)


def test_g8_config1_scalars_golden():
    # BASELINE config 1 shape [8,500,64], V=5000, E=512: loss triplet + grad norm pinned by the reference
    run_case("g8_config1_scalars", tensors=False, full_grads=False)


def test_g7_greedy_decode_token_exact():
    g = load_golden("g7_decode")
    _, _, V, E = (int(x) for x in g["dims"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    model = build_model(V, E, state)
    model.eval()
    for tag, rep in (("greedy1", 1), ("greedy5", 5)):
        f = T(g["feats"]).repeat(rep, 1, 1).cuda()
        model.noise = dict(eps_p=T(g[tag + "_noise_eps_p"]))
        with torch.no_grad():
            o = model(f, list(g[tag + "_lens"]), method="greedy", beam_size=rep)
        assert np.array_equal(o["seqs"].cpu().numpy(), g[tag + "_seqs"]), tag
        close(o["logits"][:, 0], g[tag + "_logits0"], 1e-4, 2e-5, what=tag + " logits0")


def test_g14_sampling_methods_token_exact():
    """A6: method="sample" (multinomial with temp) and method="gumbel" of sample_next_word (models/word_model.py:188-203)
    through Hybrid_VAEModel.forward(feats, feat_lens, method=, temp=) against the REFERENCE's own token ids and
    log-probabilities (golden g14), replaying the noise that run drew."""
    g = load_golden("g14_sampling")
    _, _, V, E = (int(x) for x in g["dims"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    model = build_model(V, E, state)
    model.eval()
    for tag, method in zip(g["cases"], g["methods"]):
        a, b = (int(x) for x in g[tag + "_clips"])
        lens = g["feat_lens"][a:b].copy()
        f = T(g["feats"])[a:b, :int(lens.max())].contiguous().cuda()
        model.noise = dict(eps_p=T(g[tag + "_noise_eps_p"]), sample_noise=T(g[tag + "_sample_noise"]))
        with torch.no_grad():
            o = model(f, lens, method=str(method), temp=float(g[tag + "_temp"]))
        assert np.array_equal(o["seqs"].cpu().numpy(), g[tag + "_seqs"]), tag
        steps = int(g[tag + "_steps_run"])
        close(o["sampled_logprobs"][:, :steps], g[tag + "_logprobs"], 1e-4, 2e-5, what=tag)


def test_sampling_draws_follow_the_reference_generator_order():
    """Without replayed noise the host draws eps and the per-step [N,V] sampling noise on the CPU generator in the
    reference's order (prior randn, then torch.rand / exponential_ of sample_next_word): same seed -> the oracle's
    tokens, for inference and for a scheduled-sampling training forward with method="sample"."""
    V, E = 40, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(3, 96, V, 6, seed=5, ragged=False)
    model = build_model(V, E, state)
    model.eval()
    for method, temp in (("sample", 0.8), ("gumbel", 1.3)):
        torch.manual_seed(21)
        with torch.no_grad():
            oo = O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, feat_lens.copy(), training=False,
                                  method=method, temp=temp)
        torch.manual_seed(21)
        with torch.no_grad():
            o = model(feats.cuda(), feat_lens.copy(), method=method, temp=temp)
        n = oo["_steps_run"]
        assert np.array_equal(o["seqs"].cpu().numpy()[:, :n], oo["seqs"].numpy()[:, :n]), method
    # training forward, ss_ratio < 1: the sampled word of step t-1 is fed at step t when the coin says so
    rec = {}
    torch.manual_seed(22); random.seed(22)
    with torch.no_grad():
        oo = O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, feat_lens.copy(), caps, cap_lens,
                              ss_ratio=0.5, dis_ratio=0, method="sample", temp=0.9, record=rec)
    model.train()
    model.encoder.dropout_masks = rec["dropout"]
    torch.manual_seed(22); random.seed(22)
    for m_ in rec["dropout"]:                       # the oracle drew its dropout masks first: keep the generator aligned
        torch.empty(m_.shape, dtype=torch.bool).bernoulli_(0.5)
    with torch.no_grad():
        out = model(feats.cuda(), feat_lens.copy(), caps, cap_lens, ss_ratio=0.5, dis_ratio=0, method="sample", temp=0.9)
    assert np.array_equal(out["seqs"].cpu().numpy(), oo["seqs"].numpy())
    close(out["sampled_logprobs"], oo["sampled_logprobs"], 1e-4, 2e-5, what="sampled_logprobs")


def test_scheduled_sampling_forward_vs_oracle():
    # ss_ratio < 1: the word fed at step t may be the previous argmax (device-side select, no host sync)
    V, E, B, Tt, L = 40, 64, 3, 96, 6
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, Tt, V, L, seed=3, ragged=True)
    rec = {}
    torch.manual_seed(11); random.seed(11)
    with torch.no_grad():
        oo = O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, feat_lens.copy(), caps, cap_lens,
                              ss_ratio=0.6, dis_ratio=0, record=rec)
    model = build_model(V, E, state)
    model.train()
    model.encoder.dropout_masks = rec["dropout"]
    model.noise = dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"])
    random.seed(11)
    with torch.no_grad():
        out = model(feats.cuda(), feat_lens.copy(), caps, cap_lens, ss_ratio=0.6, dis_ratio=0)
    assert np.array_equal(out["seqs"].cpu().numpy(), oo["seqs"].numpy())
    for k in ("logits", "p_means", "p_z", "p_means_utt", "attn_weights"):
        close(out[k], oo[k], 1e-4, 2e-5, what=k)


def test_g9_beam_search_token_exact():
    """N1: validation beam search (beam_size=3) against the reference's own output."""
    g = load_golden("g9_beam")
    _, _, V, E, beam = (int(x) for x in g["dims"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    model = build_model(V, E, state)
    model.eval()
    model.noise = dict(eps_beam=T(g["eps"]))
    with torch.no_grad():
        o = model(T(g["feats"]).cuda(), g["feat_lens"].copy(), method="beam", beam_size=beam)
    assert np.array_equal(o["seqs"].cpu().numpy(), g["seqs"])


def test_beam_search_call_equals_the_step_api_loop():
    """The one-call beam search against the reference's loop written with the sub-module step API (PriorRNN.forward /
    decoder.forward per step, state and history re-gathered by prev_word_inds every step, vae_model.py:905-921,961-979)
    on a ragged batch: same tokens and the same attention-weight history, bit for bit.  Also at full size (V=5000, beam 5 on
    9 clips: R = 45 rows, past the skinny GEMMs' 32-row tile and with top-k over 25 000 scores per clip), which ties the
    one-call search to the step API that tests/test_fullsize_decode_gpu.py checks against the oracle."""
    _beam_call_vs_step_loop(V=300, beam=3, ml=12, feat_lens=[160, 150, 97, 64, 33], seed=3)
    _beam_call_vs_step_loop(V=5000, beam=5, ml=20, feat_lens=[160, 160, 150, 131, 97, 97, 64, 48, 33], seed=4)


_step_loops = {}


def _beam_call_vs_step_loop(V, beam, ml, feat_lens, seed):
    """Returns what it computed (once per case; tests/test_ensemble_gpu.py holds the ensemble entry against the same loop)."""
    from acvae_amd import _lib
    key = (V, beam, ml, tuple(feat_lens), seed)
    if key in _step_loops:
        return _step_loops[key]
    E = 512
    torch.manual_seed(seed)
    model = build_model(V, E)
    model.eval()
    feats = torch.randn(len(feat_lens), max(feat_lens), 64)
    feat_lens = np.array(feat_lens)
    eps = torch.randn(len(feat_lens), ml, beam, E)
    with torch.no_grad():
        enc = model.encoder(feats.cuda(), feat_lens.copy())
        model.noise = dict(eps_beam=eps)
        got = model.beam_search(dict(enc), ml, beam)
        mem1, lens1 = enc["audio_embeds"].contiguous(), torch.as_tensor(enc["audio_embeds_lens"])
        N, S, _ = mem1.shape
        R = N * beam
        mem = mem1.repeat_interleave(beam, dim=0).contiguous()
        lens = lens1.repeat_interleave(beam)
        state = model.decoder.init_hidden(R).cuda()
        hid = model.pnet.init_hidden(R, "cuda")
        last_z = torch.zeros(R, E, device="cuda")
        top_k = torch.zeros(R, device="cuda")
        seqs = attw = None
        w = torch.full((R,), model.start_idx, dtype=torch.long, device="cuda")
        for t in range(ml):
            pn = model.pnet(w.unsqueeze(1), mem, hid, last_z, lens, eps=eps[:, t].reshape(R, E))
            dn = model.decoder(word=w.unsqueeze(1), state=state, enc_mem=mem, enc_mem_lens=lens, z=pn["z"])
            logits = dn["logits"].squeeze(1).contiguous()
            lse, scores, vals = torch.empty(R, device="cuda"), torch.empty(R, V, device="cuda"), torch.empty(R, device="cuda")
            idx, prev, w = (torch.empty(R, dtype=torch.long, device="cuda") for _ in range(3))
            st = _lib.current_stream()
            _lib.call("acvae_row_logsoftmax_argmax", logits, V, V, None, None, lse, 1, 1, R, 1, V, st)
            _lib.call("acvae_logprob_add", logits, V, lse, top_k, scores, R, V, st)
            _lib.call("acvae_topk_flat_batched", scores, beam * V, beam * V, beam, V, vals, idx, prev, w, N, beam, st)
            top_k = vals
            seqs = w.unsqueeze(1) if t == 0 else torch.cat([seqs[prev], w.unsqueeze(1)], dim=1)
            w_t = dn["weights"].unsqueeze(2)
            attw = (w_t if t == 0 else torch.cat([attw, w_t], dim=2))[prev]
            state = dn["state"][:, prev].contiguous()
            hid = (pn["hiddens_state"][0][:, prev].contiguous(), pn["hiddens_state"][1][:, prev].contiguous())
            last_z = pn["z"][prev].contiguous()
    assert np.array_equal(got["seqs"].cpu().numpy(), seqs[0::beam].cpu().numpy())
    assert torch.equal(got["attn_weights"].cpu(), attw[0::beam].cpu())
    assert got["attn_weights"].shape == (N, S, ml)
    _step_loops[key] = dict(model=model, feats=feats, feat_lens=feat_lens, eps=eps, seqs=seqs, attw=attw, top_k=top_k)
    return _step_loops[key]


DBS_CASES = [dict(beam_size=4, group_size=2), dict(beam_size=6, group_size=3, diversity_lambda=0.8, temperature=1.5,
             group_nbest=False), dict(), dict(beam_size=6, group_size=2, diversity_lambda=2.0)]


def test_g11_diverse_beam_search_token_exact():
    """N3: diverse beam search against the reference's own output (golden g11), incl. beams that finish early."""
    g = load_golden("g11_dbs")
    _, _, V, E, ML = (int(x) for x in g["dims"])
    for tag, bump in zip("ab", g["end_bump"]):
        state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
        state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
        state["decoder.classifier.bias"][O.END_IDX] += float(bump)
        model = build_model(V, E, state).eval()
        for ci, kw in enumerate(DBS_CASES):
            torch.manual_seed(40 + ci)          # the prior's randn draws come from the CPU generator in call order (F9)
            with torch.no_grad():
                o = model(T(g["feats"]).cuda(), g["feat_lens"].copy(), method="dbs", max_length=ML, **kw)
            assert np.array_equal(o["seqs"].cpu().numpy(), g[f"seqs_{tag}{ci}"]), (tag, kw)


def test_dbs_scores_kernel_vs_torch():
    from acvae_amd import _lib
    g = torch.Generator().manual_seed(9)
    N, V = 5, 5000
    logits = (torch.randn(N, V, generator=g) * 3).cuda()
    counts = torch.randint(0, 3, (V,), generator=g).float().cuda()
    prev = torch.randn(N, generator=g).cuda()
    out = torch.empty(N, V, device="cuda")
    for temp, lam, cnt, pv in ((1.0, 0.5, counts, prev), (1.7, 2.0, counts, None), (0.6, 0.0, None, prev)):
        _lib.call("acvae_dbs_scores", logits, V, temp, cnt, lam, pv, out, N, V, 0, _lib.current_stream())
        want = torch.log_softmax(torch.log_softmax(logits.cpu(), 1) / temp, 1)
        if cnt is not None:
            want = want - cnt.cpu() * lam
        if pv is not None:
            want = want + pv.cpu()[:, None]
        close(out, want, 1e-5, 1e-5, what=f"dbs scores T={temp}")


def test_single_step_modules_vs_oracle():
    """A4/A5 per-call API: pnet.forward / decoder.forward one step at a time."""
    V, E, N, S = 40, 64, 5, 9
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    model = build_model(V, E, state).eval()
    g = torch.Generator().manual_seed(2)
    mem = torch.randn(N, S, E, generator=g); lens = torch.tensor([9, 7, 4, 2, 1])
    word = torch.randint(0, V, (N, 1), generator=g)
    h = torch.randn(1, N, E, generator=g); hp = torch.randn(1, N, E, generator=g); cp = torch.randn(1, N, E, generator=g)
    lz = torch.randn(N, E, generator=g); eps = torch.randn(N, E, generator=g)
    with torch.no_grad():
        op = O.prior_step(state, word, mem, (hp[0], cp[0]), lz, lens, eps)
        od = O.decoder_step(state, word, h[0], mem, lens, op["z"])
        hp_ = model.pnet(word, mem.cuda(), (hp.cuda(), cp.cuda()), lz.cuda(), lens, eps=eps)
        hd_ = model.decoder(word=word, state=h.cuda(), enc_mem=mem.cuda(), enc_mem_lens=lens, z=hp_["z"])
    close(hp_["mean"], op["mean"], what="prior mean"); close(hp_["z"], op["z"], what="prior z")
    close(hp_["hiddens_state"][0][0], op["hiddens_state"][0], what="prior h")
    close(hp_["hiddens_state"][1][0], op["hiddens_state"][1], what="prior c")
    close(hd_["logits"][:, 0], od["logits"], 1e-4, 2e-5, what="dec logits"); close(hd_["state"][0], od["state"], what="dec h")
    close(hd_["weights"], od["weights"], what="dec attn"); close(hd_["rnn_input"][:, 0], od["rnn_input"], what="rnn_input")


@pytest.mark.parametrize("B,Tt,L,lens,flens", [
    (1, 90, 5, [5], [90]),                       # batch of one, odd sizes through every pool (90->45->22->11->5)
    (3, 250, 6, [6, 2, 2], [250, 17, 15]),       # captions of only <start><end>; a clip shorter than one encoder frame
    (2, 16, 4, [4, 3], [16, 16]),                # minimum audio length (S = 1)
])
def test_edge_shapes_vs_oracle(B, Tt, L, lens, flens):
    V, E = 44, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    g = torch.Generator().manual_seed(B * 1000 + Tt + 1)
    feats = torch.randn(B, Tt, 64, generator=g)
    caps = torch.zeros(B, L)
    for b, n in enumerate(lens):
        caps[b, 0] = 1; caps[b, n - 1] = 2
        if n > 2:
            caps[b, 1:n - 1] = torch.randint(4, V, (n - 2,), generator=g).float()
    cl, fl = np.array(lens), np.array(flens)
    ostate = {k: v.clone() for k, v in state.items()}
    rec = {}
    torch.manual_seed(3); random.seed(3)
    ores = O.OracleTrainer(ostate, V).step(feats, fl.copy(), caps, cl, 1.0, 0, record=rec, apply_update=False)
    model = build_model(V, E, state)
    model.train()
    model.encoder.dropout_masks = rec["dropout"]
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"])
    random.seed(3)
    out = model(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
    loss, ce, kl, mse = hip_loss(out, caps, cl, V)
    assert abs(float(loss.detach()) - float(ores["loss"])) <= 1e-4 * max(1.0, abs(float(ores["loss"])))
    assert np.array_equal(out["seqs"].cpu().numpy(), ores["out"]["seqs"].numpy())
    for k in ("logits", "attn_weights", "p_means", "q_means", "q_means_utt", "p_means_utt"):
        close(out[k], ores["out"][k], 1e-4, 2e-5, what=k)
    loss.backward()
    named = dict(model.named_parameters())
    def under(force):
        st2 = {k: v.clone() for k, v in state.items()}
        n2 = dict(dropout=[m.clone() for m in rec["dropout"]], eps_q=rec["eps_q"], eps_p=rec["eps_p"], relu_force=force)
        random.seed(3)
        return O.OracleTrainer(st2, V).step(feats, fl.copy(), caps, cl, 1.0, 0, noise=n2, apply_update=False)["grads"]
    grads_match_oracle(model, named, ores["grads"], rec, under)


def test_g6_trainstep_against_the_reference_adam_step():
    """TrainStep.step (forward, loss, backward, clip_grad_norm_(1.0), Adam lr 5e-4) on the g6 batch against the state
    the REFERENCE model held after its own optimiser step (golden post_*: three parameters, two BatchNorm running
    buffers).  Adam's first step moves an element by lr * g / (|g| + 1e-8): the tolerance of an element is 2e-6 plus
    the first-order effect of the gradient's own tolerance on that quotient (capped at 2 lr: elements whose gradient is
    at the 1e-8 level may land anywhere within the step); the running statistics agree to rtol 1e-5."""
    from acvae_amd.trainer import TrainStep
    g = load_golden("g6_train_step")
    B, Tt, V, E, L = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, Tt, V, L, seed=seed, ragged=bool(int(g["ragged"])))
    model = build_model(V, E, state).train()
    model.encoder.dropout_masks = unpack_masks(g)
    model.noise = dict(eps_q=T(g["noise_eps_q"]), eps_p=T(g["noise_eps_p"]))
    ts = TrainStep(model, V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0)
    random.seed(seed)
    parts = ts.step(feats.cuda(), feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
    assert abs(float(parts["loss"]) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    assert abs(float(parts["grad_norm"]) - float(g["grad_norm"])) <= 1e-3 * float(g["grad_norm"])
    coef = min(1.0, 1.0 / (float(parts["grad_norm"]) + 1e-6))
    sd = model.state_dict()
    named = dict(model.named_parameters())
    checked = 0
    for k in [k for k in g if k.startswith("post_")]:
        name, ref = k[5:], T(g[k]).double()
        got = sd[name].detach().cpu().double()
        if name in named:
            # first Adam step: u = lr * g / (|g| + 1e-8)  ->  |du| = lr * 1e-8 * |dg| / (|g| + 1e-8)^2, with the
            # gradient itself known to 2e-4 of the tensor's max (1e-2 for encoder tensors, whose gradients can carry a
            # ReLU-boundary flip: the gradient tolerances of the tests above)
            gr = named[name].grad.detach().cpu().double().abs() * coef
            dg = (1e-2 if name.startswith("encoder.") else 2e-4) * float(gr.max())
            # (the derivative is taken at the point of the interval [|g| - dg, |g| + dg] nearest zero; an element whose
            # gradient is smaller than its own uncertainty may land anywhere within the step)
            near = torch.clamp(gr - dg, min=0.0)
            tol = 2e-6 + torch.where(gr > dg, torch.clamp(ts.lr * 1e-8 * dg / (near + 1e-8) ** 2, max=2.1 * ts.lr),
                                     torch.full_like(gr, 2.1 * ts.lr))
            err = (got - ref).abs()
            assert bool((err <= tol).all()), (name, float((err / tol).max()), float(err.max()))
            assert float((tol <= 4e-6).double().mean()) > 0.5, (name, "most elements must be pinned tightly")
            assert float((got - state[name].double()).abs().max()) > 0.5 * ts.lr      # the step was taken at all
        else:
            close(got, ref, 1e-5, 1e-7, what=name)
        checked += 1
    assert checked == 5


def test_two_host_threads_two_streams_share_nothing():
    """Re-entrancy of the two-stream calls (include/acvae_hip.h, "Mutable state"): two host threads, each with its own
    model, its own pair of HIP streams and its own batch, run teacher-forced training forwards (acvae_decode_fwd forks
    the prior chain onto the side stream and joins it with events from the per-thread pool) at the same time; each
    must reproduce, bit for bit, what it computes alone."""
    import threading
    V, E = 40, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    jobs = []
    for i in range(2):
        feats, caps, fl, cl = O.synthetic_batch(3, 64, V, 7, seed=30 + i, ragged=True)
        m = build_model(V, E, state).train()
        m.encoder.p_block = m.encoder.p_fc = 0.0
        g = torch.Generator().manual_seed(40 + i)
        noise = dict(eps_q=torch.randn(3, 6, E, generator=g), eps_p=torch.randn(6, 3, E, generator=g))
        jobs.append((m, feats.cuda(), caps, fl, cl, noise, torch.cuda.Stream()))

    def run(job, out, idx, reps):
        m, feats, caps, fl, cl, noise, stream = job
        res = []
        with torch.cuda.stream(stream), torch.no_grad():
            for _ in range(reps):
                m.noise = dict(noise)
                random.seed(1)
                o = m(feats, fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
                res.append((o["logits"].clone(), o["p_z"].clone(), o["seqs"].clone()))
        stream.synchronize()
        out[idx] = res

    alone = [None, None]
    for i in range(2):
        run(jobs[i], alone, i, 1)
    both = [None, None]
    ths = [threading.Thread(target=run, args=(jobs[i], both, i, 20)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for i in range(2):
        for rep in both[i]:
            for a, b in zip(rep, alone[i][0]):
                assert torch.equal(a, b), f"thread {i}: result differs from its single-threaded run"


def test_adam_leaves_parameters_without_gradient_alone():
    """torch.optim.Adam skips a parameter whose .grad is None (no moment decay, no update); the fused flat-buffer pass
    must do the same (it then runs over the segments between such parameters)."""
    from acvae_amd.trainer import TrainStep
    assert TrainStep._segments([], 100) == [(0, 100)]
    assert TrainStep._segments([(0, 8), (40, 48)], 100) == [(8, 40), (48, 100)]
    assert TrainStep._segments([(92, 100)], 100) == [(0, 92)]
    V, E = 40, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, fl, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    model = build_model(V, E, state).train()
    ts = TrainStep(model, V)
    victim = model.decoder.attn.v
    other = model.decoder.classifier.bias

    def one():
        torch.manual_seed(3); random.seed(3)
        return ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)

    one()                                               # step 1: everybody has a gradient, moments become non-zero
    v_before, o_before = victim.detach().clone(), other.detach().clone()
    off = ts._offsets()[victim]
    m_before = ts.exp_avg[off:off + victim.numel()].clone()
    orig = ts._check_grad_aliasing

    def drop_then_check():
        victim.grad = None                              # as if this parameter had not taken part in the step
        return orig()
    ts._check_grad_aliasing = drop_then_check
    one()
    torch.cuda.synchronize()
    assert torch.equal(victim.detach(), v_before), "a parameter without gradient was moved"
    assert torch.equal(ts.exp_avg[off:off + victim.numel()], m_before), "its first moment decayed"
    assert not torch.equal(other.detach(), o_before)


def test_checkpoint_round_trip_and_torch_adam_compat():
    """{"model", "optimizer"} checkpoint in the reference's format: resuming from it continues bit for bit, and a
    torch.optim.Adam over the same parameters accepts the optimiser part (it takes the same second step)."""
    import io
    from acvae_amd.trainer import TrainStep
    V, E = 40, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, fl, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)

    def fresh():
        m = build_model(V, E, state).train()
        m.encoder.p_block = m.encoder.p_fc = 0.0
        return m, TrainStep(m, V)

    def one(ts):
        torch.manual_seed(3); random.seed(3)
        return ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)

    m1, t1 = fresh()
    one(t1)
    buf = io.BytesIO()
    torch.save({"model": m1.state_dict(), "optimizer": t1.optimizer_state_dict()}, buf)
    one(t1)                                                   # second step, uninterrupted
    ck = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    assert list(ck["model"].keys()) == list(state.keys())
    m2, t2 = fresh()
    m2.load_state_dict(ck["model"])
    t2.load_optimizer_state_dict(ck["optimizer"])
    assert t2.step_count == 1
    one(t2)                                                   # second step after the restore
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    # torch.optim.Adam over the parameters of the restored model takes the checkpoint and the same step
    m3, t3 = fresh()
    m3.load_state_dict(ck["model"])
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    opt.load_state_dict(ck["optimizer"])
    torch.manual_seed(3); random.seed(3)
    loss, _, _ = t3.forward_loss(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    loss.backward()
    torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], 1.0)
    opt.step()
    for (k, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
        if b.grad is not None:
            close(b, a, 1e-5, 1e-6, what="torch Adam vs fused " + k)


def test_train_step_goldens_without_trailing_parameter_gradients():
    """Hybrid_VAEModel lets acvae_decode_bwd leave the parameter gradients and d_q_z on the second stream, joined at the end
    of the backward pass (what every other test in this file runs with).  ACVAE_DECODE_DEFER=0 keeps everything on the main
    stream - the library's own default for plain C callers: the training-step goldens and the ragged edge shapes must hold
    that way too.  The model reads the switch when it is built, the library keeps it per process, hence the child process."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, ACVAE_DECODE_DEFER="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "g6 or g13 or edge_shapes or checkpoint"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


def test_device_rng_sampling_noise_distribution_and_word_frequencies():
    """rng="device" (opt-in): acvae_sample_noise fills the noise with a counter-based generator on the GPU instead of the
    CPU generator.  Not the reference's stream, so the checks are statistical, at significance 1e-6 (a correct generator
    fails them once in a million seeds; the seed is fixed): (1) Kolmogorov-Smirnov of 1M draws against Gumbel(0,1) / Exp(1),
    (2) chi-square of the words acvae_sample_next_word picks with that noise against softmax(logits) (gumbel; the temp
    divides all scores alike) and softmax(logits / temp) (multinomial), (3) seeds and offsets give different streams and
    the same seed the same one."""
    from scipy import stats
    from acvae_amd import _lib
    n = 1 << 20
    for code, dist in ((1, stats.gumbel_r), (2, stats.expon)):
        z = torch.empty(n + 3, device="cuda")                      # + 3: the tail that is not a multiple of four
        _lib.call("acvae_sample_noise", z, z.numel(), code, 1234, _lib.current_stream())
        z2 = torch.empty_like(z)
        _lib.call("acvae_sample_noise", z2, z2.numel(), code, 1234, _lib.current_stream())
        assert torch.equal(z, z2)
        _lib.call("acvae_sample_noise", z2, z2.numel(), code, 1235, _lib.current_stream())
        assert float((z == z2).float().mean()) < 1e-3
        zz = z.cpu().double().numpy()
        assert np.isfinite(zz).all()
        assert stats.kstest(zz, dist.cdf).pvalue > 1e-6, (code, stats.kstest(zz, dist.cdf))
        assert abs(np.corrcoef(zz[:-1], zz[1:])[0, 1]) < 5e-3       # neighbours (same Philox block) uncorrelated
    V, rows, temp = 24, 200000, 0.7
    g = torch.Generator().manual_seed(3)
    logits1 = torch.randn(V, generator=g) * 1.5
    logits = logits1.expand(rows, V).contiguous().cuda()
    for code, p in ((1, torch.softmax(logits1.double(), 0)), (2, torch.softmax(logits1.double() / temp, 0))):
        z = torch.empty(rows, V, device="cuda")
        _lib.call("acvae_sample_noise", z, z.numel(), code, 99, _lib.current_stream())
        w = torch.empty(rows, dtype=torch.long, device="cuda"); lp = torch.empty(rows, device="cuda")
        _lib.call("acvae_sample_next_word", logits, V, 0, z, V, 0, code, temp, w, lp, 1, 0, rows, 1, V, _lib.current_stream())
        cnt = np.bincount(w.cpu().numpy(), minlength=V).astype(np.float64)
        assert stats.chisquare(cnt, p.numpy() * rows).pvalue > 1e-6, (code, cnt, p * rows)
        close(lp, torch.log_softmax(logits1, 0)[w.cpu()], 1e-5, 1e-5, what="logprob of the sampled word")
        # and against the parity mode itself: 10k words from host-drawn noise (the reference's draws) next to 10k from
        # the device noise - a 2 x V homogeneity test of the two token histograms
        k = 10000
        torch.manual_seed(5)
        zh = (-torch.log(-torch.log(torch.rand(k, V) + 1e-20) + 1e-20)) if code == 1 else torch.empty(k, V).exponential_(1)
        wh = torch.empty(k, dtype=torch.long, device="cuda")
        _lib.call("acvae_sample_next_word", logits, V, 0, zh.cuda(), V, 0, code, temp, wh, lp, 1, 0, k, 1, V, _lib.current_stream())
        table = np.stack([np.bincount(wh.cpu().numpy(), minlength=V), np.bincount(w[:k].cpu().numpy(), minlength=V)])
        table = table[:, table.sum(0) > 0]
        assert stats.chi2_contingency(table)[1] > 1e-6, (code, table)


def test_device_rng_forward_is_seeded_by_the_torch_generator():
    """Hybrid_VAEModel.forward(..., method="sample", rng="device"): one CPU-generator draw seeds the device noise, so
    torch.manual_seed still fixes the captions; another seed gives other captions; the default stays the host stream."""
    V, E = 40, 64
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, _, feat_lens, _ = O.synthetic_batch(4, 96, V, 6, seed=5, ragged=False)
    model = build_model(V, E, state)
    model.eval()
    outs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        with torch.no_grad():
            outs.append(model(feats.cuda(), feat_lens.copy(), method="sample", temp=1.0, rng="device"))
    assert torch.equal(outs[0]["seqs"], outs[1]["seqs"])
    assert not torch.equal(outs[0]["seqs"], outs[2]["seqs"])
    assert int(outs[0]["seqs"].min()) >= 0 and int(outs[0]["seqs"].max()) < V
    with pytest.raises(ValueError):
        model(feats.cuda(), feat_lens.copy(), method="sample", rng="gpu")


def test_prefetched_feature_batches_give_the_same_steps():
    """TrainStep.prefetch uploads a later step's feature batch on a copy stream while the current step runs (the
    `feats = batch[0].to(device)` of Runner._forward, runners/pytorch_runner_vae.py:80, taken off the critical path): three
    optimiser steps fed that way - from page-locked and from pageable host memory - end in parameters bit-identical to three
    steps on tensors uploaded up front."""
    from acvae_amd.trainer import TrainStep
    V, E, B, Tt, L = 60, 64, 4, 96, 8
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    batches = [O.synthetic_batch(B, Tt, V, L, seed=20 + i, ragged=True) for i in range(3)]
    g = torch.Generator().manual_seed(5)
    noise = [dict(eps_q=torch.randn(B, L - 1, E, generator=g), eps_p=torch.randn(L - 1, B, E, generator=g)) for _ in range(3)]

    def run(mode):
        model = build_model(V, E, state).train()
        model.encoder._seed_base, model.encoder._calls = 5, 0
        ts = TrainStep(model, V)
        hosts = [b[0].pin_memory() if mode == "pinned" else b[0].clone() for b in batches]
        nxt = ts.prefetch(hosts[0]) if mode != "resident" else None
        for i, (feats, caps, fl, cl) in enumerate(batches):
            if mode == "resident":
                cur = feats.cuda()
            else:
                cur, nxt = nxt, (ts.prefetch(hosts[i + 1]) if i + 1 < len(batches) else None)
                assert cur.is_cuda and getattr(cur, "_acvae_ready", None) is not None
            model.noise = dict(noise[i])
            random.seed(7 + i)
            parts = ts.step(cur, fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
        ts.synchronize()
        return {k: v.detach().clone() for k, v in model.state_dict().items()}, float(parts["loss"])

    ref, ref_loss = run("resident")
    for mode in ("pinned", "pageable"):
        got, loss = run(mode)
        assert loss == ref_loss, (mode, loss, ref_loss)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (mode, k)
