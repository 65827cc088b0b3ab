"""GPU: self-critical sequence training on the HIP path - the differentiable rollout (acvae_decode_fwd_sampled with
ACVAE_FLAG_ROLLOUT_GRAD, acvae_decode_bwd on its `saved`), the policy-gradient loss (acvae_scst_loss_fwd /
acvae_logprob_bwd), ScstWrapper / NScstWrapper, scst_Loss / Nscst_Loss and TrainStep.scst_step.

Against the reference's own values (tests/golden/g18_scst.npz: forward only, the reference cannot differentiate this loss
under current torch) and, for the gradients, against the oracle by the method of tests/test_sched_sampling_gpu.py: the
oracle's natural step first (scst_util.natural_step: it draws dropout masks, eps, sampling noise and records margins), the
HIP wrapper on that noise, then the oracle once more fed the HIP path's words (noise["fed_words"]) so that both
differentiate the same graph; then the loss, EVERY parameter gradient (grads_match_oracle with its bounds as they are; the
posterior, mean_log_out and the encoder's pooled head must hold None), and the HIP words decision by decision
(words_match_by_margin as it is).  A case whose oracle, fed the HIP words, does not finish its rows at the same steps fails.

Seeds: every case below was first run with the oracle alone on the CPU (scst_util.natural_step); a seed is taken only if
under 5 % of its live decisions have a margin below 2e-4.  Shares left out at 2e-4, live decisions, smallest margin, rows
that finish before the last step, per case:
  multinomial_t10 (seed 31)  0 % of 39, 2.1e-2, row 0 at step 8        gumbel_t09 (32)       0 % of 50, 1.9e-3, none
  multinomial_t07 (33)       0 % of 50, 3.7e-2, none                   gumbel_t12 (33)       0 % of 40, 4.2e-2, none
  decdrop (32)               0 % of 26, 5.4e-3, rows 1 / 2 at 0 / 4    end_at_step0 (31)     0 % of 30, 1.4e-1, row 3 at 0, rows 0 / 1 at 8 / 9
  e512 (31)                  0 % of 20, 9.9e-3, none                   cnn14_ln (32)         0 % of 30, 6.5e-3, none
  sample_n5 (31)             0 % of 136, 1.0e-2, rows 10 / 14 at 0 / 4 rows165 (31)          0 % of 1576, 2.4e-4, 21 of 165 rows
  widths_e64_h96_a160 (31)   0 % of 39, 2.0e-2, row 0 at step 8
The <end> bias bump of end_at_step0 was chosen the same way (oracle alone: + 0.5 ends no clip at step 0, + 1.0 exactly one,
+ 1.5 one and two more by step 3, + 2.0 two)."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib, train_util
from conftest import load_golden, unpack_masks
from parity_util import close
from scst_util import (StubScorer, check_against_oracle, g18_text, hip_scst, natural_step, text_side)
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
END = O.END_IDX

CASES = {
    # V, E, B, T, method, temp: the three settings pre-checked on the CPU for this feature (seeds 31 / 32 / 33)
    "multinomial_t10": dict(V=40, E=64, B=4, T=96, method="sample", temp=1.0, seed=31),
    "gumbel_t09": dict(V=300, E=64, B=5, T=96, method="gumbel", temp=0.9, seed=32),
    "multinomial_t07": dict(V=300, E=64, B=5, T=130, method="sample", temp=0.7, seed=33),
    "gumbel_t12": dict(V=40, E=64, B=4, T=96, method="gumbel", temp=1.2, seed=33),
    "decdrop": dict(V=40, E=64, B=4, T=96, method="sample", temp=1.0, seed=32, dec_dropout=0.3),
    "end_at_step0": dict(V=40, E=64, B=4, T=96, method="sample", temp=1.0, seed=31, end_bump=1.0, end_at_0=True),    # bias[<end>] + 1
    "e512": dict(V=300, E=512, B=2, T=64, method="sample", temp=1.0, seed=31),
    "cnn14_ln": dict(V=40, E=64, B=3, T=96, method="sample", temp=1.0, seed=32, encoder="Cnn14_16k"),
    "sample_n5": dict(V=40, E=64, B=3, T=96, method="sample", temp=1.0, seed=31, sample_n=5),
    "rows165": dict(V=40, E=64, B=33, T=64, method="sample", temp=1.0, seed=31, sample_n=5),   # past the 32-row boundary
    # the decoder GRU (H) and the attention (A) wider than the embeddings: a rollout has no utterance head, so its forward and
    # acvae_decode_bwd - the only backward that runs with H != E - take any H (tests/widths_util.py)
    "widths_e64_h96_a160": dict(V=40, E=64, H=96, A=160, B=4, T=96, method="sample", temp=1.0, seed=31),
}
MAXLEN = 10


def setup(p):
    V, E = p["V"], p["E"]
    enc = p.get("encoder", "Cnn10")
    enc_embed = 512 if enc == "Cnn10" else 2048
    state = O.closed_form_state(O.state_shapes(V, E, p.get("H", E), p.get("A"), E, enc_embed, encoder=enc))
    if p.get("end_bump"):
        state["decoder.classifier.bias"][END] += p["end_bump"]
    feats, _, fl, _ = O.synthetic_batch(p["B"], p["T"], V, 8, seed=p["seed"], ragged=True)
    return state, feats, fl, text_side(V, p["B"], p["seed"])


def kwargs_of(p):
    return dict(method=p["method"], temp=p["temp"], max_length=p.get("max_length", MAXLEN), sample_n=p.get("sample_n", 1))


def natural(p, state, feats, fl):
    return natural_step(state, feats, fl, p["E"], seed=p["seed"], dec_dropout=p.get("dec_dropout", 0.0), **kwargs_of(p))


@pytest.mark.parametrize("case", list(CASES))
def test_scst_step_vs_oracle(case):
    p = CASES[case]
    state, feats, fl, (vocab, keys, key2refs) = setup(p)
    nat = natural(p, state, feats, fl)
    if p.get("end_at_0"):
        assert int((nat["sampled"]["seqs"][:, 0] == END).sum()) == 1
    if "H" in p:
        import widths_util as W
        model = W.build_model(p["V"], p["E"], p["H"], p["A"], p["E"], state)
        assert state["decoder.model.weight_ih_l0"].shape == (3 * p["H"], 3 * p["E"])
    else:
        model = build_model(p["V"], p["E"], state, encoder=p.get("encoder", "Cnn10"), dec_dropout=p.get("dec_dropout", 0.0))
    sc = StubScorer()
    out, rollout = hip_scst(model, nat, feats, fl, keys, key2refs, vocab, sc, **kwargs_of(p))
    assert out["sampled_logprobs"].requires_grad and rollout["logits"].requires_grad
    if p.get("end_at_0"):
        assert int((out["sampled_seqs"][:, 0] == END).sum()) == 1
    if kwargs_of(p)["sample_n"] > 1:
        assert out["sampled_seqs"].shape[0] == p["B"] * p["sample_n"] and "greedy_seqs" not in out
    check_against_oracle(case, model, out, rollout, nat, state, feats, fl, keys, key2refs, vocab, sc,
                         dec_dropout=p.get("dec_dropout", 0.0), **kwargs_of(p))


def test_sample_n_encode_once_vs_repeated_features_without_encoder_dropout(monkeypatch):
    """NScstWrapper encodes each clip once and repeats the memory rows; the reference's layout repeats the features and
    pays the encoder sample_n times.  With the encoder's dropout off the two are the same function: loss and every gradient
    against the oracle on feats.repeat_interleave(5, 0), within the bounds of every other case."""
    p = dict(V=40, E=64, B=3, T=96, method="sample", temp=1.0, seed=33, sample_n=5)
    state, feats, fl, (vocab, keys, key2refs) = setup(p)
    monkeypatch.setattr(O, "_dropout", lambda x, pr, training, masks, record: x)
    nat = natural(p, state, feats, fl)
    assert nat["noise"]["dropout"] == []
    model = build_model(p["V"], p["E"], state)
    model.encoder.p_block = model.encoder.p_fc = 0.0
    sc = StubScorer()
    out, rollout = hip_scst(model, nat, feats, fl, keys, key2refs, vocab, sc, **kwargs_of(p))
    check_against_oracle("encode_once", model, out, rollout, nat, state, feats, fl, keys, key2refs, vocab, sc, **kwargs_of(p))


# ---------------------------------------------------------------- the reference's own values
def _g18_model():
    g = load_golden("g18_scst")
    B, T, V, E, maxlen, n = (int(x) for x in g["dims"])
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    return g, build_model(V, E, state), maxlen, n


def test_g18_scst_wrapper_and_scst_loss():
    g, model, maxlen, _ = _g18_model()
    vocab, keys, key2refs = g18_text(g)
    sc = StubScorer()
    nat = dict(noise=dict(dropout=unpack_masks(g, "scst_"), eps_g=torch.from_numpy(g["scst_greedy_eps_p"]),
                          eps_p=torch.from_numpy(g["scst_eps_p"]), sample_noise=torch.from_numpy(g["scst_sample_noise"]),
                          dec_keep=None))
    feats = torch.from_numpy(g["feats"])
    lens = g["feat_lens"].copy()
    out, rollout = hip_scst(model, nat, feats, lens, keys, key2refs, vocab, sc, method="sample", temp=1.0, max_length=maxlen,
                            backward=False)
    assert np.array_equal(out["greedy_seqs"].cpu().numpy(), g["scst_greedy_seqs"])
    assert np.array_equal(out["sampled_seqs"].cpu().numpy(), g["scst_sampled_seqs"])
    assert np.array_equal(out["reward"].numpy(), g["scst_reward"]) and np.array_equal(out["score"].numpy(), g["scst_score"])
    print(f"g18 ScstWrapper: loss hip {float(out['loss'].detach()):.8f} reference {float(g['scst_loss']):.8f}")
    assert abs(float(out["loss"].detach()) - float(g["scst_loss"])) <= 1e-4
    steps = int(g["scst_steps"][1])
    close(out["sampled_logprobs"][:, :steps], g["scst_sampled_logprobs"][:, :steps], 1e-4, 1e-5, what="sampled_logprobs")
    # the caller's array ends up divided once, as after one model call (each rollout got its own copy)
    from acvae_amd.seq_train_model import ScstWrapper
    lens2 = g["feat_lens"].copy()
    ScstWrapper(model)(feats.cuda(), lens2, keys, key2refs, vocab, max_length=maxlen, scorer=sc, rng="device")
    assert np.array_equal(lens2, g["feat_lens"] // 16)
    # scst_Loss on the same rollouts
    lo = train_util.scst_Loss(sc)(dict(greedy_seqs=out["greedy_seqs"], sampled_seqs=out["sampled_seqs"],
                                       sampled_logprobs=out["sampled_logprobs"]), keys, key2refs, vocab)
    assert np.array_equal(lo["reward"].numpy(), g["loss_reward"]) and np.array_equal(lo["score"].numpy(), g["loss_score"])
    assert abs(float(lo["loss"]) - float(g["loss_loss"])) <= 1e-4
    assert torch.equal(lo["loss"], out["loss"])
    model.check_persistent_launches()


def test_g18_nscst_loss_encode_once():
    """The reference's Nscst_Loss over its model run on feats.repeat_interleave(5, 0) with the encoder's dropout off, against
    one encoder pass here with the memory rows repeated on the device."""
    g, model, maxlen, n = _g18_model()
    vocab, keys, key2refs = g18_text(g)
    sc = StubScorer()
    model.encoder.p_block = model.encoder.p_fc = 0.0
    nat = dict(noise=dict(dropout=[], eps_g=None, eps_p=torch.from_numpy(g["n_eps_p"]),
                          sample_noise=torch.from_numpy(g["n_sample_noise"]), dec_keep=None))
    out, rollout = hip_scst(model, nat, torch.from_numpy(g["feats"]), g["feat_lens"].copy(), keys, key2refs, vocab, sc,
                            method="sample", temp=1.0, max_length=maxlen, sample_n=n, backward=False)
    assert np.array_equal(out["sampled_seqs"].cpu().numpy(), g["n_sampled_seqs"])
    assert np.array_equal(out["score"].numpy(), g["n_score"])
    assert float(out["reward"].mean()) == pytest.approx(float(g["n_reward_mean"]), abs=1e-12)
    print(f"g18 NScstWrapper: loss hip {float(out['loss'].detach()):.8f} reference {float(g['n_loss']):.8f}")
    assert abs(float(out["loss"].detach()) - float(g["n_loss"])) <= 1e-4
    lo = train_util.Nscst_Loss(sc, sample_n=n)(dict(sampled_seqs=out["sampled_seqs"], sampled_logprobs=out["sampled_logprobs"]),
                                                keys, key2refs, vocab)
    assert np.array_equal(lo["score"].numpy(), g["n_score"])
    assert float(lo["reward"]) == pytest.approx(float(g["n_reward_mean"]), abs=1e-12)
    assert abs(float(lo["loss"]) - float(g["n_loss"])) <= 1e-4 and torch.equal(lo["loss"], out["loss"])
    model.check_persistent_launches()


# ---------------------------------------------------------------- when a graph is recorded, and that recording changes nothing
@pytest.mark.parametrize("method", ["greedy", "sample"])
def test_rollout_records_a_graph_only_in_training_with_gradients_enabled(method):
    p = CASES["multinomial_t10"]
    state, feats, fl, _ = setup(p)
    nat = natural(dict(p, method=method), state, feats, fl)
    n = nat["noise"]
    model = build_model(p["V"], p["E"], state)
    model.encoder.dropout_masks = n["dropout"]
    f = feats.cuda()

    def run(mode, grad):
        model.train(mode == "train")
        model.noise = {k: v for k, v in dict(eps_p=n["eps_p"], sample_noise=n["sample_noise"]).items() if v is not None}
        with torch.enable_grad() if grad else torch.no_grad():
            return model(f, fl.copy(), method=method, temp=1.0, max_length=MAXLEN)

    rec = run("train", True)
    assert rec["sampled_logprobs"].requires_grad and rec["logits"].requires_grad
    plain = run("train", False)
    ev = run("eval", True)
    for o in (plain, ev):
        assert not o["sampled_logprobs"].requires_grad and not o["logits"].requires_grad
        assert o["sampled_logprobs"].grad_fn is None and o["logits"].grad_fn is None
    # every output of the recorded rollout is bit-identical to the same rollout without the graph
    for k, v in rec.items():
        if torch.is_tensor(v):
            assert torch.equal(v.detach(), plain[k]), k
    for a, b in zip(rec["hiddens_state"], plain["hiddens_state"]):
        assert torch.equal(a, b)
    # the reference's loss line in plain torch works as it stands on the recorded rollout
    reward = torch.linspace(-1, 1, rec["seqs"].shape[0], device="cuda")
    mask = (rec["seqs"] != END).float()
    mask = torch.cat([torch.ones(mask.size(0), 1, device="cuda"), mask[:, :-1]], 1)
    loss = torch.sum(-rec["sampled_logprobs"] * reward[:, None] * mask, dim=1).mean()
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    assert named["decoder.classifier.weight"].grad is not None and named["encoder.conv_block1.conv1.weight"].grad is not None
    assert named["qnet.word_embedding.weight"].grad is None and named["mean_log_out.weight"].grad is None
    mine = {k: v.grad.clone() for k, v in named.items() if v.grad is not None}
    # ... and gives the gradients of the fused loss
    for v in named.values():
        v.grad = None
    rec2 = run("train", True)
    train_util.scst_policy_loss(rec2["sampled_logprobs"], rec2["seqs"], reward.cpu().numpy(), END).backward()
    torch.cuda.synchronize()
    for k, v in mine.items():
        close(named[k].grad, v, 1e-4, 1e-6 * max(float(v.abs().max()), 1e-3), what=k)
    model.check_persistent_launches()


# ---------------------------------------------------------------- TrainStep.scst_step
def test_trainstep_scst_three_steps_against_a_torch_adam_twin():
    """TrainStep.scst_step against autograd + clip_grad_norm_ + torch.optim.Adam on a twin (tests/test_optim_gpu.py's helpers
    and bounds); the posterior's parameters, mean_log_out and their Adam state are bit-identical before and after."""
    from acvae_amd.seq_train_model import ScstWrapper
    from test_optim_gpu import compare_params, fresh, sync_params
    V = 40
    feats, _, fl, _ = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    vocab, keys, key2refs = text_side(V, 3, 1)
    sc = StubScorer()
    m1, t1 = fresh()
    m3, t3 = fresh()
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    untouched = {k: p.detach().clone() for k, p in m1.named_parameters() if k.startswith(("qnet.", "mean_log_out."))}
    offs = t1._offsets()
    f = feats.cuda()
    for k in range(3):
        if k:
            sync_params(m1, m3)
        before = [p.detach().clone() for p in m1.parameters()]
        torch.manual_seed(3 + k); random.seed(3 + k)
        parts = t1.scst_step(f, fl.copy(), keys, key2refs, vocab, sc, max_length=MAXLEN)
        torch.manual_seed(3 + k); random.seed(3 + k)
        for p in m3.parameters():
            p.grad = None
        o3 = ScstWrapper(m3)(f, fl.copy(), keys, key2refs, vocab, max_length=MAXLEN, scorer=sc)
        o3["loss"].backward()
        torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], 1.0)
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(parts["sampled_seqs"], o3["sampled_seqs"]) and torch.equal(parts["loss"], o3["loss"].detach())
        assert float(np.abs(parts["reward"].numpy()).max()) > 0
        compare_params(m1, m3, f"scst step {k + 1}")
        assert any(not torch.equal(a, b) for a, b in zip(before, m1.parameters()))
    for k, p in m1.named_parameters():
        if k in untouched:
            assert torch.equal(p.detach(), untouched[k]), k
            o = offs[p]
            assert not bool(t1.exp_avg[o:o + p.numel()].any()) and not bool(t1.exp_avg_sq[o:o + p.numel()].any()), k
            assert p.grad is None, k
    t1.synchronize()


def test_scst_backward_is_bit_reproducible_from_the_first_run():
    """As tests/test_fullsize_gpu.py::test_backward_is_bit_reproducible_from_the_first_run: rollouts + loss + backward four
    times on fresh gradients (and the BatchNorm running statistics of the start) with the side stream on; every gradient
    and the loss equal the FIRST run's bit for bit."""
    p = CASES["gumbel_t09"]
    state, feats, fl, (vocab, keys, key2refs) = setup(p)
    nat = natural(p, state, feats, fl)
    model = build_model(p["V"], p["E"], state)
    assert model.use_side_stream
    sc = StubScorer()
    ref = None
    buffers = {k: b.detach().clone() for k, b in model.named_buffers()}
    for run in range(4):
        for prm in model.parameters():
            prm.grad = None
        with torch.no_grad():      # the same step each time: the greedy baseline reads the BatchNorm running statistics,
            for k, b in model.named_buffers():        # which every training forward moves
                b.copy_(buffers[k])
        out, _ = hip_scst(model, nat, feats, fl, keys, key2refs, vocab, sc, **kwargs_of(p))
        cur = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        cur["loss"] = out["loss"].detach().clone()
        if ref is None:
            ref = cur
            assert all(bool(torch.isfinite(v).all()) for v in cur.values()) and len(cur) > 30
            continue
        bad = [k for k in ref if not torch.equal(cur[k], ref[k])]
        assert not bad, (run, bad[:8])
    model.check_persistent_launches()
