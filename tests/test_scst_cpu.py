"""CPU: self-critical sequence training (SCST) without a GPU - the public interface's contracts, the host-side reward
arithmetic and sentence conversion against values the reference's own ``scst_Loss`` / ``Nscst_Loss`` / ``ScstWrapper``
produced (tests/golden/g18_scst.npz, tools/make_scst_golden.py), the oracle replaying that fixture's noise, and the oracle's
SCST gradient - which the GPU tests differentiate against and which the reference cannot compute under current torch -
against central differences of the float64 loss."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib, seq_train_model, train_util
from conftest import unpack_masks
from scst_util import StubScorer, g18_text, mask_of, oracle_rollout, oracle_scst_grads, policy_loss, reward_of, text_side


def close(a, b, rtol=1e-4, atol=1e-5):                       # tests/test_oracle_golden.py
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())


class _Model(torch.nn.Module):
    start_idx, end_idx, max_length = 1, 2, 20

    def forward(self, *a, **k):
        return {"two_inputs": (len(a), dict(k))}


# ---------------------------------------------------------------- interface contracts
@pytest.mark.parametrize("cls", [seq_train_model.ScstWrapper, seq_train_model.NScstWrapper])
def test_wrapper_arity_and_keywords(cls):
    w = cls(_Model())
    for n in (0, 1, 3, 4, 6):
        with pytest.raises(Exception, match="number of input should be either 5"):
            w(*range(n))
    # two inputs: the model's own 2-input forward, keywords passed through
    assert w(1, 2, method="greedy", max_length=7) == {"two_inputs": (2, {"method": "greedy", "max_length": 7})}
    five = (torch.zeros(1, 64, 64), [64], ["k"], {"k": ["a"]}, None)
    with pytest.raises(KeyError, match="max_length"):
        w(*five, scorer=StubScorer(), sample_n=5)
    if cls is seq_train_model.NScstWrapper:
        with pytest.raises(KeyError, match="sample_n"):
            w(*five, scorer=StubScorer(), max_length=5)
        with pytest.raises(ValueError, match="sample_n >= 2"):
            w(*five, scorer=StubScorer(), max_length=5, sample_n=1)
    with pytest.raises(ValueError, match="scorer"):
        w(*five, max_length=5, sample_n=5)
    with pytest.raises(ValueError, match="scorer"):
        w(*five, max_length=5, sample_n=5, scorer=None)


def test_losses_need_a_scorer_and_nothing_imports_pycocoevalcap():
    import sys
    with pytest.raises(ValueError, match="compute_score"):
        train_util.compute_batch_score(np.zeros((1, 3), np.int64), {"k": ["a"]}, ["k"], 1, 2, None, None)
    with pytest.raises(ValueError, match="compute_score"):
        train_util.compur_batch_score_samplen(np.zeros((1, 3), np.int64), {"k": ["a"]}, ["k"], 1, 2, None, None)
    assert "pycocoevalcap" not in sys.modules


def test_new_entry_points_refuse_null_pointers_and_bad_dimensions():
    lib = _lib.lib()
    assert lib.acvae_abi_version() == 3
    assert lib.acvae_scst_loss_fwd(None, None, None, 2, None, None, 4, 5, None) == -1
    assert lib.acvae_logprob_bwd(None, 8, None, None, None, None, 4, 8, None) == -1
    one = torch.zeros(64)
    ids = torch.zeros(64, dtype=torch.long)
    p, q = one.data_ptr(), ids.data_ptr()               # host memory: every refusal below comes before any launch
    assert lib.acvae_scst_loss_fwd(p, q, p, 2, p, p, 0, 5, None) == -1
    assert lib.acvae_scst_loss_fwd(p, q, p, 2, p, p, 4, 0, None) == -1
    assert lib.acvae_scst_loss_fwd(p, q, p, 2, p, None, 4, 5, None) == -1
    assert lib.acvae_logprob_bwd(p, 8, p, q, p, p, 0, 8, None) == -1
    assert lib.acvae_logprob_bwd(p, 8, p, q, p, p, 4, 0, None) == -1
    assert lib.acvae_logprob_bwd(p, 4, p, q, p, p, 4, 8, None) == -1          # row stride under V
    assert lib.acvae_logprob_bwd(p, 8, p, q, None, p, 4, 8, None) == -1
    assert lib.acvae_decode_saved_lse_offset(0, 5, 6, 64, 64, 64, 40, 64) == -1
    off = lib.acvae_decode_saved_lse_offset(3, 5, 6, 64, 64, 64, 40, 64)
    assert off >= 0 and off % 4 == 0 and off + 3 * 5 * 4 <= lib.acvae_decode_saved_bytes(3, 5, 6, 64, 64, 64, 40, 64)
    # the decode backward still refuses null pointers, with and without the rollout flag
    for flags in (0, _lib.FLAG_ROLLOUT_GRAD):
        assert lib.acvae_decode_bwd(*([None] * 19), 0, None, 0, 3, 5, 6, 64, 64, 64, 40, 64, None, None, None, 0.0, flags) == -1


def test_data_parallel_scst_is_refused():
    from acvae_amd.trainer import TrainStep
    ts = TrainStep.__new__(TrainStep)
    ts.world = 2
    with pytest.raises(NotImplementedError, match="data-parallel SCST"):
        ts.scst_step(None, None, None, None, None, StubScorer())


# ---------------------------------------------------------------- host arithmetic against the reference's values
def test_sentences_scores_and_rewards_match_the_reference(golden):
    g = golden("g18_scst")
    vocab, keys, key2refs = g18_text(g)
    sc = StubScorer()
    args = (key2refs, keys, O.START_IDX, O.END_IDX, vocab, sc)
    s = train_util.compute_batch_score(g["scst_sampled_seqs"], *args)
    gr = train_util.compute_batch_score(g["scst_greedy_seqs"], *args)
    assert np.array_equal(s, g["scst_score"]) and np.array_equal(s - gr, g["scst_reward"])
    assert np.array_equal(s, g["loss_score"]) and np.array_equal(s - gr, g["loss_reward"])
    crit = train_util.scst_Loss(sc)
    rs = crit.get_critical_reward(torch.from_numpy(g["scst_greedy_seqs"]), torch.from_numpy(g["scst_sampled_seqs"]), keys,
                                  key2refs, vocab, sc)
    assert np.array_equal(rs["reward"], g["loss_reward"]) and np.array_equal(rs["score"], g["loss_score"])
    # sample_n rollouts per clip: every row scored on its own, leave-one-out baseline
    n = int(g["dims"][5])
    ncrit = train_util.Nscst_Loss(sc, sample_n=n)
    keys_n = [k for k in keys for _ in range(n)]
    rn = ncrit.get_critical_reward(torch.from_numpy(g["n_sampled_seqs"]), keys_n, key2refs, vocab)
    assert np.array_equal(rn["score"], g["n_score"])
    assert float(np.mean(rn["reward"])) == pytest.approx(float(g["n_reward_mean"]), abs=1e-12)
    want, _ = reward_of(g["n_sampled_seqs"], None, keys, key2refs, vocab, sc, sample_n=n)
    assert np.array_equal(rn["reward"], want)
    assert np.allclose(rn["reward"].reshape(-1, n).sum(1), 0.0, atol=1e-12)       # a clip's rewards sum to zero
    # the fixture holds finished rows: a row that is <end> from step 1 on is a one-word sentence, one that starts with
    # <start> drops it
    seqs = g["n_sampled_seqs"]
    early = [i for i in range(len(seqs)) if (seqs[i] == O.END_IDX).any()]
    assert early, "g18's sample_n part must hold rows that finish early"
    i = early[0]
    t_end = int(np.argmax(seqs[i] == O.END_IDX))
    assert train_util._sentence(seqs[i], O.START_IDX, O.END_IDX, vocab).split() == \
        [vocab.idx2word[int(w)] for w in seqs[i][:t_end] if w != O.START_IDX]
    # the loss line itself, from the stored log-probabilities (float64 torch)
    slp = torch.from_numpy(g["n_sampled_logprobs"]).double()
    m = mask_of(torch.from_numpy(seqs)).double()
    loss = (-slp * torch.from_numpy(rn["reward"])[:, None] * m).sum(1).mean()
    close(loss.float(), torch.from_numpy(g["n_loss"]), 1e-5, 1e-6)


# ---------------------------------------------------------------- the oracle replays the fixture
def _g18_noise(g, part):
    if part == "greedy":
        return dict(eps_p=torch.from_numpy(g["scst_greedy_eps_p"]))
    if part == "sampled":
        return dict(dropout=unpack_masks(g, "scst_"), eps_p=torch.from_numpy(g["scst_eps_p"]),
                    sample_noise=torch.from_numpy(g["scst_sample_noise"]))
    return dict(eps_p=torch.from_numpy(g["n_eps_p"]), sample_noise=torch.from_numpy(g["n_sample_noise"]))


def test_oracle_replaying_g18_reproduces_the_reference(golden, monkeypatch):
    g = golden("g18_scst")
    B, T, V, E, maxlen, n = (int(x) for x in g["dims"])
    vocab, keys, key2refs = g18_text(g)
    sc = StubScorer()
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, lens = torch.from_numpy(g["feats"]), g["feat_lens"]
    st = {k: v.clone() for k, v in state.items()}
    with torch.no_grad():
        og = oracle_rollout(st, feats, lens, method="greedy", temp=1, max_length=maxlen, noise=_g18_noise(g, "greedy"),
                            training=False)
        osm = oracle_rollout(st, feats, lens, method="sample", temp=1, max_length=maxlen, noise=_g18_noise(g, "sampled"))
    assert np.array_equal(og["seqs"].numpy(), g["scst_greedy_seqs"])
    assert np.array_equal(osm["seqs"].numpy(), g["scst_sampled_seqs"])
    close(st["encoder.bn0.running_mean"], torch.from_numpy(g["scst_bn0_running_mean"]), 1e-5, 1e-7)
    reward, score = reward_of(osm["seqs"], og["seqs"], keys, key2refs, vocab, sc)
    assert np.array_equal(reward, g["scst_reward"]) and np.array_equal(score, g["scst_score"])
    steps = int(g["scst_steps"][1])
    close(osm["sampled_logprobs"], torch.from_numpy(g["scst_sampled_logprobs"])[:, :steps])
    loss = policy_loss(osm["logits"], osm["seqs"], reward)
    close(loss, torch.from_numpy(g["scst_loss"]))
    close(loss, torch.from_numpy(g["loss_loss"]))
    # sample_n rollouts per clip over repeated features, the encoder's dropout off (as the generator ran the reference)
    monkeypatch.setattr(O, "_dropout", lambda x, p, training, masks, record: x)
    with torch.no_grad():
        on = oracle_rollout({k: v.clone() for k, v in state.items()}, feats, lens, method="sample", temp=1,
                            max_length=maxlen, noise=_g18_noise(g, "n"), sample_n=n)
    assert np.array_equal(on["seqs"].numpy(), g["n_sampled_seqs"])
    rn, sn = reward_of(on["seqs"], None, keys, key2refs, vocab, sc, sample_n=n)
    assert np.array_equal(sn, g["n_score"])
    close(policy_loss(on["logits"], on["seqs"], rn), torch.from_numpy(g["n_loss"]))


# ---------------------------------------------------------------- the oracle's SCST gradient
V, E, B, Tt, MAXLEN, SEED = 40, 64, 4, 96, 10, 31
FD_TENSORS = ("decoder.word_embeddings.weight", "decoder.model.weight_hh_l0", "decoder.attn.h2attn.weight",
              "decoder.classifier.weight", "pnet.word_embedding.weight", "pnet.network.weight_ih_l0",
              "pnet.mean_log_out.weight", "ln.weight", "encoder.conv_block2.conv1.weight", "encoder.conv_block3.bn1.weight")


def _natural(dtype):
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    if dtype != torch.float32:
        state = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in state.items()}
    feats, _, fl, _ = O.synthetic_batch(B, Tt, V, 8, seed=SEED, ragged=True)
    feats = feats.to(dtype)
    vocab, keys, key2refs = text_side(V, B, SEED)
    torch.manual_seed(SEED)
    rec = {}
    with torch.no_grad():
        out = O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, fl.copy(), training=True, method="sample",
                               temp=1, max_length=MAXLEN, record=rec)
        greedy = O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, fl.copy(), training=False,
                                  method="greedy", max_length=MAXLEN)
    reward, _ = reward_of(out["seqs"], greedy["seqs"], keys, key2refs, vocab, StubScorer())
    return state, feats, fl, out, rec, reward


def test_oracle_scst_gradient_reaches_what_the_reference_trains():
    """decoder.*, pnet.*, ln.* and the encoder's convolutions and BatchNorms receive a gradient; the posterior, mean_log_out
    and the encoder's pooled head do not (None, as torch leaves a parameter the loss does not reach); a second run fed the
    first run's words and noise gives the same tokens, loss and gradients to the last bit."""
    state, feats, fl, out, rec, reward = _natural(torch.float32)
    assert np.abs(reward).max() > 0
    noise = dict(dropout=[m.clone() for m in rec["dropout"]], eps_p=rec["eps_p"], sample_noise=rec["sample_noise"],
                 fed_words=out["seqs"].clone())
    kw = dict(method="sample", temp=1, max_length=MAXLEN)
    l1, g1, o1 = oracle_scst_grads(state, feats, fl, out["seqs"], reward, noise=noise, **kw)
    noise["dropout"] = [m.clone() for m in rec["dropout"]]
    l2, g2, o2 = oracle_scst_grads(state, feats, fl, out["seqs"], reward, noise=noise, **kw)
    assert torch.equal(o1["seqs"], out["seqs"]) and torch.equal(o2["seqs"], out["seqs"]) and torch.equal(l1, l2)
    assert set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    got = set(g1)
    for k in O.trainable_keys(state):
        dead = k.startswith(("qnet.", "mean_log_out.", "encoder.embed_pooled."))
        assert (k in got) != dead, k
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in g1.values())


def test_oracle_scst_gradient_vs_central_differences():
    """'The gradient of the loss with the sampled words held constant' against central differences (h = 1e-5) of the float64
    loss, dropout masks, eps, sampling noise, ReLU decisions and fed words replayed, four directions (a random unit vector
    plus the unit gradient) in one tensor of every parameter family the loss reaches: both embedding tables, the decoder's
    GRU, attention and classifier, the prior's LSTM and head, ln, an encoder convolution and an encoder BatchNorm.  Step size,
    directions and bound are those of tests/test_sched_sampling_cpu.py: four times the worst relative disagreement of the
    same check on the teacher-forced training loss, measured in the test itself.
    Measured when this test was written: 3.7e-9 for the cross-entropy step (bound 1.5e-8) and 5.3e-9 for the SCST loss, at
    16 threads and at 3 alike; the worst tensor is encoder.conv_block2.conv1.weight, by the h^2 term (8.3e-8 at h = 4e-5,
    3e-10 at 2.5e-6)."""
    from test_sched_sampling_cpu import FD_DIRS, FD_H, _fd_worst
    ref, kref = _fd_worst(1.0, 0)
    print(f"central differences vs autograd, cross-entropy step at ss=1.0: worst {ref:.3e} ({kref})")
    assert 0 < ref < 1e-5
    state, feats, fl, out, rec, reward = _natural(torch.float64)
    words = out["seqs"].clone()
    noise = dict(dropout=[m.clone() for m in rec["dropout"]], eps_p=rec["eps_p"], sample_noise=rec["sample_noise"],
                 fed_words=words, relu_force={i: z > 0 for i, z in enumerate(rec["relu_z"])})
    kw = dict(method="sample", temp=1, max_length=MAXLEN)

    def fresh():
        return dict(noise, dropout=[m.clone() for m in rec["dropout"]])

    _, grads, o = oracle_scst_grads(state, feats, fl, words, reward, noise=fresh(), **kw)
    assert torch.equal(o["seqs"], words)

    # The differenced loss is evaluated as sum(coef * (lp - lp0)), lp0 the unperturbed log-probabilities (constants): the
    # same difference f(+h) - f(-h) as of sum(coef * lp), term for term, but the weighted sum then adds numbers of size h
    # instead of mixed-sign terms that add up to 14 in magnitude and 3.5 in value, whose float64 rounding (1.1e-15, a good ulp
    # of the loss) over the 6e-8 that the loss moves along the prior's embedding table - the smallest gradient of all, 3e-3 -
    # is by itself 1.9e-8; and each log-probability's own difference is formed from the logits' differences, not from two
    # rounded log-softmaxes.  What is left is the rounding of the logits.
    x0 = o["logits"].detach()
    p0 = torch.softmax(x0, -1)
    lp0 = torch.log_softmax(x0, -1).gather(2, words.unsqueeze(-1)).squeeze(-1)
    coef = -(torch.as_tensor(reward)[:, None] * mask_of(words).double()) / words.shape[0]
    assert float((coef * lp0).sum()) == pytest.approx(float(policy_loss(o["logits"].detach(), words, reward)), rel=1e-13)

    def loss_at(st):
        with torch.no_grad():
            oo = oracle_rollout(st, feats, fl, noise=fresh(), **kw)
            dx = oo["logits"] - x0               # lp - lp0 = dx[w] - log(sum softmax(x0) * exp(dx)), formed from the differences
            dlp = dx.gather(2, words.unsqueeze(-1)).squeeze(-1) - torch.log1p((p0 * torch.expm1(dx)).sum(-1))
            return float((coef * dlp).sum())

    gen = torch.Generator().manual_seed(5)
    worst = (0.0, None)
    for k in FD_TENSORS:
        for _ in range(FD_DIRS):
            d = torch.randn(state[k].shape, generator=gen, dtype=torch.float64)
            d = d / d.norm() + grads[k] / grads[k].norm()
            d /= d.norm()
            ad = float((grads[k] * d).sum())
            f = []
            for sgn in (1.0, -1.0):
                st = {n: v.clone() for n, v in state.items()}
                st[k] = st[k] + sgn * FD_H * d
                f.append(loss_at(st))
            e = abs((f[0] - f[1]) / (2 * FD_H) - ad) / abs(ad)
            if e > worst[0]:
                worst = (e, k)
    print(f"central differences vs autograd, SCST loss: worst {worst[0]:.3e} ({worst[1]}); bound {4 * ref:.3e}")
    assert worst[0] <= 4 * ref, (worst, ref)
