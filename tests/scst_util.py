"""Shared by the self-critical sequence training tests (test_scst_cpu.py, test_scst_gpu.py, test_scst_fullsize_gpu.py): the
stub scorer and vocabulary of tools/make_scst_golden.py, the g18 fixture's text side, and the oracle's SCST step - rollout(s)
through acvae_oracle.hybrid_forward, the reference's reward arithmetic (models/seq_train_model.py:47-65, utils/train_util.py:
315-321) and loss line, and autograd of that loss with the sampled words held constant."""
import numpy as np
import torch

import acvae_oracle as O


class StubScorer:
    """Share of the hypothesis' words found in the key's references (0 for an empty hypothesis); as in the generator."""

    def compute_score(self, references, hypotheses):
        scores = []
        for k in references:
            words = hypotheses[k][0].split()
            pool = set(w for r in references[k] for w in r.split())
            scores.append(sum(w in pool for w in words) / len(words) if words else 0.0)
        return float(np.mean(scores)), np.array(scores, dtype=np.float64)


class Vocabulary:
    def __init__(self, words):
        self.idx2word = {i: w for i, w in enumerate(words)}


def text_side(V, B, seed, nrefs=3, nwords=9):
    """Vocabulary, keys and key2refs of a synthetic batch (the generator's recipe)."""
    words = ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]
    g = torch.Generator().manual_seed(seed)
    keys = [f"clip{i}" for i in range(B)]
    refs = [[" ".join(words[int(j)] for j in torch.randint(4, V, (nwords,), generator=g)) for _ in range(nrefs)] for _ in keys]
    return Vocabulary(words), keys, dict(zip(keys, refs))


def g18_text(g):
    keys = [str(k) for k in g["keys"]]
    return Vocabulary([str(w) for w in g["words"]]), keys, {k: [str(r) for r in refs] for k, refs in zip(keys, g["refs"])}


def sentence(row, vocab):
    words = []
    for w in row:
        if w == O.START_IDX:
            continue
        if w == O.END_IDX:
            break
        words.append(vocab.idx2word[int(w)])
    return " ".join(words)


def row_scores(seqs, keys, key2refs, vocab, scorer):
    """One score per row, every row scored on its own."""
    seqs = np.asarray(seqs)
    hyp = {i: [sentence(seqs[i], vocab)] for i in range(len(keys))}
    return np.asarray(scorer.compute_score({i: key2refs[keys[i]] for i in range(len(keys))}, hyp)[1], dtype=np.float64)


def reward_of(sampled_seqs, greedy_seqs, keys, key2refs, vocab, scorer, sample_n=1):
    """sample_n == 1: sampled score - greedy score; else the leave-one-out baseline over a clip's rollouts (rows clip-major)."""
    keys_n = [k for k in keys for _ in range(sample_n)]
    score = row_scores(sampled_seqs, keys_n, key2refs, vocab, scorer)
    if sample_n == 1:
        return score - row_scores(greedy_seqs, keys, key2refs, vocab, scorer), score
    s = score.reshape(-1, sample_n)
    return (s - (s.sum(1, keepdims=True) - s) / (sample_n - 1)).reshape(-1), score


def mask_of(seqs):
    m = (seqs != O.END_IDX)
    return torch.cat([torch.ones(m.size(0), 1, dtype=torch.bool), m[:, :-1]], 1)


def policy_loss(logits, words, reward):
    """mean_n sum_t -log_softmax(logits)[words] * reward * mask over the steps that were run; `words` are constants."""
    steps = logits.shape[1]
    words = torch.as_tensor(words)[:, :steps]
    lp = torch.log_softmax(logits, -1).gather(2, words.unsqueeze(-1)).squeeze(-1)
    r = torch.as_tensor(np.asarray(reward)).to(logits.dtype)
    return (-lp * r[:, None] * mask_of(words).to(logits.dtype)).sum(1).mean()


def trainable(state):
    st = {k: v.clone() for k, v in state.items()}
    for k in O.trainable_keys(st):
        st[k].requires_grad_(True)
    return st


def repeat_noise(noise, n):
    """Noise of a rollout over clip-major repeated features whose replicas share the encoder's dropout masks."""
    if n == 1 or noise is None or noise.get("dropout") is None:
        return noise
    return dict(noise, dropout=[m.repeat_interleave(n, 0) for m in noise["dropout"]])


def oracle_rollout(state, feats, feat_lens, *, method, temp, max_length, noise, record=None, sample_n=1, dec_dropout=0.0,
                   training=True):
    """A 2-input forward of the oracle; sample_n > 1: the reference's layout, features repeated clip-major."""
    if sample_n > 1:
        feats = feats.repeat_interleave(sample_n, 0)
        feat_lens = np.repeat(np.asarray(feat_lens), sample_n)
    return O.hybrid_forward(state, feats, np.asarray(feat_lens).copy(), training=training, method=method, temp=temp,
                            max_length=max_length, noise=repeat_noise(noise, sample_n), record=record,
                            dec_dropout=dec_dropout)


def oracle_scst_grads(state, feats, feat_lens, words, reward, **kw):
    """Loss and gradients of the oracle's sampled rollout fed `words` (noise["fed_words"] must hold them), with the loss
    gathered at `words` too: 'the gradient of the loss with the sampled words held constant'.  -> (loss, {name: grad for
    every parameter the loss reaches}, out)."""
    st = trainable(state)
    out = oracle_rollout(st, feats, feat_lens, **kw)
    loss = policy_loss(out["logits"], words, reward)
    keys = O.trainable_keys(st)
    gs = torch.autograd.grad(loss, [st[k] for k in keys], allow_unused=True)
    return loss.detach(), {k: g for k, g in zip(keys, gs) if g is not None}, out


# ---------------------------------------------------------------- the oracle's natural SCST step, and the HIP step on its noise
def natural_step(state, feats, feat_lens, E, *, method, temp, max_length, seed, sample_n=1, dec_dropout=0.0):
    """The oracle alone, on the CPU generator seeded with `seed`: the encoder's dropout masks (one training pass of the
    encoder: the replicas of a clip share them), the prior's eps of the greedy and of the sampled rollout, then the greedy
    rollout in evaluation mode (sample_n == 1) and the sampled rollout in training mode, which draws and records its
    sampling noise, decoder dropout masks and decision margins.  -> dict(noise=..., greedy=, sampled=, margins=)."""
    torch.manual_seed(seed)
    B = feats.shape[0]
    masks = []
    with torch.no_grad():
        O.cnn10_forward({k: v.clone() for k, v in state.items()}, feats, np.asarray(feat_lens).copy(), True, None, masks)
        eps_g, eps_p = torch.randn(max_length, B, E), torch.randn(max_length, B * sample_n, E)
        st = {k: v.clone() for k, v in state.items()}
        greedy = None
        if sample_n == 1:
            greedy = oracle_rollout(st, feats, feat_lens, method="greedy", temp=1, max_length=max_length,
                                    noise=dict(eps_p=eps_g), training=False)
        rec = {}
        sampled = oracle_rollout(st, feats, feat_lens, method=method, temp=temp, max_length=max_length,
                                 noise=dict(dropout=[m.clone() for m in masks], eps_p=eps_p), record=rec, sample_n=sample_n,
                                 dec_dropout=dec_dropout)
    steps = sampled["_steps_run"]

    def pad(x, fill):
        if x is None:
            return None
        out = torch.full((max_length,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
        out[:steps] = x
        return out
    # steps the oracle did not run (every row had finished): the device loop still runs them, on any noise
    noise = dict(dropout=masks, eps_g=eps_g, eps_p=eps_p, sample_noise=pad(rec["sample_noise"], 1.0),
                 dec_keep=pad(rec["dec_keep"], True))
    return dict(noise=noise, greedy=greedy, sampled=sampled, margins=rec["margins"], steps=steps)


def left_out_share(margins, thr=2e-4):
    """Share of the live decisions (finished rows hold +inf) whose margin is under `thr`: the rule for taking a seed."""
    live = torch.isfinite(margins)
    return float(((margins < thr) & live).double().sum() / max(int(live.sum()), 1)), int(live.sum())


def replay_noise(nat, words, force=None):
    n = nat["noise"]
    return dict(dropout=[m.clone() for m in n["dropout"]], eps_p=n["eps_p"], sample_noise=n["sample_noise"],
                dec_keep=n["dec_keep"], fed_words=words, relu_force=force)


class _EncoderProxy:
    def __init__(self, enc, n):
        self.enc, self.n = enc, n

    def relu_masks(self):
        return [m.repeat_interleave(self.n, 0) for m in self.enc.relu_masks()]


class ModelProxy:
    """What grads_match_oracle reads of a model, with the encoder's ReLU decisions repeated clip-major `n` times (the
    oracle's layout of sample_n rollouts per clip repeats the features)."""

    def __init__(self, model, n):
        self.encoder = model.encoder if n == 1 else _EncoderProxy(model.encoder, n)


def hip_scst(model, nat, feats, feat_lens, keys, key2refs, vocab, scorer, *, method, temp, max_length, sample_n=1,
             backward=True):
    """ScstWrapper (sample_n == 1) or NScstWrapper on the HIP model over the noise of `nat`, loss.backward().  Returns the
    wrapper's output and the sampled rollout's own output dict (logits)."""
    from acvae_amd.seq_train_model import NScstWrapper, ScstWrapper
    n = nat["noise"]
    model.encoder.dropout_masks = n["dropout"] or None          # (none recorded: the case runs with dropout off)
    model.encoder.keep_saved = True
    sampled_noise = {k: v for k, v in dict(eps_p=n["eps_p"], sample_noise=n["sample_noise"], dec_keep=n["dec_keep"]).items()
                     if v is not None}
    queue = ([dict(eps_p=n["eps_g"])] if sample_n == 1 else []) + [sampled_noise]
    captured = []
    orig = model.stepwise_forward

    def stepwise(encoded, caps, cap_lens, **kw):
        model.noise = queue.pop(0)
        o = orig(encoded, caps, cap_lens, **kw)
        captured.append(o)
        return o
    model.stepwise_forward = stepwise
    try:
        kw = dict(max_length=max_length, scorer=scorer, method=method, temp=temp)
        if sample_n == 1:
            out = ScstWrapper(model)(feats.cuda(), np.asarray(feat_lens).copy(), keys, key2refs, vocab, **kw)
        else:
            out = NScstWrapper(model)(feats.cuda(), np.asarray(feat_lens).copy(), keys, key2refs, vocab, sample_n=sample_n, **kw)
    finally:
        del model.stepwise_forward
    assert not queue
    if backward:
        out["loss"].backward()
    torch.cuda.synchronize()
    return out, captured[-1]


def check_against_oracle(tag, model, out, rollout, nat, state, feats, feat_lens, keys, key2refs, vocab, scorer, *, method,
                         temp, max_length, sample_n=1, dec_dropout=0.0, tol_enc_of=None, greedy_exact=True):
    """The HIP step against the oracle fed the HIP words: reward and score (host arithmetic, exact), the steps at which rows
    finish, the loss (1e-4), the words decision by decision (words_match_by_margin) and every gradient (grads_match_oracle;
    the parameters the loss does not reach must hold None).  Returns the oracle's loss."""
    from parity_util import grads_match_oracle, words_match_by_margin
    hip_words = out["sampled_seqs"].cpu()
    greedy = out["greedy_seqs"].cpu() if sample_n == 1 else None
    reward, score = reward_of(hip_words, greedy, keys, key2refs, vocab, scorer, sample_n)
    assert np.array_equal(out["reward"].numpy(), reward) and np.array_equal(out["score"].numpy(), score)
    kw = dict(method=method, temp=temp, max_length=max_length, sample_n=sample_n, dec_dropout=dec_dropout)
    rec = {}
    loss, grads, oo = oracle_scst_grads(state, feats, feat_lens, hip_words, reward, noise=replay_noise(nat, hip_words),
                                        record=rec, **kw)
    steps = oo["_steps_run"]
    # fed the HIP words, the oracle finishes its rows at the same steps (and stops where the last HIP row has finished)
    assert torch.equal(oo["seqs"][:, :steps] == O.END_IDX, hip_words[:, :steps] == O.END_IDX), tag
    assert steps == max_length or bool((hip_words[:, steps - 1:] == O.END_IDX).all()), tag
    if sample_n == 1:          # the baseline's words feed the reward only (free-running: exact at the small sizes)
        differ = int((greedy != nat["greedy"]["seqs"]).sum())
        print(f"{tag}: {differ} greedy baseline words differ from the oracle's free-running ones")
        assert not (greedy_exact and differ), (tag, "greedy baseline words")
    got = float(out["loss"].detach())
    print(f"{tag}: loss hip {got:.6f} oracle {float(loss):.6f}; reward {np.round(reward, 3).tolist()}; {steps} steps; rows "
          f"finished early: {int((hip_words[:, :-1] == O.END_IDX).any(-1).sum())}/{len(hip_words)}")
    assert abs(got - float(loss)) <= 1e-4 * max(1.0, abs(float(loss))), (tag, got, float(loss))
    words_match_by_margin(tag, hip_words[:, :steps], rollout["logits"][:, :steps],
                          dict(logits=oo["logits"], seqs=oo["seqs"][:, :steps]), rec["margins"])
    named = dict(model.named_parameters())
    for k, p in named.items():
        if k.startswith(("qnet.", "mean_log_out.")) or ".embed_pooled." in k or ".fc1." in k:
            assert p.grad is None, (tag, k)

    def under(force):
        return oracle_scst_grads(state, feats, feat_lens, hip_words, reward, noise=replay_noise(nat, hip_words, force), **kw)[1]
    grads_match_oracle(ModelProxy(model, sample_n), named, grads, rec, under, tol_enc_of=tol_enc_of)
    model.check_persistent_launches()
    return float(loss)
