"""Write tests/golden/g18_scst.npz from the reference's self-critical sequence training, on the CPU: ``ScstWrapper``
(models/seq_train_model.py:9-92), ``scst_Loss`` and ``Nscst_Loss`` (utils/train_util.py:292-413).

The reference is imported at run time through oracle/ref_shim.py; only data is stored: inputs, keys, vocabulary words and
reference sentences, the noise each rollout drew (prior eps, Exp(1) sampling noise, encoder dropout keep-masks bit-packed),
and the reference's ``greedy_seqs``, ``sampled_seqs``, ``sampled_logprobs``, ``reward``, ``score`` and ``loss``.  Forward
values only: the reference cannot differentiate this loss under current torch (the fed word is a view of ``seqs`` that is
written in place afterwards).  Parameters are acvae_oracle.closed_form_state (never stored).  ``feat_lens`` goes in as a
list: with an array the reference's encoder divides it in place once per rollout.

Three parts, all V = 50, E = 64, three ragged clips of up to 96 frames, max_length 12:
  scst_*    ``ScstWrapper.forward``: greedy rollout in eval(), sampled rollout in train(), one generator.  The oracle makes
            the same two rollouts on the same generator and must return the same words and loss (asserted) - its record
            is the stored noise.
  loss_*    ``scst_Loss`` on those rollouts.
  n_*       ``Nscst_Loss`` (sample_n = 5) on a sampled rollout of the model in train() over
            ``feats.repeat_interleave(5, 0)`` with the encoder's dropout switched off (F.dropout replaced by the identity
            for the run), so that the five replicas of a clip see the same memory, as an encode-once implementation's do.

The scorer is a stub (share of the hypothesis' words that occur in the clip's references), defined here and again in the
tests.  Run: python tools/make_scst_golden.py  (deterministic)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import acvae_oracle as O  # noqa: E402
import ref_shim  # noqa: E402
from check_oracle_vs_reference import load_state_into  # noqa: E402

V, E, B, T, MAXLEN, SAMPLE_N, SEED = 50, 64, 3, 96, 12, 5, 31


class StubScorer:
    """Share of the hypothesis' words found in the key's references (0 for an empty hypothesis)."""

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


def text_side():
    words = ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]
    g = torch.Generator().manual_seed(SEED)
    keys = [f"clip{i}" for i in range(B)]
    refs = [[" ".join(words[int(j)] for j in torch.randint(4, V, (9,), generator=g)) for _ in range(3)] for _ in keys]
    return words, keys, refs


def pad_steps(x, fill):
    out = torch.full((MAXLEN,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    out[:x.shape[0]] = x
    return out


def pack(prefix, masks):
    d = {}
    for i, m in enumerate(masks):
        d[f"{prefix}drop{i}_bits"] = np.packbits(m.numpy().astype(np.uint8).reshape(-1))
        d[f"{prefix}drop{i}_shape"] = np.array(m.shape)
    return d


def policy_loss(slp, seqs, reward):
    mask = (seqs != O.END_IDX).float()
    mask = torch.cat([torch.ones(mask.size(0), 1), mask[:, :-1]], 1)
    return (-slp * torch.as_tensor(reward).float()[:, None] * mask).sum(1).mean()


def main():
    ref = ref_shim.load()
    import models.seq_train_model as stm
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, _, feat_lens, _ = O.synthetic_batch(B, T, V, 8, seed=SEED, ragged=True)
    words, keys, refs = text_side()
    key2refs = dict(zip(keys, refs))
    vocab, scorer = Vocabulary(words), StubScorer()
    out = dict(dims=np.array([B, T, V, E, MAXLEN, SAMPLE_N]), feats=feats.numpy(), feat_lens=np.asarray(feat_lens),
               words=np.array(words), keys=np.array(keys), refs=np.array(refs))

    # ---- ScstWrapper
    model = ref_shim.build_reference_model(ref, V, E, E)
    load_state_into(model, state)
    torch.manual_seed(SEED)
    ro = stm.ScstWrapper(model)(feats, [int(x) for x in feat_lens], keys, key2refs, vocab, max_length=MAXLEN, scorer=scorer)
    ostate = {k: v.clone() for k, v in state.items()}
    torch.manual_seed(SEED)
    rg, rs = {}, {}
    with torch.no_grad():
        og = O.hybrid_forward(ostate, feats, [int(x) for x in feat_lens], training=False, method="greedy",
                              max_length=MAXLEN, record=rg)
    os_ = O.hybrid_forward(ostate, feats, [int(x) for x in feat_lens], training=True, method="sample", temp=1,
                           max_length=MAXLEN, record=rs)
    assert torch.equal(og["seqs"], ro["greedy_seqs"]) and torch.equal(os_["seqs"], ro["sampled_seqs"])
    steps = os_["_steps_run"]
    oloss = policy_loss(os_["sampled_logprobs"], os_["seqs"][:, :steps], ro["reward"].numpy())
    assert torch.equal(oloss.detach(), ro["loss"].detach()), (float(oloss), float(ro["loss"]))
    sd = model.state_dict()
    for k in ("encoder.bn0.running_mean", "encoder.conv_block4.bn2.running_var"):
        assert torch.equal(sd[k], ostate[k]), k
    print(f"ScstWrapper: loss {float(ro['loss'].detach()):.14f}, reward {ro['reward'].tolist()}, steps greedy {og['_steps_run']} "
          f"sampled {steps}; smallest margin greedy {float(rg['margins'].min()):.2e} sampled {float(rs['margins'].min()):.2e}")
    slp = torch.zeros(B, MAXLEN)
    slp[:, :steps] = os_["sampled_logprobs"].detach()
    out.update(scst_greedy_seqs=ro["greedy_seqs"].numpy(), scst_sampled_seqs=ro["sampled_seqs"].numpy(),
               scst_sampled_logprobs=slp.numpy(), scst_reward=ro["reward"].numpy(), scst_score=ro["score"].numpy(),
               scst_loss=ro["loss"].detach().numpy(), scst_steps=np.array([og["_steps_run"], steps]),
               scst_greedy_eps_p=pad_steps(rg["eps_p"], 0.0).numpy(), scst_eps_p=pad_steps(rs["eps_p"], 0.0).numpy(),
               scst_sample_noise=pad_steps(rs["sample_noise"], 1.0).numpy(),
               scst_bn0_running_mean=sd["encoder.bn0.running_mean"].numpy())
    out.update(pack("scst_noise_", rs["dropout"]))

    # ---- scst_Loss on the same rollouts
    lo = ref.train_util.scst_Loss(scorer, device="cpu")(
        dict(greedy_seqs=ro["greedy_seqs"], sampled_seqs=ro["sampled_seqs"], sampled_logprobs=slp), keys, key2refs, vocab)
    out.update(loss_reward=lo["reward"].numpy(), loss_score=lo["score"].numpy(), loss_loss=lo["loss"].numpy())

    # ---- Nscst_Loss: sample_n rollouts per clip, features repeated clip-major, encoder dropout off
    model = ref_shim.build_reference_model(ref, V, E, E)
    load_state_into(model, state)
    model.train()
    featsN = feats.repeat_interleave(SAMPLE_N, 0)
    lensN = [int(x) for x in feat_lens for _ in range(SAMPLE_N)]
    orig = F.dropout
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    odrop = O._dropout
    O._dropout = lambda x, p, training, masks, record: x
    try:
        torch.manual_seed(SEED + 1)
        with torch.no_grad():
            rn = model(featsN, list(lensN), method="sample", temperature=1.0, max_length=MAXLEN)
        torch.manual_seed(SEED + 1)
        rec = {}
        with torch.no_grad():
            on = O.hybrid_forward({k: v.clone() for k, v in state.items()}, featsN, list(lensN), training=True,
                                  method="sample", temp=1, max_length=MAXLEN, record=rec)
    finally:
        F.dropout, O._dropout = orig, odrop
    assert torch.equal(on["seqs"], rn["seqs"])
    nsteps = on["_steps_run"]
    nslp = torch.zeros(B * SAMPLE_N, MAXLEN)
    nslp[:, :nsteps] = rn["sampled_logprobs"][:, :nsteps]
    dlp = float((nslp[:, :nsteps] - on["sampled_logprobs"]).abs().max())
    assert dlp <= 1e-5, dlp
    no = ref.train_util.Nscst_Loss(scorer, sample_n=SAMPLE_N, device="cpu")(
        dict(sampled_seqs=rn["seqs"], sampled_logprobs=nslp), keys, key2refs, vocab)
    print(f"Nscst_Loss: loss {float(no['loss']):.14f}, mean reward {float(no['reward']):.6f}, steps {nsteps}; smallest "
          f"margin {float(rec['margins'].min()):.2e}; |logprob - oracle| {dlp:.1e}; words\n{rn['seqs']}")
    out.update(n_sampled_seqs=rn["seqs"].numpy(), n_sampled_logprobs=nslp.numpy(), n_reward_mean=no["reward"].numpy(),
               n_score=no["score"].numpy(), n_loss=no["loss"].numpy(), n_steps=np.array(nsteps),
               n_eps_p=pad_steps(rec["eps_p"], 0.0).numpy(), n_sample_noise=pad_steps(rec["sample_noise"], 1.0).numpy())
    dst = os.path.join(ROOT, "tests", "golden", "g18_scst.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
