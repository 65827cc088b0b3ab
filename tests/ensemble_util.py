"""CPU restatement of ensemble greedy and ensemble beam decoding, the yardstick of test_ensemble_cpu.py / test_ensemble_gpu.py.

Composed from the oracle's validated pieces: O.cnn10_forward (Cnn10 and Cnn14_16k), O.prior_step, O.decoder_step and
O._topk_margins.  The mixing rule is runners/base_runner.py:616-618, 675-686: mean of the members' softmax, then log.  It is
carried onto Hybrid_VAEModel's step as O.beam_search runs it (prior step -> z -> decoder step), with
  - the flat top-k over beam * V at every step, t = 0 included (the beam rows of a clip differ in z);
  - greedy: a row that has produced <end> keeps emitting and feeding <end>, all max_length steps run.
The members' fp32 logits are mixed in float64 (the yardstick should add no rounding of its own to a decision), and the
decision margins are recorded per clip as O.beam_search(record=) does:
  greedy - top-1 minus top-2 of the mixture at each step up to and including the row's <end>;
  beam   - the k-th minus the (k+1)-th flat score of every step, plus the last step's first-minus-second score.
eps: per member [N, max_length, beam, E_m] (greedy: beam = 1)."""
import numpy as np
import torch
import torch.nn.functional as F

import acvae_oracle as O


def encode(state, feats, feat_lens):
    """(mem [N, S, E] after the member's ln, lens [N]) of one member; feat_lens is not modified."""
    with torch.no_grad():
        enc = O.cnn10_forward(state, feats, np.array(feat_lens).copy(), training=False)
        mem = enc["audio_embeds"]
        if "ln.weight" in state:
            mem = F.linear(mem, state["ln.weight"], state["ln.bias"])
    return mem.contiguous(), torch.as_tensor(enc["audio_embeds_lens"]).clone()


def mix_logprobs(logits_list):
    """log( mean_m softmax(logits_m) ) in float64; logits_m [R, V]."""
    probs = torch.stack([torch.softmax(l.double(), -1) for l in logits_list]).mean(0)
    return torch.log(probs)


def _dims(state):
    return O._embed_size(state), state["decoder.model.weight_hh_l0"].shape[1], state["decoder.classifier.weight"].shape[0]


@torch.no_grad()
def ensemble_greedy(states, encoded, max_length, eps, record=None):
    """-> (seqs i64 [N, max_length], logprobs f64 [N, max_length]); encoded = [encode(state_m, ...)] per member."""
    N = encoded[0][0].shape[0]
    st = []
    for state, (mem, _) in zip(states, encoded):
        E, H, _ = _dims(state)
        st.append(dict(h=mem.new_zeros(N, H), hc=(mem.new_zeros(N, E), mem.new_zeros(N, E)), lz=mem.new_zeros(N, E)))
    seqs = torch.full((N, max_length), O.END_IDX, dtype=torch.long)
    logprobs = torch.zeros(N, max_length, dtype=torch.float64)
    margins = [[] for _ in range(N)]
    done = torch.zeros(N, dtype=torch.bool)
    w = torch.full((N,), O.START_IDX, dtype=torch.long)
    for t in range(max_length):
        logits = []
        for m, (state, (mem, lens)) in enumerate(zip(states, encoded)):
            s = st[m]
            pr = O.prior_step(state, w.unsqueeze(1), mem, s["hc"], s["lz"], lens, eps[m][:, t, 0])
            d = O.decoder_step(state, w.unsqueeze(1), s["h"], mem, lens, pr["z"])
            s["h"], s["hc"], s["lz"] = d["state"], pr["hiddens_state"], pr["z"]
            logits.append(d["logits"])
        lp = mix_logprobs(logits)
        top = lp.topk(2, -1).values
        best, arg = lp.max(-1)
        for i in range(N):
            if not done[i]:
                margins[i].append(float(top[i, 0] - top[i, 1]))
        w = torch.where(done, torch.full_like(arg, O.END_IDX), arg)
        seqs[:, t] = w
        logprobs[:, t] = best
        done = done | (w == O.END_IDX)
    if record is not None:
        record["margins"] = margins
    return seqs, logprobs


@torch.no_grad()
def ensemble_beam(states, encoded, beam, max_length, eps, record=None):
    """-> (seqs i64 [N, max_length], beam 0's final score f64 [N]).  The clips' searches are independent; their beam rows
    advance together (row n * beam + j), which only saves the yardstick time."""
    N = encoded[0][0].shape[0]
    V = _dims(states[0])[2]
    R = N * beam
    st = []
    for state, (mem_all, lens_all) in zip(states, encoded):
        E, H, _ = _dims(state)
        mem = mem_all.repeat_interleave(beam, 0)
        st.append(dict(mem=mem, lens=torch.as_tensor(lens_all).repeat_interleave(beam, 0), h=mem.new_zeros(R, H),
                       hc=(mem.new_zeros(R, E), mem.new_zeros(R, E)), lz=mem.new_zeros(R, E)))
    margins = [[] for _ in range(N)]
    top_k = torch.zeros(N, beam, dtype=torch.float64)
    base = (torch.arange(N) * beam).unsqueeze(1)
    w = torch.full((R,), O.START_IDX, dtype=torch.long)
    seqs = None
    for t in range(max_length):
        logits = []
        for m, state in enumerate(states):
            s = st[m]
            if t > 0:
                s["h"] = s["h"][prev]; s["hc"] = (s["hc"][0][prev], s["hc"][1][prev]); s["lz"] = s["lz"][prev]
            pr = O.prior_step(state, w.unsqueeze(1), s["mem"], s["hc"], s["lz"], s["lens"],
                              eps[m][:, t].reshape(R, -1))
            d = O.decoder_step(state, w.unsqueeze(1), s["h"], s["mem"], s["lens"], pr["z"])
            s["h"], s["hc"], s["lz"] = d["state"], pr["hiddens_state"], pr["z"]
            logits.append(d["logits"])
        flat = (top_k.reshape(R, 1) + mix_logprobs(logits)).view(N, beam * V)
        for i in range(N):
            margins[i].extend(O._topk_margins(flat[i], beam, t == max_length - 1))
        top_k, top_words = flat.topk(beam, 1, True, True)
        prev = (base + torch.div(top_words, V, rounding_mode="trunc")).reshape(R)        # rows of the whole batch
        w = (top_words % V).reshape(R)
        seqs = w.unsqueeze(1) if t == 0 else torch.cat([seqs[prev], w.unsqueeze(1)], dim=1)
    if record is not None:
        record["margins"] = margins
    return seqs.view(N, beam, max_length)[:, 0].clone(), top_k[:, 0].clone()
