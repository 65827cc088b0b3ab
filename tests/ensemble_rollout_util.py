"""The yardstick of the ensemble rollouts (test_ensemble_rollout_cpu.py / _kernels_gpu.py / _gpu.py), in float64 numpy.

The rule of one step, for M members' logits x_m [R, V] and a noise matrix z [R, V]:
  mixture   v = log( (1/M) * sum_m softmax(x_m) ), every member at -inf -> -inf;
  score     "gumbel": (v + z) / temp;  "sample": exp(v / temp) / z, compared as its logarithm v / temp - log z (a monotone
            map: the same argmax, and no underflow at the low end of a row);
  word      the FIRST maximum of the row's scores;
  hold      a row whose previous word is end_idx gets end_idx; logprob stays v at the chosen word.
The temperature acts on the mixture, not on the members before the mixing.  `pick` states it, `pick_brute` states it again
as a plain loop over words, and `mutant=` plants the five mistakes the yardstick has to tell apart.  `rollout_twin` is the
whole rollout as a host loop over the oracle's step API, fed given words."""
import math

import numpy as np
import torch

MUTANTS = ("avg_log", "temp_per_member", "last_max", "noise_next_row", "no_hold")


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def mixture(rows, mutant=None, temp=1.0):
    """v [R, V] in float64 from the M members' rows."""
    t = temp if mutant == "temp_per_member" else 1.0
    lp = np.stack([log_softmax64(np.asarray(r, np.float64) / t) for r in rows])
    if mutant == "avg_log":
        return lp.mean(0)
    a = lp.max(0)
    safe = np.where(np.isfinite(a), a, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(a), safe + np.log(np.exp(lp - safe).sum(0) / len(rows)), -np.inf)


def log_scores(v, noise, method, temp):
    z = np.asarray(noise, np.float64)
    if method == "gumbel":
        return (v + z) / temp
    with np.errstate(divide="ignore"):
        return v / temp - np.log(z)


def pick(rows, noise, method, temp, prev_word=None, end_idx=None, mutant=None, v=None):
    """-> dict(v, score [R, V], chosen [R] (the first maximum), word [R] (after the hold), logprob [R] = v at chosen,
    gap [R]: top-1 minus top-2 score, inf where V = 1).  v: the rows' mixture where the caller has formed it already."""
    v = mixture(rows, mutant, temp) if v is None else v
    z = np.asarray(noise)
    if mutant == "noise_next_row":
        z = np.roll(z, -1, axis=0)
    s = log_scores(v, z, method, 1.0 if mutant == "temp_per_member" else temp)
    R, V = s.shape
    chosen = V - 1 - np.argmax(s[:, ::-1], -1) if mutant == "last_max" else np.argmax(s, -1)
    word = chosen.copy()
    if prev_word is not None and mutant != "no_hold":
        word[np.asarray(prev_word) == end_idx] = end_idx
    if V > 1:
        top = -np.sort(-s, -1)[:, :2]
        with np.errstate(invalid="ignore"):
            gap = top[:, 0] - top[:, 1]
    else:
        gap = np.full(R, np.inf)
    return dict(v=v, score=s, chosen=chosen, word=word, logprob=v[np.arange(R), chosen], gap=gap)


def pick_brute(rows, noise, method, temp, prev_word=None, end_idx=None):
    """The same rule, one word at a time in plain Python -> (word [R], logprob [R])."""
    M, (R, V) = len(rows), np.asarray(rows[0]).shape
    words, logprobs = [], []
    for r in range(R):
        lse = []
        for m in range(M):
            top = max(float(rows[m][r][c]) for c in range(V))
            lse.append(top + math.log(sum(math.exp(float(rows[m][r][c]) - top) for c in range(V))))
        best, best_c, best_v = None, None, None
        for c in range(V):
            p = sum(math.exp(float(rows[m][r][c]) - lse[m]) for m in range(M)) / M
            v = math.log(p) if p > 0.0 else -math.inf
            z = float(noise[r][c])
            s = (v + z) / temp if method == "gumbel" else v / temp - math.log(z)
            if best is None or s > best:                 # strict: the first maximum stays
                best, best_c, best_v = s, c, v
        held = prev_word is not None and int(prev_word[r]) == end_idx
        words.append(end_idx if held else best_c)
        logprobs.append(best_v)
    return np.array(words), np.array(logprobs)


# ------------------------------------------------------------------------------------------------ the kernel test's inputs
VS, MS, RS, TEMPS, METHODS = (1, 2, 255, 256, 257, 5000), (1, 2, 5, 8), (1, 3, 160), (0.5, 1.0, 2.0), ("gumbel", "sample")
SCALE = 2.0                       # logits N(0, 2^2), rounded to fp32


def kernel_inputs(V, M, R, method):
    """Seeded: (rows: M float32 [R, V], noise float32 [R, V]): Gumbel noise from U as the library forms it, or Exp(1)."""
    rng = np.random.default_rng([V, M, R, METHODS.index(method)])
    rows = [(rng.standard_normal((R, V)) * SCALE).astype(np.float32) for _ in range(M)]
    if method == "gumbel":
        noise = -np.log(-np.log(rng.random((R, V)) + 1e-20) + 1e-20)
    else:
        noise = np.maximum(rng.exponential(size=(R, V)), 1e-30)
    return rows, noise.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the whole rollout
@torch.no_grad()
def rollout_twin(states, encoded, sample_n, max_length, eps, noise, method, temp, feed=None):
    """The rollout as a host loop over the oracle's step API, in the style of ensemble_util.ensemble_greedy: rows
    r = n * sample_n + j share clip n's memory, every member steps on the shared word, the members' fp32 logits are mixed
    and scored in float64 by `pick`.  eps: per member [N, max_length, sample_n, E_m]; noise [max_length, R, V] (None:
    greedy, the mixture's first maximum).  feed [R, max_length] (optional): the words fed to the next step instead of the
    loop's own, so that one differing decision does not change every later one.
    -> dict(seqs i64 [R, T], logprobs f64 [R, T], gap f64 [R, T], v: the T mixtures [R, V], logits: per step the M members'
    fp32 rows [R, V])."""
    import acvae_oracle as O
    N = encoded[0][0].shape[0]
    R = N * sample_n
    st = []
    for state, (mem_all, lens_all) in zip(states, encoded):
        E, H = O._embed_size(state), state["decoder.model.weight_hh_l0"].shape[1]
        mem = mem_all.repeat_interleave(sample_n, 0)
        st.append(dict(mem=mem, lens=torch.as_tensor(lens_all).repeat_interleave(sample_n, 0), h=mem.new_zeros(R, H),
                       hc=(mem.new_zeros(R, E), mem.new_zeros(R, E)), lz=mem.new_zeros(R, E)))
    seqs = np.full((R, max_length), O.END_IDX, np.int64)
    logprobs, gaps, vs, xs = np.zeros((R, max_length)), np.zeros((R, max_length)), [], []
    w = torch.full((R,), O.START_IDX, dtype=torch.long)
    prev = None
    for t in range(max_length):
        logits = []
        for m, state in enumerate(states):
            s = st[m]
            pr = O.prior_step(state, w.unsqueeze(1), s["mem"], s["hc"], s["lz"], s["lens"], eps[m][:, t].reshape(R, -1))
            d = O.decoder_step(state, w.unsqueeze(1), s["h"], s["mem"], s["lens"], pr["z"])
            s["h"], s["hc"], s["lz"] = d["state"], pr["hiddens_state"], pr["z"]
            logits.append(d["logits"].reshape(R, -1).numpy())
        if noise is None:
            got = pick(logits, np.zeros_like(logits[0]), "gumbel", 1.0, prev, O.END_IDX)
        else:
            got = pick(logits, np.asarray(noise[t]), method, temp, prev, O.END_IDX)
        seqs[:, t], logprobs[:, t], gaps[:, t] = got["word"], got["logprob"], got["gap"]
        vs.append(got["v"])
        xs.append(logits)
        prev = np.asarray(feed[:, t]) if feed is not None else got["word"]
        w = torch.from_numpy(prev.astype(np.int64))
    return dict(seqs=seqs, logprobs=logprobs, gap=gaps, v=vs, logits=xs)
