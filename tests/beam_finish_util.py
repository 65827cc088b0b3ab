"""The yardstick of the finishing beam search, written from its definition (include/acvae_hip.h,
Hybrid_VAEModel._finishing) and not from the kernels:

  retire_step / finish   a numpy twin of steps 1-3 and of the final ranking and trace-back, in the device's arithmetic
                         (float32 records, one float32 division per score), so that the kernels are compared bit for bit;
  twin_search            the whole search over a table language model, with parent pointers and -inf rows as the device
                         keeps them (flat top-k over beam * V, sorted descending, ties to the lower flat index);
  naive_search           a deliberately naive second implementation: Python lists of hypotheses that carry their own word
                         lists, no parent pointers, no -inf rows; a hypothesis that ends leaves the list.

The table language model: ``first[j, v]`` is row j's log-probability of word v at t = 0 (the rows of a clip differ from the
first step on, as the model's rows differ in z) and ``logp[prev_word, v]`` at every later step.  Entries may be -inf (banned).

``mutant`` (twin only) plants one of the mistakes the tests must catch: "record_after_retire", "rank_raw", "trace_last"."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def length_norm(T, length_penalty):
    """norm[t] = float32((t + 1) ** length_penalty), the power formed in float64."""
    return np.array([np.float32(float(t + 1) ** float(length_penalty)) for t in range(T)], dtype=np.float32)


def retire_step(c, w, end_idx, last, mutant=None):
    """Steps 1-3 on the rows of one step.  c float32 [R] (after the top-k), w int64 [R] -> (c after retiring, f)."""
    c = np.asarray(c, np.float32).copy()
    w = np.asarray(w)
    ends = w == end_idx
    if mutant == "record_after_retire":
        c[ends] = NEG_INF
    alive = c > NEG_INF
    f = np.where(alive & (ends | bool(last)), c, NEG_INF).astype(np.float32)
    c[ends] = NEG_INF
    return c, f


def finish(parent, word, f, norm, N, beam, nbest, end_idx, attw=None, mutant=None):
    """The ranking and the trace-back.  parent / word int64 [T, R] (global rows), f float32 [T, R], norm float32 [T],
    attw float32 [T, R, S] or None -> dict(seqs [N, nbest, T], scores, logprobs [N, nbest] f32, lengths [N, nbest] i32,
    attw0 [N, S, T] or None).  A parent outside [0, R) is clamped into it."""
    T, R = f.shape
    seqs = np.full((N, nbest, T), end_idx, np.int64)
    scores = np.full((N, nbest), NEG_INF, np.float32)
    logprobs = np.full((N, nbest), NEG_INF, np.float32)
    lengths = np.zeros((N, nbest), np.int32)
    attw0 = None if attw is None else np.zeros((N, attw.shape[2], T), np.float32)
    for n in range(N):
        cands = []
        for t in range(T):
            for j in range(beam):
                fv = np.float32(f[t, n * beam + j])
                if fv > NEG_INF:
                    s = fv if mutant == "rank_raw" else np.float32(fv / np.float32(norm[t]))
                    cands.append((-float(s), t, j, s, fv))
        cands.sort(key=lambda x: x[:3])
        for q, (_, t, j, s, fv) in enumerate(cands[:nbest]):
            scores[n, q], logprobs[n, q], lengths[n, q] = s, fv, t + 1
            r = n * beam + j
            if mutant == "trace_last":                           # starts at the last step, on the same row
                t = T - 1
            for tt in range(t, -1, -1):
                seqs[n, q, tt] = word[tt, r]
                p = min(max(int(parent[tt, r]), 0), R - 1)
                if q == 0 and attw0 is not None:
                    attw0[n, :, tt] = attw[tt, p]
                r = p
    return dict(seqs=seqs, scores=scores, logprobs=logprobs, lengths=lengths, attw0=attw0)


def stable_topk(flat, k):
    """Sorted descending, ties to the lower index (-inf included): acvae_topk_flat_batched's order."""
    order = np.argsort(-flat.astype(np.float64), kind="stable")[:k]
    return flat[order], order


def twin_search(first, logp, end_idx, beam, T, length_penalty, nbest, mutant=None, record=None):
    """One clip over the table language model -> finish()'s dict for N = 1, without the clip axis."""
    V = logp.shape[1]
    c = np.zeros(beam, np.float32)
    prev = None
    parent = np.zeros((T, beam), np.int64)
    word = np.zeros((T, beam), np.int64)
    f = np.zeros((T, beam), np.float32)
    for t in range(T):
        rows = first if t == 0 else logp[prev]
        scores = (c[:, None] + rows.astype(np.float32)).astype(np.float32)
        c, idx = stable_topk(scores.reshape(-1), beam)
        parent[t], word[t] = idx // V, idx % V
        c, f[t] = retire_step(c, word[t], end_idx, t == T - 1, mutant)
        prev = word[t]
        if record is not None:
            record.setdefault("c", []).append(c.copy())
    out = finish(parent, word, f, length_norm(T, length_penalty), 1, beam, nbest, end_idx, mutant=mutant)
    return {k: v[0] for k, v in out.items() if v is not None}


def naive_search(first, logp, end_idx, beam, T, length_penalty, nbest):
    """Lists of hypotheses, each with its own words.  A step expands every hypothesis still in the list by every word it may
    take, keeps the `beam` best (score descending, then the hypothesis's place in the list, then the word), writes down the
    ones that end (or all, at the last step) and drops the ended ones from the list."""
    V = logp.shape[1]
    hyps = [(np.float32(0.0), []) for _ in range(beam)]          # None: the place holds nothing any more
    done = []
    for t in range(T):
        cands = []
        for j, h in enumerate(hyps):
            if h is None:
                continue
            score, words = h
            row = first[j] if t == 0 else logp[words[-1]]
            for v in range(V):
                s = np.float32(score + np.float32(row[v]))
                if s > NEG_INF:
                    cands.append((s, j, v, words + [v]))
        cands.sort(key=lambda x: (-float(x[0]), x[1], x[2]))
        hyps = []
        for place, (s, _, v, words) in enumerate(cands[:beam]):
            if v == end_idx or t == T - 1:
                done.append((s, t, place, words))
            hyps.append(None if v == end_idx else (s, words))
    norm = length_norm(T, length_penalty)
    ranked = sorted(((np.float32(s / norm[t]), t, place, s, words) for s, t, place, words in done),
                    key=lambda x: (-float(x[0]), x[1], x[2]))[:nbest]
    seqs = np.full((nbest, T), end_idx, np.int64)
    scores = np.full(nbest, NEG_INF, np.float32)
    logprobs = np.full(nbest, NEG_INF, np.float32)
    lengths = np.zeros(nbest, np.int32)
    for q, (s, t, _, raw, words) in enumerate(ranked):
        seqs[q, :t + 1], scores[q], logprobs[q], lengths[q] = words, s, raw, t + 1
    return dict(seqs=seqs, scores=scores, logprobs=logprobs, lengths=lengths)


def random_tables(V, beam, seed, spread=2.0):
    """A seeded table language model: log-softmax rows of normal logits."""
    rng = np.random.default_rng(seed)

    def logsoftmax(x):
        x = x - x.max(-1, keepdims=True)
        return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)

    return logsoftmax(rng.normal(0, spread, (beam, V))), logsoftmax(rng.normal(0, spread, (V, V)))
