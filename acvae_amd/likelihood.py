"""Given captions scored under the model, on the device: per-caption log-likelihood, KL, perplexity, top-1 / top-5 accuracy.

The question a user of a variational captioner asks of a trained model: how likely is THIS caption for this clip, and how
much of that does the latent carry?  The reference has no counterpart: its only loss-shaped number is the training
objective's batch scalar, label-smoothed and with the KL averaged over padded positions too.  Here one
teacher-forced forward (``ss_ratio=1``) of the 4-input ``Hybrid_VAEModel.forward`` is followed by two launches
(csrc/likelihood.hip): ``acvae_caption_terms`` turns logits, targets and the two Gaussians into per-step log-probability,
rank and KL, ``acvae_caption_sums`` adds them up per row in float64.  Nothing is label-smoothed and every sum runs over the
caption's own steps only.

Per caption row with words w_0 = <start>, w_1 .. w_L (w_L = <end>), steps t = 0 .. L - 1, target of step t = w_{t+1}:
  logprob_t = log_softmax(logits_t)[w_{t+1}],   rank_t = the target's position in the row under the first-maximum rule
  (rank_t == 0: the greedy decode would have emitted it),   kl_t = sum_e KL(q_t || p_t) (``Normal_kl_loss``'s term),
  nll = -sum_t logprob_t,  kl = sum_t kl_t,  tokens = L,  hit1 / hit5 = #{t : rank_t < 1} / #{t : rank_t < 5}.

``z="posterior"`` (``dis_ratio=0``): the decoder reads the posterior's sample at every step.  ``nll`` is the reconstruction
term and ``kl`` the masked KL of the training objective, per caption: ``nll + kl`` is the per-caption negative of what
training maximises at ``kl_weight = 1`` (without label smoothing).
``z="prior"`` (``dis_ratio=1``): every draw decodes the caption with the latent sequence the prior chain generates for
itself - exactly the generative process the 2-input forward samples from.  ``log_marginal = logmeanexp_k(-nll_k)`` over the
K draws is a Monte-Carlo estimate of log p(caption | audio): a lower bound in expectation that tightens with K, and the
perplexity is ``exp(-sum log_marginal / sum tokens)``.  (``kl`` is still reported: the posterior against the chain's own
path.)
Out of scope: an importance-weighted (IWAE) bound.  The prior conditions each step on its OWN previous sample
(``vae_model.py:797,869``), so the model never evaluates the prior's density along the posterior's sample path; a bound that
needs p(z^q) would measure another model.
"""
import math

import numpy as np
import torch

from . import _lib
from .frontend import refuse_augmented

MODES = ("posterior", "prior")
MAX_SAMPLES = 16


# ------------------------------------------------------------------------------------------------ refusals (host only)
def check_mode(z, who="score_captions"):
    if not isinstance(z, str) or z not in MODES:
        raise ValueError(f"{who}: z must be one of {MODES}, got {z!r}")
    return z


def check_samples(samples, who="score_captions"):
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not (1 <= samples <= MAX_SAMPLES):
        raise ValueError(f"{who}: 1 <= samples <= {MAX_SAMPLES} noise draws per caption, got {samples!r}")
    return int(samples)


def check_model(model, who="score_captions"):
    dec = model.decoder
    if dec.model.hidden_size != dec.embed_size:
        raise ValueError(f"{who}: the decoder's hidden_size ({dec.model.hidden_size}) must equal its embed_size "
                         f"({dec.embed_size}): scoring runs the training forward, which has that rule")


class Rows:
    """The caption rows of one scoring forward.  P (clip, caption) pairs, K draws each: the pairs sorted by caption length,
    descending and stable, as ``collate_groups`` sorts its rows, the K rows of a pair adjacent (row ``pos * K + k``).
    ``pair`` int64 [P * K]: the caller's pair of each row; ``clip`` int64 [P * K]: its clip; ``lens`` [P * K]: its caption
    length; ``place`` int64 [P]: the sorted position of the caller's pair i."""

    def __init__(self, cap_lens, clip_index, n_clips, samples, who="score_captions"):
        lens = np.asarray(cap_lens)
        if lens.ndim != 1 or lens.shape[0] < 1 or not np.issubdtype(lens.dtype, np.integer):
            raise ValueError(f"{who}: cap_lens must be a non-empty integer array, one entry per caption")
        P = lens.shape[0]
        if int(lens.min()) < 2:
            raise ValueError(f"{who}: a caption of {int(lens.min())} token(s); the shortest caption is <start> <end>")
        if clip_index is None:
            if P != n_clips:
                raise ValueError(f"{who}: {P} captions for {n_clips} clips; with several captions per clip (or another order) "
                                 "say which clip each caption belongs to with clip_index=")
            clip = np.arange(P, dtype=np.int64)
        else:
            clip = np.asarray(clip_index)
            if clip.ndim != 1 or clip.shape[0] != P or clip.dtype == bool or not np.issubdtype(clip.dtype, np.integer):
                raise ValueError(f"{who}: clip_index must be an integer array with one entry per caption ({P})")
            clip = clip.astype(np.int64)
            if int(clip.min()) < 0 or int(clip.max()) >= n_clips:
                raise ValueError(f"{who}: clip_index entries must lie in [0, {n_clips})")
        counts = np.bincount(clip, minlength=n_clips)
        if int(counts.min()) != int(counts.max()):
            raise ValueError(f"{who}: every clip needs the same number of captions (got between {int(counts.min())} and "
                             f"{int(counts.max())}): the shared-encoder forward (clip_index=) has that rule; pad the smaller "
                             "sets, e.g. by repeating one of the clip's captions, and drop the padding's records")
        order = np.argsort(-lens.astype(np.int64), kind="stable")
        self.P, self.K = P, int(samples)
        self.pair = np.repeat(order, self.K)
        self.clip = clip[self.pair]
        self.lens = lens[self.pair]
        self.place = np.empty(P, dtype=np.int64)
        self.place[order] = np.arange(P)


# ------------------------------------------------------------------------------------------------ the two launches
def caption_terms(output, targets_d, lens1_d):
    """The two launches on a teacher-forced forward's output dict (``logits`` [R, T, V], and - all four or no KL -
    ``q_means`` / ``q_logs`` / ``p_means`` / ``p_logs`` [R, T, E]); ``targets_d`` i64 [R, >= T] on the device, the target of
    step t in column t (``caps_d[:, 1:]``); ``lens1_d`` i64 [R] (``cap_lens - 1``) or None.  -> the five per-row tensors
    ``nll`` / ``kl`` f64 [R], ``tokens`` / ``hit1`` / ``hit5`` i32 [R] and the three maps ``logprob`` f32 / ``rank`` i32 /
    ``kl_steps`` f32 [R, T], invalid cells exact zeros.  No host synchronisation."""
    logits = output["logits"].detach()
    _lib.require_cuda(logits, targets_d, lens1_d)
    if logits.dtype != torch.float32 or logits.stride(2) != 1:
        logits = logits.float().contiguous()
    R, T, V = logits.shape
    dev = logits.device
    if targets_d.dtype != torch.long or targets_d.stride(1) != 1:
        targets_d = targets_d.to(torch.long).contiguous()
    if targets_d.shape[0] != R or targets_d.shape[1] < T:
        raise ValueError(f"caption_terms: targets of shape {tuple(targets_d.shape)} for logits of {R} rows and {T} steps")
    gauss = [output.get(k) for k in ("q_means", "q_logs", "p_means", "p_logs")]
    E = 0
    if any(g is None for g in gauss):
        gauss = [None] * 4
    else:
        gauss = [g.detach().float().contiguous() for g in gauss]
        E = gauss[0].shape[2]
        if any(tuple(g.shape) != (R, T, E) for g in gauss):
            raise ValueError(f"caption_terms: the Gaussians must all be [{R}, {T}, E], got {[tuple(g.shape) for g in gauss]}")
    logprob = torch.empty(R, T, device=dev)
    rank = torch.empty(R, T, dtype=torch.int32, device=dev)
    kl_steps = torch.empty(R, T, device=dev)
    nll, kl = (torch.empty(R, dtype=torch.float64, device=dev) for _ in range(2))
    tokens, hit1, hit5 = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(3))
    st = _lib.current_stream()
    _lib.call("acvae_caption_terms", logits, logits.stride(0), logits.stride(1), targets_d, targets_d.stride(0), lens1_d,
              *gauss, logprob, rank, kl_steps, R, T, V, E, st)
    _lib.call("acvae_caption_sums", logprob, rank, kl_steps, lens1_d, nll, kl, tokens, hit1, hit5, R, T, st)
    return {"nll": nll, "kl": kl, "tokens": tokens, "hit1": hit1, "hit5": hit5, "logprob": logprob, "rank": rank,
            "kl_steps": kl_steps}


# ------------------------------------------------------------------------------------------------ the front
class eval_mode:
    """``model.eval()`` and ``torch.no_grad()`` for a block; every module gets back the mode it had."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        self.grad = torch.no_grad()
        self.grad.__enter__()

    def __exit__(self, *exc):
        self.grad.__exit__(*exc)
        for m, mode in self.modes:
            m.training = mode
        return False


def _refusals(model, n_clips, cap_lens, clip_index, z, samples, frontend, who):
    refuse_augmented(frontend, who)
    check_mode(z, who)
    samples = check_samples(samples, who)
    check_model(model, who)
    return Rows(cap_lens, clip_index, n_clips, samples, who)


def encode_clips(model, feats, feat_lens, frontend, device):
    """One encoder pass over the clips -> (features on the device, the encoder's output dict)."""
    if frontend is not None:
        feats, feat_lens = frontend(feats, feat_lens, device=device)
    feats = feats.to(device)
    feat_lens = np.array(feat_lens)                    # a copy: the encoder divides its lengths in place
    return feats, feat_lens, model.encoder(feats, feat_lens)


def score_rows(model, feats, feat_lens, encoded, caps, rows, z):
    """One teacher-forced forward of ``rows`` over the clips' encoder output, the two launches, and the records put back
    into the caller's order."""
    P, K = rows.P, rows.K
    caps = torch.as_tensor(caps)
    dev = feats.device
    place_d = _lib.h2d(rows.place, dev, torch.long)     # (in front of the launches, like every small upload here)
    out = model(feats, feat_lens, caps[torch.from_numpy(rows.pair)], rows.lens, ss_ratio=1.0,
                dis_ratio=0 if z == "posterior" else 1, clip_index=rows.clip, encoder_output=encoded)
    staged = model.staged
    got = caption_terms(out, staged["caps_d"][:, 1:], staged["lens1_d"])
    rec = {k: v.view((P, K) + tuple(v.shape[1:])).index_select(0, place_d) for k, v in got.items()}
    rec["tokens"] = rec["tokens"][:, 0].contiguous()
    rec.update(z=z, samples=K)
    return rec


def score_captions(model, feats, feat_lens, caps, cap_lens, clip_index=None, z="posterior", samples=1, frontend=None):
    """How likely are these captions for these clips?

    ``feats`` [B, T, F] / ``feat_lens`` [B]: the clips (with ``frontend=`` an ``acvae_amd.frontend.LogMel``: waveforms
    [B, Lmax] and sample counts; an ``Augmented`` front end is refused).  ``caps`` [P, L] / ``cap_lens`` [P]: the captions as
    the training forward takes them, ``<start> w .. <end>`` zero-padded.  ``clip_index`` [P]: the clip of each caption (None:
    P = B, caption i belongs to clip i); every clip must have the same number of captions, the shared-encoder forward's own
    rule (pad a smaller set by repeating a caption).  All pairs of B clips x C captions (``caps`` tiled B times,
    ``clip_index = repeat(arange(B), C)``) give the B x C matrix of a retrieval evaluation.

    Runs under ``model.eval()`` and ``torch.no_grad()`` and restores the modes it found.  ONE encoder pass over the clips; every
    pair is replicated ``samples`` = K times (1 <= K <= 16) through the ``clip_index`` route, the K rows differing in their
    noise only (``model.noise`` replays ``eps_q`` [P * K, Tc, E] / ``eps_p`` [Tc, P * K, E] in the order of ``Rows``); one
    teacher-forced forward (``ss_ratio=1``; ``dis_ratio`` 0 for ``z="posterior"``, 1 for ``z="prior"`` - the module's
    docstring says what each measures), then ``caption_terms``.

    -> a record of device tensors in the CALLER's order of pairs, no host synchronisation inside:
    ``nll`` / ``kl`` f64 [P, K], ``hit1`` / ``hit5`` i32 [P, K], ``tokens`` i32 [P], the maps ``logprob`` f32 / ``rank`` i32 /
    ``kl_steps`` f32 [P, K, Tc] (exact zeros behind a caption's end), and ``z``, ``samples``.  ``Likelihood`` turns records
    into numbers.

    ValueError in front of any launch and any random draw: ``samples`` outside 1 .. 16, another ``z``, a caption shorter
    than ``<start> <end>``, unequal numbers of captions per clip, a decoder whose ``hidden_size != embed_size``."""
    who = "score_captions"
    rows = _refusals(model, len(feat_lens), cap_lens, clip_index, z, samples, frontend, who)
    device = next(model.parameters()).device
    with eval_mode(model):
        feats, feat_lens, encoded = encode_clips(model, feats, feat_lens, frontend, device)
        return score_rows(model, feats, feat_lens, encoded, caps, rows, z)


# ------------------------------------------------------------------------------------------------ the accumulator
def logmeanexp(x):
    """log(mean(exp(x))) over the last axis, max-shifted; float64."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.log(np.exp(x - m).mean(axis=-1)) + m[..., 0]


def summarize(keys, nll, kl, tokens, hit1, hit5, kl_steps, z):
    """The formulas, float64, on host arrays: ``nll`` / ``kl`` / ``hit1`` / ``hit5`` [P, K], ``tokens`` [P], ``kl_steps`` a
    list of P arrays [K, >= tokens[i]].  Per pair: nll = mean_k nll_k, kl = mean_k kl_k, log_marginal =
    logmeanexp_k(-nll_k) (``z="prior"``; None for ``z="posterior"``, where no draw's nll is a likelihood of the caption).
    Corpus: nll_per_token = sum_i s_i / sum_i tokens_i with s_i = -log_marginal_i (prior) or nll_i (posterior),
    perplexity = exp(nll_per_token), kl_per_token = sum kl / sum tokens, top1 / top5 = sum hit / (K sum tokens),
    kl_by_step[t] = the mean of kl_steps[i][:, t] over the draws of the captions with tokens_i > t."""
    nll, kl = np.asarray(nll, dtype=np.float64), np.asarray(kl, dtype=np.float64)
    tokens = np.asarray(tokens).astype(np.int64)
    P, K = nll.shape
    pair_nll, pair_kl = nll.mean(axis=1), kl.mean(axis=1)
    marg = logmeanexp(-nll) if z == "prior" else None
    score = -marg if z == "prior" else pair_nll
    n_tok = int(tokens.sum())
    per_token = float(score.sum()) / n_tok
    steps = int(tokens.max())
    by_step = []
    for t in range(steps):
        vals = [np.asarray(kl_steps[i], dtype=np.float64)[:, t] for i in range(P) if tokens[i] > t]
        by_step.append(float(np.concatenate(vals).mean()))
    pairs = [{"key": keys[i], "nll": float(pair_nll[i]), "kl": float(pair_kl[i]),
              "log_marginal": None if marg is None else float(marg[i]), "tokens": int(tokens[i])} for i in range(P)]
    return {"z": z, "samples": K, "pairs": pairs, "captions": P, "tokens": n_tok, "nll_per_token": per_token,
            "perplexity": math.exp(per_token), "kl_per_token": float(pair_kl.sum()) / n_tok,
            "top1": float(np.asarray(hit1, dtype=np.float64).sum()) / (K * n_tok),
            "top5": float(np.asarray(hit5, dtype=np.float64).sum()) / (K * n_tok), "kl_by_step": by_step}


class Likelihood:
    """``Likelihood(z=, samples=)``: ``update(keys, record)`` with the records of ``score_captions`` (one key per pair, e.g.
    ``(audio_id, caption number)``), then ``result()``.  ``update`` keeps the device tensors as they are - no copy, no
    synchronisation; ``result()`` makes ONE download and evaluates ``summarize`` in float64."""

    def __init__(self, z="posterior", samples=1):
        self.z = check_mode(z, "Likelihood")
        self.samples = check_samples(samples, "Likelihood")
        self.reset()

    def reset(self):
        self._keys, self._records = [], []

    def update(self, keys, record):
        keys = list(keys)
        if record["z"] != self.z or record["samples"] != self.samples:
            raise ValueError(f"Likelihood(z={self.z!r}, samples={self.samples}): a record of z={record['z']!r}, "
                             f"samples={record['samples']}")
        if record["nll"].shape != (len(keys), self.samples):
            raise ValueError(f"Likelihood: {len(keys)} keys for a record of shape {tuple(record['nll'].shape)}")
        self._keys += keys
        self._records.append(record)

    def result(self):
        if not self._records:
            raise ValueError("Likelihood: result() without an update")
        names = ("nll", "kl", "tokens", "hit1", "hit5", "kl_steps")
        flat = torch.cat([r[k].reshape(-1).to(torch.float64) for r in self._records for k in names]).cpu().numpy()
        cols = {k: [] for k in names}
        steps, at = [], 0
        for r in self._records:                        # every number is exact in float64 (fp32, int32 or float64 itself)
            for k in names:
                n = r[k].numel()
                cols[k].append(flat[at:at + n].reshape(tuple(r[k].shape)))
                at += n
            steps += list(cols["kl_steps"][-1])
        cat = {k: np.concatenate(cols[k], axis=0) for k in names[:-1]}
        return summarize(self._keys, cat["nll"], cat["kl"], cat["tokens"], cat["hit1"], cat["hit5"], steps, self.z)
