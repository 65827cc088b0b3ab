"""The decoding front of the inference searches, for one ``Hybrid_VAEModel`` or an ``Ensemble``: host code that touches
neither a model's weights nor autograd.  The keyword validators of a forward, plain functions of values (the model's
``_truncation`` / ``_constraints`` / ``_finishing`` / ``_rerank_check`` hand them its own, ``Ensemble.forward`` the
ensemble's); the noise builders, which draw on the CPU generator in the reference's order; one marshalling function per
kind of search, ``beam_search`` (greedy too) and ``diverse_beam_search``, each ONE library call over already encoded
members; and ``diverse_beam_search_host``, the host loop over the step API that ``dbs_impl="host"`` selects."""
import numpy as np
import torch

from . import _lib
from .streams import scratch_buffer


CONSTRAINT_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens")
CONSTRAINTS_OFF = (1.0, 0, 0, ())           # repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens
SUPPRESS_MAX = int(_lib._defs["ACVAE_SUPPRESS_MAX"])
FINISH_KEYS = ("finish_on_end", "length_penalty", "nbest")


def truncation(kwargs, rollout, records_rollout):
    """The ``top_k`` / ``top_p`` keywords of a forward -> (top_k, top_p), (0, 1.0) when both are off.

    ``top_k`` (int >= 0, 0 = off) keeps the k most probable words of a step; ``top_p`` (in (0, 1], exactly 1.0 = off) keeps
    the nucleus: the shortest prefix of the words, most probable first, whose mass reaches ``top_p``.  With both, the
    shorter prefix.  Equal logits rank by lower index.  The mass is that of the distribution the method samples from:
    softmax(logits / temp) for ``method="sample"``; softmax(logits) for ``"gumbel"``, where ``temp`` changes no word
    (it divides every score alike - in the reference too).  The draw is the untruncated one restricted to the kept
    words, on the same noise: the host's draws on the CPU generator and the device generator's counters do not depend
    on the keywords.  ``sampled_logprobs`` stays the log-probability under the FULL distribution.

    ValueError: a value out of range; truncation together with ``method="greedy"``, ``"beam"`` or ``"dbs"`` (nothing
    is sampled there); truncation in a 2-input forward (``rollout``) that records a differentiable rollout
    (``records_rollout``), where ``sampled_logprobs`` would not be the log-probability of the distribution sampled from."""
    top_k, top_p = kwargs.get("top_k", 0), kwargs.get("top_p", 1.0)
    top_k = 0 if top_k is None else top_k
    top_p = 1.0 if top_p is None else top_p
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0 or top_k > 0x7fffffff:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    try:
        p32 = float(np.float32(top_p))               # the value the kernel compares with
    except (TypeError, ValueError):
        raise ValueError(f"top_p must be a number in (0, 1] (1.0 = off), got {top_p!r}") from None
    if isinstance(top_p, bool) or not (0.0 < p32 <= 1.0):
        raise ValueError(f"top_p must lie in (0, 1] (1.0 = off), got {top_p!r}")
    top_k = int(top_k)
    if top_k == 0 and p32 == 1.0:
        return 0, 1.0
    given = " / ".join(f"{n}={v!r}" for n, v, on in (("top_k", top_k, top_k > 0), ("top_p", top_p, p32 < 1.0)) if on)
    method = kwargs.get("method", "greedy")
    if method in ("greedy", "beam", "dbs"):
        raise ValueError(f"{given} truncates sampled decoding (method='sample' or 'gumbel'): method={method!r} samples "
                         "nothing")
    if rollout and records_rollout:
        raise ValueError(f"{given} in a forward that records a differentiable rollout (train() with gradients enabled): "
                         "sampled_logprobs is the log-probability under the full distribution, not under the truncated "
                         "one the words are drawn from; use torch.no_grad() or eval()")
    return top_k, p32


def constraints(kwargs, vocab_size, end_idx, max_length, rollout, records_rollout):
    """The constrained-decoding keywords of a forward -> (repetition_penalty, no_repeat_ngram_size, min_length,
    suppress_tokens), ``CONSTRAINTS_OFF`` when nothing is on (``None`` = off for each; ``max_length``: the default).

    All act on a row's logits x at step t, in front of the selection, against the row's history h[0..t) (the words it
    has emitted; ``<start>`` is not part of it):
      ``repetition_penalty`` theta (1.0 = off; finite, > 0; the kernel uses float32(theta)): every distinct word w of h
        gets x[w] / theta if x[w] > 0, else x[w] * theta;
      ``no_repeat_ngram_size`` n (0 = off): every word that would complete an n-gram the caption already holds is banned
        (n = 1 bans every word of h);
      ``min_length`` m (0 = off; <= ``max_length``): ``end_idx`` is banned at steps t < m;
      ``suppress_tokens`` (() = off): at most ``SUPPRESS_MAX`` vocabulary ids banned at every step, ``end_idx`` not
        among them.
    A ban sets the logit to -inf; the penalty comes first and a ban wins.  Accepted with greedy / "sample" / "gumbel"
    (``top_k`` / ``top_p`` then truncate the constrained row) and "beam".

    ValueError, naming the keyword: a value out of range; ``method="dbs"`` (its rows keep no word histories for the
    constraint kernels to read: the library's diverse beam search takes no constraints); the 4-input (training) forward
    (``rollout`` False); a 2-input forward that records a differentiable rollout (``records_rollout``: the backward does
    not know the penalty's factor); a vocabulary too small for a row to keep a word,
    ``V <= len(suppress_tokens) + max_length + beam``."""
    V, end = int(vocab_size), int(end_idx)
    theta, n, m, ids = (kwargs.get(k) for k in CONSTRAINT_KEYS)
    theta = 1.0 if theta is None else theta
    n = 0 if n is None else n
    m = 0 if m is None else m
    ids = () if ids is None else ids
    try:
        th32 = float(np.float32(theta))              # the value the kernel uses
    except (TypeError, ValueError):
        raise ValueError(f"repetition_penalty must be a finite number > 0 (1.0 = off), got {theta!r}") from None
    if isinstance(theta, bool) or not (np.isfinite(th32) and th32 > 0.0):
        raise ValueError(f"repetition_penalty must be a finite number > 0 (1.0 = off), got {theta!r}")
    for name, v in (("no_repeat_ngram_size", n), ("min_length", m)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > 0x7fffffff:
            raise ValueError(f"{name} must be an integer >= 0 (0 = off), got {v!r}")
    n, m = int(n), int(m)
    max_length = kwargs.get("max_length", max_length)
    if m > max_length:
        raise ValueError(f"min_length={m} exceeds max_length={max_length}")
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().reshape(-1).tolist()
    try:
        ids = list(np.asarray(ids).reshape(-1).tolist()) if isinstance(ids, np.ndarray) else list(ids)
    except TypeError:
        raise ValueError(f"suppress_tokens must be a sequence of vocabulary ids, got {ids!r}") from None
    for w in ids:
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not (0 <= w < V):
            raise ValueError(f"suppress_tokens: {w!r} is not a vocabulary id in [0, {V})")
        if w == end:
            raise ValueError(f"suppress_tokens must not hold end_idx ({end}): no caption could end")
    if len(ids) > SUPPRESS_MAX:
        raise ValueError(f"suppress_tokens holds {len(ids)} ids, at most {SUPPRESS_MAX}")
    con = (th32, n, m, tuple(int(w) for w in ids))
    if con == CONSTRAINTS_OFF:
        return CONSTRAINTS_OFF
    given = " / ".join(f"{k}={v!r}" for k, v, on in zip(CONSTRAINT_KEYS, (theta, n, m, list(con[3])),
                                                        (th32 != 1.0, n > 0, m > 0, len(ids) > 0)) if on)
    method = kwargs.get("method", "greedy")
    if method == "dbs":
        raise ValueError(f"{given} with method='dbs': diverse beam search keeps its histories on the host and is not "
                         "constrained; use 'greedy', 'sample', 'gumbel' or 'beam'")
    if not rollout:
        raise ValueError(f"{given} in the 4-input (training) forward: a teacher-forced row has no history of its own; "
                         "constrained decoding belongs to the 2-input forward")
    if records_rollout:
        raise ValueError(f"{given} in a forward that records a differentiable rollout (train() with gradients enabled): "
                         "the backward does not know the penalty's factor; use torch.no_grad() or eval()")
    beam = int(kwargs.get("beam_size", 3)) if method == "beam" else 1
    if V <= len(ids) + int(max_length) + beam:
        raise ValueError(f"{given}: a vocabulary of {V} words may leave a row without a word; it must exceed "
                         f"len(suppress_tokens) + max_length + beam = {len(ids)} + {max_length} + {beam}")
    return con


def finishing(kwargs, max_length):
    """The finishing keywords of a beam search -> ``(length_penalty, nbest)``, or None when ``finish_on_end`` is off.

    The one definition (include/acvae_hip.h states the same for the C entries).  Rows r = n * beam + j of clip n.  As
    without finishing, step t forms ``scores[r, v] = c[r] + logmix_t[r, v]`` (after the constraints) and the flat top-k
    over the clip's beam * V scores (sorted descending, ties to the lower flat index, t = 0 included) gives row r its
    cumulative score ``c_t[r]``, parent ``p_t[r]`` and word ``w_t[r]``.  Then:
      1. r is alive iff ``c_t[r] > -inf``;
      2. if r is alive and (``w_t[r] == end_idx`` or ``t == max_length - 1``) the record is ``f_t[r] = c_t[r]``, else -inf;
      3. if ``w_t[r] == end_idx``, ``c_t[r] <- -inf``: the row is retired, all its children score -inf and lose to every
         alive candidate; where a clip has fewer than ``beam`` alive candidates the top-k takes such children: dead rows,
         never recorded.
    After the last step, per clip: the candidates are every (t, j) with ``f_t[n * beam + j] > -inf``; the score is
    ``s = f_t / norm[t]``, ``norm[t] = float32((t + 1) ** length_penalty)`` (float64 power on the host, one fp32 division
    on the device); the order is s descending, then t ascending, then j ascending, and the first ``nbest`` are returned;
    a hypothesis's words are its parents traced back from (t, r), ``end_idx`` behind t, its length t + 1.  With fewer than
    ``nbest`` candidates (only when bans leave a clip fewer than ``beam`` finite continuations) the missing slots are rows
    of ``end_idx`` with score -inf and length 0.  ``length_penalty`` 1.0 (the default) is the average log-probability per
    word, the rule of the reference's diverse beam search; 0 ranks by the raw log-probability.

    The search itself is unchanged: all ``max_length`` steps run, retired and dead rows keep being stepped, nothing is
    read back.  The output dict holds hypothesis 0 as ``seqs`` [N, T] (and ``attn_weights``, zeros behind its length),
    ``scores`` / ``lengths`` [N], and ``nbest_seqs`` [N, nbest, T], ``nbest_scores`` / ``nbest_logprobs`` (the raw f) f32
    [N, nbest], ``nbest_lengths`` int32 [N, nbest].

    ValueError: ``finish_on_end`` with a method other than "beam"; ``length_penalty`` / ``nbest`` without
    ``finish_on_end``; a ``length_penalty`` that is negative or not finite (or whose table overflows float32);
    ``nbest`` outside [1, beam_size]."""
    on, lp, nbest = (kwargs.get(k) for k in FINISH_KEYS)
    on = False if on is None else on
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"finish_on_end must be True or False, got {on!r}")
    if not on:
        for k, v in (("length_penalty", lp), ("nbest", nbest)):
            if v is not None:
                raise ValueError(f"{k}={v!r} without finish_on_end=True: it ranks finished hypotheses only")
        return None
    method = kwargs.get("method", "greedy")
    if method != "beam":
        raise ValueError(f"finish_on_end=True with method={method!r}: finishing belongs to method='beam'")
    lp = 1.0 if lp is None else lp
    try:
        lpf = float(lp)
    except (TypeError, ValueError):
        raise ValueError(f"length_penalty must be a finite number >= 0, got {lp!r}") from None
    if isinstance(lp, bool) or not (np.isfinite(lpf) and lpf >= 0.0):
        raise ValueError(f"length_penalty must be a finite number >= 0, got {lp!r}")
    beam = int(kwargs.get("beam_size", 3))
    nbest = 1 if nbest is None else nbest
    if isinstance(nbest, bool) or not isinstance(nbest, (int, np.integer)) or not (1 <= nbest <= beam):
        raise ValueError(f"nbest must be an integer in [1, beam_size = {beam}], got {nbest!r}")
    if not np.isfinite(length_norm(kwargs.get("max_length", max_length), lpf)).all():
        raise ValueError(f"length_penalty={lp!r}: max_length ** length_penalty overflows float32")
    return lpf, int(nbest)


def rerank_check(rerank, sample_n, kwargs, max_length, records_rollout):
    """The refusals of ``rerank=`` (ValueError, in front of every launch): a search (``method="beam"`` / ``"dbs"``
    returns its own best hypotheses), fewer than 2 or more than 16 candidates per clip, rows longer than the kernel
    takes, a forward that records a differentiable rollout (``records_rollout``; the picked rows are a choice among
    constants: nothing flows back through it)."""
    if rerank is None:
        return
    from . import consensus
    if not isinstance(rerank, consensus.Consensus):
        raise ValueError(f"rerank must be an acvae_amd.consensus.Consensus, got {type(rerank).__name__}")
    method = kwargs.get("method", "greedy")
    if method in ("beam", "dbs"):
        raise ValueError(f"rerank with method={method!r}: a search returns its own best hypotheses; consensus reranking "
                         "chooses among N rollouts of 'greedy', 'sample' or 'gumbel'")
    consensus.check_sample_n(sample_n, "rerank")
    max_length = kwargs.get("max_length", max_length)
    if max_length > consensus.MAX_LENGTH:
        raise ValueError(f"rerank: max_length={max_length}; the kernel takes rows of at most {consensus.MAX_LENGTH} tokens")
    if records_rollout:
        raise ValueError("rerank in a forward that records a differentiable rollout (train() with gradients enabled): "
                         "the picked rows are a choice among constants; use torch.no_grad() or eval()")


def _constraint_args(constrain):
    """(theta, n, m, ids) -> the five trailing arguments of the ``acvae_*_constrained`` entries.  The list is a HOST array
    that the entry reads before it returns; the ctypes pointer keeps the array alive until then."""
    theta, n, m, ids = constrain
    arr = np.ascontiguousarray(ids, dtype=np.int32)
    return float(theta), int(n), int(m), (arr.ctypes.data_as(_lib.ctypes.c_void_p) if len(ids) else None), len(ids)


def length_norm(max_length, length_penalty):
    """The finishing beam search's norm table, float32 [max_length]: ``norm[t] = float32((t + 1) ** length_penalty)``, the
    power formed in float64 on the host.  The device divides a record by its entry, one fp32 division."""
    def power(t):
        try:
            return float(t + 1) ** float(length_penalty)
        except OverflowError:
            return float("inf")

    with np.errstate(over="ignore"):                     # (an overflow is the caller's to refuse: finishing)
        return np.array([power(t) for t in range(int(max_length))], np.float64).astype(np.float32)


def _finishing_args(fin, max_length, N, dev):
    """(length_penalty, nbest) -> the n-best outputs and the six trailing arguments of the ``acvae_*_finishing`` entries.  The
    norm table is a HOST array that the entry reads before it returns."""
    lp, nbest = fin
    norm = length_norm(max_length, lp)
    out = {"nbest_seqs": torch.empty(N, nbest, max_length, dtype=torch.long, device=dev),
           "nbest_scores": torch.empty(N, nbest, device=dev), "nbest_logprobs": torch.empty(N, nbest, device=dev),
           "nbest_lengths": torch.empty(N, nbest, dtype=torch.int32, device=dev)}
    args = (norm.ctypes.data_as(_lib.ctypes.c_void_p), nbest, out["nbest_seqs"], out["nbest_scores"], out["nbest_logprobs"],
            out["nbest_lengths"])
    return out, args, norm


def _finishing_output(seqs, nb):
    """The dict of a finishing search: hypothesis 0 under the keys of today, the n-best list beside it."""
    return dict(nb, seqs=seqs, scores=nb["nbest_scores"][:, 0], lengths=nb["nbest_lengths"][:, 0])


def _dbs_rows(out, beam_size, group_nbest, end_idx):
    """With ``group_nbest`` the reference returns ``beam_size`` rows per clip and fills ``bdash * group_size`` of them:
    where ``group_size`` does not divide ``beam_size`` the rest hold ``end_idx`` (score -inf, length 0), as they did."""
    seqs, scores, lengths = out["seqs"], out["scores"], out["lengths"]
    extra = beam_size - seqs.shape[1] if group_nbest else 0
    if extra <= 0:
        return out
    N, _, T = seqs.shape
    return {"seqs": torch.cat([seqs, seqs.new_full((N, extra, T), end_idx)], dim=1),
            "scores": torch.cat([scores, scores.new_full((N, extra), float("-inf"))], dim=1),
            "lengths": torch.cat([lengths, lengths.new_zeros((N, extra))], dim=1)}


def _search_noise(N, max_length, beam, E, dev, replay):
    """The prior's noise of one search on the device, step-major [max_length, N, beam, E] as the library reads it.  The
    reference walks the clips one after the other; their searches are independent, so all N x beam rows advance together
    inside one library call.  Its noise order (clip-major: text_encoder.py:259 inside the clip loop) is kept by drawing
    eps[clip][t] in that order on the host; ``replay`` [N, max_length, beam, E] is uploaded instead of a draw."""
    if replay is None:
        return _lib.h2d_fill((max_length, N, beam, E), torch.float32, dev,
                             lambda buf: [torch.randn(beam, E, out=buf[t, i]) for i in range(N) for t in range(max_length)])
    return _lib.h2d(torch.as_tensor(replay).reshape(N, max_length, beam, E).transpose(0, 1).contiguous(), dev,
                    torch.float32)


def _dbs_noise(N, n_steps, bdash, E, dev):
    """The prior's noise of one diverse beam search on the device, step-major [n_steps, N, bdash, E] as the library reads
    it, drawn on the CPU generator in the reference's order: clip, then step k of the (t, group) schedule
    (text_encoder.py:259 inside those loops), ``torch.randn(bdash, E)`` each."""
    return _lib.h2d_fill((n_steps, N, bdash, E), torch.float32, dev,
                         lambda buf: [torch.randn(bdash, E, out=buf[k, i]) for i in range(N) for k in range(n_steps)])


# ---- one call per search.  A member, already encoded: (memory [N, S, E], lengths int64 [N] on the device, noise, parameter
# table, (S, E, H, A)).  ``ensemble`` picks the entry family: False, the single-model entries (one member; they keep beam
# 0's attention weights); True, the ``acvae_ensemble_*`` entries over M >= 1 members (the mixture's log-probabilities).
def _member_args(members, ensemble):
    """-> (who, widths, lead, keep): table, memory, lengths, noise and the widths S, E, H, A as four ints; for an ensemble
    tables of each, four HOST int32 arrays and ``lead`` = (M,), with what the pointers point to in ``keep`` until the call."""
    C = _lib.ctypes
    if not ensemble:
        (mem, lens, eps, table, dims), = members
        return (table, mem, lens, eps), tuple(dims), (), None
    tables = [_lib.ptr_table(m[3]) for m in members]
    params = (C.c_void_p * len(members))(*[C.cast(t, C.c_void_p).value for t in tables])
    arrays = [np.ascontiguousarray([m[4][j] for m in members], dtype=np.int32) for j in range(4)]
    who = (params,) + tuple([m[j] for m in members] for j in range(3))
    return who, tuple(a.ctypes.data for a in arrays), (len(members),), (tables, arrays)


def beam_search(members, ensemble, greedy, beam, T, V, start_idx, end_idx, con, fin):
    """Greedy (``greedy``, beam = 1, ensembles only) or beam search of width ``beam`` over ``T`` steps, ONE library call:
    the plain, ``_constrained`` (``con != CONSTRAINTS_OFF``) or ``_finishing`` (``fin`` not None: it takes the constraints
    too, on or off) entry of the family and the scratch its size function asks for.  -> {"seqs", the n-best entries of a
    finishing search, and "attn_weights" [N, S, T] (one model) or "logprobs" (ensemble: [N, T] greedy, [N] beam)}."""
    who, widths, lead, keep = _member_args(members, ensemble)
    dev, N = members[0][0].device, members[0][0].shape[0]
    base = "acvae_ensemble_search" if ensemble else "acvae_beam_search"
    kind = "_finishing" if fin is not None else "_constrained" if con != CONSTRAINTS_OFF else ""
    sb = _lib.call(base + kind + "_scratch_bytes", *lead, N, beam, T, *widths, V)
    if sb < 0:
        raise RuntimeError(f"{base}: unsupported dimensions (N={N}, beam={beam}, max_length={T})")
    scratch = scratch_buffer(sb, dev)
    seqs = torch.empty(N, T, dtype=torch.long, device=dev)
    if ensemble:
        side = torch.empty((N, T) if greedy else (N,), device=dev)
        args = (*who, *widths, *lead, start_idx, end_idx, 1 if greedy else 0, seqs, side, scratch, sb, N, beam, T, V,
                _lib.current_stream())
    else:
        side = torch.empty(N, widths[0], T, device=dev)
        args = (*who, start_idx, seqs, side, scratch, sb, N, beam, T, *widths, V, _lib.current_stream())
        args += (end_idx,) if kind else ()
    nb, fargs, _norm = _finishing_args(fin, T, N, dev) if fin is not None else (None, (), None)
    _lib.call(base + kind, *args, *(_constraint_args(con) if kind else ()), *fargs)
    out = {"seqs": seqs} if nb is None else _finishing_output(seqs, nb)
    out["logprobs" if ensemble else "attn_weights"] = side
    return out


ROLLOUT_METHODS = {"greedy": int(_lib._defs["ACVAE_SAMPLE_GREEDY"]), "gumbel": int(_lib._defs["ACVAE_SAMPLE_GUMBEL"]),
                   "sample": int(_lib._defs["ACVAE_SAMPLE_MULTINOMIAL"])}


def ensemble_rollout(members, method, temp, top_k, top_p, noise, sample_n, T, V, start_idx, end_idx, con):
    """``sample_n`` rollouts per clip over ``T`` steps from the members' mixture, ONE call (``acvae_ensemble_rollout``): the
    rows of a clip share its memory, nothing is replicated.  ``noise`` f32 [T, N * sample_n, V] on the device (None with
    ``method="greedy"``).  -> {"seqs" i64, "logprobs" f32}, both [N * sample_n, T], rows clip-major."""
    who, widths, lead, keep = _member_args(members, True)
    dev, N = members[0][0].device, members[0][0].shape[0]
    sb = _lib.call("acvae_ensemble_rollout_scratch_bytes", *lead, N, sample_n, T, *widths, V)
    if sb < 0:
        raise RuntimeError(f"acvae_ensemble_rollout: unsupported dimensions (N={N}, sample_n={sample_n}, max_length={T})")
    scratch = scratch_buffer(sb, dev)
    seqs = torch.empty(N * sample_n, T, dtype=torch.long, device=dev)
    logprobs = torch.empty(N * sample_n, T, device=dev)
    _lib.call("acvae_ensemble_rollout", *who, *widths, *lead, start_idx, end_idx, ROLLOUT_METHODS[method], float(temp), top_k,
              float(top_p), noise, seqs, logprobs, scratch, sb, N, sample_n, T, V, _lib.current_stream(),
              *_constraint_args(con))
    return {"seqs": seqs, "logprobs": logprobs}


def diverse_beam_search(members, ensemble, G, bdash, T, V, start_idx, end_idx, temperature, diversity_lambda, group_nbest,
                        beam_size):
    """Diverse beam search, ``G`` groups of ``bdash`` beams over ``T`` steps, ONE call (``acvae_[ensemble_]dbs_search``).
    -> {"seqs" [N, rows, T], "scores" f64 [N, rows], "lengths" i32 [N, rows]} through ``_dbs_rows``."""
    who, widths, lead, keep = _member_args(members, ensemble)
    dev, N = members[0][0].device, members[0][0].shape[0]
    rows = G * bdash if group_nbest else G
    seqs = torch.empty(N, rows, T, dtype=torch.long, device=dev)
    scores = torch.empty(N, rows, dtype=torch.float64, device=dev)
    lengths = torch.empty(N, rows, dtype=torch.int32, device=dev)
    name = "acvae_ensemble_dbs_search" if ensemble else "acvae_dbs_search"
    sb = _lib.call(name + "_scratch_bytes", *lead, N, G, bdash, T, *widths, V)
    if sb < 0:
        raise RuntimeError(f"{name}: unsupported dimensions (N={N}, group_size={G}, bdash={bdash}, max_length={T})")
    scratch = scratch_buffer(sb, dev)
    dims = (start_idx, end_idx, N, G, bdash, T)
    _lib.call(name, *who, *((*widths, *lead, *dims) if ensemble else (*dims, *widths)), V, float(temperature),
              float(diversity_lambda), 1 if group_nbest else 0, seqs, scores, lengths, scratch, sb, _lib.current_stream())
    return _dbs_rows({"seqs": seqs, "scores": scores, "lengths": lengths}, beam_size, group_nbest, end_idx)


@torch.no_grad()
def diverse_beam_search_host(model, encoded, max_length, beam_size, group_size, diversity_lambda, temperature, group_nbest):
    """``Hybrid_VAEModel.diverse_beam_search`` as a host loop (``dbs_impl="host"``): host bookkeeping (sequence tables,
    finished beams) as in the reference, which also reads the chosen words back every step; prior / decoder step, the
    score transform and the flat top-k are library calls.  The yardstick of the one-call search, and its stand-in beyond
    16 groups."""
    mem_all = model._projected_memory(encoded)
    dev = mem_all.device
    lens_all = torch.as_tensor(encoded["audio_embeds_lens"]).to(torch.long)
    N, S, E = mem_all.shape
    V = model.vocab_size
    bdash = beam_size // group_size
    if bdash < 1 or bdash > 16:
        raise ValueError("diverse_beam_search: beam_size // group_size must be in 1..16")
    R = N * bdash
    st = _lib.current_stream
    # The clips are independent, so they advance together: rows = clips x bdash per (t, group) step; one host read-back
    # per step for the whole batch (the reference reads back per clip and step).  The reference's noise order — clip,
    # then t, then group (text_encoder.py:259 inside those loops) — is kept by drawing every eps up front in it.
    steps = [(t, g) for t in range(max_length + group_size - 1) for g in range(group_size)
             if 0 <= t - g <= max_length - 1]
    eps_all = _lib.h2d_fill((N, len(steps), bdash, E), torch.float32, dev,
                            lambda buf: [torch.randn(bdash, E, out=buf[i, k]) for i in range(N)
                                         for k in range(len(steps))])
    mem = mem_all.repeat_interleave(bdash, dim=0).contiguous()
    lens = lens_all.repeat_interleave(bdash)
    scores = torch.empty(R, V, device=dev)
    vals = torch.empty(R, device=dev)
    idx, prev_d, nxt_d = (torch.empty(R, dtype=torch.long, device=dev) for _ in range(3))
    seq = [[np.zeros((bdash, 0), np.int64) for _ in range(group_size)] for _ in range(N)]
    score = [np.zeros((N, bdash), np.float32) for _ in range(group_size)]
    done = [[[] for _ in range(group_size)] for _ in range(N)]
    carry = [None] * group_size
    base = (np.arange(N) * bdash)[:, None]
    for k, (t, g) in enumerate(steps):
        lt = t - g
        if lt == 0:
            w = torch.full((R,), model.start_idx, dtype=torch.long, device=dev)
            state = model.decoder.init_hidden(R).to(dev)
            hid = model.pnet.init_hidden(R, dev)
            last_z = torch.zeros(R, E, device=dev)
        else:
            state0, hid0, z0, w, parent = carry[g]
            state = state0[:, parent].contiguous()
            hid = (hid0[0][:, parent].contiguous(), hid0[1][:, parent].contiguous())
            last_z = z0[parent].contiguous()
        pn = model.pnet(w.unsqueeze(1), mem, hid, last_z, lens, eps=eps_all[:, k].reshape(R, E))
        dn = model.decoder(word=w.unsqueeze(1), state=state, enc_mem=mem, enc_mem_lens=lens, z=pn["z"])
        logits = dn["logits"].squeeze(1)
        counts = None
        if g > 0:                                        # add_diversity (:298-312), one count vector per clip
            c = np.zeros((N, V), np.float32)
            for i in range(N):
                for earlier in range(g):
                    np.add.at(c[i], seq[i][earlier][:, lt], 1.0)
            counts = _lib.h2d(c, dev)
        _lib.call("acvae_dbs_scores", logits, V, float(temperature), counts, float(diversity_lambda),
                  _lib.h2d(score[g].reshape(-1), dev), scores, R, V, bdash if g > 0 else 0, st())
        _lib.call("acvae_topk_flat_batched", scores, V if lt == 0 else bdash * V, bdash * V, bdash, V, vals, idx, prev_d,
                  nxt_d, N, bdash, st())
        top = vals.cpu().numpy().reshape(N, bdash).copy()              # one read-back per step for all clips
        parent_h = prev_d.cpu().numpy().reshape(N, bdash) - base        # beam index within the clip
        nxt_h = nxt_d.cpu().numpy().reshape(N, bdash)
        last = t == max_length + g - 1
        for i in range(N):
            sq = np.concatenate([seq[i][g][parent_h[i]] if lt > 0 else seq[i][g], nxt_h[i][:, None]], axis=1)
            seq[i][g] = sq
            ended = sq[:, lt] == model.end_idx
            if last:
                ended[:] = True
            for b_ in range(bdash):
                if ended[b_]:
                    done[i][g].append({"seq": sq[b_].copy(), "score": float(top[i, b_]) / (lt + 1)})
            top[i][ended] -= np.float32(1000)
        score[g] = top
        carry[g] = (dn["state"], pn["hiddens_state"], pn["z"], nxt_d.clone(), prev_d.clone())
    rows = bdash * group_size if group_nbest else group_size
    out = torch.full((N, rows, max_length), model.end_idx, dtype=torch.long)
    out_scores = torch.zeros(N, rows, dtype=torch.float64)
    out_lengths = torch.zeros(N, rows, dtype=torch.int32)
    for i in range(N):
        ranked = [sorted(d, key=lambda x: -x["score"])[:bdash] for d in done[i]]
        chosen = sum(ranked, []) if group_nbest else [d[0] for d in ranked]
        for r, beam in enumerate(chosen):
            out[i, r, :len(beam["seq"])] = torch.from_numpy(beam["seq"])
            out_scores[i, r] = beam["score"]
            out_lengths[i, r] = len(beam["seq"])
    return _dbs_rows({"seqs": out.to(dev), "scores": out_scores.to(dev), "lengths": out_lengths.to(dev)}, beam_size,
                     group_nbest, int(model.end_idx))
