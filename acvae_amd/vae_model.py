"""Mirror of ``models/vae_model.py`` ``Hybrid_VAEModel`` (:674-894): the autoregressive-prior +
global-constraint AC-VAE.  Same constructor ``Hybrid_VAEModel(Audioencoder, Textdecoder,
posterior_model=, posterior_args=, prior_model=, prior_args=)``, same forward contract

    forward(feats, feat_lens, caps, cap_lens, ss_ratio=, dis_ratio=)   -> training dict
    forward(feats [B], feat_lens [B], caps [N], cap_lens [N], ss_ratio=, dis_ratio=, clip_index= [N])
                                                                       -> training dict of N rows over ONE encoder pass
                                                                          of the B clips (no counterpart in the reference)
    forward(feats, feat_lens, method="greedy", max_length=, ...)       -> inference dict ("seqs", ...)

and the same state-dict names.  Host code here only draws the random decisions in the reference's
order (python ``random.random()`` per step for scheduled sampling :826, CPU ``torch.randn`` for both
reparameterisations — SURVEY F9 —, ``torch.rand(1)`` per step when dis_ratio != 0 :805), allocates
outputs and wires three autograd nodes (encoder, posterior, decode loop), each ONE call into
libacvae_hip.so for forward and one for backward.
"""
import contextlib
import os
import random
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib, search, streams, text_encoder
from .streams import scratch_buffer
from .word_model import CaptionModel
from .search import CONSTRAINTS_OFF, _constraint_args, length_norm  # noqa: F401  (their earlier home: older callers)


class _DecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, mem, mem_lens_d, caps_d, lens1_d, q_z, eps_p, ss_flags, dis_flags, Tc, sampling, *weights):
        N, S, Eenc = mem.shape
        dec = model.decoder
        E, H, A, V = dec.embed_size, dec.model.hidden_size, dec.attn.attn_size, dec.vocab_size
        dev = mem.device
        train = caps_d is not None
        params = model._text_table()
        dims = (N, Tc, S, E, H, A, V, Eenc)
        saved_b = _lib.call("acvae_decode_saved_bytes", *dims)
        scratch_b = _lib.call("acvae_decode_scratch_bytes", *dims)
        if saved_b < 0:
            raise RuntimeError(f"decode: unsupported dims {dims}")
        saved = torch.empty(saved_b, dtype=torch.uint8, device=dev)
        scratch = scratch_buffer(scratch_b, dev)
        f = lambda *s: torch.empty(*s, device=dev)
        logits, outputs = f(N, Tc, V), f(N, Tc, H)
        seqs = torch.empty(N, Tc, dtype=torch.long, device=dev)
        slp, attw = f(N, Tc), f(N, Tc, S)
        pm, pl, pz = f(N, Tc, E), f(N, Tc, E), f(N, Tc, E)
        putt = f(N, 2 * E) if train else None
        hfin, hp, cp = f(N, H), f(N, E), f(N, E)
        IntArr = _lib.ctypes.c_int * Tc
        ss_arr = IntArr(*[int(bool(x)) for x in ss_flags]) if train else None
        dis_arr = IntArr(*[int(bool(x)) for x in dis_flags]) if train else IntArr(*([1] * Tc))
        mem = mem.contiguous()
        method, temp, noise = sampling["sample"] if sampling and sampling.get("sample") else (0, 1.0, None)
        keep, drop_p = sampling["emb_keep"] if sampling and sampling.get("emb_keep") else (None, 0.0)
        # a rollout whose graph is recorded (self-critical training): the call keeps what acvae_decode_bwd reads
        rollout = bool(not train and sampling and sampling.get("rollout_grad"))
        # top-k / nucleus truncation of the sampled steps: its own entry, and the size of every kept prefix beside the words
        truncate = sampling.get("truncate") if sampling else None
        kept = torch.empty(N, Tc, dtype=torch.int32, device=dev) if truncate else None
        # constrained decoding (_constraints): its own entry again, which takes the truncation arguments on or off
        constrain = sampling.get("constrain") if sampling else None
        entry, extra = "acvae_decode_fwd_sampled", ()
        if truncate or constrain:
            entry = "acvae_decode_fwd_truncated"
            extra = (int(truncate[0]), float(truncate[1]), kept) if truncate else (0, 1.0, None)
        if constrain:
            entry, extra = "acvae_decode_fwd_constrained", extra + search._constraint_args(constrain)
        _lib.persist_status(dev)                 # the device's status words are registered before the first persistent launch
        # (plain call, nothing kept: the forward entries join both streams before they return)
        _lib.call(entry, params, mem,
                  mem_lens_d, caps_d, caps_d.stride(0) if train else 0, lens1_d, q_z, eps_p, ss_arr, dis_arr, logits,
                  outputs, seqs, slp, attw, pm, pl, pz, putt, hfin, hp, cp, saved, saved_b, scratch, scratch_b, *dims, model.start_idx,
                  model.end_idx, _lib.current_stream(), model._aux_stream(), int(method), float(temp), noise, keep,
                  float(drop_p), _lib.call_flags() | (_lib.FLAG_ROLLOUT_GRAD if rollout else 0), *extra)
        ctx.set_materialize_grads(False)         # outputs the loss does not use (outputs, p_z, ..) arrive as None, not as zero tensors
        ctx.model, ctx.saved, ctx.dims, ctx.dis_arr = model, saved, dims, dis_arr
        ctx.emb_keep, ctx.emb_p, ctx.rollout = keep, float(drop_p), rollout
        # outputs kept as plain ctx attributes would form tensor -> grad_fn -> ctx -> tensor cycles that are never collected
        ctx.save_for_backward(mem, mem_lens_d, lens1_d, eps_p, outputs, attw, pl, *((logits, seqs) if rollout else ()))
        ctx.mark_non_differentiable(seqs, attw, hfin, hp, cp, *(() if rollout else (slp,)))
        if not train:
            putt = torch.zeros(0, device=dev)
            ctx.mark_non_differentiable(putt)
        if kept is not None:
            ctx.mark_non_differentiable(kept)
            return logits, outputs, seqs, slp, attw, pm, pl, pz, putt, hfin, hp, cp, kept
        return logits, outputs, seqs, slp, attw, pm, pl, pz, putt, hfin, hp, cp

    @staticmethod
    def backward(ctx, d_logits, d_outputs, _s, d_slp, _a, d_pm, d_pl, d_pz, d_putt, *_rest):
        model = ctx.model
        N, Tc, S, E, H, A, V, Eenc = ctx.dims
        mem, mem_lens_d, lens1_d, eps_p, outputs, attw, pl = ctx.saved_tensors[:7]
        dev = mem.device
        params = model._text_table()
        grads = [None] * len(params)
        mine = set(range(0, 10)) | set(range(21, 35))
        if ctx.rollout:
            mine -= {31, 32}                     # mean_log_out took no part in a rollout: None, as torch leaves it
            if d_slp is not None:                # d sampled_logprobs -> d logits, the sampled words held constant
                logits, seqs = ctx.saved_tensors[7:]
                off = _lib.call("acvae_decode_saved_lse_offset", *ctx.dims)
                lse = ctx.saved[off:off + N * Tc * 4].view(torch.float32)
                dl = torch.empty(N, Tc, V, device=dev)
                _lib.call("acvae_logprob_bwd", logits, V, lse, seqs, d_slp.contiguous().float(), dl, N * Tc, V,
                          _lib.current_stream())
                d_logits = dl if d_logits is None else dl.add_(d_logits)
        for i, p in enumerate(params):
            if p is not None and p.requires_grad and i in mine:
                grads[i] = _lib.grad_buffer(model._grad_views, p)
        c = lambda t: None if t is None else t.contiguous().float()
        d_mem = torch.empty(N, S, Eenc, device=dev)
        d_qz = None if ctx.rollout else torch.empty(N, Tc, E, device=dev)
        scratch_b = _lib.call("acvae_decode_scratch_bytes", *ctx.dims)
        scratch = scratch_buffer(scratch_b, dev, tag="decode")
        ups = [c(t) for t in (d_logits, d_outputs, d_pm, d_pl, d_pz, d_putt)]
        main, aux = _lib.current_stream(), model._aux_stream()
        flags = _lib.call_flags(defer=model.defer_param_grads) | (_lib.FLAG_ROLLOUT_GRAD if ctx.rollout else 0)
        defers = bool(_lib.lib().acvae_decode_bwd_defers(ctx.dis_arr, Tc, main, aux, flags))   # a yes / no answer, not a status
        cur = torch.cuda.current_stream()
        side = model.streams.get("decode", cur) if defers else None
        # side: the call then leaves the parameter gradients trailing on the second stream, and autograd frees what they
        # read (saved, the upstream gradients, the encoder memory itself without an ln projection) while it still runs.
        # EVERY tensor argument is kept, not a chosen few: one kept without need only delays the reuse of its block until the
        # second stream has passed, one that is missing is a silent wrong gradient, and which of them the trailing work reads
        # is decided in csrc/decoder.hip, not here.
        _lib.call_keeping(side, "acvae_decode_bwd", params, grads, mem, mem_lens_d, lens1_d, eps_p, ctx.dis_arr, outputs, attw,
                          pl, *ups, d_mem, d_qz, ctx.saved, ctx.saved.numel(), scratch, scratch_b, *ctx.dims, main, aux,
                          ctx.emb_keep, ctx.emb_p, flags)
        if model._grad_ready_cb is not None:
            ev = torch.cuda.Event()
            ev.record(cur)
            if not defers:                       # every gradient this call writes is ordered on the current stream
                model._grad_ready_cb("decode", ev)
            else:                                # ... or on the decode calls' second stream: a second event behind its trailing work
                ev_aux = torch.cuda.Event()
                ev_aux.record(side)
                model._grad_ready_cb("decode_deferred", (ev, ev_aux))
        if defers:
            # The parameter gradients are still being computed on the decode calls' second stream (beside the posterior's and
            # the encoder's backward, which start now: d_mem and d_q_z are complete on the current stream).  Their consumers:
            # the gradient exchange (the event above) and whoever reads .grad after backward() - joined here at the end of
            # the pass.
            streams.join_after_backward(cur, side, params)
        ctx.saved = None
        outs = [next((g for p, g in zip(params, grads) if p is w), None) for w in model._decode_weights()]
        return (None, d_mem, None, None, None, d_qz, None, None, None, None, None, *outs)


def clip_rows(clip_index, n_clips, n_rows):
    """Validate the ``clip_index`` of a shared-encoder training forward (row r of the captions belongs to clip
    ``clip_index[r]``) and build the lists its kernels read: -> (index int64 [N], offsets int32 [B + 1], rows int32 [N], k),
    ``offsets`` / ``rows`` being the CSR lists of each clip's rows, ascending within a clip.  Raises ValueError for anything
    but an integer array of N entries in [0, B) in which every clip occurs the same number of times k >= 1: the shared pass
    equals the step on the repeated batch because the BatchNorm statistics over the B clips are those over the repeated batch
    and its backward means scale by exactly k, which holds only for equal multiplicities."""
    if isinstance(clip_index, torch.Tensor):
        clip_index = clip_index.detach().cpu().numpy()
    idx = np.asarray(clip_index)
    if idx.dtype == object or idx.dtype == bool or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"clip_index must be an integer array, got dtype {idx.dtype}")
    if idx.ndim != 1 or idx.shape[0] != n_rows:
        raise ValueError(f"clip_index must have one entry per caption row ({n_rows}), got shape {tuple(idx.shape)}")
    if n_clips < 1 or n_rows < 1:
        raise ValueError(f"clip_index: need at least one clip and one caption row, got {n_clips} clips and {n_rows} rows")
    idx = idx.astype(np.int64)
    if int(idx.min()) < 0 or int(idx.max()) >= n_clips:
        raise ValueError(f"clip_index entries must lie in [0, {n_clips}), got [{int(idx.min())}, {int(idx.max())}]")
    counts = np.bincount(idx, minlength=n_clips)
    if int(counts.min()) != int(counts.max()):
        raise ValueError(f"clip_index: every clip must occur the same number of times (got between {int(counts.min())} and "
                         f"{int(counts.max())} rows per clip): BatchNorm over the clips equals BatchNorm over the repeated batch "
                         "only for equal multiplicities")
    offsets = np.zeros(n_clips + 1, dtype=np.int32)
    np.cumsum(counts, out=offsets[1:])
    rows = np.argsort(idx, kind="stable").astype(np.int32)
    return idx, offsets, rows, int(counts[0])


class _ShareRowsFn(torch.autograd.Function):
    """Encoder memory of the B clips -> the N caption rows (acvae_rows_gather); the backward folds the rows' memory gradients
    into their clips' in ascending row order (acvae_rows_fold: no atomics, bit-reproducible)."""

    @staticmethod
    def forward(ctx, src, index_d, offsets_d, rows_d):
        src = src.contiguous()
        B, N, R = src.shape[0], index_d.shape[0], src[0].numel()
        dst = torch.empty((N,) + tuple(src.shape[1:]), device=src.device)
        _lib.call("acvae_rows_gather", src, index_d, dst, B, N, R, _lib.current_stream())
        ctx.dims, ctx.shape = (B, N, R), tuple(src.shape)
        ctx.save_for_backward(offsets_d, rows_d)
        return dst

    @staticmethod
    def backward(ctx, d_dst):
        offsets_d, rows_d = ctx.saved_tensors
        B, N, R = ctx.dims
        d_dst = d_dst.contiguous().float()
        d_src = torch.empty(ctx.shape, device=d_dst.device)
        _lib.call("acvae_rows_fold", d_dst, offsets_d, rows_d, d_src, B, N, R, _lib.current_stream())
        return d_src, None, None, None


class Hybrid_VAEModel(CaptionModel):
    def __init__(self, Audioencoder: nn.Module, Textdecoder: nn.Module, **kwargs):
        super().__init__(Audioencoder, Textdecoder, **kwargs)
        E = Textdecoder.embed_size
        self.qnet = getattr(text_encoder, kwargs["posterior_model"])(
            word_dim=E, embed_size=E, vocab_size=Textdecoder.vocab_size, **kwargs["posterior_args"])
        self.pnet = getattr(text_encoder, kwargs["prior_model"])(
            word_dim=E, audiofeats_size=E, embed_size=E, vocab_size=Textdecoder.vocab_size, **kwargs["prior_args"])
        self.mean_log_out = nn.Linear(E, 2 * E)
        if E != Audioencoder.embed_size:
            self.ln = nn.Linear(Audioencoder.embed_size, E)
            nn.init.xavier_uniform_(self.ln.weight)
        nn.init.xavier_uniform_(self.mean_log_out.weight)
        self.qnet._owner = weakref.ref(self)
        self.pnet._owner = weakref.ref(self)
        self.decoder._owner = weakref.ref(self)
        self._encproj_cache = {}
        self.streams = streams.SecondStreams()
        self.use_side_stream = os.environ.get("ACVAE_SIDE_STREAM", "1") != "0"
        # the decode backward leaves its parameter gradients trailing on the second stream beside the encoder backward
        # (_DecodeFn.backward joins it; ACVAE_FLAG_DEFER_PARAM_GRADS per call); ACVAE_DECODE_DEFER=0 or
        # model.defer_param_grads = False keeps everything on the main stream
        self.defer_param_grads = True
        self.staged = None         # device copies of caps / cap_lens-1 made by the last training forward
        self.noise = None          # optional replay: dict(eps_q=[N,Tc,E], eps_p=[Tc,N,E], q_keep=[Lq-1,N,Tc,2Hq] (a stacked
        #                            posterior's dropout masks, text_encoder.posterior_keep_masks)) consumed by the next forward
        #                            that draws: a call refused for its arguments before anything is drawn (ValueError /
        #                            TypeError in front of the encoder, e.g. a bad clip_index) leaves it pending for the next
        self._grad_views = None    # {param: flat-gradient view}, set by the train-step harness
        self._grad_ready_cb = None # called with "text" once every text-side gradient has been written

    # ---- plumbing: the text-side parameter table in state-dict order (include/acvae_hip.h)
    def _text_table(self):
        d, q, p = self.decoder, self.qnet, self.pnet
        g, qn, pn = d.model, q.network, p.network
        t = [d.embedding_table(), g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0,
             d.classifier.weight, d.classifier.bias, d.attn.v, d.attn.h2attn.weight, d.attn.h2attn.bias,
             q.word_embedding.weight, qn.weight_ih_l0, qn.weight_hh_l0, qn.bias_ih_l0, qn.bias_hh_l0,
             qn.weight_ih_l0_reverse, qn.weight_hh_l0_reverse, qn.bias_ih_l0_reverse, qn.bias_hh_l0_reverse,
             q.token_mean_log.weight, q.token_mean_log.bias,
             p.word_embedding.weight, p.word_attn.v, p.word_attn.h2attn.weight, p.word_attn.h2attn.bias,
             pn.weight_ih_l0, pn.weight_hh_l0, pn.bias_ih_l0, pn.bias_hh_l0, p.mean_log_out.weight, p.mean_log_out.bias,
             self.mean_log_out.weight, self.mean_log_out.bias]
        t += [self.ln.weight, self.ln.bias] if hasattr(self, "ln") else [None, None]
        assert len(t) == _lib.ENUMS_TEXT_N
        return t

    def _decode_weights(self):
        t = self._text_table()
        return [p for i, p in enumerate(t) if p is not None and (i < 10 or i >= 21)]

    def _set_grad_views(self, views):
        self._grad_views = views
        self.encoder._grad_views = views

    def _encproj(self, which, enc_mem):
        """Hoisted encoder half of an attention (0: decoder.attn, 1: pnet.word_attn) for single-step calls; cached per
        memory tensor so a beam-search loop projects the clip once instead of once per step.

        The entry is that of ``enc_mem`` AND of the ``h2attn`` weights it was computed from: the key holds the memory's and
        the weights' address and ``_version`` (``load_state_dict``, an in-place edit and a re-seated ``.data`` all show
        there), and whoever changes parameters behind torch's back - the fused optimiser writes the flat buffer through raw
        pointers - calls ``drop_step_caches()``; ``TrainStep`` does after every update.  What nothing here can see is a
        change of ``enc_mem``'s CONTENTS that leaves its ``_version`` alone, i.e. a library call that writes into a tensor
        which then comes back as ``enc_mem``: such a caller calls ``drop_step_caches()`` itself."""
        attn = self.decoder.attn if which == 0 else self.pnet.word_attn
        w, b = attn.h2attn.weight, attn.h2attn.bias
        key = (which, enc_mem.data_ptr(), tuple(enc_mem.shape), enc_mem._version,
               w.data_ptr(), w._version, b.data_ptr(), b._version)
        hit = self._encproj_cache.get(which)
        if hit is not None and hit[0] == key:
            return hit[1]
        N, S, E = enc_mem.shape
        H, A = self.decoder.model.hidden_size, self.decoder.attn.attn_size
        out = torch.empty(N, S, A if which == 0 else E, device=enc_mem.device)
        _lib.call("acvae_attn_precompute", self._text_table(), which, enc_mem, out, N, S, E, H, A,
                  _lib.current_stream())
        self._encproj_cache[which] = (key, out, enc_mem)      # keep enc_mem alive so its address cannot be reused
        return out

    def drop_step_caches(self):
        """Forget what the step API and the decoder keep between calls (the hoisted attention projections of ``_encproj``,
        the projected embedding table): for whoever changed parameters or an encoder memory's contents in a way torch's
        version counters do not show."""
        self._encproj_cache.clear()
        self.decoder._table_cache = None

    def _projected_memory(self, encoded):
        """The contiguous encoder memory [N, S, E] after the optional ``ln`` projection (vae_model.py:754-755)."""
        mem = encoded["audio_embeds"].contiguous()
        if hasattr(self, "ln"):
            N, S, Eenc = mem.shape
            E = self.decoder.embed_size
            proj = torch.empty(N, S, E, device=mem.device)
            _lib.call("acvae_gemm_nt", mem, Eenc, self.ln.weight, Eenc, self.ln.bias, proj, E, N * S, E, Eenc, 0,
                      _lib.current_stream())
            mem = proj
        return mem

    @torch.no_grad()
    def beam_search(self, encoded, max_length, beam_size, **constraints):
        """Validation beam search, models/vae_model.py:896-995: beams expanded over the flat beam*V log-probabilities of
        a clip, states re-gathered by prev_word_inds.  By default it returns beam 0 at the last step, as the reference
        does (it never fills done_beams, :986-995): a row that has emitted ``<end>`` is expanded like any other.  With
        ``finish_on_end=True`` hypotheses finish at ``<end>``, are scored by ``logprob / length ** length_penalty`` and the
        ``nbest`` best are returned (see ``_finishing``).
        All clips advance together; no host synchronisation inside the loop.

        ``constraints``: ``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``, ``suppress_tokens`` (see
        ``_constraints``), applied to every beam row's logits against the row's own word history; and ``finish_on_end``,
        ``length_penalty``, ``nbest``."""
        whole = dict(constraints, method="beam", max_length=max_length, beam_size=beam_size)
        con = self._constraints(whole, rollout=True)
        fin = self._finishing(whole)
        unknown = set(constraints) - set(search.CONSTRAINT_KEYS) - set(search.FINISH_KEYS)
        if unknown:
            raise TypeError(f"beam_search: unexpected keyword(s) {sorted(unknown)}")
        replay = self.noise.get("eps_beam") if self.noise is not None else None
        self.noise = None
        member = self._search_member(
            encoded, lambda N, E, dev: search._search_noise(N, max_length, beam_size, E, dev, replay))
        return search.beam_search([member], False, False, beam_size, max_length, self.vocab_size, int(self.start_idx),
                                  int(self.end_idx), con, fin)

    def _search_member(self, encoded, noise):
        """A member as ``acvae_amd.search`` takes it -> (memory [N, S, E], lengths i64 [N], noise, table, (S, E, H, A)).
        ``noise(N, E, device)`` draws on the host while the encoder runs: the lengths' pageable upload waits for the stream."""
        mem = self._projected_memory(encoded)
        eps = noise(mem.shape[0], mem.shape[2], mem.device)
        lens = torch.as_tensor(encoded["audio_embeds_lens"]).to(device=mem.device, dtype=torch.long).contiguous()
        dims = (mem.shape[1], mem.shape[2], self.decoder.model.hidden_size, self.decoder.attn.attn_size)
        return mem, lens, eps, self._text_table(), dims

    @torch.no_grad()
    def diverse_beam_search(self, encoded, max_length, beam_size, group_size, diversity_lambda, temperature, group_nbest,
                            dbs_impl="device"):
        """CaptionModel.diverse_beam_search (models/word_model.py:297-394) with this model's hooks (vae_model.py:
        997-1040): per clip, ``group_size`` groups of ``bdash = beam_size // group_size`` beams; group g runs one
        step behind group g-1 and its log-probabilities at a local step are lowered by ``diversity_lambda`` x the
        number of the earlier groups' beams that hold each word at that step; finished beams score logprob / length.
        The whole search is ONE library call (``acvae_dbs_search``, include/acvae_hip.h has the definition) with no host
        synchronisation.  Returns, on the device, {"seqs": i64 [N, rows, max_length], "scores": f64 [N, rows] (logprob /
        length of each returned beam), "lengths": i32 [N, rows]}, rows = ``beam_size`` with ``group_nbest`` (the first
        ``bdash * group_size`` are beams, see ``search._dbs_rows``) else ``group_size``.

        ``dbs_impl="host"`` runs the loop over the step API that the call replaces (``diverse_beam_search_host``: the same
        tokens and scores bit for bit, three read-backs per step); it is also taken when ``group_size > 16``, the library's
        limit."""
        if dbs_impl not in ("device", "host"):
            raise ValueError(f"dbs_impl must be 'device' or 'host', not {dbs_impl!r}")
        bdash = beam_size // group_size
        if bdash < 1 or bdash > 16:
            raise ValueError("diverse_beam_search: beam_size // group_size must be in 1..16")
        if dbs_impl == "host" or group_size > 16:
            return self.diverse_beam_search_host(encoded, max_length, beam_size, group_size, diversity_lambda, temperature,
                                                 group_nbest)
        G, T = int(group_size), int(max_length)
        member = self._search_member(encoded, lambda N, E, dev: search._dbs_noise(N, T * G, bdash, E, dev))
        return search.diverse_beam_search([member], False, G, bdash, T, self.vocab_size, int(self.start_idx), int(self.end_idx),
                                          temperature, diversity_lambda, group_nbest, beam_size)

    diverse_beam_search_host = search.diverse_beam_search_host     # (``dbs_impl="host"``: the loop over the step API)
    _search_noise = staticmethod(search._search_noise)             # (its earlier home, as the three names above)

    def check_persistent_launches(self, device=None):
        """Raise if a persistent decode / posterior launch on the model's device gave up (its outputs are NaN then).  Call
        behind a synchronisation point; TrainStep does at its in-flight event."""
        dev = device if device is not None else next(self.parameters()).device
        _lib.check_persist_status(dev)

    def _aux_stream(self):
        """Second HIP stream handle for the decode calls (prior chain beside the decoder chain), or None."""
        return self.streams.aux_handle() if self.use_side_stream else None

    # ---- reference API
    def train_forward(self, encoded, caps, cap_lens, **kwargs):
        return self.stepwise_forward(encoded, caps, cap_lens, **kwargs)

    def inference_forward(self, encoded, **kwargs):
        method = kwargs.get("method", "greedy")
        max_length = kwargs.get("max_length", self.max_length)
        if kwargs.get("rerank") is not None:
            raise ValueError("rerank belongs to the N-samples-per-clip routes, which know N: rollout_shared_encoder / "
                             "forward_batch_shared_encoder / evaluate(beam_size=N)")
        self._truncation(kwargs, rollout=True)
        self._constraints(kwargs, rollout=True)
        self._finishing(kwargs)
        if method == "beam":                                              # vae_model.py:884-886
            return self.beam_search(encoded, max_length, kwargs.get("beam_size", 3),
                                    **{k: kwargs[k] for k in search.CONSTRAINT_KEYS + search.FINISH_KEYS if k in kwargs})
        if method == "dbs":                                               # vae_model.py:887-893
            return self.diverse_beam_search(encoded, max_length, kwargs.get("beam_size", 5), kwargs.get("group_size", 5),
                                            kwargs.get("diversity_lambda", 0.5), kwargs.get("temperature", 1.0),
                                            kwargs.get("group_nbest", True), dbs_impl=kwargs.get("dbs_impl", "device"))
        return self.stepwise_forward(encoded, None, None, **kwargs)     # greedy / "gumbel" / anything else = multinomial

    def forward(self, *input, **kwargs):
        """models/vae_model.py:732-760.

        ``clip_index`` (training forward only, default None = the reference's contract, one feature row per caption row):
        several captions per clip over one encoder pass.  ``feats`` is then [B, T, F] and ``feat_lens`` has B entries (still
        divided in place by the encoder), ``caps`` / ``cap_lens`` have N = B * k rows and ``clip_index[r]`` names the clip of
        row r, in any order (``acvae_amd.batch.collate_groups`` sorts the rows by caption length).  Every output has N rows.
        The loss and every parameter gradient are those of the forward on ``feats[clip_index]``; see ``_share_rows`` for why
        and for the two departures (shared dropout masks, ``running_var``'s Bessel factor).  ``clip_rows`` says what is
        refused (ValueError).  ``encoder_output`` (with ``clip_index`` only, default None = nothing changes): the dict an
        earlier ``self.encoder(feats, feat_lens)`` call returned for these B clips; the encoder is then not run and
        ``feat_lens`` is used for its length alone, the number of clips: it is neither read nor divided (``acvae_amd.likelihood``
        scores several ways over one encoder pass with it).

        ``top_k`` (default 0 = off) / ``top_p`` (default 1.0 = off) with ``method="sample"`` or ``"gumbel"``: every sampled
        word is drawn among the ``top_k`` most probable words and / or the nucleus of mass ``top_p`` only (see
        ``_truncation``); the output dict then also holds ``"kept"``, int32 [N, Tc], the number of words each draw chose from.

        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_length`` / ``suppress_tokens`` (all off by default; 2-input
        forward only): constrained decoding on the device, see ``_constraints``.  ``"logits"`` then holds the constrained
        rows and ``"sampled_logprobs"`` is their log-softmax at the chosen word.

        ``finish_on_end`` (default False) / ``length_penalty`` (1.0) / ``nbest`` (1) with ``method="beam"``: hypotheses
        finish at ``<end>`` and are ranked by a length-normalised score, see ``_finishing``.  ``seqs`` / ``attn_weights``
        are then hypothesis 0's and the dict also holds ``scores``, ``lengths`` and the ``nbest_*`` entries.

        ``method="dbs"`` (``beam_size``, ``group_size``, ``diversity_lambda``, ``temperature``, ``group_nbest``): diverse beam
        search as one library call, see ``diverse_beam_search``; ``dbs_impl="host"`` (default ``"device"``) runs the host loop
        over the step API instead, with the same tokens and scores."""
        if kwargs.get("rerank") is not None:                   # (refusals come in front of the encoder's launches)
            raise ValueError("rerank in the training forward: there is nothing to choose among" if len(input) == 4 else
                             "rerank belongs to the N-samples-per-clip routes, which know N: rollout_shared_encoder / "
                             "forward_batch_shared_encoder / evaluate(beam_size=N)")
        self._truncation(kwargs, rollout=len(input) == 2)
        self._constraints(kwargs, rollout=len(input) == 2)
        self._finishing(kwargs)
        self._forward_token = getattr(self, "_forward_token", 0) + 1     # per-forward caches (decoder.embedding_table)
        clip_index = kwargs.pop("clip_index", None)
        if clip_index is not None and len(input) != 4:
            raise ValueError("clip_index belongs to the training forward (feats, feat_lens, caps, cap_lens)")
        encoder_output = kwargs.pop("encoder_output", None)
        if encoder_output is not None and (len(input) != 4 or clip_index is None):
            raise ValueError("encoder_output belongs to the training forward with clip_index=")
        if len(input) == 4:
            feats, feat_lens, caps, cap_lens = input
            # mean_log_out = Linear(embed_size, .) is fed the pooled GRU outputs (acvae_decode_fwd refuses the shape too:
            # here the refusal comes in front of the encoder's launches and names the widths)
            if self.decoder.model.hidden_size != self.decoder.embed_size:
                raise ValueError(f"training forward: the decoder's hidden_size ({self.decoder.model.hidden_size}) must equal "
                                 f"its embed_size ({self.decoder.embed_size}); other hidden sizes decode only (the "
                                 "2-input forward, beam search, rollouts)")
            # one encoder pass shared by the clips' captions: B clips, N = B * k caption rows (see _share_rows)
            share = None if clip_index is None else clip_rows(clip_index, len(feat_lens), len(cap_lens))
            if share is not None and feats.shape[0] != len(feat_lens):
                raise ValueError(f"clip_index: {feats.shape[0]} feature rows for {len(feat_lens)} feature lengths")
            n_rows = feats.shape[0] if share is None else len(cap_lens)
            # The posterior (42 serial BiGRU steps of tiny kernels) does not depend on the encoder: run it on a side
            # HIP stream beside the MFMA-bound encoder; autograd replays its backward on that stream too, where it
            # overlaps with the encoder backward.
            main = torch.cuda.current_stream()
            side = self.streams.get("posterior", main) if self.use_side_stream else main
            eps_q = None if self.noise is None else self.noise.get("eps_q")
            q_keep = None if self.noise is None else self.noise.get("q_keep")
            lens1 = np.asarray(cap_lens) - 1
            q_p = self.qnet.keep_p()
            if q_p > 0:
                # a stacked posterior's inter-layer dropout masks: nn.GRU draws them inside self.network(...), i.e. in front
                # of the posterior's randn (text_encoder.py:190,196); uploaded from the page-locked ring, in front of the encoder
                q, Tc = self.qnet, int(lens1.max())
                if q_keep is None:
                    q_keep = _lib.h2d_fill((q.num_layers - 1, n_rows, Tc, 2 * q.hidden_size), torch.uint8,
                                           feats.device, lambda buf: text_encoder.posterior_keep_masks(
                                               lens1, Tc, q.hidden_size, q.num_layers, q_p, out=buf))
                else:
                    q_keep = _lib.h2d(q_keep, feats.device, torch.uint8).contiguous()
            if eps_q is None:          # same generator order as the reference: the posterior's randn precedes the per-step draws
                eps_q = torch.randn(n_rows, int(lens1.max()), self.decoder.embed_size)
            # Host-side draws and the small H2D copies of the decode loop go in front of the encoder launch: a
            # pageable-memory copy waits for the stream to drain, which behind the encoder would stall the host.
            prep = self._host_prepare(n_rows, feats.device, caps, cap_lens, kwargs)
            if share is not None:                                  # (index on the host, index / offsets / rows on the device)
                share = (share[0],) + tuple(_lib.h2d(a, feats.device) for a in share[:3])
            # (caps_d and the masks are read by the posterior's forward and backward on the side stream)
            with streams.beside(main, side, prep["caps_d"], q_keep) as on_side:
                # The encoder is queued FIRST and the posterior second (it still starts at once: the side stream only waits
                # for what main held before this point).  Autograd runs the later-created node first, so in the backward
                # the posterior's kernels and its gradient bucket are queued before the long encoder backward: under data
                # parallelism the 20 MB posterior bucket then travels beside the encoder backward instead of behind it.
                encoded = self.encoder(feats, feat_lens) if encoder_output is None else encoder_output
                if share is not None:
                    encoded = self._share_rows(encoded, *share)
                qnetout = on_side(self.qnet, prep["caps_d"], cap_lens, eps=eps_q, keep=q_keep)
            encoded["_prep"] = prep
            encoded.update(qnetout)
            return self.train_forward(encoded, caps, cap_lens, **kwargs)
        if len(input) == 2:
            feats, feat_lens = input
            encoded = self.encoder(feats, feat_lens)
            return self.inference_forward(encoded, **kwargs)
        raise Exception("Number of input should be either 4 (feats, feat_lens, caps, cap_lens) or 2 (feats, feat_lens)")

    def _share_rows(self, encoded, index, index_d, offsets_d, rows_d):
        """The encoder's outputs for the B clips -> the N caption rows of ``forward(..., clip_index=)``: ``audio_embeds`` through
        the autograd node that folds the rows' gradients back into the clips', the pooled embedding and the lengths (known on
        the host) gathered likewise.  With an ``ln`` projection the gather acts on the encoder's own (2048-wide) rows and the
        projection stays per row, inside the decode call.

        The loss and every parameter gradient equal those of the 4-input forward on the batch in which each clip is repeated
        k times: BatchNorm's batch mean and biased variance over the clips are those over the repeated batch, the ReLU
        decisions are the same, every layer is linear in the upstream gradient and the BatchNorm-backward means scale by
        exactly k.  Two departures from that step: the rows of a clip share the encoder's dropout masks, and
        ``running_var`` carries the Bessel factor M / (M - 1) of the B clips, not kM / (kM - 1)."""
        mem, pooled = encoded["audio_embeds"], encoded["audio_embeds_pooled"].detach().contiguous()
        B, N = mem.shape[0], index_d.shape[0]
        pooled_rows = torch.empty(N, pooled.shape[1], device=pooled.device)
        _lib.call("acvae_rows_gather", pooled, index_d, pooled_rows, B, N, pooled.shape[1], _lib.current_stream())
        lens = torch.as_tensor(encoded["audio_embeds_lens"])[torch.from_numpy(index)]
        return {"audio_embeds": _ShareRowsFn.apply(mem, index_d, offsets_d, rows_d), "audio_embeds_pooled": pooled_rows,
                "state": None, "audio_embeds_lens": lens, "audio_embeds_lens_dev": _lib.h2d(lens, mem.device, torch.long)}

    def rollout_shared_encoder(self, feats, feat_lens, sample_n, **kwargs):
        """A 2-input forward with ``sample_n`` rollouts per clip that runs the encoder ONCE per clip: the memory rows are
        repeated on the device, clip-major (row ``n * sample_n + j``), and autograd folds the rows' memory gradients back
        into the clip's.  In train() the replicas of a clip therefore share the encoder's dropout masks and the BatchNorm
        statistics are those of the clips, not of the repeated batch.

        ``rerank`` (an ``acvae_amd.consensus.Consensus``, default None = nothing changes): consensus reranking of the
        clip's rollouts on the device, see ``_rerank``."""
        rerank = kwargs.pop("rerank", None)
        self._rerank_check(rerank, sample_n, kwargs)
        self._truncation(kwargs, rollout=True)
        self._constraints(kwargs, rollout=True)
        self._forward_token = getattr(self, "_forward_token", 0) + 1
        encoded = self.encoder(feats, feat_lens)
        n = int(sample_n)
        lens = torch.as_tensor(np.asarray(encoded["audio_embeds_lens"])).repeat_interleave(n, dim=0)
        rep = {"audio_embeds": encoded["audio_embeds"].repeat_interleave(n, dim=0),
               "audio_embeds_pooled": encoded["audio_embeds_pooled"].repeat_interleave(n, dim=0),
               "audio_embeds_lens": lens, "state": None}
        return self._rerank(self.inference_forward(rep, **kwargs), rerank, n)

    def _rerank_check(self, rerank, sample_n, kwargs):
        search.rerank_check(rerank, sample_n, kwargs, self.max_length, self._records_rollout())

    def _rerank(self, output, rerank, sample_n):
        """Consensus reranking of an N-samples-per-clip output (rows clip-major), on the device and without a
        synchronisation: ``seqs`` becomes the picked rows [B, T] - per clip the rollout that agrees most with the clip's
        other rollouts under CIDEr-D (``acvae_amd.consensus``) - and the dict gains ``candidates`` [B * N, T] (the rollouts),
        ``consensus_scores`` f64 [B, N] and ``consensus_best`` i64 [B].  Every other entry keeps its B * N rows."""
        if rerank is None:
            return output
        got = rerank.select(output["seqs"], sample_n, int(self.start_idx), int(self.end_idx))
        output["candidates"] = output["seqs"]
        output["seqs"] = got["seqs"]
        output["consensus_scores"] = got["scores"]
        output["consensus_best"] = got["best"]
        return output

    def _records_rollout(self):
        """A 2-input forward records a graph (self-critical training) only in train() with gradients enabled and something
        to train; every other 2-input forward is the inference path."""
        return torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())

    # ---- the keyword validators of a forward: acvae_amd.search's (which documents them), on this model's values
    def _truncation(self, kwargs, rollout=False):
        return search.truncation(kwargs, rollout, self._records_rollout())

    def _constraints(self, kwargs, rollout=False):
        return search.constraints(kwargs, self.vocab_size, self.end_idx, self.max_length, rollout, self._records_rollout())

    def _finishing(self, kwargs):
        return search.finishing(kwargs, self.max_length)

    def _host_prepare(self, N, dev, caps, cap_lens, kwargs):
        """The decode loop's host-side random decisions, in the reference's per-step order (scheduled-sampling coin
        :826, prior noise text_encoder.py:259 on the CPU generator (F9), disentangle coin :802-806), and the device
        copies of the caption ids / lengths / noise."""
        E = self.decoder.embed_size
        train = caps is not None
        if train:
            lens1 = np.asarray(cap_lens) - 1
            Tc = int(max(cap_lens)) - 1
            ss_ratio, dis_ratio = kwargs["ss_ratio"], kwargs["dis_ratio"]
        else:
            Tc = kwargs.get("max_length", self.max_length)
        replay = self.noise
        self.noise = None
        ss_flags, dis_flags = [], []
        draw = replay is None or replay.get("eps_p") is None
        # sample_next_word's method (models/word_model.py:173-207): "greedy", "gumbel", anything else = multinomial
        # sampling with `temp`.  The non-greedy branches draw one [N,V] tensor per step on the CPU generator right after
        # the step's prior noise (and dis_ratio coin): torch.rand for the Gumbel noise (:189-191), and - inside
        # torch.multinomial(., 1) - empty(N,V).exponential_(1).  Both are drawn here in that order and uploaded once.
        method = kwargs.get("method", "greedy")
        temp = float(kwargs.get("temp", 1))
        V = self.vocab_size
        code = 0 if method == "greedy" else (1 if method == "gumbel" else 2)
        top_k, top_p = self._truncation(kwargs, rollout=not train)
        constrain = self._constraints(kwargs, rollout=not train)
        # rng="device" (or model.sample_rng = "device") - opt-in, not the reference's stream: ONE draw on the CPU generator
        # seeds a counter-based generator on the device that fills the [Tc,N,V] noise (acvae_sample_noise); same
        # distributions, so the captions are samples of the same model, but not the words the reference would draw from
        # this torch seed.  The default ("host") reproduces the reference's draws one for one.
        rng = kwargs.get("rng", getattr(self, "sample_rng", "host"))
        if rng not in ("host", "device"):
            raise ValueError(f"rng must be 'host' or 'device', got {rng!r}")
        sample_noise = None
        device_noise = bool(code) and rng == "device" and (replay is None or replay.get("sample_noise") is None)
        if code and not device_noise and (replay is None or replay.get("sample_noise") is None):
            sample_noise = torch.empty(Tc, N, V)
        # the decoder's word-embedding nn.Dropout (models/decoder.py:33,184): one [N,1,E] Bernoulli draw per step, made
        # by decoder.forward, i.e. after the step's prior noise and disentangle coin and before sample_next_word
        drop_p = float(self.decoder.dropoutlayer.p) if self.decoder.training else 0.0   # nn.Dropout acts on decoder.training alone,
        # also in the 2-input forward of a model left in train() (models/decoder.py:184)
        dec_keep = None
        if drop_p > 0.0 and (replay is None or replay.get("dec_keep") is None):
            dec_keep = torch.empty(Tc, N, E, dtype=torch.bool)

        def host_draws(eps):            # eps: [Tc, N, E] staging slot (None when the noise is replayed)
            for t in range(Tc):
                if train:
                    ss_flags.append(random.random() < ss_ratio)                    # :826
                if eps is not None:
                    torch.randn(N, E, out=eps[t])                                    # text_encoder.py:259 (CPU, F9)
                if train:
                    dis_flags.append(bool(dis_ratio != 0 and torch.rand(1) <= dis_ratio))   # :802-806
                if dec_keep is not None:
                    dec_keep[t].bernoulli_(1 - drop_p)
                if sample_noise is not None:
                    if code == 1:
                        U = torch.rand(N, V)                                          # word_model.py:189-191
                        torch.neg(torch.log(-torch.log(U + 1e-20) + 1e-20), out=sample_noise[t])
                    else:
                        sample_noise[t].exponential_(1)                               # torch.multinomial(prob, 1)

        if draw:
            eps_p = _lib.h2d_fill((Tc, N, E), torch.float32, dev, host_draws)
        else:
            host_draws(None)
            eps_p = _lib.h2d(replay["eps_p"][:Tc], dev, torch.float32).contiguous()
        caps_d = lens1_d = None
        if train:
            caps_d = _lib.h2d(caps, dev, torch.long).contiguous()
            lens1_d = _lib.h2d(lens1, dev, torch.long)
        sampling = {}
        if device_noise:
            seed = int(torch.randint(0, 2 ** 62, (1,)))             # after the step draws: torch.manual_seed fixes it
            noise_d = torch.empty(Tc, N, V, device=dev, dtype=torch.float32)
            _lib.call("acvae_sample_noise", noise_d, noise_d.numel(), code, seed, _lib.current_stream())
            sampling["sample"] = (code, temp, noise_d)
        elif code:
            if sample_noise is None:
                sample_noise = torch.as_tensor(replay["sample_noise"])[:Tc]
            sampling["sample"] = (code, temp, _lib.h2d(sample_noise, dev, torch.float32).contiguous())
        if top_k > 0 or top_p < 1.0:
            sampling["truncate"] = (top_k, top_p)
        if constrain != search.CONSTRAINTS_OFF:
            sampling["constrain"] = constrain
        if drop_p > 0.0:
            if dec_keep is None:
                dec_keep = torch.as_tensor(replay["dec_keep"])[:Tc]
            sampling["emb_keep"] = (_lib.h2d(dec_keep.to(torch.uint8), dev).contiguous(), drop_p)
        return {"Tc": Tc, "ss_flags": ss_flags, "dis_flags": dis_flags, "eps_p": eps_p, "caps_d": caps_d,
                "lens1_d": lens1_d, "sampling": sampling}

    def stepwise_forward(self, encoded, caps, cap_lens, **kwargs):
        """models/vae_model.py:700-730 with decode_step (:792-816), prepare_decoder_input (:818-848) and
        stepwise_process_step (:850-869) fused into one device-side loop."""
        mem = encoded["audio_embeds"]
        dev = mem.device
        N = mem.shape[0]
        E = self.decoder.embed_size
        train = caps is not None
        mem_lens_d = encoded.get("audio_embeds_lens_dev")
        if mem_lens_d is None:
            mem_lens_d = _lib.h2d(encoded["audio_embeds_lens"], dev, torch.long)
        prep = encoded.pop("_prep", None) or self._host_prepare(N, dev, caps, cap_lens, kwargs)
        # A rollout records a graph (self-critical training: sampled_logprobs differentiable, the words constants) only in
        # train() with gradients enabled and something to train; every other 2-input forward is the inference path as before.
        record = train or self._records_rollout()
        if record and not train:
            prep["sampling"] = dict(prep.get("sampling") or {}, rollout_grad=True)
        Tc, ss_flags, dis_flags, eps_p = prep["Tc"], prep["ss_flags"], prep["dis_flags"], prep["eps_p"]
        caps_d, lens1_d = prep["caps_d"], prep["lens1_d"]
        q_z = encoded["q_z"] if train else None
        self.staged = {"caps_d": caps_d, "lens1_d": lens1_d}           # device copies the loss can reuse
        with contextlib.nullcontext() if record else torch.no_grad():
            outs = _DecodeFn.apply(self, mem, mem_lens_d, caps_d, lens1_d, q_z, eps_p, ss_flags, dis_flags, Tc,
                                   prep.get("sampling"), *self._decode_weights())
        logits, outputs, seqs, slp, attw, pm, pl, pz, putt, hfin, hp, cp = outs[:12]
        output = {"seqs": seqs, "logits": logits, "outputs": outputs, "sampled_logprobs": slp,
                  "attn_weights": attw.transpose(1, 2), "p_means": pm, "p_logs": pl, "p_z": pz,
                  "state": hfin.unsqueeze(0), "hiddens_state": (hp.unsqueeze(0), cp.unsqueeze(0)), "last_z": pz[:, -1]}
        if len(outs) > 12:                        # top_k / top_p: the number of words every draw chose from
            output["kept"] = outs[12]
        if train:
            for k in ("q_means", "q_logs", "q_z", "q_means_utt", "q_logs_utt"):
                output[k] = encoded[k]
            output["p_means_utt"] = putt
            output["p_logs_utt"] = None
        return output
