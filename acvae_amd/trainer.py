"""Train-step harness: the body of ``Runner.train``'s inner loop (``runners/pytorch_runner_vae.py:286,
311-324``) around the HIP model — zero_grad, ``_forward`` (:76-98), loss = CE + kl_weight*KL (+ alpha*MSE),
backward, ``clip_grad_norm_(max_grad_norm)``, ``optimizer.step`` (Adam, AdamW or SGD from the config, :219; see
acvae_amd/optim.py) — with the MI355X-specific plumbing:

  * all parameters live in ONE flat fp32 buffer and all gradients in another (the backward kernels write
    straight into it), so the global-norm clip is one reduction and Adam is one fused pass
    (acvae_grad_norm / acvae_adam_step), and the data-parallel exchange is three large RCCL all-reduces
    (text-side bucket and the encoder's last ConvBlock, each launched from inside the backward as soon as its
    gradients are queued and overlapped with the rest of the encoder backward, then the remaining 5 MB of the
    encoder) instead of ~60 per-tensor buckets;
  * one process per GPU over ``torch.distributed`` (backend "nccl" = RCCL over xGMI); gradients are
    averaged like torch DDP does (reference :204-207); BatchNorm statistics stay local per rank (the
    reference uses plain BatchNorm2d) and rank 0's running buffers are broadcast before each forward
    (DDP's default broadcast_buffers=True).
"""
import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, streams
from .optim import (FlatOptimizer, check_coverage, check_group, check_groups, chunk_table, group_segments, resolve,
                    resolve_groups)
from .train_util import KLObjective, LabelSmoothingLoss, MSELoss, Normal_kl_loss, combine_losses


class FlatGradExchange:
    """Data-parallel gradient exchange over one flat buffer split into ordered buckets.

    ``ready(i, after=...)`` launches the asynchronous SUM all-reduce of bucket i (called from the backward as soon as
    the bucket's gradients are queued, so it overlaps with the rest of the backward); ``finish()`` waits for all of
    them and returns the factor 1/world that the consumer folds into its next kernel (norm / Adam), which makes it an
    average like torch DDP's.  Device-agnostic (RCCL on MI355X, gloo in the CPU tests).

    Stream contract (RCCL): a collective is ordered behind the stream that is CURRENT when it is issued, nothing else.
    Nothing here relies on which stream that happens to be: every bucket is issued from a dedicated exchange stream
    that first waits for (a) an event recorded on the announcing stream behind the last kernel queued there - the
    producer of the bucket - and (b) every event in ``after`` (recorded behind the last kernel that writes into the
    bucket on any OTHER stream).  ``finish()`` orders the collectives in front of the caller's current stream.
    A bucket larger than ``max_chunk`` elements goes on the wire as several collectives (first byte sooner; the ring
    pipelines them).  ``issued`` records the (bucket, chunk) sequence: it must be identical on every rank."""

    def __init__(self, flat, bucket_sizes, group=None, max_chunk=8 << 20):
        self.flat, self.group = flat, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.max_chunk = int(max_chunk)
        self.slices, off = [], 0
        for n in bucket_sizes:
            self.slices.append((off, off + n))
            off += n
        assert off <= flat.numel()
        self._works, self._done, self.issued = [], set(), []
        self._xstream = None

    def begin(self):
        self._works, self._done, self.issued = [], set(), []

    def ready(self, i, after=()):
        if self.world == 1 or i in self._done:
            return
        self._done.add(i)
        a, b = self.slices[i]
        if b <= a:
            return
        ctx = contextlib.nullcontext()
        if self.flat.is_cuda:
            dev = self.flat.device
            produced = torch.cuda.Event()
            produced.record(torch.cuda.current_stream(dev))       # behind the kernels the announcing node just queued
            if self._xstream is None:
                self._xstream = torch.cuda.Stream(dev)
            self._xstream.wait_event(produced)
            for ev in after:
                if ev is not None:
                    self._xstream.wait_event(ev)
            ctx = torch.cuda.stream(self._xstream)
        k = 0
        with ctx:
            while a < b:
                e = min(b, a + self.max_chunk)
                self._works.append(dist.all_reduce(self.flat[a:e], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                self.issued.append((i, k))
                a, k = e, k + 1

    def finish(self):
        for i in range(len(self.slices)):
            self.ready(i)                      # any bucket nobody announced (e.g. frozen sub-model)
        for w in self._works:
            w.wait()
        self._works = []
        return 1.0 / self.world


def max_over_ranks(value, device="cpu", group=None):
    """bench.py timing contract: the step time of the job is the MAX over ranks."""
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return float(t.item())


def kl_weight_for(epoch, epochs, beta):
    """runners/pytorch_runner_vae.py:286: max(0.5, epoch/epochs*beta)"""
    return max(0.5, float(epoch) / epochs * beta)


def kl_weight_cyclical(step, cycle_steps, ratio=0.5, beta=1.0, floor=0.0):
    """Cyclical KL weight (Fu et al. 2019): within each cycle of ``cycle_steps`` steps the weight rises linearly from ``floor``
    to ``beta`` over the first ``ratio`` of the cycle, then holds ``beta`` until the cycle ends and the next starts at ``floor``
    again.  ``step`` counts from 0.  A host function, as ``kl_weight_for``: its value goes to ``TrainStep.step(kl_weight=)``."""
    if cycle_steps < 1 or not 0.0 < ratio <= 1.0 or step < 0:
        raise ValueError(f"kl_weight_cyclical: step {step} >= 0, cycle_steps {cycle_steps} >= 1 and 0 < ratio {ratio} <= 1 wanted")
    pos = (step % cycle_steps) / float(cycle_steps)            # where in the cycle, [0, 1)
    return float(floor + (beta - floor) * min(1.0, pos / ratio))


def ema_decay_at(decay, t, warmup=False):
    """The EMA decay of the update that follows ``t`` applied updates: ``decay``, or with ``warmup`` min(decay, (1 + t) /
    (10 + t)) (the first update averages with 1/10, the tenth with 10/19, ...).  A host float: nothing is synchronised."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def check_accumulation(accum_steps, ema_decay, ema_warmup):
    """ValueError for what TrainStep(accum_steps=, ema_decay=, ema_warmup=) refuses; host arithmetic only."""
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, (int, np.integer)) or accum_steps < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, not {accum_steps!r}")
    if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), not {ema_decay!r}")
    if ema_warmup and ema_decay is None:
        raise ValueError("ema_warmup=True needs ema_decay")


DEFAULT_MAX_SKIPS = 50
_UNSET = object()                                   # max_skips not given: DEFAULT_MAX_SKIPS with the guard, nothing without
# the guard record of include/acvae_hip.h (acvae_guard_record) as int32 words
GUARD_RECORD_BYTES = 112
_GUARD_OK, _GUARD_WINDOW_BAD = 8, 9                 # int32 word offsets; the four int64 counters are words 0..7


def check_guard(nonfinite, max_skips=_UNSET, optimizer=None, groups=()):
    """ValueError for what TrainStep(nonfinite=, max_skips=) refuses; host arithmetic only.  ``groups``: the resolved
    param-group dicts of ``optimizer`` (the momentum rule needs them)."""
    if nonfinite not in (None, "skip"):
        raise ValueError(f"nonfinite must be None or 'skip', not {nonfinite!r}")
    if max_skips is not _UNSET and max_skips is not None:
        if isinstance(max_skips, bool) or not isinstance(max_skips, (int, np.integer)) or max_skips < 1:
            raise ValueError(f"max_skips must be a positive integer or None, not {max_skips!r}")
    if max_skips is not _UNSET and nonfinite is None:
        raise ValueError("max_skips= needs nonfinite='skip'")
    if nonfinite is not None and optimizer == "SGD" and any(float(g.get("momentum", 0)) != 0 for g in groups):
        raise ValueError("nonfinite='skip' does not support SGD with momentum != 0: whether a parameter's momentum buffer "
                         "exists (the 'first update writes the buffer' flag) is tracked on the host per parameter and cannot "
                         "follow a decision made on the device; plain SGD (momentum=0), Adam and AdamW are supported")


def _group_property(key):
    def only_group(self):
        groups = self.optimizer.param_groups
        if len(groups) != 1:
            raise ValueError(f"TrainStep.{key} is the value of the only param group; this TrainStep has {len(groups)}: "
                             f"read and set ts.optimizer.param_groups[i][{key!r}]")
        return groups[0]

    def get(self):
        return only_group(self).get(key)

    def set(self, value):
        group = only_group(self)                    # (raises before the value is looked at)
        group[key] = tuple(value) if key == "betas" else value
    return property(get, set, doc=f"optimizer.param_groups[0][{key!r}]")


class TrainStep:
    """One training step (see the module docstring).  ``optimizer`` / ``optimizer_args`` are the reference's
    conf["optimizer"] / conf["optimizer_args"]: "Adam", "AdamW" or "SGD" with torch's arguments and torch's defaults
    (``lr`` defaults to 5e-4 for all three; ``betas`` / ``eps`` / ``weight_decay`` given here are overridden by the same
    key in ``optimizer_args``).  ``self.optimizer`` is a ``torch.optim.Optimizer`` (acvae_amd.optim.FlatOptimizer) that LR
    schedulers can drive; ``lr``, ``betas``, ``eps`` and ``weight_decay`` are views of its param group.

    ``kl_reduction`` / ``free_bits`` / ``free_bits_over``: the variational term (``acvae_amd.train_util.KLObjective``).  With the
    defaults ("all", None) it is the reference's ``Normal_kl_loss``, the mean over all N x (Tc - 1) positions, padded ones
    included, by the launches it always was.  ``kl_reduction="valid"`` averages over the positions the
    cross-entropy runs over; ``free_bits=lam`` clamps the KL from below per latent dimension ("dim") or per position
    ("cell").  ``parts`` then also carries the device diagnostics ``kl_raw``, ``kl_dims``, ``kl_steps`` and ``gates_open``.
    Under data parallelism the divisor D is the rank's own count of positions, the rule the cross-entropy already follows
    (each rank averages over its own tokens and the gradients are averaged over ranks).  ``scst_step`` has no KL term.

    ``accum_steps=k`` (k > 1): every call of ``step()`` / ``scst_step()`` is one micro-step.  Its backward writes the flat
    gradient buffer as always and ``acvae_grad_accumulate`` adds that to a second flat buffer, ``flat_acc``; the first k - 1
    micro-steps of a window stop there (``parts["applied"]`` is False, no ``grad_norm``), the k-th clips and applies the MEAN
    of the window's gradients, each micro-step normalised over its own tokens: torch's ``(loss / k).backward()`` idiom, and the
    rule the ranks of a data-parallel step follow.  ``step_count``, Adam's bias correction and LR schedulers count applied
    updates; BatchNorm running statistics move at every micro-step.  A parameter is left alone by the update only if no
    micro-step of the window gave it a gradient.  ``flush()`` applies a window that is not full (the end of an epoch).  Under
    data parallelism only the k-th micro-step (or ``flush()``) exchanges gradients: one all-reduce of ``flat_acc`` behind the
    last accumulate launch, in pieces of ``exchange.max_chunk`` elements, not overlapped with the backward.

    ``ema_decay=d``: ``flat_ema``, an exponential moving average of the whole flat parameter buffer, moved by one
    ``acvae_ema_step`` behind every applied update with decay d (``ema_warmup=True``: ``ema_decay_at``).  ``ema_weights()``
    runs the model on it, ``ema_state_dict()`` / ``load_ema_state_dict()`` checkpoint it.  Every rank of a data-parallel job
    computes the same average from the same parameters.

    With ``accum_steps=1`` and ``ema_decay=None`` neither buffer exists and a step is the launches it always was.

    ``param_groups``: None, or 1..8 dicts ``{"params": iterable of Parameters, **overrides}`` in torch's convention
    (``acvae_amd.optim.split_params`` builds the common recipe).  A group may override ``lr``, ``betas``, ``eps``,
    ``weight_decay`` (SGD: ``lr``, ``momentum``, ``weight_decay``); everything else comes from ``optimizer_args`` and is one
    value for the whole flat buffer.  Every trainable parameter must be in exactly one group (frozen ones are ignored, the
    encoder's pooled head may be listed or left out).  ``optimizer.param_groups`` then holds those groups and every one is
    read on every step.  One group runs the launches it always ran; two or more run ``acvae_grad_norm_groups`` and one
    grouped update over a chunk table that is uploaded once per distinct set of parameters without a gradient.  Clipping
    stays global; ``parts["grad_norm_groups"]`` (device, [G]) is each group's share of ``parts["grad_norm"]``.  ``ts.lr`` and
    its siblings raise with several groups.  Checkpoints index the parameters through the groups' lists in the order given,
    as torch does.

    ``nonfinite="skip"``: the non-finite guard.  A step (with ``accum_steps`` > 1: a window) is judged on the device: it is
    bad when the gradient norm, the loss of any of its micro-steps or any floating-point module buffer (BatchNorm running
    statistics) after any of its forwards is NaN or +-inf.  A bad step leaves the training state bit for bit as it was before
    it: flat parameters, optimiser state, ``flat_ema``, the floating-point buffers, and the count that Adam's bias correction
    and ``ema_warmup`` use, so the next good step is the one a run that never saw the bad batch would have made.  Nothing is
    read back for it: ``acvae_guard_witness`` looks at the loss and the buffers, ``acvae_guard_decide`` forms the decision and
    the bias-correction scalars from the device's own count of applied updates, the guarded update and EMA return at once on a
    skip, and ``acvae_guard_restore`` puts the buffers' snapshot (taken at the start of the step or window) back.  The update
    always runs as the grouped launches (a one-group chunk table for one group) and the norm is always computed, also with
    ``max_grad_norm`` None / 0 (the clip itself then stays off).  ``parts["update_ok"]`` is a device int32 view of the last
    decision (read it before the next update overwrites it); ``guard_counts()`` synchronises and returns ``applied`` /
    ``skipped`` / ``streak``.  ``max_skips`` (default 50, None: no limit): once more than that many updates in a row were
    skipped, ``step()`` raises RuntimeError naming the counts, where it waits for the step two behind it anyway
    (``max_steps_in_flight``), or ``synchronize()`` does.  ``step_count`` and LR schedulers keep counting ATTEMPTED updates, as
    ``torch.amp.GradScaler`` leaves the scheduler to its caller: update k runs at the learning rate of attempt k with the bias
    correction of the applied updates before it.  Checkpoints store the applied count as torch's per-parameter ``step``.
    Under data parallelism the witness's flag is all-reduced (MAX, 4 bytes) before the decision, so every rank decides
    alike.  Not covered: SGD with momentum (refused), a finite but huge norm, loss scaling, integer buffers
    (``num_batches_tracked`` moves on a skipped step), un-counting the LR scheduler, naming the offending clip."""

    lr = _group_property("lr")
    betas = _group_property("betas")
    eps = _group_property("eps")
    weight_decay = _group_property("weight_decay")

    def __init__(self, model, vocab_size, lr=5e-4, betas=None, eps=None, weight_decay=None, max_grad_norm=1.0,
                 label_smoothing=True, smoothing=0.1, alpha=1.0, global_loss="MSE", process_group=None,
                 broadcast_buffers=True, data_parallel=True, precision=None, optimizer="Adam", optimizer_args=None,
                 kl_reduction="all", free_bits=None, free_bits_over="dim", accum_steps=1, ema_decay=None, ema_warmup=False,
                 param_groups=None, nonfinite=None, max_skips=_UNSET):
        check_accumulation(accum_steps, ema_decay, ema_warmup)                   # (before anything is built)
        check_guard(nonfinite, max_skips)
        self.accum_steps = int(accum_steps)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.micro_count = 0                        # position inside the accumulation window
        self.ema_updates = 0                        # applied updates the average has seen (ema_warmup's t)
        self._window_skipped = None                 # ranges without a gradient in EVERY micro-step of the window so far
        self._in_ema = False
        kl_objective = KLObjective(kl_reduction, free_bits, free_bits_over)      # (refuses bad values before anything is built)
        group = resolve(optimizer, optimizer_args, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        groups = None
        if param_groups is not None:                # (refused before anything is built, too)
            groups = resolve_groups(optimizer, group, param_groups)
            head = model.encoder._head()
            check_coverage(groups, [p for p in model.parameters() if p.requires_grad], (head.weight, head.bias))
        check_guard(nonfinite, max_skips, optimizer, [group] if groups is None else groups)
        self.nonfinite = nonfinite
        self.max_skips = None if nonfinite is None else (DEFAULT_MAX_SKIPS if max_skips is _UNSET else max_skips)
        self.optimizer_name = optimizer
        self.model = model
        if precision is not None:                   # "f32" | "bf16" (bf16 forward / fp32 loss: BASELINE configs[2])
            model.encoder.compute_dtype = precision
        self.vocab = vocab_size
        self.max_grad_norm = max_grad_norm
        self.smoothing = smoothing if label_smoothing else 0.0
        self.alpha, self.global_loss = alpha, global_loss
        if alpha is not None and global_loss != "MSE":
            raise NotImplementedError("global_loss other than 'MSE' (the shipped q_logs_utt/p_logs_utt are None)")
        self.criterion = LabelSmoothingLoss(vocab_size, self.smoothing)
        self.kl_objective = None if (kl_reduction == "all" and free_bits is None) else kl_objective
        self.kl_loss = Normal_kl_loss() if self.kl_objective is None else self.kl_objective
        self.mse_loss = MSELoss()
        self.pg = process_group
        self.data_parallel = data_parallel          # False: a purely local step inside an initialised process group
        self.world = dist.get_world_size(process_group) if self._dist() else 1
        self.broadcast_buffers = broadcast_buffers
        self.step_count = 0
        self.max_steps_in_flight = int(os.environ.get("ACVAE_STEPS_IN_FLIGHT", "2"))
        self._in_flight = []
        self._copy_stream = None
        self._flatten(group if groups is None else groups[0])      # (which state exists is the same in every group)
        # checkpoints index parameters through these lists (torch's rule): model.parameters(), or the groups as given
        self._group_lists = [list(model.parameters())] if groups is None else [g["params"] for g in groups]
        self.optimizer = FlatOptimizer(self, model.parameters() if groups is None else groups, optimizer, group)
        gi = {id(p): k for k, ps in enumerate(self._group_lists) for p in ps}
        self._group_of = [gi.get(id(p), 0) for p in self.order]          # in flat order
        self._tables = {}                           # (skipped, SGD-started) -> (device chunk table, partials, segments)
        self.group_norms = None
        if len(self._group_lists) > 1:
            self.group_norms = torch.zeros(len(self._group_lists), device=self.flat_p.device)
        self._pending = None                        # (gscale, total_norm, skipped, stream) while step() applies the update
        # Buckets in flat order, each announced from inside the backward as soon as its gradients are queued:
        #   0 decoder + prior + heads (everything acvae_decode_bwd writes, 76 MB at V=5000): behind the decode backward,
        #     i.e. before the encoder backward has even started;
        #   1 posterior (20 MB): behind the posterior backward, which runs on the side stream beside the encoder's;
        #   2 encoder up to the last ConvBlock (5 MB): at the end of the encoder backward - the only exposed part;
        #   3 the last ConvBlock (72 % of Cnn10's encoder gradients, 14 MB): from acvae_encoder_bwd_hooked's callback
        #     right after that block's kernels are queued, while the shallower blocks still run.
        # Buckets over 32 MB go out in 32 MB pieces.
        # With accum_steps > 1 the same buckets lie over flat_acc and go out behind the window's last accumulate launch.
        self.exchange = FlatGradExchange(self._grad_src, [self.n_text_dec, self.n_text - self.n_text_dec,
                                                       self.n_enc - self.n_enc_deep, self.n_enc_deep], process_group)
        if self.world == 1:
            self.exchange.world = 1
        if self.world > 1:                         # single process: no exchange, no callbacks out of the backward
            model._grad_ready_cb = self._on_grads_ready
            model.encoder._grad_ready_cb = self._on_grads_ready
        self._buf_work = None
        self._decode_event = self._decode_aux_event = self._text_event = None
        self._decode_deferred = self._projemb_seen = False
        self._proj_emb = isinstance(model.decoder.word_embeddings, torch.nn.Sequential)
        # The BatchNorm-buffer broadcast issued at the end of step() is joined wherever the buffers are read outside
        # step(): any forward of the model or of its encoder (validation right after the last training step, reference
        # runners/pytorch_runner_vae.py:339-345) and state_dict() (checkpointing).
        if self.world > 1:
            join = lambda *_a, **_k: self.sync_buffers()
            model.register_forward_pre_hook(join)
            model.encoder.register_forward_pre_hook(join)
            model.register_state_dict_pre_hook(join)
        if self._dist():
            dist.broadcast(self.flat_p, src=0, group=self.pg)
            if self.flat_buf is not None:
                dist.broadcast(self.flat_buf, src=0, group=self.pg)
        self.flat_ema = None if self.ema_decay is None else self.flat_p.clone()      # (after rank 0's parameters arrived)
        self._guard = None
        if nonfinite is not None:
            self._build_guard()

    def _build_guard(self):
        """The guard's device record (zeroed: nothing applied, nothing skipped), the buffers' snapshot, the norms' scratch
        for one group and the page-locked ring the counters of the steps in flight are copied to."""
        dev = self.flat_p.device
        rec = torch.zeros(GUARD_RECORD_BYTES // 4, dtype=torch.int32, device=dev)
        self._guard = rec
        self._guard_counters = rec[:8].view(torch.int64)          # applied, skipped, streak, ema_updates
        self._guard_ok = rec[_GUARD_OK:_GUARD_OK + 1]
        self._guard_flag = rec[_GUARD_WINDOW_BAD:_GUARD_WINDOW_BAD + 1]
        self._buf_snapshot = None if self.flat_buf is None else torch.empty_like(self.flat_buf)
        self._guard_norms = self.group_norms if self.group_norms is not None else torch.zeros(1, device=dev)
        slots = max(self.max_steps_in_flight, 0) + 2
        self._guard_host = torch.zeros(slots, 4, dtype=torch.int64).pin_memory()
        self._guard_slot = 0
        self._guard_in_flight = []                  # the slot of every event in _in_flight (None: no decision in that call)
        self._guard_last = None

    def _dist(self):
        return self.data_parallel and dist.is_available() and dist.is_initialized() and \
            (self.pg is not None or dist.get_world_size() > 1)

    # ------------------------------------------------------------------ flat parameter / gradient storage
    def _flatten(self, group):
        model = self.model
        enc_params = set(model.encoder.parameters())
        head = model.encoder._head()                                # embed_pooled / fc1: no gradient on this path
        never = {head.weight, head.bias}
        params = [p for p in model.parameters() if p.requires_grad]
        qset = set(model.qnet.parameters())
        text = [p for p in params if p not in enc_params]
        text = [p for p in text if p not in qset] + [p for p in text if p in qset]   # decode-written first, posterior last
        n_q = sum(1 for p in text if p in qset)
        enc = [p for p in params if p in enc_params and p not in never]
        deep = set(model.encoder._deep_block()[0].parameters())
        enc = [p for p in enc if p not in deep] + [p for p in enc if p in deep]
        n_deep = sum(1 for p in enc if p in deep)
        tail = [p for p in params if p in never]
        order = text + enc + tail
        dev = order[0].device
        _lib.require_cuda(order[0])
        sizes = [(p.numel() + 3) // 4 * 4 for p in order]          # keep every view 16-B aligned
        total = sum(sizes)
        self.flat_p = torch.zeros(total, device=dev)
        self.flat_g = torch.zeros(total, device=dev)
        # optimiser state: only what the chosen optimiser keeps (Adam: exactly the two moments, as always)
        self.exp_avg = self.exp_avg_sq = self.max_exp_avg_sq = self.momentum_buffer = None
        self._sgd_started = set()                   # SGD with momentum: parameters whose buffer exists
        if "betas" in group:
            self.exp_avg = torch.zeros(total, device=dev)
            self.exp_avg_sq = torch.zeros(total, device=dev)
            if group["amsgrad"]:
                self.max_exp_avg_sq = torch.zeros(total, device=dev)
        elif group["momentum"] != 0:
            self.momentum_buffer = torch.zeros(total, device=dev)
        views, off = {}, 0
        for p, sz in zip(order, sizes):
            pv = self.flat_p[off:off + p.numel()].view_as(p)
            pv.copy_(p.data)
            p.data = pv
            views[p] = self.flat_g[off:off + p.numel()].view_as(p)
            off += sz
        self.n_text = sum(sizes[:len(text)])
        self.n_text_dec = sum(sizes[:len(text) - n_q])
        self.n_enc = sum(sizes[len(text):len(text) + len(enc)])
        self.n_enc_deep = sum(sizes[len(text) + len(enc) - n_deep:len(text) + len(enc)])
        self.n_active = self.n_text + self.n_enc
        self.order, self.views, self.never = order, views, never
        model._set_grad_views(views)
        # BatchNorm running statistics in one buffer (for the DDP-style broadcast)
        bufs = [b for n, b in model.named_buffers() if b.dtype.is_floating_point]
        self.flat_buf = None
        if bufs:
            self.flat_buf = torch.zeros(sum(b.numel() for b in bufs), device=dev)
            off = 0
            for b in bufs:
                v = self.flat_buf[off:off + b.numel()].view_as(b)
                v.copy_(b.data); b.data = v
                off += b.numel()
        # accumulation: the buffer the window's gradients are summed in; the norm and the update then read it instead of flat_g
        self.flat_acc = torch.zeros(total, device=dev) if self.accum_steps > 1 else None
        self._grad_src = self.flat_g if self.flat_acc is None else self.flat_acc
        self.norm_partials = torch.empty(_lib.call("acvae_grad_norm_partials"), device=dev)
        self.total_norm = torch.zeros(1, device=dev)

    # ------------------------------------------------------------------ gradient exchange
    def _on_grads_ready(self, tag, event=None):
        """Called from inside the backward, on the thread and with the stream of the autograd node that just queued
        its kernels: ("decode", event) after acvae_decode_bwd unless it left gradients trailing on the side stream
        (`event` = recorded behind its last kernel), "text" after the posterior backward (every text-side gradient is
        queued now), ("encoder_block", b) from acvae_encoder_bwd_hooked after ConvBlock b, "encoder" when the encoder
        is through.  The order of these calls is fixed by the autograd graph, hence identical on every rank.
        With accum_steps > 1 nothing is exchanged from inside a backward (DDP's no_sync): flat_acc goes out behind the
        window's last accumulate launch (_apply_window)."""
        if self.accum_steps > 1:
            return
        if tag == "decode":
            self._decode_event = event
            if not self._proj_emb:               # with projected embeddings their gradients are still to come ("projemb")
                self.exchange.ready(0)
        elif tag == "decode_deferred":
            # trailing-gradient mode: the decode backward's parameter gradients are still running on the decode calls' SECOND
            # stream: `event` = (event on the main stream, event behind the trailing work on the second stream)
            self._decode_event, self._decode_aux_event = event
            self._decode_deferred = True
        elif tag == "projemb":
            # _ProjTableFn's backward: the last three decode-side gradients.  Autograd runs it after the decode backward
            # and - the node being older than the posterior's - normally after "text" as well; bucket 0 goes out behind
            # the decode backward (event), the side stream's trailing work and the posterior backward (text event) and
            # the kernels just queued on the current stream.  Should it ever fire before "text" in trailing-gradient
            # mode, nothing on this stream covers the side stream's work yet: leave the bucket to "text".
            self._projemb_seen = True
            if self._text_event is not None or not self._decode_deferred:
                self.exchange.ready(0, after=(self._decode_event, self._decode_aux_event, self._text_event))
        elif tag == "text":
            if torch.cuda.is_available() and self.flat_g.is_cuda:
                self._text_event = torch.cuda.Event()
                self._text_event.record(torch.cuda.current_stream())
            # decode-written gradients not announced yet (trailing-gradient mode): they were queued on the decode calls' second
            # stream (`_decode_aux_event`) or on the main stream behind `_decode_event`; with projected embeddings bucket 0
            # waits for "projemb"
            if not self._proj_emb or self._projemb_seen:
                self.exchange.ready(0, after=(self._decode_event, self._decode_aux_event))
            self.exchange.ready(1)
        elif isinstance(tag, tuple):
            if tag[1] == self.model.encoder._deep_block()[1]:
                self.exchange.ready(3)
        else:
            self.exchange.ready(3)
            self.exchange.ready(2)

    # ------------------------------------------------------------------ one optimiser step
    def forward_loss(self, feats, feat_lens, caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5, clip_index=None,
                     frontend=None):
        """Runner._forward(mode='train') + the loss line (:315-318).  Returns (loss, parts, output).  ``clip_index`` and
        ``frontend``: see ``step``."""
        if frontend is not None:
            feats, feat_lens = frontend(feats, feat_lens, device=self.flat_p.device)
        share = {} if clip_index is None else {"clip_index": clip_index}
        out = self.model(feats, feat_lens, caps, cap_lens, ss_ratio=ss_ratio, dis_ratio=dis_ratio, **share)
        staged = getattr(self.model, "staged", None) or {}
        lens1 = staged.get("lens1_d")
        if lens1 is None:
            lens1 = np.asarray(cap_lens) - 1
        caps_src = staged.get("caps_d")
        targets = (caps if caps_src is None else caps_src)[:, 1:1 + out["logits"].shape[1]].to(torch.long)
        ce = self.criterion.masked(out["logits"], targets, lens1)     # == criterion(packed_logits, packed targets)
        diag = {}
        if self.kl_objective is None:
            kl = self.kl_loss(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"])
        else:                                       # D from the host's lengths: nothing is read back
            T = out["q_means"].shape[1]
            host = np.clip(np.asarray(cap_lens).astype(np.int64) - 1, 0, T)
            if torch.is_tensor(lens1) and lens1.is_cuda:
                kl = self.kl_objective(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"], lens1, divisor=int(host.sum()))
            else:
                kl = self.kl_objective(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"], host)
            diag = dict(self.kl_objective.last)
        mse = None
        if self.alpha is not None:
            mse = self.mse_loss(out["q_means_utt"], out["p_means_utt"])
        loss = combine_losses(ce, kl, mse, kl_weight, self.alpha if self.alpha is not None else 0.0)    # ce + w kl + alpha mse
        return loss, {"ce": ce.detach(), "kl": kl.detach(), "mse": None if mse is None else mse.detach(), **diag}, out

    def prefetch(self, feats_host):
        """Queue the upload of a LATER step's feature batch now, on a copy stream of its own: the 8 MB host-to-device copy
        that Runner._forward makes in front of every step (`feats = batch[0].to(device)`, runners/pytorch_runner_vae.py:80)
        then travels beside the step that is running instead of in front of the next encoder.  Returns the device tensor to
        hand to step(); step() makes its stream wait for the copy.  Page-locked input is copied from where it lies;
        pageable input is staged through the package's page-locked ring first (a host memcpy).  An int16 tensor is PCM for
        step(..., frontend=) and arrives as int16 whether it is page-locked or pageable (a pageable one used to arrive cast
        to fp32, unlike a page-locked one; no step without frontend= accepts int16 features, so nothing relied on that
        cast); every other dtype arrives as before.  Typical loop:
            nxt = ts.prefetch(batch0)
            for batch in batches[1:] + [None]:
                cur, nxt = nxt, (ts.prefetch(batch) if batch is not None else None)
                ts.step(cur, ...)"""
        dev = self.flat_p.device
        t = torch.as_tensor(feats_host)
        if t.is_cuda:
            return t
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self._copy_stream):
            # int16 is PCM for step(..., frontend=): it travels as it is (a cast would drop the kernel's 1/32768 scale)
            d = t.to(dev, non_blocking=True) if t.is_pinned() else _lib.h2d(t if t.dtype == torch.int16 else t.float(), dev)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        d._acvae_ready = ev
        return d

    def step(self, feats, feat_lens, caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5, augment=None,
             clip_index=None, frontend=None):
        """One training step.  ``augment``: one ``acvae_amd.augment.AugmentParams`` per clip (a batch's column from
        ``CaptionDataset(..., augment=...)``): the rolls and masks run on the device before the encoder.

        ``clip_index`` (``Hybrid_VAEModel.forward``): one encoder pass shared by the captions of a clip.  ``feats`` /
        ``feat_lens`` (and ``augment``) then hold the B clips, ``caps`` / ``cap_lens`` the N = B * k caption rows, and
        ``clip_index[r]`` names the clip of row r (``acvae_amd.batch.collate_groups`` builds such batches).  The loss and
        the gradients are those of the step on the batch with every clip repeated k times.  Under data parallelism nothing
        changes: the graph has one more node between the decode loop and the encoder.

        ``frontend`` (``acvae_amd.frontend.LogMel``): ``feats`` / ``feat_lens`` are waveforms ``[B, Lmax]`` (fp32 or int16 PCM,
        on the host or uploaded by ``prefetch``) and their sample counts; the log-mel features are formed on the step's
        stream in front of the encoder, with no gradient through them.  Not together with ``augment`` (ValueError: the
        augment records are drawn per frame on host features); ``frontend=fe.augmented(...)`` augments such a batch."""
        if frontend is not None:                    # first: a refused call touches nothing of the step's state
            from .frontend import refuse_augment
            refuse_augment(augment)
        self._refuse_inside_ema("step")
        self.sync_buffers()
        self._guard_snapshot()
        ready = getattr(feats, "_acvae_ready", None)
        if ready is not None:                       # a batch uploaded by prefetch(): order this step behind its copy
            streams.hand_over(feats, ready)
        if augment is not None:
            from .augment import apply
            if not feats.is_cuda:
                feats = _lib.h2d(torch.as_tensor(feats).float(), self.flat_p.device)
            feats = apply(feats, feat_lens, augment)
        self._decode_event = self._decode_aux_event = self._text_event = None
        self._decode_deferred = self._projemb_seen = False
        for p in self.order:
            p.grad = None                                             # optimizer.zero_grad(set_to_none=True)
        loss, parts, _ = self.forward_loss(feats, feat_lens, caps, cap_lens, ss_ratio, dis_ratio, kl_weight, clip_index,
                                           frontend)
        return self._backward_and_update(loss, parts)

    def scst_step(self, feats, feat_lens, keys, key2refs, vocabulary, scorer, sample_n=1, max_length=None, **kwargs):
        """One self-critical training step (models/seq_train_model.py): greedy baseline and sampled rollout through
        ``ScstWrapper`` (``sample_n == 1``) or ``sample_n`` rollouts per clip over one encoder pass through ``NScstWrapper``,
        then the same backward, clip and fused update as ``step()``.  With ``scorer=acvae_amd.cider.CiderD(vocabulary)`` the
        reward (CIDEr-D) is computed on the device and the step has no device-to-host copy: ``reward`` / ``score`` in the
        returned dict are device tensors.  Any other scorer needs the words on the host: one synchronisation per step,
        between the rollouts and the loss.  Parameters the loss does not reach (the posterior,
        ``mean_log_out``) get no gradient and the optimiser leaves them and their state alone, as torch's does.
        ``kwargs``: ``temperature`` / ``temp`` / ``method`` / ``rng`` as the wrappers take them."""
        if self.world > 1:
            raise NotImplementedError("data-parallel SCST: the gradient exchange waits for the posterior's bucket, which a "
                                      "rollout never announces; run scst_step in a single process")
        from .seq_train_model import NScstWrapper, ScstWrapper
        self._refuse_inside_ema("scst_step")
        self.sync_buffers()
        self._guard_snapshot()
        self._decode_event = self._decode_aux_event = self._text_event = None
        self._decode_deferred = self._projemb_seen = False
        for p in self.order:
            p.grad = None
        kwargs = dict(kwargs, scorer=scorer, max_length=self.model.max_length if max_length is None else max_length)
        if int(sample_n) > 1:
            out = NScstWrapper(self.model)(feats, feat_lens, keys, key2refs, vocabulary, sample_n=int(sample_n), **kwargs)
        else:
            out = ScstWrapper(self.model)(feats, feat_lens, keys, key2refs, vocabulary, **kwargs)
        parts = {k: out[k] for k in ("reward", "score", "sampled_seqs") if k in out}
        if "greedy_seqs" in out:
            parts["greedy_seqs"] = out["greedy_seqs"]
        return self._backward_and_update(out["loss"], parts)

    def _guard_snapshot(self):
        """At the start of a step or window: the floating-point buffers as a skipped update has to leave them (one
        device-to-device copy; under data parallelism rank 0's broadcast of the previous step has been joined)."""
        if self._guard is not None and self.micro_count == 0 and self.flat_buf is not None:
            self._buf_snapshot.copy_(self.flat_buf)

    def _guard_witness(self, loss):
        """Behind the backward (the forward's buffer writes and everything trailing on the second stream are in front of
        the current stream by now): OR into the record whether the loss or a buffer is non-finite."""
        l = loss.detach()
        if l.dtype != torch.float32 or l.numel() != 1 or not l.is_cuda:
            raise RuntimeError("nonfinite='skip' needs the loss as one fp32 scalar on the device")
        nb = 0 if self.flat_buf is None else self.flat_buf.numel()
        _lib.call("acvae_guard_witness", l, self.flat_buf, nb, self._guard, _lib.current_stream())

    def _backward_and_update(self, loss, parts):
        self.exchange.begin()
        loss.backward()
        if self._guard is not None:
            self._guard_witness(loss)
        if self.accum_steps == 1:
            gscale = self.exchange.finish()
            self._update(self._check_grad_aliasing(), gscale, _lib.current_stream())
            parts["loss"] = loss.detach()
            parts["grad_norm"] = self.total_norm
            if self._norm_by_group():
                parts["grad_norm_groups"] = self.group_norms
            if self._guard is not None:
                parts["update_ok"] = self._guard_ok
        else:
            # one micro-step: the backward has written flat_g (and its trailing work on the second stream is joined to the
            # current stream, as for the norm); add it to the window's sum where the norm would be launched
            skipped = set(self._check_grad_aliasing())
            _lib.call("acvae_grad_accumulate", self.flat_acc, self.flat_g, self.n_active, int(self.micro_count == 0),
                      _lib.current_stream())
            self._window_skipped = skipped if self.micro_count == 0 else self._window_skipped & skipped
            self.micro_count += 1
            parts["loss"] = loss.detach()
            parts["applied"] = self.micro_count == self.accum_steps
            if parts["applied"]:
                self._apply_window()
                parts["grad_norm"] = self.total_norm
                if self._norm_by_group():
                    parts["grad_norm_groups"] = self.group_norms
                if self._guard is not None:
                    parts["update_ok"] = self._guard_ok
        # DDP's broadcast_buffers: rank 0's BatchNorm running statistics reach the other ranks before the next forward
        # touches them.  Issued here, behind this step's kernels and off the next step's critical path; joined by
        # sync_buffers() at the start of the next step (or by the caller before an evaluation pass).
        if self.world > 1 and self.broadcast_buffers and self.flat_buf is not None:
            self._buf_work = dist.broadcast(self.flat_buf, src=0, group=self.pg, async_op=True)
        # Bound how far the host may run ahead of the GPU.  Unbounded, the first steps of a run queue several steps'
        # worth of launches, the runtime grows its queues / kernel-argument / signal pools while the GPU is working and
        # those steps run 31-36 ms instead of 28.7 (tools/step_times.py); two steps of slack hide every host hiccup.
        if self.max_steps_in_flight > 0:
            ev = torch.cuda.Event()
            ev.record()
            self._in_flight.append(ev)
            if self._guard is not None:
                self._guard_in_flight.append(self._guard_last)
                self._guard_last = None
            if len(self._in_flight) > self.max_steps_in_flight:
                self._in_flight.pop(0).synchronize()
                if self._guard is not None:         # that step's counters have arrived in page-locked memory
                    self._check_streak(self._guard_in_flight.pop(0))
                # a persistent launch of that step that could not complete has poisoned the step with NaN and raised the
                # device's status word: turn it into an error at the first synchronisation point the loop has anyway
                _lib.check_persist_status(self.flat_p.device)
        return parts

    def _update(self, skipped, gscale, st):
        """Norm of gscale * (the gradient buffer), the fused update with the clip coefficient from it, and the EMA."""
        if self._guard is not None:
            return self._update_guarded(skipped, gscale, st)
        tn = None
        if self._norm_by_group():
            table, partials, _ = self._chunk_table(skipped)
            _lib.call("acvae_grad_norm_groups", self._grad_src, table, table.shape[0], len(self._group_lists), gscale,
                      partials, self.group_norms, self.total_norm, st)
            tn = self.total_norm
        elif self.max_grad_norm is not None and self.max_grad_norm > 0:
            _lib.call("acvae_grad_norm", self._grad_src, self.n_active, gscale, self.norm_partials, self.total_norm, st)
            tn = self.total_norm
        self.step_count += 1
        self._pending = (gscale, tn, skipped, st)
        try:
            self.optimizer.step()                  # the instance attribute: an LR scheduler's step tracking sees the call
        finally:
            self._pending = None
            # the fused update writes the flat parameter buffer through raw pointers: no _version moves, so what the model
            # caches per weight (attention projections of the step API, projected embedding table) is dropped by hand
            self.model.drop_step_caches()
        if self.flat_ema is not None:
            d = ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup)
            _lib.call("acvae_ema_step", self.flat_ema, self.flat_p, self.flat_p.numel(), d, st)
            self.ema_updates += 1

    def _update_guarded(self, skipped, gscale, st):
        """_update with the guard: norm -> decide -> guarded update -> guarded EMA -> restore, all on ``st``; then the
        counters start their way to page-locked memory."""
        table, partials, _ = self._chunk_table(skipped)
        _lib.call("acvae_grad_norm_groups", self._grad_src, table, table.shape[0], len(self._group_lists), gscale,
                  partials, self._guard_norms, self.total_norm, st)
        if self.world > 1:
            # the exchanged gradients, hence the norm, are the same on every rank; the witness is local
            dist.all_reduce(self._guard_flag, op=dist.ReduceOp.MAX, group=self.pg)
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        self.step_count += 1                        # attempted updates: what LR schedulers count, too
        self._pending = (gscale, self.total_norm if clip else None, skipped, st)
        try:
            self.optimizer.step()                  # -> _apply_guarded: the decision and the guarded update
        finally:
            self._pending = None
            self.model.drop_step_caches()
        if self.flat_ema is not None:
            _lib.call("acvae_ema_step_guarded", self.flat_ema, self.flat_p, self.flat_p.numel(), self._guard, st)
        if self.flat_buf is not None:
            _lib.call("acvae_guard_restore", self.flat_buf, self._buf_snapshot, self.flat_buf.numel(), self._guard, st)
        if self.max_skips is not None:
            slot, self._guard_slot = self._guard_slot, (self._guard_slot + 1) % self._guard_host.shape[0]
            self._guard_host[slot].copy_(self._guard_counters, non_blocking=True)
            self._guard_last = slot

    def _apply_guarded(self, groups, gscale, tn, skipped, st):
        """The decision (bias-correction scalars and EMA weight from the device's counts and the groups as they are now)
        and the guarded grouped update; one group is a one-group chunk table."""
        name, G = self.optimizer_name, len(groups)
        check_groups(name, groups)
        table, _, _ = self._chunk_table(skipped)
        arr = lambda vals: (ctypes.c_double * G)(*[float(v) for v in vals])
        n, mg, g0 = self.n_active, float(self.max_grad_norm or 0.0), groups[0]
        lr = arr(g["lr"] for g in groups)
        ema = -1.0 if self.flat_ema is None else self.ema_decay
        if name == "SGD":
            if any(float(g["momentum"]) != 0 for g in groups):
                raise RuntimeError("SGD momentum became non-zero under nonfinite='skip' (the guard supports plain SGD only)")
            _lib.call("acvae_guard_decide", self._guard, self.total_norm, 1, G, lr, None, None, ema, int(self.ema_warmup), st)
            _lib.call("acvae_sgd_groups_step_guarded", self.flat_p, self._grad_src, n, table, table.shape[0], G, lr,
                      arr(g["weight_decay"] for g in groups), gscale, mg, tn, self._guard, st)
            return
        if bool(g0["amsgrad"]) != (self.max_exp_avg_sq is not None):
            raise RuntimeError("amsgrad cannot change after TrainStep was built (it decides which state exists)")
        b1, b2 = arr(g["betas"][0] for g in groups), arr(g["betas"][1] for g in groups)
        _lib.call("acvae_guard_decide", self._guard, self.total_norm, 0, G, lr, b1, b2, ema, int(self.ema_warmup), st)
        _lib.call("acvae_adamw_groups_step_guarded", self.flat_p, self._grad_src, self.exp_avg, self.exp_avg_sq,
                  self.max_exp_avg_sq, n, table, table.shape[0], G, lr, b1, b2, arr(g["eps"] for g in groups),
                  arr(g["weight_decay"] for g in groups), int(bool(g0["decoupled_weight_decay"])), int(bool(g0["amsgrad"])),
                  gscale, mg, tn, self._guard, st)

    def _check_streak(self, slot):
        """``slot`` of the page-locked ring holds the counters of a step whose work has completed: raise once more than
        ``max_skips`` updates in a row were skipped."""
        if slot is None or self.max_skips is None:
            return
        applied, skipped, streak, _ = (int(v) for v in self._guard_host[slot])
        if streak > self.max_skips:
            raise RuntimeError(f"TrainStep(nonfinite='skip'): {streak} updates in a row were non-finite and skipped "
                               f"(max_skips={self.max_skips}; applied {applied}, skipped {skipped}, streak {streak}); the "
                               "parameters, the optimiser state and the buffers are those of the last applied update")

    def guard_counts(self):
        """{"applied", "skipped", "streak"} of the guard's device record; synchronises the device."""
        if self._guard is None:
            raise RuntimeError("TrainStep.guard_counts() needs TrainStep(..., nonfinite='skip')")
        torch.cuda.synchronize(self.flat_p.device)
        applied, skipped, streak, _ = (int(v) for v in self._guard_counters.cpu())
        return {"applied": applied, "skipped": skipped, "streak": streak}

    def _applied_count(self):
        """What Adam's bias correction counts: the host's step count, or with the guard the device's (a read-back)."""
        if self._guard is None:
            return self.step_count
        return int(self._guard_counters[0].item())

    def _apply_window(self):
        """Close the accumulation window of ``micro_count`` micro-steps: all-reduce flat_acc (data parallel), then the norm
        and the update with grad_scale 1 / (micro_count * world): the mean over micro-steps and ranks."""
        m, self.micro_count = self.micro_count, 0
        skipped, self._window_skipped = sorted(self._window_skipped), None
        # every bucket of flat_acc behind an event recorded on this stream now, i.e. behind the accumulate launch
        self.exchange.begin()
        self.exchange.finish()
        self._update(skipped, 1.0 / (m * self.exchange.world), _lib.current_stream())

    def flush(self):
        """Apply the micro-steps accumulated so far as one update (a window cut short, e.g. by the end of an epoch): the mean
        over those ``micro_count`` micro-steps.  Returns {"applied": True, "grad_norm": device scalar}, or None when the
        window is empty (or accum_steps == 1) and nothing was done.  Under data parallelism it issues the exchange, so every
        rank must call it at the same point, with the same number of micro-steps behind it."""
        self._refuse_inside_ema("flush")
        if self.micro_count == 0:
            return None
        self._apply_window()
        out = {"applied": True, "grad_norm": self.total_norm}
        if self._norm_by_group():
            out["grad_norm_groups"] = self.group_norms
        return out

    def _norm_by_group(self):
        return self.group_norms is not None and self.max_grad_norm is not None and self.max_grad_norm > 0

    def _chunk_table(self, skipped):
        """(device table int32 [n_chunks, 3], partials [n_chunks], number of segments) of the grouped launches for this set of
        parameters without a gradient (and, under SGD with momentum, this set of started buffers): built and uploaded once
        per distinct set, so the usual step uploads nothing."""
        skip = {a for a, _ in skipped}
        offs = [off for _, off in self._active_params((), self.n_active)]
        n_par = len(offs)                           # the active range is the first n_par parameters of the flat order
        skipped_idx = frozenset(i for i, off in enumerate(offs) if off in skip)
        first_idx = frozenset()
        if self.momentum_buffer is not None:
            first_idx = frozenset(i for i, p in enumerate(self.order[:n_par]) if p not in self._sgd_started)
        key = (skipped_idx, first_idx)
        hit = self._tables.get(key)
        if hit is None:
            sizes = [(p.numel() + 3) // 4 * 4 for p in self.order[:n_par]]
            chunk = int(_lib.call("acvae_opt_chunk_elems"))
            table = chunk_table(sizes, self._group_of[:n_par], skipped_idx, first_idx, chunk)
            if table.shape[0] == 0:
                raise RuntimeError("TrainStep: no parameter has a gradient")
            dev = self.flat_p.device
            hit = (torch.from_numpy(table).to(dev), torch.empty(table.shape[0], device=dev),
                   len(group_segments(sizes, self._group_of[:n_par], skipped_idx, first_idx)))
            self._tables[key] = hit
        return hit

    def _apply_groups(self, groups, gscale, tn, skipped, st):
        """Two or more param groups: one grouped launch over the chunk table, every group's dict as it is now."""
        name, G = self.optimizer_name, len(groups)
        check_groups(name, groups)
        table, _, _ = self._chunk_table(skipped)
        arr = lambda vals: (ctypes.c_double * G)(*[float(v) for v in vals])
        n, mg, g0 = self.n_active, float(self.max_grad_norm or 0.0), groups[0]
        if name == "SGD":
            mom = float(g0["momentum"]) != 0
            if mom and self.momentum_buffer is None:
                raise RuntimeError("SGD momentum became non-zero, but TrainStep was built with momentum == 0 (no buffer)")
            _lib.call("acvae_sgd_groups_step", self.flat_p, self._grad_src, self.momentum_buffer if mom else None, n, table,
                      table.shape[0], G, arr(g["lr"] for g in groups), arr(g["momentum"] for g in groups),
                      arr(g["weight_decay"] for g in groups), float(g0["dampening"]), int(bool(g0["nesterov"])), gscale, mg,
                      tn, st)
            if mom:
                self._sgd_started.update(p for p, _ in self._active_params(skipped, n))
            return
        if bool(g0["amsgrad"]) != (self.max_exp_avg_sq is not None):
            raise RuntimeError("amsgrad cannot change after TrainStep was built (it decides which state exists)")
        _lib.call("acvae_adamw_groups_step", self.flat_p, self._grad_src, self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq,
                  n, table, table.shape[0], G, arr(g["lr"] for g in groups), arr(g["betas"][0] for g in groups),
                  arr(g["betas"][1] for g in groups), arr(g["eps"] for g in groups), arr(g["weight_decay"] for g in groups),
                  int(bool(g0["decoupled_weight_decay"])), int(bool(g0["amsgrad"])), self.step_count, gscale, mg, tn, st)

    def _apply_update(self):
        """The fused update of the step that step() is running, with the hyperparameters of the param groups as they are
        now (host floats: no synchronisation).  One group: the one-group entries and launches; more: _apply_groups."""
        if self._pending is None:
            raise RuntimeError("TrainStep.optimizer.step() applies the update of the step that TrainStep.step() is running "
                               "(it needs that step's gradients and norm): call TrainStep.step(...) instead")
        gscale, tn, skipped, st = self._pending
        if self._guard is not None:
            return self._apply_guarded(self.optimizer.param_groups, gscale, tn, skipped, st)
        if len(self.optimizer.param_groups) > 1:
            return self._apply_groups(self.optimizer.param_groups, gscale, tn, skipped, st)
        g = self.optimizer.param_groups[0]
        check_group(self.optimizer_name, g)
        n, mg = self.n_active, float(self.max_grad_norm or 0.0)
        if self.optimizer_name == "SGD":
            mom = float(g["momentum"])
            if mom != 0 and self.momentum_buffer is None:
                raise RuntimeError("SGD momentum became non-zero, but TrainStep was built with momentum == 0 (no buffer)")
            # torch.optim.SGD starts a parameter's buffer from its first gradient: split the segments by whether the
            # buffer exists, so that every launch has one `first` flag
            segs = self._sgd_segments(skipped, n) if mom != 0 else [(a, b, False) for a, b in self._segments(skipped, n)]
            for a, b, first in segs:
                _lib.call("acvae_sgd_step", self.flat_p[a:b], self._grad_src[a:b],
                          self.momentum_buffer[a:b] if mom != 0 else None, b - a, g["lr"], mom, g["dampening"],
                          g["weight_decay"], int(bool(g["nesterov"])), int(first), gscale, mg, tn, st)
            if mom != 0:
                self._sgd_started.update(p for p, _ in self._active_params(skipped, n))
            return
        if bool(g["amsgrad"]) != (self.max_exp_avg_sq is not None):
            raise RuntimeError("amsgrad cannot change after TrainStep was built (it decides which state exists)")
        b1, b2 = g["betas"]
        # torch.optim.Adam leaves a parameter whose .grad is None alone (no moment decay, no update): the fused pass
        # then runs over the segments between such parameters (their gradient slices are zero, so the norm is unaffected).
        # On this path every parameter gets a gradient every step and the loop runs once over the whole buffer.
        for a, b in self._segments(skipped, n):
            if not g["amsgrad"] and not g["decoupled_weight_decay"]:
                _lib.call("acvae_adam_step", self.flat_p[a:b], self._grad_src[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b],
                          b - a, g["lr"], b1, b2, g["eps"], g["weight_decay"], self.step_count, gscale, mg, tn, st)
            else:
                _lib.call("acvae_adamw_step", self.flat_p[a:b], self._grad_src[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b],
                          self.max_exp_avg_sq[a:b] if g["amsgrad"] else None, b - a, g["lr"], b1, b2, g["eps"],
                          g["weight_decay"], int(bool(g["decoupled_weight_decay"])), int(bool(g["amsgrad"])),
                          self.step_count, gscale, mg, tn, st)

    def _active_params(self, skipped, n):
        """(parameter, offset) of every parameter in the active range that has a gradient this step."""
        skip = {a for a, _ in skipped}
        out, off = [], 0
        for p in self.order:
            if off >= n:
                break
            if off not in skip:
                out.append((p, off))
            off += (p.numel() + 3) // 4 * 4
        return out

    def _sgd_segments(self, skipped, n):
        """[(a, b, first)]: maximal runs of parameters with a gradient whose momentum buffer does (first=False) or does
        not yet (first=True) exist."""
        segs = []
        for p, off in self._active_params(skipped, n):
            end, first = off + (p.numel() + 3) // 4 * 4, p not in self._sgd_started
            if segs and segs[-1][1] == off and segs[-1][2] == first:
                segs[-1][1] = end
            else:
                segs.append([off, end, first])
        return [tuple(s) for s in segs]

    def synchronize(self):
        """Wait for every queued step and raise if one of their persistent launches gave up (acvae_persist_status_register)."""
        torch.cuda.synchronize(self.flat_p.device)
        self._in_flight.clear()
        _lib.check_persist_status(self.flat_p.device)
        if self._guard is not None:
            slots = [s for s in self._guard_in_flight + [self._guard_last] if s is not None]
            self._guard_in_flight, self._guard_last = [], None
            if slots:
                self._check_streak(slots[-1])

    def sync_buffers(self):
        """Join the asynchronous BatchNorm-buffer broadcast of the previous step (a stream dependency under RCCL)."""
        if self._buf_work is not None:
            self._buf_work.wait()
            self._buf_work = None

    def _check_grad_aliasing(self):
        """The backward kernels write into the flat gradient buffer and autograd is expected to adopt those
        views as .grad; if it cloned one instead, repair the alias; if a parameter got no gradient at all, zero its
        slice and report it: returns the list of (offset, end) ranges of active parameters without a gradient."""
        skipped, off = [], 0
        for p in self.order:
            v = self.views[p]
            sz = (p.numel() + 3) // 4 * 4
            if p.grad is None:
                if off < self.n_active:
                    v.zero_()
                    skipped.append((off, off + sz))
            elif p.grad.data_ptr() != v.data_ptr():
                p.grad = v            # autograd cloned the view; the flat buffer (already all-reduced) is authoritative
            off += sz
        return skipped

    @staticmethod
    def _segments(skipped, n):
        if not skipped:
            return [(0, n)]
        segs, cur = [], 0
        for a, b in skipped:
            if a > cur:
                segs.append((cur, a))
            cur = max(cur, b)
        if cur < n:
            segs.append((cur, n))
        return segs

    def state_dict(self):
        sd = {"step": self._applied_count(), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        if self.flat_ema is not None:
            if self._guard is not None:             # the device's count is the one the warm-up uses
                self.ema_updates = int(self._guard_counters[3].item())
            sd["ema"], sd["ema_updates"] = self.flat_ema, self.ema_updates
        if self.accum_steps > 1:
            sd["micro_count"] = self.micro_count
        return sd

    # ------------------------------------------------------------------ the averaged weights
    def _refuse_inside_ema(self, what):
        if self._in_ema:
            raise RuntimeError(f"TrainStep.{what}() inside ema_weights(): the model holds the averaged weights; leave the "
                               "context before training on")

    def _swap_ema(self):
        tmp = self.flat_p.clone()
        self.flat_p.copy_(self.flat_ema)
        self.flat_ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with ts.ema_weights(): validate(model)``: the model on the averaged weights.  The contents of the flat parameter
        buffer and of ``flat_ema`` change places (every ``p.data`` view stays what it is), what the model caches per weight is
        dropped and a pending BatchNorm-buffer broadcast is joined; on exit, also when the body raised, the training weights
        are back bit for bit.  ``step()``, ``scst_step()`` and ``flush()`` raise RuntimeError inside.  The BatchNorm running
        statistics are the live ones: they are moving averages of the training run already, and are not averaged again."""
        if self.flat_ema is None:
            raise RuntimeError("TrainStep.ema_weights() needs TrainStep(..., ema_decay=)")
        self._refuse_inside_ema("ema_weights")
        self.sync_buffers()
        self._swap_ema()
        self._in_ema = True
        self.model.drop_step_caches()
        try:
            yield self.model
        finally:
            self._swap_ema()
            self._in_ema = False
            self.model.drop_step_caches()

    def ema_state_dict(self):
        """The averaged parameters as clones in ``model.state_dict()``'s layout and names, with the live buffers (and any
        parameter outside the flat buffer as it is): loads into the reference's model."""
        if self.flat_ema is None:
            raise RuntimeError("TrainStep.ema_state_dict() needs TrainStep(..., ema_decay=)")
        self._refuse_inside_ema("ema_state_dict")
        table, named = self._offsets(), dict(self.model.named_parameters())
        out = collections.OrderedDict()
        for k, v in self.model.state_dict().items():
            p = named.get(k)
            if p is not None and p in table:
                out[k] = self.flat_ema[table[p]:table[p] + p.numel()].view_as(p).clone()
            else:
                out[k] = v.detach().clone()
        return out

    def load_ema_state_dict(self, sd):
        """Inverse of ``ema_state_dict``: the parameters of ``sd`` become the average.  Its buffers are not read (they are the
        model's own, which ``model.load_state_dict`` restores)."""
        if self.flat_ema is None:
            raise RuntimeError("TrainStep.load_ema_state_dict() needs TrainStep(..., ema_decay=)")
        self._refuse_inside_ema("load_ema_state_dict")
        table = self._offsets()
        todo = [(k, p) for k, p in self.model.named_parameters() if p in table]
        for k, p in todo:
            if k not in sd:
                raise KeyError(f"load_ema_state_dict: no {k!r}")
            if tuple(sd[k].shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict: {k!r} has shape {tuple(sd[k].shape)}, the parameter {tuple(p.shape)}")
        for k, p in todo:
            self.flat_ema[table[p]:table[p] + p.numel()].copy_(sd[k].reshape(-1))

    # ------------------------------------------------------------------ checkpoint in the reference's format
    def _offsets(self):
        off, table = 0, {}
        for p in self.order:
            table[p] = off
            off += (p.numel() + 3) // 4 * 4
        return table

    def _state_buffers(self):
        """{torch state key: flat buffer} of the chosen optimiser."""
        if self.optimizer_name == "SGD":
            return {} if self.momentum_buffer is None else {"momentum_buffer": self.momentum_buffer}
        bufs = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        if self.max_exp_avg_sq is not None:
            bufs["max_exp_avg_sq"] = self.max_exp_avg_sq
        return bufs

    def optimizer_state_dict(self):
        """The optimiser state in the ``state_dict()`` layout of ``torch.optim.<optimizer>`` (Adam / AdamW: ``step``,
        ``exp_avg``, ``exp_avg_sq`` and ``max_exp_avg_sq`` with amsgrad; SGD: ``momentum_buffer``), parameters indexed in
        ``model.parameters()`` order (the optimiser of the reference is built from it, ``runners/pytorch_runner_vae.py:
        219, 233-236``), the param group with the keys of the torch class, so that ``{"model": model.state_dict(),
        "optimizer": ts.optimizer_state_dict()}`` is the checkpoint the reference writes (``:380-388``) and a
        ``torch.optim.<optimizer>`` over a reference model loads it.  ``ts.optimizer.state_dict()`` is this."""
        table = self._offsets()
        # the reference builds its optimiser over ALL model.parameters(); with param_groups= the ids enumerate the groups'
        # lists in the order given (torch's rule), so torch.optim.<optimizer> over the same groups loads the result
        params = [p for ps in self._group_lists for p in ps]
        bufs = self._state_buffers()
        sgd = self.optimizer_name == "SGD"
        state = {}
        applied = 0 if sgd else self._applied_count()      # with the guard: the device's count (a read-back)
        for i, p in enumerate(params):
            # torch's optimisers hold no state for a parameter that never had a gradient (frozen ones, and the pooled
            # head embed_pooled / fc1 whose output this path does not consume): no entry, like a reference checkpoint
            if not bufs or p not in table or p in self.never:
                continue
            if (sgd and p not in self._sgd_started) or (not sgd and applied == 0):
                continue
            o = table[p]
            st = {} if sgd else {"step": torch.tensor(float(applied))}
            for k, flat in bufs.items():
                st[k] = flat[o:o + p.numel()].view_as(p).clone()
            state[i] = st
        out, first = [], 0
        for pg, ps in zip(self.optimizer.param_groups, self._group_lists):
            group = {k: v for k, v in pg.items() if k != "params"}
            group["params"] = list(range(first, first + len(ps)))
            first += len(ps)
            out.append(group)
        return {"state": state, "param_groups": out}

    def load_optimizer_state_dict(self, sd):
        """Inverse of ``optimizer_state_dict`` (also accepts the state dict of the matching ``torch.optim`` class built
        over the same model): resume training where the checkpoint left off.  ``ts.optimizer.load_state_dict()`` is this."""
        table = self._offsets()
        params = [p for ps in self._group_lists for p in ps]
        if len(sd["param_groups"]) != len(self._group_lists):
            raise ValueError("TrainStep's optimizer has exactly one param group" if len(self._group_lists) == 1 else
                             f"the checkpoint has {len(sd['param_groups'])} param group(s), this TrainStep "
                             f"{len(self._group_lists)}")
        loaded = [{k: v for k, v in g.items() if k != "params"} for g in sd["param_groups"]]
        if len(loaded) > 1:
            for i, (g, ps) in enumerate(zip(sd["param_groups"], self._group_lists)):
                if len(g["params"]) != len(ps):
                    raise ValueError(f"param group {i} of the checkpoint holds {len(g['params'])} parameters, this "
                                     f"TrainStep's {len(ps)}")
            check_groups(self.optimizer_name, loaded)
        group = loaded[0]
        check_group(self.optimizer_name, group)
        bufs = self._state_buffers()
        sgd = self.optimizer_name == "SGD"
        if sgd and group.get("momentum", 0) != 0 and not bufs:
            raise ValueError("checkpoint has SGD momentum, but this TrainStep was built with momentum == 0 (no buffer)")
        if not sgd and bool(group.get("amsgrad", False)) != ("max_exp_avg_sq" in bufs):
            raise ValueError(f"checkpoint has amsgrad={bool(group.get('amsgrad', False))}, this TrainStep the opposite")
        for pg, g in zip(self.optimizer.param_groups, loaded):
            for k, v in g.items():
                pg[k] = tuple(v) if k == "betas" else v
        steps = set()
        for flat in bufs.values():
            flat.zero_()
        self._sgd_started = set()
        for i, st in sd["state"].items():
            p = params[int(i)]
            if p not in table:
                continue                                   # frozen here: nothing to resume
            o = table[p]
            for k, flat in bufs.items():
                if st.get(k) is None:
                    if sgd:
                        continue
                    raise ValueError(f"optimizer state {i}: no {k!r}")
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state {i}: shape {tuple(st[k].shape)} does not match parameter "
                                     f"{tuple(p.shape)} (state indexed over a different parameter list?)")
                flat[o:o + p.numel()].copy_(st[k].reshape(-1))
                if sgd:
                    self._sgd_started.add(p)
            if "step" in st:
                steps.add(int(float(st["step"])))
        # one step counter for the flat buffer: per-parameter counts that differ (legal under DDP's
        # find_unused_parameters) resume at the largest, which is exact for every parameter that was never skipped
        if not sgd:
            self.step_count = max(steps) if steps else 0
            if self._guard is not None:             # the device's count of applied updates resumes there; no streak is open
                self._guard_counters[0] = self.step_count
                self._guard_counters[2] = 0
