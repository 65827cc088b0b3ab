"""Loss modules of the training loop on the HIP path: mirrors of ``utils/train_util.py``
(``LabelSmoothingLoss`` :234-251, ``Normal_kl_loss`` :253-266, length-mask helpers :198-231) and of the
masked dict-style losses of ``losses/loss.py`` (:12-70).  Same constructor arguments and forward
signatures; the arithmetic is in libacvae_hip.so (acvae_ls_ce_*, acvae_gauss_kl_*, acvae_mse_*).

Self-critical sequence training: ``scst_Loss`` / ``Nscst_Loss`` (:292-413) and the sentence scoring of
``utils/score_util.py`` (``compute_batch_score`` / ``compur_batch_score_samplen``).  With ``scorer=acvae_amd.cider.CiderD(vocabulary)``
the reward is computed on the device from the token ids (acvae_ciderd_scores / acvae_ciderd_reward) and the words never reach the
host; with any other scorer object the reward arithmetic runs on the host in numpy as in the reference.  The loss and its
gradient are acvae_scst_loss_fwd / acvae_logprob_bwd.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib


def _dev_scalar(dev):
    return torch.empty(1, device=dev)


class _CEFn(torch.autograd.Function):
    """Label-smoothed CE over rows (n,t) of logits [N,T,V]; row valid iff t < lens1[n] (None: all)."""

    @staticmethod
    def forward(ctx, logits, targets, lens1, smoothing, reduction):
        _lib.require_cuda(logits)
        logits = logits.float()
        if not logits.is_contiguous():   # the backward writes dlogits with the same (contiguous) strides
            logits = logits.contiguous()
        N, T, V = logits.shape
        dev = logits.device
        targets = targets.to(device=dev, dtype=torch.long)
        if targets.stride(-1) != 1:
            targets = targets.contiguous()
        lens_d = None if lens1 is None else torch.as_tensor(lens1).to(device=dev, dtype=torch.long).contiguous()
        lse = torch.empty(N, T, device=dev)
        rows = torch.empty(N, T, device=dev)
        out = _dev_scalar(dev)
        st = _lib.current_stream()
        _lib.call("acvae_row_logsoftmax_argmax", logits, logits.stride(0), logits.stride(1), None, None, lse, T, 1, N,
                  T, V, st)
        _lib.call("acvae_ls_ce_fwd", logits, logits.stride(0), logits.stride(1), targets, targets.stride(0), lens_d,
                  lse, float(smoothing), reduction, rows, out, N, T, V, st)
        ctx.logits, ctx.targets, ctx.lens_d, ctx.lse = logits, targets, lens_d, lse
        ctx.smoothing, ctx.reduction = float(smoothing), reduction
        return rows if reduction == 0 else out[0]

    @staticmethod
    def backward(ctx, g):
        logits = ctx.logits
        N, T, V = logits.shape
        dl = torch.empty(N, T, V, device=logits.device)
        g = g.contiguous().float()
        _lib.call("acvae_ls_ce_bwd", logits, logits.stride(0), logits.stride(1), ctx.targets, ctx.targets.stride(0),
                  ctx.lens_d, ctx.lse, ctx.smoothing, ctx.reduction, None if ctx.reduction == 0 else g.reshape(1),
                  g if ctx.reduction == 0 else None, dl, N, T, V, _lib.current_stream())
        return dl, None, None, None, None


_RED = {"none": 0, "mean": 1, "sum": 2}


def masked_label_smoothing_ce(logits, targets, lens1, smoothing=0.0, reduction="mean"):
    """CE over the unpadded tokens of batch-major logits [N,T,V] without materialising the packed copy."""
    return _CEFn.apply(logits, targets, lens1, smoothing, _RED[reduction])


class LabelSmoothingLoss(nn.Module):
    """utils/train_util.py:234-251 — forward(logit [R,V] packed rows, target [R]) -> mean over rows."""

    def __init__(self, classes, smoothing=0.0, device=0, dim=-1):
        super().__init__()
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.cls = classes
        self.dim = dim
        self.device = device

    def forward(self, logit, target):
        return _CEFn.apply(logit.unsqueeze(1), target.reshape(-1, 1), None, self.smoothing, 1)

    def masked(self, logits, targets, lens1):
        """Same value as packing first (runner :89-95) then forward(): mean over tokens t < lens1[n]."""
        return _CEFn.apply(logits, targets, lens1, self.smoothing, 1)


class MaskedCrossEntropyLoss(nn.Module):
    """losses/loss.py:12-37 — forward({"logits","targets","lens"}), reduction in none|mean|sum."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction
        self.smoothing = 0.0

    def forward(self, output):
        return _CEFn.apply(output["logits"], output["targets"], output["lens"], self.smoothing, _RED[self.reduction])


class MaskedLabelSmoothingLoss(MaskedCrossEntropyLoss):
    """losses/loss.py:39-70."""

    def __init__(self, smoothing=0.0, dim=-1, reduction="mean"):
        super().__init__(reduction)
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.dim = dim


class _KLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu1, lv1, mu2, lv2):
        _lib.require_cuda(mu1, lv1, mu2, lv2)
        ts = [t.contiguous().float() for t in (mu1, lv1, mu2, lv2)]
        E = ts[0].shape[-1]
        rows = ts[0].numel() // E
        dev = ts[0].device
        part = torch.empty(_lib.call("acvae_kl_partials", rows * E), device=dev)
        out = _dev_scalar(dev)
        _lib.call("acvae_gauss_kl_fwd", *ts, part, out, rows, E, _lib.current_stream())
        ctx.ts, ctx.rows, ctx.E = ts, rows, E
        return out[0]

    @staticmethod
    def backward(ctx, g):
        outs = [torch.empty_like(t) if ctx.needs_input_grad[i] else None for i, t in enumerate(ctx.ts)]
        _lib.call("acvae_gauss_kl_bwd", *ctx.ts, g.contiguous().float().reshape(1), *outs, ctx.rows, ctx.E,
                  _lib.current_stream())
        return tuple(outs)


class Normal_kl_loss(nn.Module):
    """utils/train_util.py:253-266 — KL(N(mu1,e^lv1) || N(mu2,e^lv2)), sum over the last dim, mean over
    ALL leading positions (padded ones included)."""

    def __init__(self, device=0, dim=-1):
        super().__init__()
        self.dim = dim
        self.device = device

    def forward(self, mu1, lv1, mu2, lv2):
        return _KLFn.apply(mu1, lv1, mu2, lv2)


class _KLObjectiveFn(torch.autograd.Function):
    """acvae_kl_objective_fwd / bwd (csrc/kl_objective.hip).  Returns the scalar and, not differentiable, the diagnostics."""

    @staticmethod
    def forward(ctx, mu_q, lv_q, mu_p, lv_p, lens_d, D, lam, over_cell):
        _lib.require_cuda(mu_q, lv_q, mu_p, lv_p, lens_d)
        ts = [t.contiguous().float() for t in (mu_q, lv_q, mu_p, lv_p)]
        R, T, E = ts[0].shape
        dev = ts[0].device
        free = lam is not None
        nbytes = _lib.call("acvae_kl_objective_scratch_bytes", R, T, E)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        kl, raw = _dev_scalar(dev), _dev_scalar(dev)
        dims, steps = torch.empty(E, device=dev), torch.empty(T, device=dev)
        n_open = torch.empty(1, dtype=torch.int32, device=dev)
        gates = torch.empty(R * T if over_cell else E, dtype=torch.uint8, device=dev) if free else None
        _lib.call("acvae_kl_objective_fwd", *ts, lens_d, D, int(free), int(over_cell), lam if free else 0.0, kl, raw, dims,
                  steps, n_open, gates, scratch, nbytes, R, T, E, _lib.current_stream())
        ctx.ts, ctx.lens_d, ctx.gates, ctx.args = ts, lens_d, gates, (D, int(over_cell), R, T, E)
        diag = (raw[0], dims, steps, n_open[0])
        ctx.mark_non_differentiable(*diag)
        return (kl[0], *diag)

    @staticmethod
    def backward(ctx, g, *_unused):
        D, over_cell, R, T, E = ctx.args
        outs = [torch.empty_like(t) if ctx.needs_input_grad[i] else None for i, t in enumerate(ctx.ts)]
        _lib.call("acvae_kl_objective_bwd", *ctx.ts, ctx.lens_d, D, over_cell, ctx.gates, g.contiguous().float().reshape(1),
                  *outs, R, T, E, _lib.current_stream())
        return (*outs, None, None, None, None)


class KLObjective(nn.Module):
    """The variational term of the objective with its controls (include/acvae_hip.h: acvae_kl_objective_fwd has the
    definitions).  With k[r,t,e] the term of ``Normal_kl_loss``:

    ``reduction``  "all": every cell (r, t), divisor D = R * T - what ``Normal_kl_loss`` averages over, padded positions
                   included;  "valid": the cells t < lens1[r] only, D = sum(lens1) - the positions the
                   cross-entropy runs over, and the per-caption KL that ``acvae_amd.likelihood.score_captions`` reports.
    ``free_bits``  None: KL = (1/D) sum over the cells and e of k.  lam >= 0 (0.0 is a clamp, not None):
                   ``free_bits_over="dim"``: KL = sum_e max(m_e, lam), m_e the mean of k[., e] over the cells (Kingma et al.
                   2016); "cell": KL = (1/D) sum over the cells of max(s_c, lam), s_c = sum_e k[c, e].  A dimension or cell
                   at or under lam gets no gradient (the gate is strict).

    ``forward(mu_q, lv_q, mu_p, lv_p, lens1=None, divisor=None)``: four [R, T, E] tensors -> a device scalar with autograd.
    ``lens1`` (``cap_lens - 1``) is a host array or a device tensor, required for "valid".  From a host array D is summed on the
    host and nothing is read back; for a device tensor pass ``divisor=`` (the sum of min(lens1, T)) or one read-back finds
    it.  Under data parallelism D is the rank's own, the rule the cross-entropy already follows.
    ``.last`` holds the diagnostics of the latest call, device tensors written by the forward: ``kl_raw`` (the unclamped KL
    under the same reduction), ``kl_dims`` [E] (m_e), ``kl_steps`` [T] (mean s_c over the rows that hold step t),
    ``gates_open`` (int32: open gates; without free bits E, or the number of cells for "cell")."""

    def __init__(self, reduction="all", free_bits=None, free_bits_over="dim"):
        super().__init__()
        if reduction not in ("all", "valid"):
            raise ValueError(f"KLObjective: reduction must be 'all' or 'valid', got {reduction!r}")
        if free_bits_over not in ("dim", "cell"):
            raise ValueError(f"KLObjective: free_bits_over must be 'dim' or 'cell', got {free_bits_over!r}")
        if free_bits is not None:
            if isinstance(free_bits, (bool, np.bool_)) or not isinstance(free_bits, (int, float, np.integer, np.floating)):
                raise ValueError(f"KLObjective: free_bits must be None or a number >= 0, got {free_bits!r}")
            free_bits = float(free_bits)
            if not (0.0 <= free_bits < float("inf")):
                raise ValueError(f"KLObjective: free_bits must be finite and >= 0, got {free_bits!r}")
        self.reduction, self.free_bits, self.free_bits_over = reduction, free_bits, free_bits_over
        self.last = {}

    def forward(self, mu_q, lv_q, mu_p, lv_p, lens1=None, divisor=None):
        shape = tuple(mu_q.shape)
        if len(shape) != 3 or any(tuple(t.shape) != shape for t in (lv_q, mu_p, lv_p)) or min(shape) < 1:
            raise ValueError("KLObjective: the four Gaussians must share one shape [R, T, E], got "
                             f"{[tuple(t.shape) for t in (mu_q, lv_q, mu_p, lv_p)]}")
        R, T, E = shape
        lens_d, D = None, R * T
        if self.reduction == "valid":
            if lens1 is None:
                raise ValueError("KLObjective: reduction='valid' needs lens1 (cap_lens - 1)")
            if torch.is_tensor(lens1) and lens1.is_cuda:
                if tuple(lens1.shape) != (R,):
                    raise ValueError(f"KLObjective: lens1 of shape {tuple(lens1.shape)} for {R} rows")
                lens_d = lens1.to(torch.long).contiguous()
                D = int(lens_d.clamp(0, T).sum()) if divisor is None else int(divisor)      # (the one read-back)
            else:
                host = np.asarray(lens1.cpu() if torch.is_tensor(lens1) else lens1)
                if host.shape != (R,) or host.dtype.kind not in "iu":
                    raise ValueError(f"KLObjective: lens1 must be {R} integers, got shape {host.shape}, dtype {host.dtype}")
                if host.min() < 0 or host.max() > T:
                    raise ValueError(f"KLObjective: lens1 outside [0, {T}]")
                D = int(host.sum())
                if divisor is not None and int(divisor) != D:
                    raise ValueError(f"KLObjective: divisor {divisor} is not sum(lens1) = {D}")
            if not 1 <= D <= R * T:
                raise ValueError(f"KLObjective: {D} valid cells (D == 0: a batch of nothing but padding has no mean)")
            if lens_d is None:
                lens_d = _lib.h2d(torch.as_tensor(host.astype(np.int64)), mu_q.device)
        kl, kl_raw, dims, steps, n_open = _KLObjectiveFn.apply(mu_q, lv_q, mu_p, lv_p, lens_d, D, self.free_bits,
                                                               self.free_bits_over == "cell")
        self.last = {"kl_raw": kl_raw, "kl_dims": dims, "kl_steps": steps, "gates_open": n_open}
        return kl


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _lib.require_cuda(a, b)
        a, b = a.contiguous().float(), b.contiguous().float()
        part = torch.empty(_lib.call("acvae_kl_partials", a.numel()), device=a.device)
        out = _dev_scalar(a.device)
        _lib.call("acvae_mse_fwd", a, b, part, out, a.numel(), _lib.current_stream())
        ctx.a, ctx.b = a, b
        return out[0]

    @staticmethod
    def backward(ctx, g):
        da = torch.empty_like(ctx.a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(ctx.b) if ctx.needs_input_grad[1] else None
        _lib.call("acvae_mse_bwd", ctx.a, ctx.b, g.contiguous().float().reshape(1), da, db, ctx.a.numel(),
                  _lib.current_stream())
        return da, db


class _CombineLossFn(torch.autograd.Function):
    """loss = ce + w_kl * kl (+ w_mse * mse) on device scalars (runners/pytorch_runner_vae.py:315-320): one launch forward, one
    backward - the same arithmetic as the tensor expression, without its dozen scalar kernels on the step's critical path."""

    @staticmethod
    def forward(ctx, ce, kl, mse, w_kl, w_mse):
        _lib.require_cuda(ce, kl)
        out = _dev_scalar(ce.device)
        _lib.call("acvae_loss_combine_fwd", ce.reshape(1), kl.reshape(1), None if mse is None else mse.reshape(1), float(w_kl),
                  float(w_mse), out, _lib.current_stream())
        ctx.w = (float(w_kl), float(w_mse), mse is not None)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        w_kl, w_mse, has_mse = ctx.w
        gs = torch.empty(3, device=g.device)
        _lib.call("acvae_loss_combine_bwd", g.contiguous().float().reshape(1), w_kl, w_mse, gs[0:1], gs[1:2],
                  gs[2:3] if has_mse else None, _lib.current_stream())
        return gs[0], gs[1], (gs[2] if has_mse else None), None, None


def combine_losses(ce, kl, mse=None, kl_weight=1.0, alpha=0.0):
    """ce + kl_weight * kl + alpha * mse as the runner forms it, fused (device scalars in, device scalar out)."""
    return _CombineLossFn.apply(ce, kl, mse, kl_weight, alpha if mse is not None else 0.0)


class MSELoss(nn.Module):
    """nn.MSELoss() as used for the global constraint (runners/pytorch_runner_vae.py:220,317)."""

    def forward(self, a, b):
        return _MSEFn.apply(a, b)


# ---- self-critical sequence training
def _need_scorer(scorer):
    if scorer is None:
        raise ValueError("SCST needs a scorer: pass scorer=<object with compute_score(references, hypotheses) -> (score, "
                         "per-key scores)>, e.g. pycocoevalcap's Cider(), or acvae_amd.cider.CiderD(vocabulary), the package's own "
                         "CIDEr-D on the device")
    return scorer


def _on_device(scorer):
    """True for the package's own scorer: its reward is computed on the device, from the token ids where they lie."""
    from .cider import CiderD
    return isinstance(scorer, CiderD)


def _sentence(row, start_idx, end_idx, vocabulary):
    words = []
    for w_t in row:
        if w_t == start_idx:
            continue
        if w_t == end_idx:
            break
        words.append(vocabulary.idx2word[w_t])
    return " ".join(words)


def compute_batch_score(decode_res, key2refs, keys, start_idx, end_idx, vocabulary, scorer):
    """utils/score_util.py:5-52 - decode_res [N, max_length] token ids -> one score per row; rows that share a key are
    scored once, by the first of them."""
    scorer = _need_scorer(scorer)
    decode_res = np.asarray(decode_res)
    hypothesis, references = {}, {}
    for i in range(len(keys)):
        if keys[i] in hypothesis:
            continue
        hypothesis[keys[i]] = [_sentence(decode_res[i], start_idx, end_idx, vocabulary)]
        references[keys[i]] = key2refs[keys[i]]
    _, scores = scorer.compute_score(references, hypothesis)
    key2score = {key: scores[i] for i, key in enumerate(references.keys())}
    return np.array([key2score[keys[i]] for i in range(decode_res.shape[0])], dtype=np.float64)


def compur_batch_score_samplen(decode_res, key2refs, keys, start_idx, end_idx, vocabulary, scorer):
    """utils/score_util.py:56-96 (the name is the reference's) - every row scored on its own against key2refs[keys[i]]."""
    scorer = _need_scorer(scorer)
    decode_res = np.asarray(decode_res)
    hypothesis, references = {}, {}
    for i in range(len(keys)):
        hypothesis[i] = [_sentence(decode_res[i], start_idx, end_idx, vocabulary)]
        references[i] = key2refs[keys[i]]
    _, scores = scorer.compute_score(references, hypothesis)
    return scores


class _ScstLossFn(torch.autograd.Function):
    """mean_n sum_t -sampled_logprobs * reward * mask with mask[n,0] = 1, mask[n,t] = seqs[n,t-1] != <end> (:401-409)."""

    @staticmethod
    def forward(ctx, slp, seqs, reward, end_idx):
        _lib.require_cuda(slp, seqs)
        slp = slp.contiguous().float()
        N, T = slp.shape
        dev = slp.device
        seqs = seqs.to(device=dev, dtype=torch.long).contiguous()
        if torch.is_tensor(reward) and reward.is_cuda:          # a device reward (acvae_ciderd_reward) is used where it lies
            reward = reward.to(device=dev, dtype=torch.float32).contiguous()
        else:
            reward = _lib.h2d(torch.as_tensor(np.asarray(reward, dtype=np.float32)), dev).contiguous()
        coef = torch.empty(N, T, device=dev)
        out = _dev_scalar(dev)
        _lib.call("acvae_scst_loss_fwd", slp, seqs, reward, int(end_idx), coef, out, N, T, _lib.current_stream())
        ctx.coef = coef
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return ctx.coef * g, None, None, None


def scst_policy_loss(sampled_logprobs, seqs, reward, end_idx):
    """The loss line shared by scst_Loss, Nscst_Loss and the wrappers of acvae_amd.seq_train_model; reward [N]: host
    values, or a device tensor (the f32 reward of acvae_ciderd_reward)."""
    return _ScstLossFn.apply(sampled_logprobs, seqs, reward, end_idx)


def _seqs_to_host(*seqs):
    """Token tensors -> numpy with ONE device synchronisation for all of them."""
    if all(torch.is_tensor(s) and s.is_cuda for s in seqs):
        flat = torch.cat([s.reshape(-1) for s in seqs]).cpu().numpy()
        out, off = [], 0
        for s in seqs:
            out.append(flat[off:off + s.numel()].reshape(tuple(s.shape)))
            off += s.numel()
        return out
    return [s.cpu().numpy() if torch.is_tensor(s) else np.asarray(s) for s in seqs]


class scst_Loss(nn.Module):
    """utils/train_util.py:355-413 - forward(output with "greedy_seqs", "sampled_seqs", "sampled_logprobs", keys, key2refs,
    vocabulary) adds "reward" (sampled score - greedy score), "score" and "loss" to `output`."""

    def __init__(self, scorer, reduction="mean", device=0):
        super().__init__()
        self.reduction = reduction
        self.scorer = scorer
        self.device = device
        self.pad_idx, self.start_idx, self.end_idx = 0, 1, 2

    def get_critical_reward(self, greedy_seqs, sampled_seqs, keys, key2refs, vocabulary, scorer):
        greedy_seqs, sampled_seqs = _seqs_to_host(greedy_seqs, sampled_seqs)
        args = (key2refs, keys, self.start_idx, self.end_idx, vocabulary, scorer)
        sampled_score = compute_batch_score(sampled_seqs, *args)
        greedy_score = compute_batch_score(greedy_seqs, *args)
        return {"reward": sampled_score - greedy_score, "score": sampled_score}

    def forward(self, output, keys, key2refs, vocabulary):
        if _on_device(self.scorer):            # reward and score stay device tensors; nothing is read back
            rs = self.scorer.prepare(keys, key2refs, "batch", device=output["sampled_seqs"].device).reward(
                output["sampled_seqs"], output["greedy_seqs"], 1, self.start_idx, self.end_idx)
            output["reward"], output["score"] = rs["reward"], rs["score"]
            output["loss"] = scst_policy_loss(output["sampled_logprobs"], output["sampled_seqs"], rs["reward"], self.end_idx)
            return output
        rs = self.get_critical_reward(output["greedy_seqs"], output["sampled_seqs"], keys, key2refs, vocabulary,
                                      self.scorer)
        output["reward"] = torch.as_tensor(rs["reward"])
        output["score"] = torch.as_tensor(rs["score"])
        output["loss"] = scst_policy_loss(output["sampled_logprobs"], output["sampled_seqs"], rs["reward"], self.end_idx)
        return output


def leave_one_out_reward(sampled_score, sample_n):
    """:315-321 - rows clip-major [N * sample_n]: each sample's score minus the mean score of its clip's other samples."""
    s = np.asarray(sampled_score, dtype=np.float64).reshape(-1, sample_n)
    baseline = (s.sum(1, keepdims=True) - s) / (s.shape[1] - 1)
    return (s - baseline).reshape(-1)


class Nscst_Loss(nn.Module):
    """utils/train_util.py:292-353 - sample_n rollouts per clip, clip-major rows; the baseline of a rollout is the mean
    score of the clip's other rollouts.  forward(output with "sampled_seqs", "sampled_logprobs", keys [N clips], ...) ->
    {"reward": mean reward, "score", "loss"}."""

    def __init__(self, scorer, reduction="mean", sample_n=5, device=0):
        super().__init__()
        self.reduction = reduction
        self.sample_n = sample_n
        self.scorer = scorer
        self.device = device
        self.pad_idx, self.start_idx, self.end_idx = 0, 1, 2

    def get_critical_reward(self, sampled_seqs, keys, key2refs, vocabulary):
        sampled_seqs, = _seqs_to_host(sampled_seqs)
        score = np.asarray(compur_batch_score_samplen(sampled_seqs, key2refs, keys, self.start_idx, self.end_idx,
                                                      vocabulary, self.scorer), dtype=np.float64)
        return {"reward": leave_one_out_reward(score, self.sample_n), "score": score.reshape(-1)}

    def forward(self, output, keys, key2refs, vocabulary):
        keys = [key for key in keys for _ in range(self.sample_n)]
        if _on_device(self.scorer):            # device tensors out; "reward" is the mean of the float64 rewards
            rs = self.scorer.prepare(keys, key2refs, "rows", device=output["sampled_seqs"].device).reward(
                output["sampled_seqs"], None, self.sample_n, self.start_idx, self.end_idx)
            loss = scst_policy_loss(output["sampled_logprobs"], output["sampled_seqs"], rs["reward"], self.end_idx)
            return {"reward": rs["reward_mean"][0], "score": rs["score"], "loss": loss}
        rs = self.get_critical_reward(output["sampled_seqs"], keys, key2refs, vocabulary)
        loss = scst_policy_loss(output["sampled_logprobs"], output["sampled_seqs"], rs["reward"], self.end_idx)
        return {"reward": torch.as_tensor(rs["reward"]).mean(), "score": torch.as_tensor(rs["score"]), "loss": loss}


# ---- length helpers (utils/train_util.py:198-231); host-side index logic, used by callers of the modules
def generate_length_mask(lens):
    lens = torch.as_tensor(lens)
    T = int(lens.max())
    return torch.arange(T).unsqueeze(0) < lens.view(-1, 1)


def load_pretrained_model(model: nn.Module, pretrained, outputfun):
    """Reference utils/train_util.py:17-30: load the entries of a checkpoint (a state dict, or one wrapped under "model")
    whose names exist in `model` with the same shape; everything else keeps its current value.  A PANNs checkpoint's
    spectrogram_extractor.*, logmel_extractor.* and fc_audioset.* have no counterpart and are skipped.  A missing file is
    reported through `outputfun` and nothing is loaded."""
    import os
    if not os.path.exists(pretrained):
        outputfun(f"Loading pretrained model from {pretrained} failed!")
        return
    state_dict = torch.load(pretrained, map_location="cpu")
    if "model" in state_dict:
        state_dict = state_dict["model"]
    model_dict = model.state_dict()
    pretrained_dict = {k: v for k, v in state_dict.items() if k in model_dict and model_dict[k].shape == v.shape}
    model_dict.update(pretrained_dict)
    model.load_state_dict(model_dict, strict=True)
