"""Ensemble decoding: greedy, beam and diverse beam search over several trained models at once.

Mirrors ``BaseRunner.ensemble`` / ``_ensemble_batch`` / ``_ensemble_batch_beam_search`` (``runners/base_runner.py:397-694``,
inherited by the VAE runner): at every step the members' word probabilities are averaged (mean of softmax, then log,
:616-618, 675-680) and the word is picked from the average.  The whole search is ONE library call
(``acvae_ensemble_search``): per step every member runs its prior step and its decoder step on its own states, one
``acvae_ensemble_mix`` launch forms the mixture's log-probabilities, and the pick is the mix kernel's own argmax (greedy) or
the flat top-k of ``acvae_beam_search`` (beam).  ``method="dbs"`` is ``acvae_ensemble_dbs_search``, likewise one call: the mixture's
log-probabilities take the logits' place in ``Hybrid_VAEModel.diverse_beam_search``.  ``Ensemble.rollout`` draws N captions
per clip from the mixture (``acvae_ensemble_rollout``, one call: the same driver, one ``acvae_ensemble_mix_sample`` launch per
step); it has no counterpart in the reference.

The reference's ensemble code cannot run a ``Hybrid_VAEModel`` (it calls ``model.decoder`` without ``z`` and never runs
the prior network), so its mixing rule is carried onto this model's step as ``Hybrid_VAEModel.beam_search`` runs it.  Two
departures, both documented in INTEGRATION.md:
  - every member's encoder gets its own copy of ``feat_lens`` (the reference hands one array to all of them, each of which
    divides it in place, :576-578); the caller's array is left untouched;
  - the beam search expands the flat ``beam * V`` scores of a clip at every step, t = 0 included, because the beam rows of a
    clip differ in ``z`` from the first step on (the reference takes row 0 only at t = 0, :681-682).
"""
import copy
import json
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from . import _lib, search
from .batch import collate_fn
from .evaluate import accuracy_check, accuracy_rows, captions_per_clip, collect_predictions, predictions_payload
from .frontend import refuse_augmented
from .seq_train_model import ScstWrapper
from .vae_model import Hybrid_VAEModel

MAX_MEMBERS = int(_lib._defs["ACVAE_ENSEMBLE_MAX"])


class Ensemble(nn.Module):
    """``Ensemble(models)``: the members in an ``nn.ModuleList`` (``ScstWrapper`` / ``NScstWrapper`` unwrapped, as
    base_runner.py:428-429 does).  Members may differ in encoder class, embedding size and frame rate; vocabulary size,
    ``start_idx`` and ``end_idx`` are shared.

    ``noise`` (optional replay, consumed by the next forward as ``Hybrid_VAEModel.noise`` is):
    ``{"eps": [tensor [N, max_length, beam, E_m] per member]}``.  Without it member m's noise is drawn on the CPU
    generator with the calls its own ``beam_search`` would make (clip-major, ``torch.randn(beam, E_m)``), members in
    order: ``Ensemble([m])`` under a seed consumes the generator exactly as ``m.beam_search`` does."""

    def __init__(self, models):
        super().__init__()
        models = [m.model if isinstance(m, ScstWrapper) else m for m in models]
        if len(models) == 0:
            raise ValueError("Ensemble: no members")
        if len(models) > MAX_MEMBERS:
            raise ValueError(f"Ensemble: {len(models)} members, at most {MAX_MEMBERS}")
        for m in models:
            if not isinstance(m, Hybrid_VAEModel):
                raise ValueError(f"Ensemble: members must be Hybrid_VAEModel, got {type(m).__name__}")
        first = models[0]
        for m in models[1:]:
            for what in ("vocab_size", "start_idx", "end_idx"):
                if int(getattr(m, what)) != int(getattr(first, what)):
                    raise ValueError(f"Ensemble: members differ in {what} ({getattr(first, what)} and {getattr(m, what)})")
        devices = {next(m.parameters()).device for m in models}
        if len(devices) != 1:
            raise ValueError(f"Ensemble: members on different devices {sorted(str(d) for d in devices)}")
        self.models = nn.ModuleList(models)
        self.vocab_size, self.start_idx, self.end_idx = int(first.vocab_size), int(first.start_idx), int(first.end_idx)
        self.noise = None

    @torch.no_grad()
    def forward(self, feats, feat_lens, method="greedy", beam_size=5, max_length=20, repetition_penalty=None,
                no_repeat_ngram_size=None, min_length=None, suppress_tokens=None, finish_on_end=False, length_penalty=None,
                nbest=None, group_size=5, diversity_lambda=0.5, temperature=1.0, group_nbest=True):
        """-> ``{"seqs": int64 [N, max_length], "logprobs": f32}`` on the device.  ``logprobs``: greedy [N, max_length], the
        mixture's log-probability of each chosen word (entries behind a row's ``end_idx`` carry no meaning); beam [N], beam
        0's final score.  A greedy row that has produced ``end_idx`` keeps ``end_idx`` to the end (base_runner.py:584,
        622-630).

        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_length`` / ``suppress_tokens``: constrained decoding
        (``acvae_amd.search.constraints``), applied to every member's logits in front of the mixing; ``logprobs`` are then
        those of the constrained mixture.

        ``finish_on_end`` / ``length_penalty`` / ``nbest`` with ``method="beam"``: hypotheses finish at ``end_idx`` and are
        ranked by a length-normalised score (``acvae_amd.search.finishing``).  ``seqs`` is then hypothesis 0, ``logprobs``
        [N] its raw log-probability, and the dict also holds ``scores``, ``lengths`` and the ``nbest_*`` entries.

        ``method="dbs"`` with ``beam_size`` / ``group_size`` / ``diversity_lambda`` / ``temperature`` / ``group_nbest``:
        diverse beam search over the mixture (``Hybrid_VAEModel.diverse_beam_search``; ``acvae_ensemble_dbs_search``, one
        call).  -> ``{"seqs": int64 [N, rows, max_length], "scores": f64 [N, rows], "lengths": int32 [N, rows]}``, rows =
        ``beam_size`` with ``group_nbest`` (as for a single model) else ``group_size``.  Member m's noise is drawn with
        the calls its own search would make, members in order.  The decoding constraints and the finishing keywords are
        refused with it, as for a single model; ``group_size`` is at most 16."""
        if method not in ("greedy", "beam", "dbs"):
            raise ValueError(f"Ensemble: method must be 'greedy', 'beam' or 'dbs', not {method!r}")
        beam, T = 1 if method == "greedy" else int(beam_size), int(max_length)
        if method == "dbs":
            G = int(group_size)
            bdash = beam // G if G >= 1 else 0
            if bdash < 1 or bdash > 16:
                raise ValueError("Ensemble: beam_size // group_size must be in 1..16")
            if G > 16:
                raise ValueError(f"Ensemble: group_size {G}, at most 16 (a single model falls back to its host loop)")
            if not float(temperature) > 0:
                raise ValueError(f"Ensemble: temperature must be > 0, not {temperature!r}")
        keywords = dict(method=method, beam_size=beam, max_length=T, repetition_penalty=repetition_penalty,
                        no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, suppress_tokens=suppress_tokens,
                        finish_on_end=finish_on_end, length_penalty=length_penalty, nbest=nbest)
        con = search.constraints(keywords, self.vocab_size, self.end_idx, T, True, False)   # (no_grad: nothing is recorded)
        fin = search.finishing(keywords, T)
        replay = self.noise.get("eps") if self.noise is not None else None
        self.noise = None
        if replay is not None and len(replay) != len(self.models):
            raise ValueError(f"Ensemble: noise['eps'] holds {len(replay)} tensors for {len(self.models)} members")
        _lib.require_cuda(feats)
        members = []
        for k, model in enumerate(self.models):
            model.eval()                                                   # base_runner.py:573-574
            model._forward_token = getattr(model, "_forward_token", 0) + 1     # per-forward caches, as Hybrid_VAEModel.forward
            encoded = model.encoder(feats, copy.copy(np.asarray(feat_lens)))    # its own copy: the encoder divides it in place
            if method == "dbs":
                if replay is not None:
                    raise ValueError("Ensemble: noise['eps'] replays a beam search's noise, not a diverse beam search's")
                noise = lambda N, E, dev: search._dbs_noise(N, T * G, bdash, E, dev)
            else:
                noise = lambda N, E, dev: search._search_noise(N, T, beam, E, dev, None if replay is None else replay[k])
            members.append(model._search_member(encoded, noise))
        if method == "dbs":
            return search.diverse_beam_search(members, True, G, bdash, T, self.vocab_size, self.start_idx, self.end_idx,
                                              temperature, diversity_lambda, group_nbest, beam)
        return search.beam_search(members, True, method == "greedy", beam, T, self.vocab_size, self.start_idx, self.end_idx,
                                  con, fin)

    @torch.no_grad()
    def rollout(self, feats, feat_lens, sample_n=1, method="sample", temp=1.0, top_k=None, top_p=None, rng="device",
                max_length=20, repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, suppress_tokens=None,
                rerank=None):
        """``sample_n`` captions per clip drawn from the mixture, ONE library call (``acvae_ensemble_rollout``) behind one
        encoder pass per member and clip -> ``{"seqs": int64, "logprobs": f32}``, both [N * sample_n, max_length] on the
        device, rows clip-major (row ``n * sample_n + j``) as ``Hybrid_VAEModel.rollout_shared_encoder`` returns them.
        ``logprobs``: the mixture's log-probability (at temperature 1, under the full distribution) of each chosen word;
        a row that has produced ``end_idx`` keeps it to the end, and the entries behind it carry no meaning.

        ``method``: "sample" (multinomial), "gumbel", or "greedy" (the rows of a clip then differ by their prior noise
        alone; ``sample_n=1`` is ``forward(method="greedy")`` bit for bit on the same ``eps``).  ``temp`` acts on the
        MIXTURE: the members are mixed at temperature 1 and the mixture's log-probabilities are divided by ``temp``; the
        members' logits are not tempered before the mixing.  ``top_k`` / ``top_p`` (``acvae_amd.search.truncation``)
        truncate the mixture's row; the decoding constraints (``acvae_amd.search.constraints``) act on every member's
        logits in front of the mixing.  ``rerank`` (an ``acvae_amd.consensus.Consensus``): ``seqs`` becomes the picked rows
        [N, max_length] beside ``candidates``, ``consensus_scores`` and ``consensus_best``, as
        ``Hybrid_VAEModel._rerank`` leaves them.

        Noise.  Member m's prior noise is drawn on the CPU generator as its own search would (clip-major,
        ``torch.randn(sample_n, E_m)`` per clip and step), members in order.  The word noise [max_length, N * sample_n, V]:
        ``rng="device"`` (the default: there is no reference stream to reproduce) draws ONE seed on the CPU generator and
        fills it on the device (``acvae_sample_noise``); ``rng="host"`` draws it on the CPU generator step by step, as a
        single model's 2-input forward does.  ``self.noise = {"eps": [tensor [N, max_length, sample_n, E_m] per member],
        "sample_noise": [max_length, N * sample_n, V]}`` (either key may be absent) replays them and is consumed by this
        call.

        ValueError in front of any work: a method other than the three, ``sample_n`` < 1, a ``temp`` that is not finite
        and > 0, an unknown ``rng``, truncation with "greedy", and what ``search.constraints`` / ``search.rerank_check``
        refuse (``rerank`` with fewer than 2 or more than 16 rows per clip, or with ``max_length`` > 64)."""
        if method not in search.ROLLOUT_METHODS:
            raise ValueError(f"Ensemble.rollout: method must be 'greedy', 'sample' or 'gumbel', not {method!r}")
        if isinstance(sample_n, bool) or not isinstance(sample_n, (int, np.integer)) or sample_n < 1:
            raise ValueError(f"Ensemble.rollout: sample_n must be an integer >= 1, got {sample_n!r}")
        if rng not in ("host", "device"):
            raise ValueError(f"rng must be 'host' or 'device', got {rng!r}")
        try:
            temp32 = float(np.float32(temp))                               # the value the kernel divides by
        except (TypeError, ValueError):
            raise ValueError(f"Ensemble.rollout: temp must be a finite number > 0, got {temp!r}") from None
        if isinstance(temp, bool) or not (np.isfinite(temp32) and temp32 > 0.0):
            raise ValueError(f"Ensemble.rollout: temp must be a finite number > 0, got {temp!r}")
        n, T, V = int(sample_n), int(max_length), self.vocab_size
        keywords = dict(method=method, max_length=T, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                        no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, suppress_tokens=suppress_tokens)
        top_k, top_p = search.truncation(keywords, True, False)            # (no_grad: nothing is recorded)
        con = search.constraints(keywords, V, self.end_idx, T, True, False)
        search.rerank_check(rerank, n, keywords, T, False)
        replay = self.noise if self.noise is not None else {}
        self.noise = None
        eps_replay, word_replay = replay.get("eps"), replay.get("sample_noise")
        if eps_replay is not None and len(eps_replay) != len(self.models):
            raise ValueError(f"Ensemble: noise['eps'] holds {len(eps_replay)} tensors for {len(self.models)} members")
        _lib.require_cuda(feats)
        members = []
        for k, model in enumerate(self.models):
            model.eval()
            model._forward_token = getattr(model, "_forward_token", 0) + 1
            encoded = model.encoder(feats, copy.copy(np.asarray(feat_lens)))    # its own copy: the encoder divides it in place
            members.append(model._search_member(encoded, lambda N, E, dev: search._search_noise(
                N, T, n, E, dev, None if eps_replay is None else eps_replay[k])))
        dev, R = members[0][0].device, members[0][0].shape[0] * n
        noise, code = None, search.ROLLOUT_METHODS[method]
        if method != "greedy":
            if word_replay is not None:
                noise = _lib.h2d(torch.as_tensor(word_replay)[:T].reshape(T, R, V), dev, torch.float32).contiguous()
            elif rng == "device":
                seed = int(torch.randint(0, 2 ** 62, (1,)))                # after the members' draws: torch.manual_seed fixes it
                noise = torch.empty(T, R, V, device=dev)
                _lib.call("acvae_sample_noise", noise, noise.numel(), code, seed, _lib.current_stream())
            else:
                host = torch.empty(T, R, V)
                for t in range(T):                                         # Hybrid_VAEModel._host_prepare's draws, per step
                    if method == "gumbel":
                        torch.neg(torch.log(-torch.log(torch.rand(R, V) + 1e-20) + 1e-20), out=host[t])
                    else:
                        host[t].exponential_(1)
                noise = _lib.h2d(host, dev, torch.float32)
        out = search.ensemble_rollout(members, method, temp32, top_k, top_p, noise, n, T, V, self.start_idx, self.end_idx, con)
        if rerank is not None:                                             # as Hybrid_VAEModel._rerank
            got = rerank.select(out["seqs"], n, self.start_idx, self.end_idx)
            out.update(candidates=out["seqs"], seqs=got["seqs"], consensus_scores=got["scores"], consensus_best=got["best"])
        return out


def ensemble_evaluate(models_or_ensemble, items, vocabulary, caption_output=None, dcase_format=False, zh=False,
                      batch_size=32, frontend=None, sample_n=None, rerank=None, diversity=None, **kwargs):
    """The decoding half of ``BaseRunner.ensemble`` (base_runner.py:433-478): ``items`` are ``(audio_id, feature [T, F])`` as
    for ``evaluate()``, batched with ``collate_fn([1])`` (no replication); ``kwargs`` (``method``, ``beam_size``,
    ``max_length``, the constrained-decoding keywords and ``finish_on_end`` / ``length_penalty`` / ``nbest``, with
    ``nbest > 1`` the clip's n-best list is written as its ``captions``; with ``method="dbs"`` its ``group_size`` /
    ``diversity_lambda`` / ``temperature`` / ``group_nbest``, and every returned beam is written as one of the clip's
    ``captions``, as ``evaluate`` does for a single model) go to ``Ensemble.forward``.  Writes the JSON payload of
    ``evaluate()`` or, with ``dcase_format``, the
    reference's two-column CSV (``file_name``, ``caption_predicted``).  ``frontend`` (``acvae_amd.frontend.LogMel``): the items are
    ``(audio_id, 1-D waveform)`` and the log-mel features are formed on the device, once for all members.  Returns the payload
    dict.  ``accuracy`` (an ``acvae_amd.accuracy.Accuracy``, default None = nothing changes): the rows the file shows (one
    caption per clip; the filled rows of ``method="dbs"``; the n-best list of a finishing search) are handed to it with the
    batch's keys before they are downloaded, as ``evaluate(accuracy=)`` does, with the same refusals in front of any work;
    read ``accuracy.result()`` afterwards.  METEOR and SPICE stay outside.

    ``sample_n`` (default None = every call and launch of today): the batches go through ``Ensemble.rollout`` instead,
    ``sample_n`` captions per clip from the mixture, and ``kwargs`` are ``rollout``'s (``method``, ``temp``, ``top_k``,
    ``top_p``, ``rng``, ``max_length``, the constrained-decoding keywords).  The file shows the clip's ``sample_n`` captions
    or, with ``rerank`` (an ``acvae_amd.consensus.Consensus``), the one it picks.  ``diversity`` (an
    ``acvae_amd.diversity.Diversity``) is handed the clip's ``sample_n`` rollouts (with ``rerank`` its candidates) and
    ``accuracy`` the rows the file shows, both on the device before the download, with the refusals ``evaluate()`` makes
    for the same arguments.  ``rerank`` and ``diversity`` need ``sample_n``: a search returns its own best hypotheses."""
    refuse_augmented(frontend, "ensemble_evaluate")
    accuracy = kwargs.pop("accuracy", None)
    shown = per_clip = None
    if sample_n is None:
        for name, v in (("rerank", rerank), ("diversity", diversity)):
            if v is not None:
                raise ValueError(f"ensemble_evaluate({name}=) needs sample_n: it acts on a clip's sampled captions")
    else:                                          # (refusals come in front of any work, rollout's own in its first batch)
        max_length = kwargs.get("max_length", 20)
        search.rerank_check(rerank, sample_n, dict(kwargs, method=kwargs.get("method", "sample")), max_length, False)
        if diversity is not None:
            from .diversity import MAX_LENGTH, Diversity
            if not isinstance(diversity, Diversity):
                raise ValueError(f"diversity must be an acvae_amd.diversity.Diversity, got {type(diversity).__name__}")
            per_clip = diversity.check(sample_n, "ensemble_evaluate(diversity=)")
            if max_length > MAX_LENGTH:
                raise ValueError(f"ensemble_evaluate(diversity=): max_length={max_length}; the kernel takes rows of at most "
                                 f"{MAX_LENGTH} tokens")
        if accuracy is not None:                   # the captions the file shows per clip: with rerank the picked one
            shown = accuracy_check(accuracy, 1 if rerank is not None else sample_n, max_length, zh, "ensemble_evaluate")
    if accuracy is not None and sample_n is None:  # one search per clip: the captions it returns, by forward's defaults
        counts = dict(method=kwargs.get("method", "greedy"), beam_size=kwargs.get("beam_size", 5),
                      group_size=kwargs.get("group_size", 5), group_nbest=kwargs.get("group_nbest", True))
        if kwargs.get("finish_on_end"):
            shown = kwargs.get("nbest") or 1
        else:
            shown = captions_per_clip(counts, False) if counts["method"] == "dbs" else 1
        shown = accuracy_check(accuracy, shown, kwargs.get("max_length", 20), zh, "ensemble_evaluate")
    ens = models_or_ensemble if isinstance(models_or_ensemble, Ensemble) else Ensemble(models_or_ensemble)
    device = next(ens.parameters()).device
    collate = collate_fn([1, ])
    key2pred = {}
    pending = []

    def flush():
        if not pending:
            return
        batch = collate(list(pending))
        pending.clear()
        if frontend is not None:
            batch[1], batch[-1] = frontend(batch[1], batch[-1], device=device)
        if sample_n is not None:
            output = ens.rollout(batch[1].to(device), batch[-1], sample_n=sample_n, rerank=rerank, **kwargs)
            rows = output["seqs"]
            if diversity is not None:              # the clip's rollouts as they stand on the device: nothing comes back
                diversity.update(output.get("candidates", rows), per_clip)
            if rerank is None:                     # every rollout is one of the clip's captions
                rows = rows.reshape(len(batch[0]), sample_n, rows.shape[-1])
        else:
            output = ens(batch[1].to(device), batch[-1], **kwargs)
            rows = output["nbest_seqs"] if "nbest_seqs" in output and output["nbest_seqs"].shape[1] > 1 else output["seqs"]
        if accuracy is not None:                   # the rows the file shows, as they stand on the device
            accuracy.update(batch[0], accuracy_rows(rows, shown), shown)
        collect_predictions(batch[0], rows.cpu().numpy(), vocabulary, zh, key2pred)

    for item in items:
        if frontend is not None:                   # collate_fn pads into float32: PCM becomes the samples it stands for
            item = (item[0], frontend.to_float(item[1]))
        pending.append(item)
        if len(pending) == batch_size:
            flush()
    flush()
    payload = predictions_payload(key2pred, zh)
    if caption_output is not None:
        with open(Path(caption_output), "w", newline="") as fh:
            if dcase_format:                                               # base_runner.py:463-467, 475-476
                import csv
                writer = csv.writer(fh, lineterminator="\n")
                writer.writerow(["file_name", "caption_predicted"])
                for key, preds in key2pred.items():
                    writer.writerow([key, "".join(preds[0]) if zh else preds[0]])
            else:
                json.dump(payload, fh, indent=4)
    return payload
