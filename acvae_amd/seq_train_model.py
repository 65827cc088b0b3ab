"""Mirror of ``models/seq_train_model.py``: self-critical sequence training around a captioning model.

``ScstWrapper(model)`` (:9-92): the greedy rollout in ``eval()`` under ``no_grad`` scores the baseline, the sampled rollout in
``train()`` is differentiated; ``NScstWrapper(model)`` (:95-166): ``sample_n`` sampled rollouts per clip, each one's baseline
the mean score of the others.  Same ``forward`` arity contract (5 inputs ``feats, feat_lens, keys, key2refs, vocabulary`` or
2), keyword names (``max_length``, ``temperature``, ``scorer``, ``sample_n``) and output keys (``greedy_seqs``,
``sampled_seqs``, ``reward``, ``score``, ``loss``).

Where this departs from the reference, on purpose:
  * ``temperature`` is passed on as the reference passes it, and as there the sampler reads ``temp``
    (models/word_model.py:176), so the rollout samples at temperature 1 unless ``temp=`` is given;
  * each rollout gets its own copy of ``feat_lens`` (the reference hands one array to both, and the encoder divides it in
    place each time); the caller's array ends up divided once, as after one model call;
  * ``NScstWrapper`` encodes each clip ONCE and repeats the memory rows ``sample_n`` times on the device (the reference's
    runner repeats the features); rows are clip-major (row ``n * sample_n + j``); the replicas of a clip share the
    encoder's dropout masks;
  * the words come back to the host once per call for the reward (one synchronisation), whatever the number of rollouts;
  * with ``scorer=acvae_amd.cider.CiderD(vocabulary)`` they do not come back at all: the reference side of CIDEr-D is prepared
    and uploaded before the first rollout, the rows are scored on the device behind the last one, and ``reward`` / ``score``
    are device tensors.
"""
import copy

import numpy as np
import torch
import torch.nn as nn

from . import train_util

_ARITY = ("number of input should be either 5 (feats, feat_lens, keys, key2refs, vocabulary) "
          "or 2 (feats, feat_lens)!")


def _sample_kwargs(kwargs, *extra):
    if "max_length" not in kwargs:
        raise KeyError("max_length")
    out = {"temperature": kwargs.get("temperature", 1.0), "max_length": kwargs["max_length"]}
    for k in ("temp", "rng") + extra:          # `temp` is what sample_next_word reads; rng="device": Philox noise on the device
        if k in kwargs:
            out[k] = kwargs[k]
    return out


class ScstWrapper(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *input, **kwargs):
        if len(input) != 5 and len(input) != 2:
            raise Exception(_ARITY)
        if len(input) == 2:
            return self.model(*input, **kwargs)
        return self.scst(*input, **kwargs)

    def scst(self, feats, feat_lens, keys, key2refs, vocabulary, **kwargs):
        sample_kwargs = _sample_kwargs(kwargs)
        scorer = train_util._need_scorer(kwargs.get("scorer"))
        output = {}
        tables = None
        if train_util._on_device(scorer):                      # queued in front of the rollouts; depends on the references only
            tables = scorer.prepare(keys, key2refs, "batch", device=next(self.model.parameters()).device)
        self.model.eval()                                      # baseline (:38-41)
        with torch.no_grad():
            greedy = self.model(feats, copy.copy(feat_lens), method="greedy", **sample_kwargs)
        output["greedy_seqs"] = greedy["seqs"]
        self.model.train()                                     # :43-45
        sampled = self.model(feats, feat_lens, method=kwargs.get("method", "sample"), **sample_kwargs)
        output["sampled_seqs"] = sampled["seqs"]
        output["sampled_logprobs"] = sampled["sampled_logprobs"]
        if tables is not None:
            rs = tables.reward(sampled["seqs"], greedy["seqs"], 1, self.model.start_idx, self.model.end_idx)
        else:
            rs = self.get_self_critical_reward(greedy["seqs"], sampled["seqs"], keys, key2refs, vocabulary, scorer)
        output["reward"] = torch.as_tensor(rs["reward"])
        output["score"] = torch.as_tensor(rs["score"])
        output["loss"] = train_util.scst_policy_loss(sampled["sampled_logprobs"], sampled["seqs"], rs["reward"],
                                                     self.model.end_idx)
        return output

    def get_self_critical_reward(self, greedy_seqs, sampled_seqs, keys, key2refs, vocabulary, scorer):
        greedy_seqs, sampled_seqs = train_util._seqs_to_host(greedy_seqs, sampled_seqs)
        args = (key2refs, keys, self.model.start_idx, self.model.end_idx, vocabulary, scorer)
        sampled_score = train_util.compute_batch_score(sampled_seqs, *args)
        greedy_score = train_util.compute_batch_score(greedy_seqs, *args)
        return {"reward": sampled_score - greedy_score, "score": sampled_score}


class NScstWrapper(ScstWrapper):
    def forward(self, *input, **kwargs):
        if len(input) != 5 and len(input) != 2:
            raise Exception(_ARITY)
        if len(input) == 2:
            return self.model(*input, **kwargs)
        return self.nscst(*input, **kwargs)

    def nscst(self, feats, feat_lens, keys, key2refs, vocabulary, **kwargs):
        if "sample_n" not in kwargs:
            raise KeyError("sample_n")
        sample_n = int(kwargs["sample_n"])
        if sample_n < 2:
            raise ValueError("NScstWrapper: the leave-one-out baseline needs sample_n >= 2")
        sample_kwargs = _sample_kwargs(kwargs)
        scorer = train_util._need_scorer(kwargs.get("scorer"))
        keys_n = [k for k in keys for _ in range(sample_n)]
        tables = None
        if train_util._on_device(scorer):
            tables = scorer.prepare(keys_n, key2refs, "rows", device=next(self.model.parameters()).device)
        self.model.train()
        sampled = self.model.rollout_shared_encoder(feats, feat_lens, sample_n, method=kwargs.get("method", "sample"),
                                                    **sample_kwargs)
        if tables is not None:
            rs = tables.reward(sampled["seqs"], None, sample_n, self.model.start_idx, self.model.end_idx)
        else:
            rs = self.get_critical_reward(sampled["seqs"], keys_n, key2refs, vocabulary, scorer, sample_n)
        output = {"sampled_seqs": sampled["seqs"], "sampled_logprobs": sampled["sampled_logprobs"],
                  "reward": torch.as_tensor(rs["reward"]).reshape(-1), "score": torch.as_tensor(rs["score"]).reshape(-1)}
        output["loss"] = train_util.scst_policy_loss(sampled["sampled_logprobs"], sampled["seqs"], rs["reward"],
                                                     self.model.end_idx)
        return output

    def get_critical_reward(self, sampled_seqs, keys, key2refs, vocabulary, scorer, sample_n):
        """keys: one per row (clip-major).  Every row is scored on its own, as Nscst_Loss does (utils/train_util.py:307):
        compute_batch_score would score the rows that share a key once."""
        sampled_seqs, = train_util._seqs_to_host(sampled_seqs)
        score = train_util.compur_batch_score_samplen(sampled_seqs, key2refs, keys, self.model.start_idx,
                                                      self.model.end_idx, vocabulary, scorer)
        return {"reward": train_util.leave_one_out_reward(score, sample_n), "score": np.asarray(score, dtype=np.float64).reshape(-1)}
