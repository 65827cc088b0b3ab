"""N2 — the evaluation wrapper around the inference twin (host logic).

Mirrors ``BaseRunner.evaluate`` / ``_convert_idx2sentence`` (``runners/base_runner.py:146-157, 199-293``): decode every
clip of an evaluation set (greedy, N z-samples per clip, beam or diverse beam search), turn the token ids into
sentences with the training vocabulary and write the prediction file the reference's scoring scripts read:

    {"predictions": [{"filename": id, "caption": str, "tokens": str}, ...]}                       one caption per clip
    {"predictions": [{"filename": id, "captions": [{"caption", "cap_id", "tokens"}, ...]}, ...]}  N captions per clip

Of the scoring (pycocoevalcap BLEU/ROUGE/CIDEr/METEOR/SPICE, base_runner.py:295-320) BLEU, ROUGE-L and CIDEr are scored on
the device with ``accuracy=`` (acvae_amd/accuracy.py); METEOR and SPICE need Java and stay outside.
"""
import io
import json
import pickle
from pathlib import Path

import numpy as np
import torch

from .batch import collate_fn, forward_batch, forward_batch_shared_encoder
from .frontend import refuse_augmented


class Vocabulary(object):
    """``utils/build_vocab.py:9-28``: word <-> index maps; unknown words map to ``<unk>``."""

    def __init__(self):
        self.word2idx = {}
        self.idx2word = {}
        self.idx = 0

    def add_word(self, word):
        if word not in self.word2idx:
            self.word2idx[word] = self.idx
            self.idx2word[self.idx] = word
            self.idx += 1

    def __call__(self, word):
        return self.word2idx[word] if word in self.word2idx else self.word2idx["<unk>"]

    def __len__(self):
        return len(self.word2idx)


class _VocabUnpickler(pickle.Unpickler):
    """The reference pickles ``utils.build_vocab.Vocabulary`` instances (``config["vocab_file"]``); resolve that
    class name to the one above so its vocabulary files load without the reference tree on the path."""

    def find_class(self, module, name):
        if name == "Vocabulary" and module.split(".")[-1] == "build_vocab":
            return Vocabulary
        return super().find_class(module, name)


def load_vocabulary(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray)):
        return _VocabUnpickler(io.BytesIO(path_or_bytes)).load()
    with open(path_or_bytes, "rb") as fh:
        return _VocabUnpickler(fh).load()


def convert_idx2sentence(word_ids, vocabulary, zh=False):
    """base_runner.py:146-157: words up to (not including) the first ``<end>``, ``<start>`` dropped; a space-joined
    string, or the word list itself when ``zh``."""
    words = []
    for word_id in word_ids:
        word = vocabulary.idx2word[int(word_id)]
        if word == "<end>":
            break
        if word != "<start>":
            words.append(word)
    return words if zh else " ".join(words)


def collect_predictions(keys, seqs, vocabulary, zh, key2pred):
    """base_runner.py:247-266: append the sentence(s) of every row of ``seqs`` ([rows, len], or [rows, k, len] when a
    search returns k hypotheses per row) to ``key2pred[key of that row]``."""
    for key, seq in zip(keys, seqs):
        rows = seq if getattr(seq, "ndim", 1) > 1 else [seq]
        for row in rows:
            key2pred.setdefault(key, []).append(convert_idx2sentence(row, vocabulary, zh))
    return key2pred


def predictions_payload(key2pred, zh=False):
    """base_runner.py:272-292: the JSON document, clips in first-seen order."""
    def entry(pred):
        return {"caption": "".join(pred) if zh else pred, "tokens": " ".join(pred) if zh else pred}

    out = []
    for key, preds in key2pred.items():
        if len(preds) > 1:
            caps = []
            for i, pred in enumerate(preds):
                e = entry(pred)
                caps.append({"caption": e["caption"], "cap_id": i, "tokens": e["tokens"]})
            out.append({"filename": key, "captions": caps})
        else:
            e = entry(preds[0])
            out.append({"filename": key, "caption": e["caption"], "tokens": e["tokens"]})
    return {"predictions": out}


def captions_per_clip(kwargs, finishing):
    """The number of caption rows a clip gets from a decode with these keywords (``rerank`` apart)."""
    beam, method = kwargs["beam_size"], kwargs["method"]
    if finishing:                                  # the n-best list of one search per clip
        return kwargs.get("nbest", 1)
    if method == "dbs":                            # the filled rows: bdash * group_size beams, or one per group
        groups = kwargs.get("group_size", 5)
        return (beam // groups) * groups if kwargs.get("group_nbest", True) else groups
    return beam                                    # beam_size rollouts (or searches) per clip over one encoder pass


def _diversity_check(diversity, model, kwargs, finishing):
    """The refusals of ``diversity=`` (ValueError, in front of any work) -> the number of captions a clip gets from this
    call, which is the N of ``diversity.update`` (None without the keyword)."""
    if diversity is None:
        return None
    from .diversity import MAX_LENGTH, Diversity
    if not isinstance(diversity, Diversity):
        raise ValueError(f"diversity must be an acvae_amd.diversity.Diversity, got {type(diversity).__name__}")
    per_clip = diversity.check(captions_per_clip(kwargs, finishing), "evaluate(diversity=)")
    max_length = kwargs.get("max_length", getattr(model, "max_length", None))
    if max_length is not None and max_length > MAX_LENGTH:
        raise ValueError(f"evaluate(diversity=): max_length={max_length}; the kernel takes rows of at most {MAX_LENGTH} tokens")
    return per_clip


def accuracy_check(accuracy, per_clip, max_length, zh, who="evaluate"):
    """The refusals of ``accuracy=`` (ValueError, in front of any work): ``per_clip`` captions a clip gets in the file, rows
    of ``max_length`` tokens -> the N of ``accuracy.update`` (None without the keyword)."""
    if accuracy is None:
        return None
    from .accuracy import MAX_LENGTH, Accuracy
    if not isinstance(accuracy, Accuracy):
        raise ValueError(f"accuracy must be an acvae_amd.accuracy.Accuracy, got {type(accuracy).__name__}")
    if zh:
        raise ValueError(f"{who}(accuracy=): zh=True is not scored: the references are split at whitespace")
    per_clip = accuracy.check(per_clip, f"{who}(accuracy=)")
    if max_length is not None and max_length > MAX_LENGTH:
        raise ValueError(f"{who}(accuracy=): max_length={max_length}; the kernel takes rows of at most {MAX_LENGTH} tokens")
    if max_length is not None and accuracy.width is not None and max_length != accuracy.width:
        raise ValueError(f"{who}(accuracy=): max_length={max_length} after updates with rows of {accuracy.width} tokens: all "
                         "updates of one object share one row width (reset() starts over)")
    return per_clip


def accuracy_rows(rows, per_clip):
    """The rows of a batch that the file shows, on the device, as ``accuracy.update`` takes them: [B * per_clip, T].  A
    diverse beam search's rows beyond ``per_clip`` are the end_idx filler of ``search._dbs_rows`` and stay out (the one case
    in which the rows are copied: everywhere else this is a view)."""
    if rows.dim() == 3:
        rows = rows[:, :per_clip]
    return rows.reshape(-1, rows.shape[-1])


def evaluate_likelihood(model, items, key2caps, vocabulary, output=None, batch_size=1, z=("posterior", "prior"), samples=1,
                        frontend=None, device=None):
    """Score the GIVEN captions of an evaluation set under the model (``acvae_amd.likelihood`` says what is measured): held-out
    likelihood and perplexity, per-caption KL, teacher-forced top-1 / top-5 word accuracy.

    ``items``: ``(audio_id, feature [T, F])`` as ``evaluate`` takes them (``frontend=``: ``(audio_id, 1-D waveform)``; an
    ``Augmented`` front end is refused), batched ``batch_size`` clips at a time.  ``key2caps[audio_id]``: the clip's captions,
    tokenized as the vocabulary's words are (strings split at whitespace, or word lists, as for ``Accuracy``); a word outside
    the vocabulary maps to ``<unk>``; ``<start>`` / ``<end>`` are added here.  ``z``: a mode or a tuple of modes; ONE encoder
    pass per batch is shared by the modes, each of which is one ``score_captions`` forward with ``samples`` draws per caption.
    -> ``{mode: Likelihood.result()}``, the pairs keyed ``[audio_id, caption number]``; written to ``output`` as JSON.

    The items stream batch by batch, as in ``evaluate``; ``key2caps`` is checked as a whole first.

    ValueError in front of any launch and any random draw: what ``score_captions`` refuses (``samples`` outside 1 .. 16, an
    unknown mode, a decoder with ``hidden_size != embed_size``, unequal numbers of captions per clip in ``key2caps`` while
    ``batch_size > 1``: pad the smaller sets, or score one clip per batch), an entry of ``key2caps`` without captions, a
    caption without words.  An item whose id ``key2caps`` lacks is known only when it arrives: ValueError in front of its own
    batch's launches."""
    from . import likelihood as lk
    who = "evaluate_likelihood"
    modes = (z,) if isinstance(z, str) else tuple(z)
    if not modes:
        raise ValueError(f"{who}: no mode in z")
    refuse_augmented(frontend, who)
    for mode in modes:
        lk.check_mode(mode, who)
    samples = lk.check_samples(samples, who)
    lk.check_model(model, who)
    start, end = vocabulary("<start>"), vocabulary("<end>")
    # the captions are checked as a whole, in front of any work and without touching the items, which stream batch by
    # batch as in ``evaluate`` (a lazily loading set is never held in memory at once)
    tokens, counts = {}, set()
    for audio_id, given in key2caps.items():
        given = list(given) if given is not None else []
        if not given:
            raise ValueError(f"{who}: clip {audio_id!r} has no captions")
        rows_ = []
        for cap in given:
            words = cap.split() if isinstance(cap, str) else list(cap)
            if not words:
                raise ValueError(f"{who}: clip {audio_id!r} has a caption without words")
            rows_.append([start] + [vocabulary(w) for w in words] + [end])
        tokens[audio_id] = rows_
        counts.add(len(rows_))
    if batch_size > 1 and len(counts) > 1:
        raise ValueError(f"{who}: every clip needs the same number of captions (got between {min(counts)} and {max(counts)}) "
                         f"when clips share a batch (batch_size={batch_size}): the shared-encoder forward (clip_index=) has that "
                         "rule; pad the smaller sets, e.g. by repeating one of the clip's captions, or use batch_size=1")
    device = device if device is not None else next(model.parameters()).device
    meters = {mode: lk.Likelihood(mode, samples) for mode in modes}
    collate = collate_fn([1, ])
    pending = []

    def flush():
        if not pending:
            return
        chunk = list(pending)
        pending.clear()
        keys = [[audio_id, i] for audio_id, _ in chunk for i in range(len(tokens[audio_id]))]
        caps = [cap for audio_id, _ in chunk for cap in tokens[audio_id]]
        clip = np.array([b for b, (audio_id, _) in enumerate(chunk) for _ in tokens[audio_id]], dtype=np.int64)
        lens = np.array([len(c) for c in caps], dtype=np.int64)
        rows = lk.Rows(lens, clip, len(chunk), samples, who)
        padded = np.zeros((len(caps), int(lens.max())), dtype=np.int64)
        for row, cap in zip(padded, caps):
            row[:len(cap)] = cap
        batch = collate(chunk)
        feats, feat_lens, encoded = lk.encode_clips(model, batch[1], batch[-1], frontend, device)
        for mode in modes:
            meters[mode].update(keys, lk.score_rows(model, feats, feat_lens, encoded, torch.from_numpy(padded), rows, mode))

    with lk.eval_mode(model):
        for audio_id, data in items:
            if audio_id not in tokens:
                raise ValueError(f"{who}: clip {audio_id!r} has no captions in key2caps")
            if frontend is not None:               # collate_fn pads into float32: PCM becomes the samples it stands for
                data = frontend.to_float(data)
            pending.append((audio_id, data))
            if len(pending) == batch_size:
                flush()
        flush()
    payload = {mode: meters[mode].result() for mode in modes}
    if output is not None:
        with open(Path(output), "w") as fh:
            json.dump(payload, fh, indent=4)
    return payload


def evaluate(model, items, vocabulary, caption_output=None, zh=False, batch_size=1, device=None, frontend=None,
             **kwargs):
    """Decode an evaluation set and (optionally) write the prediction file.

    ``items``: iterable of ``(audio_id, feature [T, F] tensor)`` in the order of the reference's ``CaptionEvalDataset``;
    they are batched with ``collate_fn([1])`` exactly as its DataLoader does.  ``kwargs`` go to the model as in
    ``evaluate(**kwargs)`` there: ``method`` ("greedy" | "beam" | "dbs"), ``beam_size`` (with "greedy": z-samples per
    clip), ``max_length``.  Sampled decoding, which the reference's evaluation does not offer: ``method="sample"`` (or
    ``"gumbel"``) with ``temp``, ``rng`` ("host" | "device") and the truncation keywords ``top_k`` (the k most probable
    words of each step, 0 = off) and ``top_p`` (the nucleus of that mass, 1.0 = off), e.g. ``method="sample", beam_size=5,
    top_p=0.9, rng="device"`` for five sampled captions per clip; ``top_k`` / ``top_p`` with any other method are a
    ValueError (``Hybrid_VAEModel._truncation``).  Constrained decoding, with every method but "dbs":
    ``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``, ``suppress_tokens`` (``Hybrid_VAEModel._constraints``),
    e.g. ``method="beam", beam_size=3, no_repeat_ngram_size=3``.  ``finish_on_end=True`` with ``method="beam"`` (and
    ``length_penalty``, ``nbest``; ``Hybrid_VAEModel._finishing``): ONE beam search of width ``beam_size`` per clip, no
    replicas, whose hypotheses finish at ``<end>``; the file holds hypothesis 0 per clip or, with ``nbest > 1``, the clip's
    n-best list as its ``captions``.  ``method="dbs"`` (``group_size``, ``diversity_lambda``, ``temperature``,
    ``group_nbest``): one diverse beam search per clip, one library call per batch, every returned beam one of the clip's
    ``captions``; ``dbs_impl="host"`` runs the host loop over the step API instead (same captions).  ``rerank`` (an ``acvae_amd.consensus.Consensus``): with
    ``beam_size=N`` rollouts per clip (2 <= N <= 16; "greedy", "sample" or "gumbel"), the caption written per clip is the
    rollout that agrees most with the clip's other rollouts under CIDEr-D, chosen on the device
    (``Hybrid_VAEModel._rerank``); the file then has the one-caption-per-clip form.  ``frontend`` (``acvae_amd.frontend.LogMel``): the items are ``(audio_id, 1-D waveform)``, fp32
    or int16 PCM (``acvae_amd.frontend.read_wav``); the log-mel features are formed on the device in front of either
    forward path.  ``diversity`` (an ``acvae_amd.diversity.Diversity``, default None = nothing changes): wherever a clip gets
    2 .. 16 captions (``beam_size=N`` rollouts, with ``rerank`` its candidates; the filled rows of ``method="dbs"``; the
    n-best list of a finishing search), their n-gram statistics are counted on the device before the rows are downloaded,
    one launch per batch and no copy; read ``diversity.result()`` afterwards (Div1, Div2, gDiv1, mBLeu_1..4).  One caption
    per clip or more than 16, or ``max_length > 64``: ValueError in front of any work.  The payload and the file are the
    same with and without it.  ``accuracy`` (an ``acvae_amd.accuracy.Accuracy``, default None = nothing changes): the rows the
    file shows (one caption per clip, with ``rerank`` the picked one; the ``beam_size=N`` rollouts; the filled rows of
    ``method="dbs"``; the n-best list of a finishing search) are handed to it with the batch's keys before they are
    downloaded, no launch and no copy; read ``accuracy.result()`` afterwards (Bleu_1..4, ROUGE_L, CIDEr against the clips'
    references).  A wrong type, more than 16 captions per clip, ``max_length > 64``, another N or row width than the
    object's earlier updates, or ``zh=True``: ValueError in front of any work.  ``accuracy`` and ``diversity`` work
    together.  Returns the payload dict."""
    refuse_augmented(frontend, "evaluate")
    kwargs.setdefault("method", "greedy")
    kwargs.setdefault("beam_size", 1)
    collate = collate_fn([1, ])
    model.eval()
    if kwargs.get("rerank") is None:
        kwargs.pop("rerank", None)                 # absent and None alike: every call runs what it ran before
    else:                                          # (refusals come in front of any work)
        if not hasattr(model, "_rerank_check"):
            raise ValueError(f"rerank: {type(model).__name__} has no N-samples-per-clip route to rerank")
        model._rerank_check(kwargs["rerank"], kwargs["beam_size"], kwargs)
    finishing = bool(kwargs.get("finish_on_end"))
    if finishing:                                  # (its refusals too come in front of any work)
        if not hasattr(model, "_finishing"):
            raise ValueError(f"finish_on_end: {type(model).__name__} has no finishing beam search")
        model._finishing(kwargs)
    diversity = kwargs.pop("diversity", None)      # (None: nothing else changes, every call runs what it ran before)
    per_clip = _diversity_check(diversity, model, kwargs, finishing)
    accuracy = kwargs.pop("accuracy", None)        # (likewise)
    shown = None
    if accuracy is not None:                       # the captions the file shows per clip: with rerank the picked one
        shown = 1 if "rerank" in kwargs else captions_per_clip(kwargs, finishing)
        shown = accuracy_check(accuracy, 1 if shown is None else shown,
                               kwargs.get("max_length", getattr(model, "max_length", None)), zh)
    key2pred = {}
    pending = []

    def measure(output):
        """The clip's captions as they stand on the device, clip-major, to ``diversity.update``: nothing comes back."""
        if finishing:
            rows = output["nbest_seqs"]
        elif kwargs["method"] == "dbs":            # (the filled rows only, not the end_idx filler of search._dbs_rows)
            rows = output["seqs"][:, :per_clip]
        else:
            rows = output["candidates"] if "candidates" in output else output["seqs"]
        diversity.update(rows.reshape(-1, rows.shape[-1]), per_clip)

    def flush():
        if not pending:
            return
        batch = collate(list(pending))
        pending.clear()
        clip_keys = list(batch[0])                 # (the N-samples route replaces batch[0] by the replicated keys)
        with torch.no_grad():
            if finishing:                          # one search per clip: beam_size is its width, not a number of replicas
                output = forward_batch(model, batch, "validation", device=device, frontend=frontend, **kwargs)
            elif kwargs["beam_size"] > 1 and kwargs["method"] != "dbs":     # N samples per clip: one encoder pass per clip
                output = forward_batch_shared_encoder(model, batch, device=device, frontend=frontend, **kwargs)
            else:
                output = forward_batch(model, batch, "eval", device=device, frontend=frontend, **kwargs)
            if diversity is not None:
                measure(output)
        rows = output["nbest_seqs"] if finishing and output["nbest_seqs"].shape[1] > 1 else output["seqs"]
        if accuracy is not None:                   # the rows the file shows, as they stand on the device
            accuracy.update(clip_keys, accuracy_rows(rows, shown), shown)
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
        with open(Path(caption_output), "w") as fh:
            json.dump(payload, fh, indent=4)
    return payload
