"""Time the self-critical training step (TrainStep.scst_step) on one MI355X.  Not product, not the project's benchmark
(bench.py measures the cross-entropy step); it writes down numbers that had not been measured.

    python tools/bench_scst.py [--B 32 --T 1000 --steps 20 --warmup 5] [--only n1|n5|n5_repeat] [--scorer stub|host|device]

Shape: BASELINE configs[1] (B = 32, T = 1000, V = 5000, E = 512), max_length 20, multinomial sampling with the noise made on
the device (rng="device": the reference's CPU-generator draws of [20, N, 5000] noise cost the host more than the step).
The scorer: `stub` - of negligible cost (the step without a reward's cost); `host` - CIDEr-D as a dictionary scorer on the
host (tests/cider_util.py, what a pycocoevalcap-style scorer costs); `device` - acvae_amd.cider.CiderD, the reward computed
on the device.  `host` and `device` score against synthetic references, 5 per clip of 8-16 words drawn from the 5000-word
vocabulary with a seed; `device` also reports the host time of CiderD.prepare() per step and the size of its upload.
Three steps are timed, warm-up then the mean of `--steps` steps, wall clock around a
synchronised loop:
  n1         sample_n = 1: greedy baseline + one sampled rollout (ScstWrapper)
  n5         sample_n = 5, each clip encoded once, memory rows repeated on the device (NScstWrapper)
  n5_repeat  sample_n = 5 the reference's way: the features repeated five times through the encoder, Nscst_Loss
and each is split into phases by HIP events on the step's stream in a second pass (encoder forwards, rollouts, the host's
reward between them and the loss, loss, backward + gradient norm, update).  A phase is the span between two events on the
stream, so time the stream spends waiting for the host inside a phase counts for that phase."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acvae_amd import train_util  # noqa: E402
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder  # noqa: E402
from acvae_amd.encoder import Cnn10  # noqa: E402
from acvae_amd.trainer import TrainStep  # noqa: E402
from acvae_amd.vae_model import Hybrid_VAEModel  # noqa: E402

V, E, MAXLEN = 5000, 512, 20


class CheapScorer:
    """One score per key from the hypothesis' length: no string work beyond what the sentence conversion already did."""

    def compute_score(self, references, hypotheses):
        s = np.array([(len(hypotheses[k][0]) % 7) / 7.0 for k in references])
        return float(s.mean()), s


class Vocabulary:
    def __init__(self):
        self.idx2word = [f"w{i}" for i in range(V)]


def make_scorer(kind, vocab):
    if kind == "stub":
        return CheapScorer()
    if kind == "host":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from cider_util import DictCiderD
        return DictCiderD()
    from acvae_amd.cider import CiderD
    return CiderD(vocab)


def synthetic_refs(keys, vocab, seed=7, nrefs=5):
    rng = np.random.default_rng(seed)
    return {k: [" ".join(vocab.idx2word[int(i)] for i in rng.integers(4, V, rng.integers(8, 17))) for _ in range(nrefs)]
            for k in keys}


def build():
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    m = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                        prior_model="PriorRNN", prior_args={"hidden_size": E})
    return m.cuda().train()


class Phases:
    """HIP events around the phases of a step, by wrapping the calls that begin and end them."""

    def __init__(self, model, ts):
        self.model, self.ts, self.marks, self.on = model, ts, [], False
        self._wrap(model.encoder, "forward", "encoder forward")
        self._wrap(model, "stepwise_forward", "rollout")
        self._wrap(train_util, "scst_policy_loss", "loss")
        self._wrap(ts, "_backward_and_update", "backward + norm + update")
        self._wrap(ts.optimizer, "step", "update")

    def _wrap(self, obj, name, tag):
        orig = getattr(obj, name)

        def wrapped(*a, **k):
            if not self.on:
                return orig(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(*a, **k)
            e1.record()
            self.marks.append((tag, e0, e1))
            return out
        setattr(obj, name, wrapped)

    def report(self, steps):
        torch.cuda.synchronize()
        tot = {}
        for tag, e0, e1 in self.marks:
            tot.setdefault(tag, [0.0, 0])
            tot[tag][0] += e0.elapsed_time(e1)
            tot[tag][1] += 1
        if "update" in tot:
            tot["backward + norm"] = [tot["backward + norm + update"][0] - tot["update"][0], tot["update"][1]]
            del tot["backward + norm + update"]
        return ", ".join(f"{tag} {ms / steps:.2f} ms ({n // steps} per step)" for tag, (ms, n) in tot.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--scorer", default="stub", choices=("stub", "host", "device"))
    args = ap.parse_args()
    B, T = args.B, args.T
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, T, 64, generator=g).cuda()
    lens = np.full(B, T)
    keys = [f"clip{i}" for i in range(B)]
    vocab = Vocabulary()
    key2refs = {k: ["w4 w5 w6"] for k in keys} if args.scorer == "stub" else synthetic_refs(keys, vocab)
    scorer = make_scorer(args.scorer, vocab)
    feats5 = feats.repeat_interleave(5, 0)
    lens5 = np.repeat(lens, 5)

    def make(mode):
        model = build()
        ts = TrainStep(model, V)
        crit = train_util.Nscst_Loss(scorer, sample_n=5)
        crit.end_idx = model.end_idx

        def step():
            if mode == "n1":
                return ts.scst_step(feats, lens.copy(), keys, key2refs, vocab, scorer, max_length=MAXLEN, rng="device")
            if mode == "n5":
                return ts.scst_step(feats, lens.copy(), keys, key2refs, vocab, scorer, sample_n=5, max_length=MAXLEN,
                                    rng="device")
            for p in ts.order:                       # the reference's way: the encoder sees every clip five times
                p.grad = None
            out = model(feats5, lens5.copy(), method="sample", max_length=MAXLEN, rng="device")
            lo = crit(dict(sampled_seqs=out["seqs"], sampled_logprobs=out["sampled_logprobs"]), keys, key2refs, vocab)
            return ts._backward_and_update(lo["loss"], {})
        return model, ts, step

    results = {}
    for mode in ("n1", "n5", "n5_repeat"):
        if args.only and mode != args.only:
            continue
        model, ts, step = make(mode)
        for _ in range(args.warmup):
            step()
        ts.synchronize()
        prep = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            parts = step()
            prep.append(getattr(scorer, "last_prepare_s", 0.0))
        ts.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        results[mode] = ms
        if args.scorer == "device":
            nbytes = scorer.prepare(keys if mode == "n1" else [k for k in keys for _ in range(5)], key2refs,
                                    "batch" if mode == "n1" else "rows").nbytes
            print(f"{mode}: CiderD.prepare() {np.mean(prep) * 1e3:.3f} ms of host time per step (max {np.max(prep) * 1e3:.3f}), "
                  f"one upload of {nbytes} B")
        ph = Phases(model, ts)
        ph.on = True
        nph = max(2, args.steps // 4)
        for _ in range(nph):
            step()
        ts.synchronize()
        print(f"{mode}: {ms:.2f} ms per SCST step, scorer {args.scorer} (B={B}, T={T}, V={V}, E={E}, max_length {MAXLEN}; mean of {args.steps} after "
              f"{args.warmup} warm-up; loss {float(parts['loss']):.4f})")
        print(f"{mode}: phases, mean of {nph} further steps: {ph.report(nph)}")
        ph.on = False
        del model, ts, step, ph
        torch.cuda.empty_cache()
    if "n5" in results and "n5_repeat" in results:
        print(f"sample_n = 5: encode-once {results['n5']:.2f} ms vs features repeated five times {results['n5_repeat']:.2f} ms "
              f"({results['n5_repeat'] / results['n5']:.2f} x)")


if __name__ == "__main__":
    main()
