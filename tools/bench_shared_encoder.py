"""Time the cross-entropy training step that shares one encoder pass among a clip's captions
(TrainStep.step(..., clip_index=)) against what the package could do before, on one MI355X.  Not product, not the project's
benchmark (bench.py measures the plain step); it writes down numbers that had not been measured.

    python tools/bench_shared_encoder.py [--B 32 --k 5 --T 1000 --steps 20 --warmup 5] [--only shared|five_plain|repeated]
    python tools/bench_shared_encoder.py --kernel-report DIR       # after: rocprofv3 --kernel-trace --stats -d DIR ... -- python
                                                                   #        tools/bench_shared_encoder.py --only shared

Shape: BASELINE configs[1] (T = 1000, F = 64, V = 5000, E = 512), 22-token captions, fp32, B = 32 clips with k = 5 captions
each (160 caption rows), full optimiser steps, warm-up then the mean of `--steps` steps, wall clock around a synchronised
loop.  Three ways through the same 160 captions:
  shared      one step(clip_index=): the encoder sees the 32 clips once, posterior / decode loop / losses see 160 rows
  five_plain  five plain steps of 32 rows (the clips with their j-th caption, j = 0..4): the reference sampler's epoch
  repeated    one plain step with the features repeated to 160 rows
A second pass splits the step on its main stream with HIP events: the encoder's forward, the encoder's backward (from the
moment the gradient of its output exists to the end of backward()), and the rest - the text side on 160 rows (which runs on
the per-step launches: the persistent kernels take at most 32 rows), the gather / fold, losses, norm and update.

--kernel-report reads a rocprofv3 kernel trace of the shared step and prints the two new kernels' time and the bandwidth
they reach: bytes moved = (B + N) * R * 4 per call (every source row read once, every destination row written once; the
rows a clip shares are re-read through the caches), against the 8 TB/s peak."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, E, L = 5000, 512, 22
PEAK_GBS = 8000.0


def build():
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    m = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                        prior_model="PriorRNN", prior_args={"hidden_size": E})
    return m.cuda().train()


class Phases:
    """HIP events on the step's main stream: around the encoder's forward, at the start of its backward (a hook on the
    gradient of its output) and at the end of backward()."""

    def __init__(self, model, ts):
        self.on, self.steps = False, []
        enc_forward, finish = model.encoder.forward, ts.exchange.finish

        def forward(*a, **k):
            if not self.on:
                return enc_forward(*a, **k)
            ev = self.steps[-1]
            ev["f0"].record()
            out = enc_forward(*a, **k)
            ev["f1"].record()
            out["audio_embeds"].register_hook(lambda g: ev["b0"].record())
            return out

        def finished(*a, **k):
            if self.on:
                self.steps[-1]["b1"].record()
            return finish(*a, **k)
        model.encoder.forward, ts.exchange.finish = forward, finished

    def step(self, fn):
        ev = {n: torch.cuda.Event(enable_timing=True) for n in ("t0", "f0", "f1", "b0", "b1", "t1")}
        self.steps.append(ev)
        ev["t0"].record()
        fn()
        ev["t1"].record()

    def report(self):
        torch.cuda.synchronize()
        n = len(self.steps)
        tot = sum(e["t0"].elapsed_time(e["t1"]) for e in self.steps) / n
        fwd = sum(e["f0"].elapsed_time(e["f1"]) for e in self.steps) / n
        bwd = sum(e["b0"].elapsed_time(e["b1"]) for e in self.steps) / n
        return tot, fwd, bwd


def kernel_report(directory, B, N, R):
    traces = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    per = {"rows_gather_kernel": [], "rows_fold_kernel": []}
    with open(traces[0]) as fh:
        for r in csv.DictReader(fh):
            for name in per:
                if name in r["Kernel_Name"]:
                    per[name].append((int(r["Grid_Size_X"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    nbytes = (B + N) * R * 4
    for name, calls in per.items():
        if not calls:
            raise SystemExit(f"{name}: no dispatch in {traces[0]}")
        grid = max(g for g, _ in calls)                     # the gather of the pooled embedding [B, 512] is the same kernel
        big, small = [u for g, u in calls if g == grid], [u for g, u in calls if g != grid]
        mean = float(np.mean(big))
        print(f"{name}: {len(big)} calls on the encoder memory [{B} -> {N}, {R}]: mean {mean:.2f} us, min {min(big):.2f}, max "
              f"{max(big):.2f}; {nbytes / 1e6:.1f} MB moved -> {nbytes / mean / 1e3:.0f} GB/s = "
              f"{nbytes / mean / 1e3 / PEAK_GBS:.1%} of the {PEAK_GBS / 1e3:.0f} TB/s peak"
              + (f"; {len(small)} calls on the pooled embedding [{B} -> {N}, 512] ({(B + N) * 512 * 4 / 1e3:.0f} KB): mean "
                 f"{float(np.mean(small)):.2f} us" if small else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("shared", "five_plain", "repeated"))
    ap.add_argument("--kernel-report", default=None, metavar="DIR")
    args = ap.parse_args()
    B, k, T = args.B, args.k, args.T
    N = B * k
    if args.kernel_report:
        return kernel_report(args.kernel_report, B, N, (T // 16) * 512)
    if args.steps < 10:
        raise SystemExit("--steps: the mean of at least 10 steps")
    from acvae_amd.trainer import TrainStep
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, T, 64, generator=g).cuda()
    lens = np.full(B, T)
    clip_index = np.repeat(np.arange(B), k)[torch.randperm(N, generator=g).numpy()]     # rows in any order, e.g. the collate's
    caps = torch.randint(4, V, (N, L), generator=g).float()
    caps[:, 0], caps[:, -1] = 1, 2
    cap_lens = np.full(N, L)
    feats_rep = feats[torch.from_numpy(clip_index).cuda()].contiguous()
    # the j-th caption of every clip, in clip order: five batches of 32 (clip, caption) pairs
    rows_of = [np.flatnonzero(clip_index == c) for c in range(B)]
    plain = [np.array([rows_of[c][j] for c in range(B)]) for j in range(k)]

    def make(mode):
        model = build()
        ts = TrainStep(model, V)

        def step():
            if mode == "shared":
                ts.step(feats, lens.copy(), caps, cap_lens, 1.0, 0, 0.5, clip_index=clip_index)
            elif mode == "repeated":
                ts.step(feats_rep, np.full(N, T), caps, cap_lens, 1.0, 0, 0.5)
            else:
                for rows in plain:
                    ts.step(feats, lens.copy(), caps[rows], cap_lens[rows], 1.0, 0, 0.5)
        return model, ts, step

    results = {}
    for mode in ("shared", "five_plain", "repeated"):
        if args.only and mode != args.only:
            continue
        model, ts, step = make(mode)
        for _ in range(args.warmup):
            step()
        ts.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ts.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        results[mode] = ms
        print(f"{mode}: {ms:.2f} ms for {N} captions = {N / ms:.2f} k captions/s (B={B}, k={k}, T={T}, V={V}, E={E}, {L}-token "
              f"captions, fp32; mean of {args.steps} after {args.warmup} warm-up)", flush=True)
        if mode != "five_plain":
            ph = Phases(model, ts)
            ph.on = True
            for _ in range(max(3, args.steps // 4)):
                ph.step(step)
            tot, fwd, bwd = ph.report()
            rest = tot - fwd - bwd
            print(f"{mode}: main stream, mean of {len(ph.steps)} further steps: {tot:.2f} ms = encoder forward {fwd:.2f} + encoder "
                  f"backward {bwd:.2f} + the rest {rest:.2f} ({rest / tot:.0%}: text side on {N} rows, "
                  f"{'gather / fold, ' if mode == 'shared' else ''}losses, norm, update)", flush=True)
        del model, ts, step
        torch.cuda.empty_cache()
    if "shared" in results:
        for other in ("five_plain", "repeated"):
            if other in results:
                print(f"shared {results['shared']:.2f} ms vs {other} {results[other]:.2f} ms: {results[other] / results['shared']:.2f} x")


if __name__ == "__main__":
    main()
