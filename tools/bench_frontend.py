"""Time the log-mel front end (acvae_amd.frontend.LogMel -> acvae_logmel_fwd) on one MI355X.  Not product, not the
project's benchmark (bench.py measures the training step from finished features); it writes down numbers that had not been
measured.

    python tools/bench_frontend.py [--B 32 --seconds 10 --launches 20 --warmup 5] [--no-step] [--steps 20]

Kernel: for each PANNs preset a batch of B clips of `--seconds` s, fp32 and int16 PCM already on the device; every launch
timed on its own with HIP events, the median of `--launches` after `--warmup`.  Executed FLOP = N T n_fft 4 nb (the DFT as
a GEMM: per frame n_fft terms for the real and the imaginary part of nb bins, 2 FLOP per multiply-add), over the 157.3
TFLOP/s fp32 matrix peak.  The mel product, the squares and the log are not counted.

Step: TrainStep.step at BASELINE configs[1] (Cnn10, V = 5000, E = 512, 22-token captions, fp32, B clips of `--seconds` s at
32 kHz = 1001 frames), the batch in page-locked host memory and uploaded inside the timed loop: finished features (8 MB),
fp32 waveforms with frontend= (41 MB) and int16 waveforms with frontend= (20 MB).  Wall clock around a synchronised loop,
mean of `--steps` after `--warmup`."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
V, E, L = 5000, 512, 22


def kernel_times(fe, waves, lens, launches, warmup):
    for _ in range(warmup):
        fe(waves, lens)
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fe(waves, lens)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def bench_kernel(args):
    from acvae_amd.frontend import LogMel
    for name, fe in (("panns_32k", LogMel.panns_32k()), ("panns_16k", LogMel.panns_16k())):
        Ls = int(args.seconds * fe.sample_rate)
        g = torch.Generator().manual_seed(1)
        f32 = (0.1 * torch.randn(args.B, Ls, generator=g)).cuda()
        i16 = (f32 * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        lens = np.full(args.B, Ls)
        T = int(fe.n_frames(Ls))
        flop = args.B * T * fe.n_fft * 4 * fe.n_bins
        for kind, w in (("fp32", f32), ("int16", i16)):
            ms = kernel_times(fe, w, lens, args.launches, args.warmup)
            med = statistics.median(ms)
            print(f"{name} {kind}: B={args.B} x {args.seconds:g} s -> [{args.B}, {T}, {fe.n_mels}]: median {med:.3f} ms of "
                  f"{len(ms)} launches (min {min(ms):.3f}, max {max(ms):.3f}) after {args.warmup} warm-up; {flop / 1e9:.1f} GFLOP "
                  f"executed -> {flop / med / 1e9:.1f} TFLOP/s = {flop / med / 1e9 / PEAK_TFLOPS:.1%} of the {PEAK_TFLOPS} "
                  f"TFLOP/s fp32 matrix peak (event pairs include the launch and the 128-B upload of the lengths)", flush=True)


def bench_step(args):
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.frontend import LogMel
    from acvae_amd.trainer import TrainStep
    from acvae_amd.vae_model import Hybrid_VAEModel
    fe = LogMel.panns_32k()
    B, Ls = args.B, int(args.seconds * fe.sample_rate)
    g = torch.Generator().manual_seed(3)
    waves = 0.1 * torch.randn(B, Ls, generator=g)
    pcm = (waves * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    wl = np.full(B, Ls)
    feats, fl = fe(waves, wl)
    feats_host = feats.cpu().pin_memory()
    waves, pcm = waves.pin_memory(), pcm.pin_memory()
    caps = torch.randint(4, V, (B, L), generator=g).float()
    caps[:, 0], caps[:, -1] = 1, 2
    cl = np.full(B, L)
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().train()
    ts = TrainStep(model, V)
    dev = ts.flat_p.device
    variants = (("features, 8 MB upload", lambda: ts.step(feats_host.to(dev, non_blocking=True), fl.copy(), caps, cl, 1.0, 0, 0.5)),
                ("frontend=, fp32 waveforms", lambda: ts.step(waves, wl, caps, cl, 1.0, 0, 0.5, frontend=fe)),
                ("frontend=, int16 waveforms", lambda: ts.step(pcm, wl, caps, cl, 1.0, 0, 0.5, frontend=fe)))
    for rnd in range(2):                            # twice, alternating: the spread between the rounds is the noise
        for name, step in variants:
            for _ in range(args.warmup):
                step()
            ts.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            ts.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            print(f"step, round {rnd}: {name}: {ms:.2f} ms (B={B}, {int(fe.n_frames(Ls))} frames, V={V}, E={E}, fp32; mean of "
                  f"{args.steps} after {args.warmup} warm-up)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_frontend.py needs an MI355X: nothing here can be measured on the host")
    bench_kernel(args)
    if not args.no_step:
        bench_step(args)


if __name__ == "__main__":
    main()
