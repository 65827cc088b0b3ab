"""Time the resampler (acvae_amd.frontend.Resample -> acvae_resample_fwd) on one MI355X, beside the log-mel kernel it
feeds.  Not product, not the project's benchmark; it writes down numbers that had not been measured.

    python tools/bench_resample.py [--B 32 --seconds 10 --launches 20 --warmup 5] [--no-step] [--steps 20]

Kernel: 44.1 -> 32 kHz and 48 -> 32 kHz (kaiser_best), a batch of B clips of `--seconds` s, fp32 and int16 PCM already on
the device.  Two figures per case: the median of `--launches` launches timed one by one with HIP events (each pair includes
the launch and the 128-B upload of the lengths), and the mean of the same number of launches between one pair of events
(back to back: the launch overhead overlaps the kernel before it).  The log-mel kernel at 32 kHz is timed the same way in
the same session: it is the yardstick.
Executed FLOP, from the shapes: rows x K x phases x 2 with rows = the blocks of the clip rounded up to the workgroup's 64,
phases = 32 per phase tile, and K = 32 x the K-steps the kernel visits (band skipping) or all rows of H rounded up to 32
(without).  Bytes: the samples read once plus the outputs written once, over the 8 TB/s HBM peak.

Step: TrainStep.step at BASELINE configs[1] (as tools/bench_frontend.py) from int16 waveforms in page-locked host memory,
uploaded inside the timed loop: 32 kHz with frontend=LogMel.panns_32k(), and 44.1 kHz with
frontend=LogMel.panns_32k().at_input_rate(44100).  Two alternating rounds; the spread between them is the noise."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_frontend import E, L, PEAK_TFLOPS, V, kernel_times     # noqa: E402

PEAK_TBS = 8.0


def back_to_back(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def flops(rs, lens):
    """(executed with band skipping, executed without) for clips of ``lens`` samples."""
    bank, index = rs.kernel_tables()
    blocks = -(-rs.out_len(np.asarray(lens)) // rs.kernel_up)
    rows = int((-(-blocks // 64) * 64).sum())
    band = int(index[:, 1].sum()) * 32 * 32
    full = -(-rs.n_rows // 32) * 32 * bank.shape[0] * 32
    return 2 * rows * band, 2 * rows * full


def bench_kernel(args):
    from acvae_amd.frontend import LogMel, Resample
    fe = LogMel.panns_32k()
    for orig in (44100, 48000):
        rs = Resample.kaiser_best(orig, 32000)
        Ls = int(args.seconds * orig)
        g = torch.Generator().manual_seed(1)
        f32 = (0.1 * torch.randn(args.B, Ls, generator=g)).cuda()
        i16 = (f32 * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        lens = np.full(args.B, Ls)
        Lo = int(rs.out_len(Ls))
        band, full = flops(rs, lens)
        for kind, w in (("fp32", f32), ("int16", i16)):
            ms = kernel_times(rs, w, lens, args.launches, args.warmup)
            med, b2b = statistics.median(ms), back_to_back(lambda: rs(w, lens), args.launches)
            nbytes = w.numel() * w.element_size() + args.B * Lo * 4
            floor_us = nbytes / (PEAK_TBS * 1e12) * 1e6
            print(f"resample {orig} -> 32000 {kind}: B={args.B} x {args.seconds:g} s -> [{args.B}, {Lo}]: median {med:.3f} ms of "
                  f"{len(ms)} single launches (min {min(ms):.3f}, max {max(ms):.3f}), {b2b:.3f} ms per launch back to back; "
                  f"{band / 1e9:.2f} GFLOP executed ({full / 1e9:.2f} without band skipping) -> {band / b2b / 1e9:.1f} TFLOP/s = "
                  f"{band / b2b / 1e9 / PEAK_TFLOPS:.1%} of the {PEAK_TFLOPS} TFLOP/s fp32 matrix peak; {nbytes / 1e6:.1f} MB moved, "
                  f"floor {floor_us:.1f} us at {PEAK_TBS:g} TB/s = {floor_us / b2b / 1e3:.1%} of the time", flush=True)
    Ls = int(args.seconds * 32000)
    g = torch.Generator().manual_seed(1)
    i16 = (0.1 * torch.randn(args.B, Ls, generator=g) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).cuda()
    lens = np.full(args.B, Ls)
    ms = kernel_times(fe, i16, lens, args.launches, args.warmup)
    print(f"logmel panns_32k int16 (the yardstick, same session): median {statistics.median(ms):.3f} ms of {len(ms)} single "
          f"launches, {back_to_back(lambda: fe(i16, lens), args.launches):.3f} ms per launch back to back", flush=True)


def bench_step(args):
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.frontend import LogMel
    from acvae_amd.trainer import TrainStep
    from acvae_amd.vae_model import Hybrid_VAEModel
    fe = LogMel.panns_32k()
    both = fe.at_input_rate(44100)
    B = args.B
    g = torch.Generator().manual_seed(3)
    pcm32 = (0.1 * torch.randn(B, int(args.seconds * 32000), generator=g) * 32768.0).round().clamp(-32768, 32767)
    pcm44 = (0.1 * torch.randn(B, int(args.seconds * 44100), generator=g) * 32768.0).round().clamp(-32768, 32767)
    pcm32, pcm44 = pcm32.to(torch.int16).pin_memory(), pcm44.to(torch.int16).pin_memory()
    wl32, wl44 = np.full(B, pcm32.shape[1]), np.full(B, pcm44.shape[1])
    assert int(both.n_frames(wl44)[0]) == int(fe.n_frames(wl32)[0])
    caps = torch.randint(4, V, (B, L), generator=g).float()
    caps[:, 0], caps[:, -1] = 1, 2
    cl = np.full(B, L)
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().train()
    ts = TrainStep(model, V)
    variants = (("32 kHz int16 waveforms, frontend=LogMel", lambda: ts.step(pcm32, wl32, caps, cl, 1.0, 0, 0.5, frontend=fe)),
                ("44.1 kHz int16 waveforms, frontend=at_input_rate(44100)",
                 lambda: ts.step(pcm44, wl44, caps, cl, 1.0, 0, 0.5, frontend=both)))
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
            print(f"step, round {rnd}: {name}: {ms:.2f} ms (B={B}, {int(fe.n_frames(wl32)[0])} frames, V={V}, E={E}, fp32; mean "
                  f"of {args.steps} after {args.warmup} warm-up)", flush=True)


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
        raise SystemExit("tools/bench_resample.py needs an MI355X: nothing here can be measured on the host")
    bench_kernel(args)
    if not args.no_step:
        bench_step(args)


if __name__ == "__main__":
    main()
