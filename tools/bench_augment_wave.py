"""Time the augmentation of batches formed from waveforms (acvae_amd.augment.apply_plans -> acvae_augment_window,
acvae_amd.frontend.Augmented) on one MI355X.  Not product, not the project's benchmark; it writes down numbers that had
not been measured, to stdout and to --out (default profiles/r11_wave_augment.txt).

    python tools/bench_augment_wave.py [--B 32 --launches 50 --rounds 7 --warmup 5] [--no-step] [--steps 20] [--out FILE]

(a) acvae_augment_window with no windows against acvae_spec_augment on the same tables (a roll, 2 time and 2 frequency
    masks per clip, as parse_augments' defaults draw them with p = 1) at B x 1000 x 64: the two entries share one body.
    `--rounds` alternating rounds of `--launches` launches between one pair of HIP events (back to back), the table already
    on the device; per entry the median of the rounds and their min - max, which is the session's run-to-run spread.
(b) the same with one crop firing, [B, 3000, 64] -> [B, 1000, 64], beside acvae_spec_augment on the already cropped batch.
(c) TrainStep.step at BASELINE configs[1] (as tools/bench_frontend.py) from int16 waveforms in page-locked host memory,
    uploaded inside the timed loop: frontend=LogMel.panns_32k(), and the same front end
    .augmented(parse_augments(["randomcrop", "timeroll", "timemask", "freqmask"])).  Two alternating rounds; the spread
    between them is the noise.  Beside it the host time of one batch's draws (draw_shape x B) and of window_table."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_frontend import E, L, V     # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def back_to_back(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches * 1e3          # us


def rounds(variants, args):
    """{name: [us per launch, one figure per round]}, the variants alternating inside every round."""
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    out = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            out[name].append(back_to_back(fn, args.launches))
    return out


def report(what, times, nbytes):
    for name, us in times.items():
        med = statistics.median(us)
        say(f"{what}: {name}: median {med:.1f} us per launch over {len(us)} rounds (min {min(us):.1f}, max {max(us):.1f}; "
            f"spread {max(us) - min(us):.1f} us); {nbytes[name] / 1e6:.1f} MB read once + written once -> "
            f"{nbytes[name] / med / 1e6:.2f} TB/s")


def bench_kernel(args):
    from acvae_amd import _lib
    from acvae_amd import augment as A
    B, F, To = args.B, 64, 1000
    aug = A.parse_augments(["timeroll", "timemask", "freqmask"], p=1.0)
    st = _lib.current_stream()
    g = torch.Generator().manual_seed(1)

    def device_tables(plans, src_lens, T):
        tab, out_lens = A.window_table(plans, src_lens, T, F)
        up = torch.from_numpy(np.concatenate([np.asarray(src_lens, np.int32), tab.reshape(-1)])).cuda()
        old = A.table([p.params for p in plans], out_lens, int(out_lens.max()), F)
        upo = torch.from_numpy(np.concatenate([out_lens.astype(np.int32), old.reshape(-1)])).cuda()
        return up, upo

    # (a) no windows
    random.seed(1); np.random.seed(1)
    lens = np.full(B, To)
    plans = [aug.draw_shape(To, F) for _ in range(B)]
    x = torch.randn(B, To, F, generator=g).cuda()
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    up, upo = device_tables(plans, lens, To)
    old = lambda: _lib.call("acvae_spec_augment", x, y1, upo, upo[B:], B, To, F, A.TABLE_WIDTH, st)                # noqa: E731
    new = lambda: _lib.call("acvae_augment_window", x, y2, up, up[B:], B, To, To, F, A.WINDOW_TABLE_WIDTH, st)      # noqa: E731
    times = rounds((("acvae_spec_augment", old), ("acvae_augment_window, no windows", new)), args)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), "the two entries differ"
    nb = 2 * x.numel() * 4
    report(f"(a) [{B}, {To}, {F}], roll + 2 + 2 masks", times, {k: nb for k in times})
    a, b = (statistics.median(times[k]) for k in times)
    say(f"(a) difference of the medians: {b - a:+.1f} us ({(b - a) / a:+.1%}); outputs bit-equal")

    # (b) one crop firing, 3000 -> 1000 frames
    T = 3000
    random.seed(2); np.random.seed(2)
    crop = A.parse_augments(["timeroll", "randomcrop", "timeroll", "timemask", "freqmask"], p=1.0)
    crop.ops = [op if op[0] != "crop" else A.Augment.crop(To, 1.0) for op in crop.ops]
    plans = [crop.draw_shape(T, F) for _ in range(B)]
    assert all(len(p.windows) == 1 for p in plans)
    xs = torch.randn(B, T, F, generator=g).cuda()
    up, upo = device_tables(plans, np.full(B, T), T)
    rows = torch.from_numpy(np.stack([np.roll(p.source_rows(), -p.params.shift) for p in plans])).cuda()
    xc = torch.gather(xs, 1, rows[:, :, None].expand(B, To, F)).contiguous()       # the host crop, for the yardstick
    old = lambda: _lib.call("acvae_spec_augment", xc, y1, upo, upo[B:], B, To, F, A.TABLE_WIDTH, st)                # noqa: E731
    new = lambda: _lib.call("acvae_augment_window", xs, y2, up, up[B:], B, T, To, F, A.WINDOW_TABLE_WIDTH, st)      # noqa: E731
    times = rounds((("acvae_spec_augment on the cropped batch", old), (f"acvae_augment_window, crop {T} -> {To}", new)), args)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), "the two entries differ"
    report(f"(b) [{B}, {T}, {F}] -> [{B}, {To}, {F}]", times, {k: nb for k in times})
    a, b = (statistics.median(times[k]) for k in times)
    say(f"(b) difference of the medians: {b - a:+.1f} us ({(b - a) / a:+.1%}); outputs bit-equal")


def bench_step(args):
    from acvae_amd import augment as A
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.frontend import LogMel
    from acvae_amd.trainer import TrainStep
    from acvae_amd.vae_model import Hybrid_VAEModel
    fe = LogMel.panns_32k()
    aug = A.parse_augments(["randomcrop", "timeroll", "timemask", "freqmask"])
    afe = fe.augmented(aug)
    B = args.B
    g = torch.Generator().manual_seed(3)
    pcm = (0.1 * torch.randn(B, 10 * 32000, generator=g) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
    wl = np.full(B, pcm.shape[1])
    frames = int(fe.n_frames(wl)[0])

    random.seed(7); np.random.seed(7)
    t0 = time.perf_counter()
    for _ in range(200):
        plans = [aug.draw_shape(frames, 64) for _ in range(B)]
    t_draw = (time.perf_counter() - t0) / 200 * 1e6
    t0 = time.perf_counter()
    for _ in range(200):
        A.window_table(plans, np.full(B, frames), frames, 64)
    t_tab = (time.perf_counter() - t0) / 200 * 1e6
    say(f"(c) host: draw_shape x {B} clips of {frames} frames: {t_draw:.0f} us per batch; window_table: {t_tab:.0f} us per batch "
        f"(mean of 200)")

    caps = torch.randint(4, V, (B, L), generator=g).float()
    caps[:, 0], caps[:, -1] = 1, 2
    cl = np.full(B, L)
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().train()
    ts = TrainStep(model, V)
    variants = (("frontend=LogMel.panns_32k()", lambda: ts.step(pcm, wl, caps, cl, 1.0, 0, 0.5, frontend=fe)),
                ("frontend=fe.augmented(randomcrop, timeroll, timemask, freqmask)",
                 lambda: ts.step(pcm, wl, caps, cl, 1.0, 0, 0.5, frontend=afe)))
    got = {name: [] for name, _ in variants}
    random.seed(9); np.random.seed(9)
    for rnd in range(2):                            # twice, alternating: the spread between the rounds is the noise
        for name, step in variants:
            for _ in range(args.warmup):
                step()
            ts.synchronize()
            t0 = time.perf_counter()
            crops = 0
            for _ in range(args.steps):
                step()
                crops += sum(len(p.windows) for p in afe.last_plans) if "augmented" in name else 0
            ts.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            got[name].append(ms)
            say(f"(c) step, round {rnd}: {name}: {ms:.2f} ms (B={B}, {frames} frames, V={V}, E={E}, fp32, int16 waveforms uploaded "
                f"inside the step; mean of {args.steps} after {args.warmup} warm-up"
                + (f"; {crops} crops fired in {args.steps * B} clips)" if "augmented" in name else ")"))
    a, b = (statistics.mean(v) for v in got.values())
    say(f"(c) difference of the means: {b - a:+.2f} ms ({(b - a) / a:+.1%})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_wave_augment.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_augment_wave.py needs an MI355X: nothing here can be measured on the host")
    bench_kernel(args)
    if not args.no_step:
        bench_step(args)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
