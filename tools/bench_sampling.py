"""Top-k / nucleus sampling beside the untruncated path, both in the same process (never against an older record).

(i)  The stand-alone kernel, acvae_sample_next_word_truncated, on 32 x 5000 and 160 x 5000 rows of 3 randn logits with
     device-generated Exp(1) noise (method "sample", temp 1): top_k = 40, top_p = 0.9, both - and "off", which is the
     untruncated kernel (acvae_sample_next_word).  "b2b": the mean of --launches launches between one pair of HIP events;
     "single": launches timed one by one, each between its own pair of events (median, min - max): a lone launch pays
     the launch itself.
(ii) The sampled decode at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20), five samples per
     clip over one encoder pass (rollout_shared_encoder), method="sample", rng="device", with and without top_p = 0.9,
     alternating; every timed call runs the encoder too and ends in a device synchronise.

  python tools/bench_sampling.py [--reps 9] [--launches 50] [--json out.json]
  python tools/bench_sampling.py --trace        a short run of both for rocprofv3 --kernel-trace --stats:
      rocprofv3 --kernel-trace --stats -d DIR -o sampling -- python tools/bench_sampling.py --trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_KERNARG_POOL_SIZE", str(32 << 20))

B, T, V, E, MAXLEN, SAMPLES = 32, 1000, 5000, 512, 20, 5
SETTINGS = (("off", 0, 1.0), ("top_k=40", 40, 1.0), ("top_p=0.9", 0, 0.9), ("top_k=40 top_p=0.9", 40, 0.9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--json")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from acvae_amd import _lib
    if os.environ.get("ACVAE_DEV_LIB"):      # this TOOL's hook: time another build of the library (tools/ab_build.py)
        _lib.use_library(os.environ["ACVAE_DEV_LIB"])
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling.py measures on the GPU: none found")
    st = _lib.current_stream
    record = {"kernel": [], "decode": []}

    # ---- (i) the kernel alone
    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for rows in (B, B * SAMPLES):
        x = torch.randn(rows, V, generator=torch.Generator().manual_seed(rows)).cuda() * 3
        z = torch.empty(rows, V, device="cuda")
        _lib.call("acvae_sample_noise", z, z.numel(), 2, 1234, st())
        w = torch.empty(rows, dtype=torch.long, device="cuda")
        lp = torch.empty(rows, device="cuda")
        kept = torch.empty(rows, dtype=torch.int32, device="cuda")
        for name, k, p in SETTINGS:
            if name == "off":
                def launch():
                    _lib.call("acvae_sample_next_word", x, V, 0, z, V, 0, 2, 1.0, w, lp, 1, 0, rows, 1, V, st())
            else:
                def launch(k=k, p=p):
                    _lib.call("acvae_sample_next_word_truncated", x, V, 0, z, V, 0, 2, 1.0, w, lp, 1, 0, rows, 1, V, k, p,
                              kept, st())
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            if args.trace:
                continue
            e0, e1 = pair()
            e0.record()
            for _ in range(args.launches):
                launch()
            e1.record(); torch.cuda.synchronize()
            b2b = e0.elapsed_time(e1) / args.launches * 1e3
            single = []
            for _ in range(args.launches):
                e0, e1 = pair()
                e0.record(); launch(); e1.record(); torch.cuda.synchronize()
                single.append(e0.elapsed_time(e1) * 1e3)
            rec = dict(rows=rows, V=V, setting=name, b2b_us=b2b,
                       single_us=dict(median=statistics.median(single), min=min(single), max=max(single)),
                       kept_mean=None if name == "off" else float(kept.float().mean()))
            record["kernel"].append(rec)
            print("kernel %3d x %d  %-20s b2b %7.2f us   single %7.2f us (%.2f - %.2f)%s" % (
                rows, V, name, b2b, rec["single_us"]["median"], min(single), max(single),
                "" if name == "off" else "   mean kept %.1f" % rec["kept_mean"]), flush=True)

    # ---- (ii) the sampled decode, five samples per clip
    import bench
    model = bench.build_model().cuda().eval()
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)

    def run(**kw):
        with torch.no_grad():
            return model.rollout_shared_encoder(feats, fl.copy(), SAMPLES, method="sample", max_length=MAXLEN, rng="device", **kw)

    def timed(**kw):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run(**kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = (("untruncated", {}), ("top_p=0.9", dict(top_p=0.9)))
    for _, kw in variants:
        for _ in range(3):
            run(**kw)
    torch.cuda.synchronize()
    if args.trace:
        return
    times = {name: [] for name, _ in variants}
    for _ in range(args.reps):                             # alternating
        for name, kw in variants:
            times[name].append(timed(**kw))
    for name, _ in variants:
        t = times[name]
        rec = dict(variant=name, rows=B * SAMPLES, ms=dict(median=statistics.median(t), min=min(t), max=max(t)),
                   captions_per_s=B * SAMPLES / statistics.median(t) * 1e3)
        record["decode"].append(rec)
        print("decode %-12s %d clips x %d samples: %.2f ms/batch (%.2f - %.2f) = %.0f captions/s" % (
            name, B, SAMPLES, rec["ms"]["median"], min(t), max(t), rec["captions_per_s"]), flush=True)
    base, trunc = (statistics.median(times[n]) for n, _ in variants)
    print("top_p=0.9 costs %+.2f ms per batch (%+.1f %% of the untruncated call, %.1f us per decode step)" % (
        trunc - base, (trunc - base) / base * 100, (trunc - base) / MAXLEN * 1e3))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"kernel: rows x {V}, method sample, temp 1; decode: configs[4] shape, {B} clips x {SAMPLES} "
                       f"samples, T={T}, V={V}, E={E}, max_length {MAXLEN}, rng=device, encoder inside the timed call",
                       "reps": args.reps, "launches": args.launches, **record}, fh, indent=1)


if __name__ == "__main__":
    main()
