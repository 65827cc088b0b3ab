"""Diversity statistics through evaluate() beside the same call without them and beside the host route, in one process.

The sampled decode at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20), five samples per clip
over one encoder pass, method="sample", rng="device", one batch of 32 clips through acvae_amd.evaluate.evaluate; every timed
call runs the encoder, downloads the rows and builds the payload as evaluate does; plain and diversity alternate, the host
route is timed in a phase of its own behind them:
  plain      evaluate(...) without the keyword
  diversity  evaluate(..., diversity=d), d.reset() in front of every call; and d.result() timed on its own
  host       the plain call, then the payload's token strings scored by the dictionary scorer of tests/diversity_util.py
             (the route a user had before, without the reference's tokenizer)
Then the kernel alone on synthetic caption-like rows for N = 5 and N = 16, 32 clips, back to back between one pair of HIP
events.

  python tools/bench_diversity.py [--reps 15] [--launches 200] [--json out.json]
  python tools/bench_diversity.py --plain-only     the plain variant alone (also runs on a tree without the feature)
  python tools/bench_diversity.py --trace          the kernel alone, a few launches per N, for
      rocprofv3 --kernel-trace -d DIR -o diversity -- python tools/bench_diversity.py --trace
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
START, END = 1, 2


class Vocabulary:
    def __init__(self, words):
        self.idx2word = {i: w for i, w in enumerate(words)}


def synthetic_rows(n, seed):
    """Caption-like token rows [n, MAXLEN]: 6..19 Zipf-distributed words, then <end>."""
    import numpy as np
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 60)
    p /= p.sum()
    rows = np.full((n, MAXLEN), END, dtype=np.int64)
    for r in rows:
        k = rng.integers(6, MAXLEN)
        r[:k] = 4 + rng.choice(len(p), k, p=p)
    return rows


def stats(t):
    q = statistics.quantiles(t, n=4)
    return dict(median=statistics.median(t), q1=q[0], q3=q[2], min=min(t), max=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_diversity.py measures on the GPU: none found")
    words = ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]
    vocab = Vocabulary(words)
    record = {"evaluate": [], "kernel": []}
    div = None
    if not args.plain_only:
        from acvae_amd.diversity import Diversity
        div = Diversity(vocab)

    def kernel_alone(n):
        rows = torch.as_tensor(synthetic_rows(B * n, n)).cuda()
        for _ in range(5):
            div.stats(rows, n)
        torch.cuda.synchronize()
        if args.trace:
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            div.stats(rows, n)
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / args.launches * 1e3
        record["kernel"].append(dict(clips=B, sample_n=n, b2b_us=us))
        print("kernel synthetic %d clips x %2d: %.2f us per call, back to back (with the host's two allocations and the "
              "clearing of `seen`)" % (B, n, us), flush=True)

    if args.trace:
        for n in (5, 16):
            kernel_alone(n)
        return

    import bench
    from acvae_amd import evaluate as EV
    model = bench.build_model().cuda().eval()
    g = torch.Generator().manual_seed(1)
    items = [(f"clip{i}", torch.randn(T, 64, generator=g)) for i in range(B)]
    kw = dict(method="sample", rng="device", beam_size=SAMPLES, max_length=MAXLEN, batch_size=B)

    def plain():
        out = EV.evaluate(model, items, vocab, **kw)
        torch.cuda.synchronize()
        return out

    def diversity():
        div.reset()
        out = EV.evaluate(model, items, vocab, diversity=div, **kw)
        torch.cuda.synchronize()
        return out

    def host():
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import diversity_util
        payload = plain()
        return diversity_util.diversity(diversity_util.clips_of_payload(payload))

    variants = [("plain", plain)] + ([] if args.plain_only else [("diversity", diversity), ("host", host)])
    times = {name: [] for name, _ in variants}
    for phase in ([v for v in variants if v[0] != "host"], [v for v in variants if v[0] == "host"]):
        for _, fn in phase:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):                         # alternating within a phase
            for name, fn in phase:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in variants:
        s = stats(times[name])
        record["evaluate"].append(dict(variant=name, ms=s))
        print("evaluate %-9s %d clips x %d samples: %.3f ms/batch  quartiles %.3f - %.3f  min - max %.3f - %.3f" % (
            name, B, SAMPLES, s["median"], s["q1"], s["q3"], s["min"], s["max"]), flush=True)
    if not args.plain_only:
        med = {name: statistics.median(times[name]) for name, _ in variants}
        print("diversity= costs %+.3f ms per batch (%+.1f %%) on the device, the host route %+.3f ms (%+.1f %%)" % (
            med["diversity"] - med["plain"], (med["diversity"] - med["plain"]) / med["plain"] * 100,
            med["host"] - med["plain"], (med["host"] - med["plain"]) / med["plain"] * 100))
        t = []
        for _ in range(args.reps):
            diversity()
            t0 = time.perf_counter()
            res = div.result()
            t.append((time.perf_counter() - t0) * 1e3)
        record["result_ms"] = stats(t)
        want = host()
        record["numbers"] = {k: res[k] for k in ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_4")}
        print("result(): %.3f ms (median of %d); Div1 %.4f Div2 %.4f gDiv1 %d mBLeu_1 %.4f mBLeu_4 %.4f (random weights)" % (
            statistics.median(t), args.reps, res["Div1"], res["Div2"], res["gDiv1"], res["mBLeu_1"], res["mBLeu_4"]))
        print("the host route's numbers for its own rollouts: Div1 %.4f Div2 %.4f mBLeu_4 %.4f" % (
            want["Div1"], want["Div2"], want["mBLeu_4"]))
        for n in (5, 16):
            kernel_alone(n)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape, {B} clips x {SAMPLES} samples, T={T}, V={V}, E={E}, max_length {MAXLEN}, "
                       "method=sample, rng=device, through evaluate()", "reps": args.reps, "launches": args.launches,
                       **record}, fh, indent=1)


if __name__ == "__main__":
    main()
