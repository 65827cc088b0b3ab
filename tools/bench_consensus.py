"""Consensus reranking beside the same call without it and beside the host route, all in one process.

The sampled decode at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20), five samples per clip
over one encoder pass (rollout_shared_encoder), method="sample", rng="device"; every timed call runs the encoder too and
ends in a device synchronise; plain and rerank alternate, the host route is timed in a phase of its own behind them (its
host work between two calls would leave the device idle and slow whichever call came next):
  plain    the call as it is without the keyword
  rerank   rerank=Consensus(vocabulary, corpus): one more launch, nothing comes back
  host     the plain call, then the words downloaded, turned into strings and scored by the dictionary scorer of
           tests/consensus_util.py (the route a user had before), argmax on the host
The idf table comes from a synthetic corpus (--keys clips of five captions over the vocabulary).  Then the kernel alone on
the decode's own rows (N = 5) and on synthetic caption-like rows for N = 5 and N = 16, back to back between one pair of
HIP events.

  python tools/bench_consensus.py [--reps 15] [--launches 200] [--json out.json]
  python tools/bench_consensus.py --plain-only     the plain variant alone (also runs on a tree without the feature)
  python tools/bench_consensus.py --trace          the kernel alone, a few launches per N, for
      rocprofv3 --kernel-trace -d DIR -o consensus -- python tools/bench_consensus.py --trace
      (N = 5 launches have 320-thread workgroups, N = 16 launches 1024-thread ones)
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


def synthetic_corpus(words, n_keys, seed):
    """n_keys clips of five captions of 6..16 words, the words Zipf-distributed over the vocabulary."""
    import numpy as np
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(words) - 3)
    p /= p.sum()
    return {f"clip{k}": [" ".join(words[4 + int(i)] for i in rng.choice(len(p), rng.integers(6, 17), p=p)) for _ in range(5)]
            for k in range(n_keys)}


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
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--json")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_consensus.py measures on the GPU: none found")
    words = ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]
    vocab = Vocabulary(words)
    record = {"decode": [], "kernel": []}
    rr = None
    if not args.plain_only:
        from acvae_amd.consensus import Consensus
        t0 = time.perf_counter()
        corpus = synthetic_corpus(words, args.keys, 3)
        rr = Consensus(vocab, corpus)
        record["table"] = dict(keys=args.keys, entries=int(rr.idf_keys.size), build_s=time.perf_counter() - t0)
        print("idf table: %d corpus keys, %d entries, built in %.2f s" % (args.keys, rr.idf_keys.size, record["table"]["build_s"]),
              flush=True)

    def kernel_alone(tag, rows, n):
        rows = torch.as_tensor(rows).cuda()
        for _ in range(5):
            rr.select(rows, n, START, END)
        torch.cuda.synchronize()
        if args.trace:
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            rr.select(rows, n, START, END)
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / args.launches * 1e3
        record["kernel"].append(dict(rows=tag, clips=rows.shape[0] // n, sample_n=n, b2b_us=us))
        print("kernel %-22s %d clips x %2d: %.2f us per call, back to back (with the host's three allocations)" % (
            tag, rows.shape[0] // n, n, us), flush=True)

    if args.trace:
        for n in (5, 16):
            kernel_alone("synthetic", synthetic_rows(B * n, n), n)
        return

    import bench
    model = bench.build_model().cuda().eval()
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)

    def run(**kw):
        with torch.no_grad():
            return model.rollout_shared_encoder(feats, fl.copy(), SAMPLES, method="sample", max_length=MAXLEN, rng="device", **kw)

    def plain():
        run()
        torch.cuda.synchronize()

    def rerank():
        run(rerank=rr)
        torch.cuda.synchronize()

    def host_pick(seqs):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import cider_util
        import consensus_util
        if "idf" not in host_pick.__dict__:
            host_pick.idf, host_pick.log_d = consensus_util.corpus_idf(corpus)
        scores = consensus_util.clip_scores(seqs, SAMPLES, vocab, cider_util.sentence_of, host_pick.idf, host_pick.log_d)
        return scores.argmax(axis=1)

    def host():
        seqs = run()["seqs"].cpu().numpy()
        return seqs[np.arange(B) * SAMPLES + host_pick(seqs)]

    variants = [("plain", plain)] + ([] if args.plain_only else [("rerank", rerank), ("host", host)])
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
        record["decode"].append(dict(variant=name, ms=s, captions_per_s=B * SAMPLES / s["median"] * 1e3))
        print("decode %-7s %d clips x %d samples: %.3f ms/batch  quartiles %.3f - %.3f  min - max %.3f - %.3f" % (
            name, B, SAMPLES, s["median"], s["q1"], s["q3"], s["min"], s["max"]), flush=True)
    if not args.plain_only:
        med = {name: statistics.median(times[name]) for name, _ in variants}
        print("rerank costs %+.3f ms per batch (%+.1f %%) on the device, %+.3f ms (%+.1f %%) by the host route" % (
            med["rerank"] - med["plain"], (med["rerank"] - med["plain"]) / med["plain"] * 100,
            med["host"] - med["plain"], (med["host"] - med["plain"]) / med["plain"] * 100))
        out = run(rerank=rr)
        torch.cuda.synchronize()
        agree = int((host_pick(out["candidates"].cpu().numpy()) == out["consensus_best"].cpu().numpy()).sum())
        record["agree"] = agree
        print("the device and the host route pick the same rollout for %d of %d clips" % (agree, B))
        kernel_alone("decode's own rollouts", out["candidates"], SAMPLES)
        for n in (5, 16):
            kernel_alone("synthetic", synthetic_rows(B * n, n), n)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape, {B} clips x {SAMPLES} samples, T={T}, V={V}, E={E}, max_length {MAXLEN}, "
                       "method=sample, rng=device, encoder inside the timed call", "reps": args.reps, "launches": args.launches,
                       **record}, fh, indent=1)


if __name__ == "__main__":
    main()
