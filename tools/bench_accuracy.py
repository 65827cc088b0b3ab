"""Accuracy scoring (BLEU, ROUGE-L, CIDEr on the device) through evaluate() beside the same call without it, and result()
beside the host route, in one process.

The beam-3 validation decode at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20), method="beam",
beam_size=3, one batch of 32 clips through acvae_amd.evaluate.evaluate; every timed call runs the encoder, downloads the rows
and builds the payload as evaluate does; plain and accuracy alternate:
  plain      evaluate(...) without the keyword
  accuracy   evaluate(..., accuracy=a), a.reset() in front of every call (update only: no launch)
Then an evaluation set of 1000 clips with five references each, synthetic caption-like rows and references:
  result     a.update(keys, rows) + a.result(): the reference tables, one upload, acvae_accuracy_stats, acvae_ciderd_scores,
             one download, the formulas
  host       the same rows as token strings through the dictionary scorers of tests/accuracy_util.py (the route a user had
             before, without the reference's tokenizer)
and the kernel alone on those rows, back to back between one pair of HIP events.

  python tools/bench_accuracy.py [--reps 15] [--launches 200] [--json out.json]
  python tools/bench_accuracy.py --plain-only     the plain variant alone (also runs on a tree without the feature)
  python tools/bench_accuracy.py --trace          the kernel alone, a few launches, for
      rocprofv3 --kernel-trace --stats -d DIR -o accuracy -- python tools/bench_accuracy.py --trace
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

B, T, V, E, MAXLEN, BEAM = 32, 1000, 5000, 512, 20, 3
CLIPS, REFS = 1000, 5
START, END = 1, 2


class Vocabulary:
    def __init__(self, words):
        self.idx2word = {i: w for i, w in enumerate(words)}


def synthetic_set(clips, refs, seed, words):
    """Caption-like token rows [clips, MAXLEN] (6..19 Zipf-distributed words, then <end>) and per clip `refs` reference
    strings: the row's words with a fifth of them redrawn, a few dropped, and now and then a word the vocabulary lacks."""
    import numpy as np
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 60)
    p /= p.sum()
    rows = np.full((clips, MAXLEN), END, dtype=np.int64)
    key2refs = {}
    for b, r in enumerate(rows):
        k = rng.integers(6, MAXLEN)
        r[:k] = 4 + rng.choice(len(p), k, p=p)
        mine = []
        for _ in range(refs):
            ids = [int(w) if rng.random() >= 0.2 else 4 + int(rng.choice(len(p), p=p)) for w in r[:k] if rng.random() >= 0.1]
            ids = ids or [4]
            mine.append(" ".join("okapi" if rng.random() < 0.02 else words[w] for w in ids))
        key2refs[f"clip{b}"] = mine
    return rows, key2refs


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
        raise SystemExit("bench_accuracy.py measures on the GPU: none found")
    words = ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]
    vocab = Vocabulary(words)
    record = {"evaluate": []}

    if not args.plain_only:
        from acvae_amd import _lib
        from acvae_amd.accuracy import RECORD, Accuracy
        rows, key2refs = synthetic_set(CLIPS, REFS, 7, words)
        keys = list(key2refs)
        big = Accuracy(vocab, key2refs)
        dev_rows = torch.as_tensor(rows).cuda()

        def kernel_alone():
            tabs = big.reference_tables(keys)
            d = [torch.from_numpy(t).cuda() for t in tabs]
            rec = torch.empty(CLIPS, RECORD, dtype=torch.int32, device="cuda")

            def launch():
                _lib.call("acvae_accuracy_stats", dev_rows, MAXLEN, CLIPS, 1, MAXLEN, START, END, V, d[0], tabs[0].size, d[1],
                          tabs[1].size - 1, d[2], CLIPS, rec, _lib.current_stream())
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            if args.trace:
                return
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                launch()
            e1.record(); torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / args.launches * 1e3
            record["kernel"] = dict(rows=CLIPS, references=CLIPS * REFS, reference_words=int(tabs[0].size), b2b_us=us)
            print("kernel %d rows x %d references (%d reference words): %.2f us per launch, back to back" % (
                CLIPS, REFS, tabs[0].size, us), flush=True)

        if args.trace:
            kernel_alone()
            return

    import bench
    from acvae_amd import evaluate as EV
    model = bench.build_model().cuda().eval()
    g = torch.Generator().manual_seed(1)
    items = [(f"clip{i}", torch.randn(T, 64, generator=g)) for i in range(B)]
    kw = dict(method="beam", beam_size=BEAM, max_length=MAXLEN, batch_size=B)
    small = None if args.plain_only else Accuracy(vocab, {k: key2refs[k] for k in keys[:B]})

    def plain():
        out = EV.evaluate(model, items, vocab, **kw)
        torch.cuda.synchronize()
        return out

    def accuracy():
        small.reset()
        out = EV.evaluate(model, items, vocab, accuracy=small, **kw)
        torch.cuda.synchronize()
        return out

    variants = [("plain", plain)] + ([] if args.plain_only else [("accuracy", accuracy)])
    times = {name: [] for name, _ in variants}
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                             # alternating
        for name, fn in variants:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in variants:
        s = stats(times[name])
        record["evaluate"].append(dict(variant=name, ms=s))
        print("evaluate %-9s %d clips, beam %d: %.3f ms/batch  quartiles %.3f - %.3f  min - max %.3f - %.3f" % (
            name, B, BEAM, s["median"], s["q1"], s["q3"], s["min"], s["max"]), flush=True)
    if not args.plain_only:
        med = {name: statistics.median(times[name]) for name, _ in variants}
        print("accuracy= costs %+.3f ms per batch (%+.1f %%)" % (
            med["accuracy"] - med["plain"], (med["accuracy"] - med["plain"]) / med["plain"] * 100))
        t0 = time.perf_counter()
        res = small.result()
        print("result() of that batch (%d clips x %d captions), first call: %.3f ms; Bleu_1 %.4f ROUGE_L %.4f CIDEr %.4f "
              "(random weights against synthetic references)" % (B, BEAM, (time.perf_counter() - t0) * 1e3, res["Bleu_1"],
                                                                  res["ROUGE_L"], res["CIDEr"]))

        def result():
            big.reset()
            big.update(keys, dev_rows)
            return big.result()

        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import accuracy_util
        strings = [[" ".join(words[int(w)] for w in r[:list(r).index(END)])] for r in rows]

        def host():
            return accuracy_util.accuracy(strings, keys, key2refs)

        for name, fn, reps in (("result", result, args.reps), ("host", host, 3)):
            fn()
            t = []
            for _ in range(reps):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = fn()
                t.append((time.perf_counter() - t0) * 1e3)
            record[name + "_ms"] = stats(t) if reps > 3 else dict(median=statistics.median(t), min=min(t), max=max(t))
            record[name + "_numbers"] = {k: out[k] for k in ("Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr")}
            print("%-6s %d clips x %d references: %.3f ms (median of %d, min - max %.3f - %.3f); Bleu_1 %.6f Bleu_4 %.6f "
                  "ROUGE_L %.6f CIDEr %.6f" % (name, CLIPS, REFS, statistics.median(t), reps, min(t), max(t), out["Bleu_1"],
                                               out["Bleu_4"], out["ROUGE_L"], out["CIDEr"]), flush=True)
        print("of result(): CiderD.prepare on the host %.3f ms (the last call)" % (big._cider.last_prepare_s * 1e3))
        kernel_alone()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape, {B} clips, T={T}, V={V}, E={E}, max_length {MAXLEN}, method=beam, "
                       f"beam_size={BEAM}, through evaluate(); result(): {CLIPS} clips x {REFS} references",
                       "reps": args.reps, "launches": args.launches, **record}, fh, indent=1)


if __name__ == "__main__":
    main()
