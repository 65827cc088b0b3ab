"""The finishing beam search beside the plain one, in one process and alternating (never against an older record).

At the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20), method="beam", beam_size 3, through the
2-input forward evaluate() calls: the encoder runs inside every timed call and a window ends in a device synchronise.
  off  the plain call
  on   finish_on_end=True, length_penalty=1.0, nbest=3
A window repeats one variant until a second has passed and reports ms per batch; the variants alternate, window by window.

  python tools/bench_finishing_beam.py [--windows 8] [--json out.json]
  python tools/bench_finishing_beam.py --off-only    only the plain call: runs on a tree without the feature too, which is how
                                                     the parent commit is measured in the same session
  python tools/bench_finishing_beam.py --trace       a few finishing calls and nothing else, to run under a kernel trace
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
ON = dict(finish_on_end=True, length_penalty=1.0, nbest=BEAM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_finishing_beam.py measures on the GPU: none found")
    import bench
    model = bench.build_model().cuda().eval()
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)

    def beam(**kw):
        with torch.no_grad():
            return model(feats, fl.copy(), method="beam", beam_size=BEAM, max_length=MAXLEN, **kw)

    if args.trace:
        for _ in range(5):
            beam(**ON)
        torch.cuda.synchronize()
        return
    variants = [("off", {})] + ([] if args.off_only else [("on", ON)])
    for _, kw in variants:
        for _ in range(5):
            beam(**kw)
    torch.cuda.synchronize()

    def window(kw):
        n = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        while True:
            beam(**kw)
            n += 1
            if n % 8 == 0:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= args.seconds:
                    break
        return (time.perf_counter() - t0) * 1e3 / n

    times = {name: [] for name, _ in variants}
    for _ in range(args.windows):                          # alternating
        for name, kw in variants:
            times[name].append(window(kw))
    record = []
    for name, _ in variants:
        t = sorted(times[name])
        record.append(dict(variant=name, ms=dict(median=statistics.median(t), min=t[0], max=t[-1], windows=times[name])))
        print("%-4s %.3f ms/batch median of %d windows of >= %.1f s (range %.3f - %.3f)" % (
            name, statistics.median(t), len(t), args.seconds, t[0], t[-1]), flush=True)
    if not args.off_only:
        off, on = (statistics.median(times[s]) for s in ("off", "on"))
        print("finishing costs %+.3f ms per batch (%+.2f %%), %+.2f us per decode step" % (
            on - off, (on - off) / off * 100, (on - off) / MAXLEN * 1e3))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape, {B} clips, T={T}, V={V}, E={E}, max_length {MAXLEN}, beam_size {BEAM}; "
                       "encoder inside the timed call", "on": ON, "windows": args.windows, "variants": record}, fh, indent=1)


if __name__ == "__main__":
    main()
