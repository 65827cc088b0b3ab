"""Constrained decoding beside the unconstrained calls, all in one process and alternating (never against an older record).

At the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20):
  sample  method="sample", rng="device", five samples per clip over one encoder pass (rollout_shared_encoder);
  beam    method="beam", beam_size 3 (the 2-input forward);
each with every control off and with all four on (repetition_penalty 1.3, no_repeat_ngram_size 3, min_length 5,
suppress_tokens [0, 1, 3]).  Every timed call runs the encoder too and ends in a device synchronise.  The difference is
printed per decode step.

  python tools/bench_constrained.py [--reps 15] [--json out.json]
  python tools/bench_constrained.py --off-only     only the unconstrained calls: runs on a tree without the feature too,
                                                   which is how the parent commit is measured in the same session
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

B, T, V, E, MAXLEN, SAMPLES, BEAM = 32, 1000, 5000, 512, 20, 5, 3
ON = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_length=5, suppress_tokens=[0, 1, 3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json")
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_constrained.py measures on the GPU: none found")
    import bench
    model = bench.build_model().cuda().eval()
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)

    def sample(**kw):
        with torch.no_grad():
            return model.rollout_shared_encoder(feats, fl.copy(), SAMPLES, method="sample", max_length=MAXLEN, rng="device", **kw)

    def beam(**kw):
        with torch.no_grad():
            return model(feats, fl.copy(), method="beam", beam_size=BEAM, max_length=MAXLEN, **kw)

    def timed(fn, kw):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(**kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = [("sample off", sample, {}), ("beam off", beam, {})]
    if not args.off_only:
        variants += [("sample on", sample, ON), ("beam on", beam, ON)]
    for _, fn, kw in variants:
        for _ in range(3):
            fn(**kw)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(args.reps):                             # alternating
        for name, fn, kw in variants:
            times[name].append(timed(fn, kw))
    record = []
    for name, _, _ in variants:
        t = sorted(times[name])
        q1, q3 = t[len(t) // 4], t[(3 * len(t)) // 4]
        record.append(dict(variant=name, ms=dict(median=statistics.median(t), min=t[0], max=t[-1], q1=q1, q3=q3)))
        print("%-11s %.3f ms/batch median (quartiles %.3f - %.3f, range %.3f - %.3f)" % (
            name, statistics.median(t), q1, q3, t[0], t[-1]), flush=True)
    if not args.off_only:
        for what in ("sample", "beam"):
            off, on = (statistics.median(times[f"{what} {s}"]) for s in ("off", "on"))
            print("%s: all four controls cost %+.3f ms per batch (%+.1f %%), %+.1f us per decode step" % (
                what, on - off, (on - off) / off * 100, (on - off) / MAXLEN * 1e3))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape, {B} clips, T={T}, V={V}, E={E}, max_length {MAXLEN}; sample: {SAMPLES} "
                       f"samples per clip, rng=device; beam: beam_size {BEAM}; encoder inside the timed call",
                       "controls": ON, "reps": args.reps, "variants": record}, fh, indent=1)


if __name__ == "__main__":
    main()
