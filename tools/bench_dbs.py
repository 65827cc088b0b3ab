"""The `dbs beam_size=5 batch=32` line of tools/bench_infer.py (BASELINE configs[4] twin) alone, repeated: captions/s of
evaluate(method="dbs", beam_size=5, group_size=5, max_length=20) over 64 clips of 1000 frames, end to end.

  --impl device | host | default   the one-call search, the host loop (dbs_impl="host"), or no keyword at all (a tree from
                                   before the keyword existed: run this file from that tree)
  --members M                      M > 1: ensemble_evaluate over M models (device route only)
  --reps R                         timed repetitions behind one warm-up; median, min and max are printed

One JSON line at the end.  A/B: run the two trees (or the two routes) in alternating processes of one session and compare
the medians against the spread between two runs of the same tree."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_KERNARG_POOL_SIZE", str(32 << 20))
import torch  # noqa: E402

import bench  # noqa: E402
from acvae_amd import evaluate as EV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--impl", default="device", choices=("device", "host", "default"))
ap.add_argument("--members", type=int, default=1)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tag", default="")
args = ap.parse_args()

T = 1000
models = []
for m in range(args.members):
    torch.manual_seed(100 + m)
    models.append(bench.build_model().cuda().eval())
voc = EV.Vocabulary()
for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(bench.V - 4)]:
    voc.add_word(w)
g = torch.Generator().manual_seed(1)
items = [(f"clip{i}", torch.randn(T, 64, generator=g)) for i in range(64)]
kw = dict(method="dbs", beam_size=5, group_size=5, max_length=20, batch_size=args.batch)
if args.impl != "default":
    kw["dbs_impl"] = args.impl


def run(n_items):
    if args.members > 1:
        from acvae_amd.ensemble import ensemble_evaluate
        if args.impl == "host":
            raise SystemExit("--members > 1 has no host route")
        return ensemble_evaluate(models, n_items, voc, **{k: v for k, v in kw.items() if k != "dbs_impl"})
    return EV.evaluate(models[0], n_items, voc, **kw)


run(items[:args.batch])                                  # warm-up
rates = []
for _ in range(args.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(items)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    caps = sum(len(p.get("captions", [0])) for p in out["predictions"])
    rates.append(caps / dt)
print(json.dumps({"tag": args.tag, "impl": args.impl, "members": args.members, "batch": args.batch, "clips": len(items),
                  "captions": caps, "reps": args.reps, "captions_per_s_median": round(statistics.median(rates), 1),
                  "captions_per_s_min": round(min(rates), 1), "captions_per_s_max": round(max(rates), 1)}), flush=True)
