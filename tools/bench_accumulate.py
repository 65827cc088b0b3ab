#!/usr/bin/env python3
"""Measurements behind profiles/r21_accumulation.txt: gradient accumulation and the weight EMA of TrainStep
(accum_steps=, ema_decay=), all at bench.py's shape (32 clips of 1000 frames, 22-token captions, V = 5000, E = 512).

    python tools/bench_accumulate.py --ab PARENT [--out DIR] [--runs N] [--steps K] [--warmup W]
        `python bench.py --gpus 1 --steps K --warmup W` in this tree and in PARENT (a checkout of the parent commit, built),
        alternating, N runs each, every run a process of its own                                        -> DIR/r21_ab.txt
    python tools/bench_accumulate.py [--out DIR] [--calls N] [--reverse]
        time per call of TrainStep.step, device-synchronised around every call, for the plain step, the non-final and the
        final micro-step at accum_steps=4, and the same with ema_decay; one TrainStep and one model each, alternating
                                                                                                        -> DIR/r21_steps.txt
    rocprofv3 --kernel-trace --stats -d TRACE -o t --output-format csv -- python tools/bench_accumulate.py --kernels [--out DIR]
        windows of accum_steps=4 with ema_decay under Adam (adam_kernel) and AdamW (opt_kernel)   -> DIR/r21_kernel_meta.json
    python tools/bench_accumulate.py --kernel-report TRACE [--out DIR]
        reads the trace and the meta file (no GPU)                                                      -> DIR/r21_kernels.txt
"""
import argparse
import csv
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0            # HBM3E peak of the MI355X (spec); about 6300 GB/s is what a float4 copy reaches


def write(out_dir, name, lines):
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, name), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def ab(parent, out_dir, runs, steps, warmup):
    trees = {"this tree": ROOT, "parent": os.path.abspath(parent)}
    got = {k: [] for k in trees}
    for r in range(runs):
        for name, tree in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=tree, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"bench.py failed in {tree} ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            got[name].append((res["ms_per_step"], res["config"]["loss_last_step"]))
            print(f"run {r + 1} {name}: {res['ms_per_step']:.3f} ms per step, loss {res['config']['loss_last_step']!r}", flush=True)
    lines = [f"python bench.py --gpus 1 --steps {steps} --warmup {warmup}, this tree and a checkout of the parent commit alternating, "
             f"{runs} processes each, ms per step (and the last step's loss):"]
    for name, v in got.items():
        ms = [x for x, _ in v]
        lines.append(f"  {name:10s} " + "  ".join(f"{x:7.3f}" for x in ms) + f"   median {statistics.median(ms):7.3f}  spread "
                     f"{max(ms) - min(ms):.3f}   loss {sorted(set(l for _, l in v))}")
    a, b = [x for x, _ in got["this tree"]], [x for x, _ in got["parent"]]
    lines.append(f"  median difference this tree - parent {statistics.median(a) - statistics.median(b):+.3f} ms; the parent's own "
                 f"spread {max(b) - min(b):.3f} ms")
    write(out_dir, "r21_ab.txt", lines)


def _setup():
    import torch
    import bench
    feats_host, caps, feat_lens, cap_lens = bench.synthetic(1)
    feats = feats_host.cuda()

    def make(**kw):
        from acvae_amd.trainer import TrainStep
        return TrainStep(bench.build_model().cuda().train(), bench.V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0, **kw)

    def step(ts):
        random.seed(0)
        return ts.step(feats, feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
    return torch, make, step


def steps(out_dir, calls, reverse=False):
    torch, make, step = _setup()
    variants = {"plain": {}, "accum_steps=4": dict(accum_steps=4), "ema_decay=0.999": dict(ema_decay=0.999),
                "accum_steps=4, ema_decay=0.999": dict(accum_steps=4, ema_decay=0.999)}
    if reverse:                                          # the objects made (and their buffers allocated) in the opposite order
        variants = dict(reversed(list(variants.items())))
    runs = {name: (make(**kw), {"plain": [], "non-final": [], "final": []}) for name, kw in variants.items()}
    for ts, _ in runs.values():
        for _ in range(8):
            step(ts)
        ts.flush()
    torch.cuda.synchronize()
    for _ in range(calls // 4):
        for name, (ts, v) in runs.items():
            for _ in range(4):                           # one window (or four plain steps), every call timed on its own
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parts = step(ts)
                torch.cuda.synchronize()
                kind = "plain" if "applied" not in parts else ("final" if parts["applied"] else "non-final")
                v[kind].append((time.perf_counter() - t0) * 1e3)
    ts0 = runs["plain"][0]
    lines = [f"TrainStep.step, resident features, 32 clips x 1000 frames, {ts0.n_active} active of {ts0.flat_p.numel()} flat elements; "
             "device-synchronised before and after every call (so a call cannot overlap the next one's host work: the times are",
             "above bench.py's pipelined ms per step), windows alternating between the variants, objects made in the order "
             + ("listed" if not reverse else "listed (the reverse of the default)") + ", ms per call:"]
    base = statistics.median(runs["plain"][1]["plain"])
    for name, (ts, v) in runs.items():
        ts.synchronize()
        for kind, x in v.items():
            if x:
                lines.append(f"  {name:32s} {kind:10s} n {len(x):3d}  median {statistics.median(x):7.3f}  min {min(x):7.3f}  max {max(x):7.3f}"
                             f"  ({statistics.median(x) - base:+.3f} to the plain step)")
    write(out_dir, "r21_steps_reverse.txt" if reverse else "r21_steps.txt", lines)


def kernels(out_dir):
    torch, make, step = _setup()
    meta = {}
    for opt in ("Adam", "AdamW"):
        ts = make(optimizer=opt, accum_steps=4, ema_decay=0.999)
        for _ in range(6 * 4):
            step(ts)
        ts.synchronize()
        meta = {"n_active": ts.n_active, "total": ts.flat_p.numel()}
    os.makedirs(out_dir, exist_ok=True)
    json.dump(meta, open(os.path.join(out_dir, "r21_kernel_meta.json"), "w"))
    print(meta)


def kernel_report(trace_dir, out_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace found under {trace_dir}")
    meta = json.load(open(os.path.join(out_dir, "r21_kernel_meta.json")))
    n, total = meta["n_active"], meta["total"]
    # bytes each launch must move once, per element of its range
    # (the trace may hold mangled or demangled names)
    kinds = [(("accumulate_kernelILb1", "accumulate_kernel<true>"), "accumulate_kernel<first>", n, 8),
             (("accumulate_kernelILb0", "accumulate_kernel<false>"), "accumulate_kernel<add>", n, 12),
             (("ema_kernel",), "ema_kernel", total, 12), (("sqsum_kernel",), "sqsum_kernel", n, 4),
             (("opt_kernel",), "opt_kernel<Adam> (AdamW)", n, 28), (("adam_kernel",), "adam_kernel (Adam)", n, 28)]
    times = {}
    for r in csv.DictReader(open(paths[0])):
        for keys, label, _, _ in kinds:
            if any(k in r["Kernel_Name"] for k in keys):
                times.setdefault(label, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = [f"rocprofv3 --kernel-trace, windows of accum_steps=4 with ema_decay at bench.py's shape under Adam and AdamW; {n} active of "
             f"{total} flat fp32 elements.  The first two launches of a kind are left out (warm-up).  bytes = what the launch must move once; GB/s over the median "
             f"kernel time; {HBM_PEAK_GBS / 1e3:.0f} TB/s is the HBM peak (spec).  Each buffer is about 100 MB and the last-level cache holds 256 MiB,"
             " so part of what the launch in front left behind can still be there: these are not pure HBM rates.",
             f"{'kernel':28s} {'n':>4s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'GB/s':>7s} {'of HBM peak':>11s}"]
    for _, label, elems, per in kinds:
        v = times.get(label, [])[2:]
        if not v:
            lines.append(f"{label:28s}    0  (not in the trace)")
            continue
        med, nbytes = statistics.median(v), elems * per
        lines.append(f"{label:28s} {len(v):4d} {med:10.1f} {min(v):8.1f} {max(v):8.1f} {nbytes / 1e6:8.1f} {nbytes / med / 1e3:7.0f} "
                     f"{nbytes / med / 1e3 / HBM_PEAK_GBS:11.1%}")
    write(out_dir, "r21_kernels.txt", lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_accumulate_out")
    ap.add_argument("--ab", metavar="PARENT")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--reverse", action="store_true", help="step times: make the four objects in the opposite order")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-report", metavar="TRACE")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab, a.out, a.runs, a.steps, a.warmup)
    elif a.kernel_report:
        kernel_report(a.kernel_report, a.out)
    elif a.kernels:
        kernels(a.out)
    else:
        steps(a.out, a.calls, a.reverse)
