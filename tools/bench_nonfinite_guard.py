#!/usr/bin/env python3
"""Measurements behind profiles/r23_nonfinite_guard.txt: TrainStep(nonfinite="skip") at bench.py's shape (32 clips of 1000
frames, 22-token captions, V = 5000, E = 512) under AdamW with clipping.

    python tools/bench_nonfinite_guard.py --ab PARENT [--out DIR] [--runs N] [--steps K] [--warmup W]
        `python bench.py --gpus 1 --steps K --warmup W` in this tree and in PARENT (a checkout of the parent commit, built),
        alternating, N runs each, every run a process of its own                                        -> DIR/r23_ab.txt
    python tools/bench_nonfinite_guard.py [--out DIR] [--calls N]
        time per call of TrainStep.step, device-synchronised around every call, guard off / guard on / two groups without
        the guard alternating                                                                           -> DIR/r23_steps.txt
    rocprofv3 --kernel-trace --stats -d TRACE -o t --output-format csv -- python tools/bench_nonfinite_guard.py --kernels [--out DIR]
        K steps of "two groups" (the unguarded grouped update), then K steps with the guard             -> DIR/r23_kernel_meta.json
    python tools/bench_nonfinite_guard.py --kernel-report TRACE [--out DIR]
        reads the trace and the meta file (no GPU)                                                      -> DIR/r23_kernels.txt
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
KERNEL_STEPS = 12
VARIANTS = ("guard off", "guard on", "two groups")


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
    write(out_dir, "r23_ab.txt", lines)


def _setup():
    import torch
    import bench
    feats_host, caps, feat_lens, cap_lens = bench.synthetic(1)
    feats = feats_host.cuda()

    def make(variant):
        from acvae_amd.trainer import TrainStep
        model = bench.build_model().cuda().train()
        kw = {}
        if variant == "guard on":
            kw["nonfinite"] = "skip"
        if variant == "two groups":
            enc = list(model.encoder.parameters())
            ids = {id(p) for p in enc}
            kw["param_groups"] = [{"params": enc}, {"params": [p for p in model.parameters() if id(p) not in ids]}]
        return TrainStep(model, bench.V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0, optimizer="AdamW", **kw)

    def step(ts):
        random.seed(0)
        return ts.step(feats, feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
    return torch, make, step


def steps(out_dir, calls):
    torch, make, step = _setup()
    runs = {v: (make(v), []) for v in VARIANTS}
    for ts, _ in runs.values():
        for _ in range(8):
            step(ts)
    torch.cuda.synchronize()
    for _ in range(calls // 4):
        for name, (ts, v) in runs.items():
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(ts)
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
    ts0 = runs["guard off"][0]
    nbuf = 0 if ts0.flat_buf is None else ts0.flat_buf.numel()
    lines = [f"TrainStep.step under AdamW with clipping, resident features, 32 clips x 1000 frames, {ts0.n_active} active of "
             f"{ts0.flat_p.numel()} flat elements, {nbuf} floats of module buffers; device-synchronised before and after every call "
             "(the times are above bench.py's pipelined ms per step), four calls of a variant at a time, the variants alternating, "
             "ms per call:"]
    base = statistics.median(runs["guard off"][1])
    for name, (ts, v) in runs.items():
        ts.synchronize()
        extra = f"  counts {ts.guard_counts()}" if name == "guard on" else ""
        lines.append(f"  {name:10s} n {len(v):3d}  median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}"
                     f"  ({statistics.median(v) - base:+.3f} to guard off){extra}")
    write(out_dir, "r23_steps.txt", lines)


def kernels(out_dir):
    torch, make, step = _setup()
    meta = {"steps": KERNEL_STEPS}
    for v in ("two groups", "guard on"):
        ts = make(v)
        for _ in range(KERNEL_STEPS):
            step(ts)
        ts.synchronize()
        meta.update(n_active=ts.n_active, total=ts.flat_p.numel(), n_buf=0 if ts.flat_buf is None else ts.flat_buf.numel())
        table, _, segments = ts._chunk_table(())
        meta[v] = {"segments": segments, "chunks": int(table.shape[0])}
        del ts
    os.makedirs(out_dir, exist_ok=True)
    json.dump(meta, open(os.path.join(out_dir, "r23_kernel_meta.json"), "w"))
    print(meta)


def kernel_report(trace_dir, out_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace found under {trace_dir}")
    meta = json.load(open(os.path.join(out_dir, "r23_kernel_meta.json")))
    n, K = meta["n_active"], meta["steps"]
    keys = ("opt_groups_kernel", "sqsum_chunks_kernel", "norm_groups_final_kernel", "guard_witness_kernel", "guard_decide_kernel",
            "guard_restore_kernel")
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))
    times = {}
    for r in rows:
        for key in keys:
            if key in r["Kernel_Name"]:
                times.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = [f"rocprofv3 --kernel-trace, {K} steps of two identical groups without the guard, then {K} steps with the guard (one "
             f"group), AdamW with clipping at bench.py's shape, one process, one trace; {n} active fp32 elements, {meta['n_buf']} "
             "floats of module buffers.",
             f"  two groups: {meta['two groups']['segments']} segments, {meta['two groups']['chunks']} chunks; guard on: "
             f"{meta['guard on']['segments']} segment(s), {meta['guard on']['chunks']} chunks",
             "The first two launches of a kind and variant are left out (warm-up).  spread = (max - min) / median of the launches kept.",
             f"{'kernel':44s} {'n':>3s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>7s} {'x unguarded':>11s}"]
    med = {}

    def row(label, v, base=None):
        v = v[2:]
        if not v:
            lines.append(f"{label:44s}   0  (not in the trace)")
            return
        m = statistics.median(v)
        med[label] = m
        ratio = f"{m / med[base]:11.3f}" if base in med else "          -"
        lines.append(f"{label:44s} {len(v):3d} {m:10.1f} {min(v):8.1f} {max(v):8.1f} {(max(v) - min(v)) / m:7.1%} {ratio}")

    for key in ("opt_groups_kernel", "sqsum_chunks_kernel", "norm_groups_final_kernel"):
        v = times.get(key, [])
        row(f"{key}, two groups, no guard", v[:K])
        row(f"{key}, guard on", v[K:2 * K], f"{key}, two groups, no guard")
    for key in ("guard_witness_kernel", "guard_decide_kernel", "guard_restore_kernel"):
        row(key, times.get(key, []))
    a, b = med.get("opt_groups_kernel, guard on"), med.get("opt_groups_kernel, two groups, no guard")
    if a and b:
        lines.append(f"guarded grouped update against the unguarded one: {a / b:.3f} x (held to 1.10 x: "
                     f"{'inside' if a / b <= 1.10 else 'MISSED'})")
    write(out_dir, "r23_kernels.txt", lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_nonfinite_guard_out")
    ap.add_argument("--ab", metavar="PARENT")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=48)
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
        steps(a.out, a.calls)
