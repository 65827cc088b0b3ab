#!/usr/bin/env python3
"""Measurements behind profiles/r22_param_groups.txt: TrainStep(param_groups=) at bench.py's shape (32 clips of 1000 frames,
22-token captions, V = 5000, E = 512) under AdamW, with one group, two groups (encoder / text) and split_params.

    python tools/bench_param_groups.py --ab PARENT [--out DIR] [--runs N] [--steps K] [--warmup W]
        `python bench.py --gpus 1 --steps K --warmup W` in this tree and in PARENT (a checkout of the parent commit, built),
        alternating, N runs each, every run a process of its own                                        -> DIR/r22_ab.txt
    python tools/bench_param_groups.py [--lib LIB] [--out DIR] [--calls N]
        time per call of TrainStep.step, device-synchronised around every call, the three variants alternating; the number
        of segments and chunks of each                                                                  -> DIR/r22_steps.txt
    rocprofv3 --kernel-trace --stats -d TRACE -o t --output-format csv -- python tools/bench_param_groups.py --kernels [--lib LIB] [--out DIR]
        K steps of each variant, one after the other                                                    -> DIR/r22_kernel_meta.json
    python tools/bench_param_groups.py --kernel-report TRACE [--out DIR] [--tag T]
        reads the trace and the meta file (no GPU)                                                      -> DIR/r22_kernels[_T].txt

--lib LIB loads another build of the library (one compiled with -DACVAE_OPT_CHUNK=C): the candidates for the chunk size.
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
KERNEL_STEPS = 12
VARIANTS = ("one group", "two groups", "split_params")


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
    write(out_dir, "r22_ab.txt", lines)


def _setup(lib):
    from acvae_amd import _lib
    if lib:
        _lib.use_library(lib)
    import torch
    import bench
    from acvae_amd import optim
    feats_host, caps, feat_lens, cap_lens = bench.synthetic(1)
    feats = feats_host.cuda()

    def groups_of(variant, model):
        if variant == "one group":
            return None
        if variant == "two groups":
            enc = list(model.encoder.parameters())
            ids = {id(p) for p in enc}
            return [{"params": enc, "lr": 5e-5}, {"params": [p for p in model.parameters() if id(p) not in ids]}]
        return optim.split_params(model, encoder_lr=5e-5)

    def make(variant):
        from acvae_amd.trainer import TrainStep
        model = bench.build_model().cuda().train()
        return TrainStep(model, bench.V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0, optimizer="AdamW",
                         param_groups=groups_of(variant, model))

    def step(ts):
        random.seed(0)
        return ts.step(feats, feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
    return torch, _lib, make, step


def _shape(ts, _lib):
    """(groups, segments, chunks, chunk size) of a TrainStep's usual step."""
    chunk = int(_lib.call("acvae_opt_chunk_elems"))
    if ts.group_norms is None:
        return 1, 1, 0, chunk
    table, _, segments = ts._chunk_table(())
    return len(ts.optimizer.param_groups), segments, int(table.shape[0]), chunk


def steps(out_dir, calls, lib):
    torch, _lib, make, step = _setup(lib)
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
    ts0 = runs["one group"][0]
    lines = [f"TrainStep.step under AdamW, resident features, 32 clips x 1000 frames, {ts0.n_active} active of {ts0.flat_p.numel()} flat "
             "elements; device-synchronised before and after every call (the times are above bench.py's pipelined ms per step), "
             "four calls of a variant at a time, the variants alternating, ms per call:"]
    base = statistics.median(runs["one group"][1])
    for name, (ts, v) in runs.items():
        ts.synchronize()
        G, segs, chunks, chunk = _shape(ts, _lib)
        uploads = len(ts._tables)
        lines.append(f"  {name:14s} groups {G}  segments {segs:4d}  chunks {chunks:5d} of at most {chunk}  tables uploaded {uploads}  "
                     f"n {len(v):3d}  median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}"
                     f"  ({statistics.median(v) - base:+.3f} to one group)")
    write(out_dir, "r22_steps.txt", lines)


def kernels(out_dir, lib):
    torch, _lib, make, step = _setup(lib)
    meta = {"variants": {}}
    for v in VARIANTS:
        ts = make(v)
        for _ in range(KERNEL_STEPS):
            step(ts)
        ts.synchronize()
        G, segs, chunks, chunk = _shape(ts, _lib)
        meta.update(n_active=ts.n_active, total=ts.flat_p.numel(), chunk=chunk, steps=KERNEL_STEPS)
        meta["variants"][v] = {"groups": G, "segments": segs, "chunks": chunks}
        del ts
    os.makedirs(out_dir, exist_ok=True)
    json.dump(meta, open(os.path.join(out_dir, "r22_kernel_meta.json"), "w"))
    print(meta)


def kernel_report(trace_dir, out_dir, tag):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace found under {trace_dir}")
    meta = json.load(open(os.path.join(out_dir, "r22_kernel_meta.json")))
    n, K = meta["n_active"], meta["steps"]
    names = {"sqsum_kernel": "sqsum_kernel", "norm_final_kernel": "norm_final_kernel", "opt_kernel": "opt_kernel<Adam> (AdamW)",
             "sqsum_chunks_kernel": "sqsum_chunks_kernel", "norm_groups_final_kernel": "norm_groups_final_kernel",
             "opt_groups_kernel": "opt_groups_kernel<Adam>"}
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))
    times = {}
    for r in rows:
        for key, label in names.items():
            if key in r["Kernel_Name"]:                  # (mangled or demangled; no name of these six contains another)
                times.setdefault(label, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    # the grouped kernels ran K times under "two groups", then K times under "split_params"
    lines = [f"rocprofv3 --kernel-trace, {K} steps each of one group, two groups (encoder / text) and split_params under AdamW at bench.py's "
             f"shape, one process, one trace; {n} active fp32 elements; chunks of at most {meta['chunk']} elements.",
             "  " + "; ".join(f"{v}: {d['groups']} groups, {d['segments']} segments, {d['chunks']} chunks" for v, d in meta["variants"].items()),
             "The first two launches of a kind and variant are left out (warm-up).  bytes = what the launch must move once; TB/s over "
             f"the median kernel time; {HBM_PEAK_GBS / 1e3:.0f} TB/s is the HBM peak (spec).  spread = (max - min) / median of the launches kept.",
             f"{'kernel':40s} {'n':>3s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>7s} {'MB':>7s} {'TB/s':>6s} {'x one group':>11s}"]
    med = {}

    def row(label, v, nbytes, base=None):
        v = v[2:]
        if not v:
            lines.append(f"{label:40s}   0  (not in the trace)")
            return
        m = statistics.median(v)
        med[label] = m
        rate = f"{nbytes / m / 1e6:6.2f}" if nbytes else "     -"
        ratio = f"{m / med[base]:11.3f}" if base in med else "          -"
        lines.append(f"{label:40s} {len(v):3d} {m:10.1f} {min(v):8.1f} {max(v):8.1f} {(max(v) - min(v)) / m:7.1%} {nbytes / 1e6:7.1f} {rate} {ratio}")

    row("sqsum_kernel", times.get("sqsum_kernel", []), 4 * n)
    row("norm_final_kernel", times.get("norm_final_kernel", []), 0)
    row("opt_kernel<Adam> (AdamW)", times.get("opt_kernel<Adam> (AdamW)", []), 28 * n)
    for i, variant in enumerate(VARIANTS[1:]):
        chunks = meta["variants"][variant]["chunks"]
        for label, base, per in (("sqsum_chunks_kernel", "sqsum_kernel", 4), ("norm_groups_final_kernel", "norm_final_kernel", 0),
                                 ("opt_groups_kernel<Adam>", "opt_kernel<Adam> (AdamW)", 28)):
            v = times.get(label, [])
            row(f"{label}, {variant}", v[i * K:(i + 1) * K], per * n + (12 * chunks if per else 0), base)
    for variant in VARIANTS[1:]:
        a = med.get(f"sqsum_chunks_kernel, {variant}", 0) + med.get(f"norm_groups_final_kernel, {variant}", 0)
        b = med.get("sqsum_kernel", 0) + med.get("norm_final_kernel", 0)
        if a and b:
            lines.append(f"norm, both launches, {variant}: {a:.1f} us against {b:.1f} us with one group ({a / b:.3f} x)")
    write(out_dir, f"r22_kernels{'_' + tag if tag else ''}.txt", lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_param_groups_out")
    ap.add_argument("--ab", metavar="PARENT")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--lib", help="another build of the library (a chunk-size candidate)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-report", metavar="TRACE")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab, a.out, a.runs, a.steps, a.warmup)
    elif a.kernel_report:
        kernel_report(a.kernel_report, a.out, a.tag)
    elif a.kernels:
        kernels(a.out, a.lib)
    else:
        steps(a.out, a.calls, a.lib)
