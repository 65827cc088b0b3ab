#!/usr/bin/env python3
"""Measurements behind profiles/r20_kl_objective.txt: the KL objective of the training step (acvae_amd.train_util.KLObjective).

    python tools/bench_kl_objective.py [--out DIR] [--steps K] [--rounds N]
        TrainStep.step at bench.py's shape (32 clips of 1000 frames, captions of 8..22 tokens, V = 5000, E = 512) with the
        default KL (Normal_kl_loss) and with kl_reduction="valid" + free bits per dimension and per cell: one TrainStep and one
        model each, alternating in rounds of K steps inside one process                                -> DIR/r20_steps.txt
    rocprofv3 --kernel-trace -d TRACE -o t --output-format csv -- python tools/bench_kl_objective.py --kernels [--out DIR]
        acvae_kl_objective_fwd + bwd against acvae_gauss_kl_fwd + bwd on the same tensors, alternating, at (32, 21, 512)
        and (160, 21, 512); writes the labels of its calls in order                           -> DIR/r20_kernel_labels.json
    python tools/bench_kl_objective.py --kernel-report TRACE [--out DIR]
        reads the trace and the labels (no GPU)                                                     -> DIR/r20_kernels.txt
"""
import argparse
import csv
import glob
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("kl_obj_slab_kernel", "kl_obj_finish_kernel", "kl_obj_scalar_kernel", "kl_obj_bwd_kernel")
OLD = ("kl_fwd_kernel", "final_sum_kernel", "kl_bwd_kernel")
SHAPES = ((32, 21, 512), (160, 21, 512))


def kernels(out_dir):
    import torch
    from acvae_amd import _lib
    labels = []
    st = _lib.current_stream()
    for R, T, E in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(R)
        ts = [torch.randn(R, T, E, device="cuda", generator=g) * .5 for _ in range(4)]
        lens = torch.randint(7, T + 1, (R,), device="cuda", generator=g)
        D = int(lens.sum())
        nbytes = _lib.call("acvae_kl_objective_scratch_bytes", R, T, E)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        kl, raw, n_open = torch.empty(1, device="cuda"), torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
        dims, steps = torch.empty(E, device="cuda"), torch.empty(T, device="cuda")
        gates = torch.empty(R * T, dtype=torch.uint8, device="cuda")
        grads = [torch.empty(R, T, E, device="cuda") for _ in range(4)]
        g1 = torch.ones(1, device="cuda")
        part = torch.empty(_lib.call("acvae_kl_partials", R * T * E), device="cuda")

        def new(over_cell, tag):
            _lib.call("acvae_kl_objective_fwd", *ts, lens, D, 1, over_cell, 0.05 if not over_cell else 10.0, kl, raw, dims, steps,
                      n_open, gates, scratch, nbytes, R, T, E, st)
            _lib.call("acvae_kl_objective_bwd", *ts, lens, D, over_cell, gates, g1, *grads, R, T, E, st)
            labels.append([tag, 4])                      # slab, finish, scalar, bwd

        def old(tag):
            _lib.call("acvae_gauss_kl_fwd", *ts, part, kl, R * T, E, st)
            _lib.call("acvae_gauss_kl_bwd", *ts, g1, *grads, R * T, E, st)
            labels.append([tag, 3])                      # fwd, final sum, bwd

        for _ in range(4):
            new(0, "warmup"); new(1, "warmup"); old("warmup")
        torch.cuda.synchronize()
        for _ in range(36):
            new(0, f"R{R}.objective_dim"); old(f"R{R}.normal_kl"); new(1, f"R{R}.objective_cell")
        torch.cuda.synchronize()
        print(f"R={R}: D = {D} of {R * T} cells, gates open {int(n_open)}")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(labels, open(os.path.join(out_dir, "r20_kernel_labels.json"), "w"))
    print("calls labelled:", len(labels))


def kernel_report(trace_dir, out_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace found under {trace_dir}")
    rows = [r for r in csv.DictReader(open(paths[0])) if any(k in r["Kernel_Name"] for k in NEW + OLD)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = json.load(open(os.path.join(out_dir, "r20_kernel_labels.json")))
    if len(rows) != sum(n for _, n in labels):
        sys.exit(f"{len(rows)} dispatches in the trace for {sum(n for _, n in labels)} labelled")
    times, i, seq = {}, 0, []
    for lab, n in labels:                                # (a label names one call and the number of its dispatches)
        seq.append((lab, rows[i:i + n]))
        i += n
    for lab, rs in seq:
        if lab == "warmup":
            continue
        for r in rs:
            name = next(k for k in NEW + OLD if k in r["Kernel_Name"])
            times.setdefault((lab, name), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = ["acvae_kl_objective_fwd + bwd (reduction valid, free bits) against acvae_gauss_kl_fwd + bwd on the same tensors, T = 21,",
           "E = 512, fp32; kernel time from rocprofv3 --kernel-trace, 36 alternating calls per line, one buffer set (resident in the",
           "last-level cache).  bytes = what the launch must move once: forward 4 inputs (the valid cells only for the objective),",
           "backward 4 inputs + 4 outputs; GB/s over the median; 8 TB/s is the HBM peak.",
           f"{'case':24s} {'kernel':22s} {'n':>3s} {'median us':>10s} {'min':>7s} {'max':>7s} {'MB':>7s} {'GB/s':>7s} {'of 8 TB/s':>9s}"]
    totals = {}
    for (lab, name), v in times.items():
        R = int(lab.split(".")[0][1:])
        full = R * 21 * 512 * 4
        nbytes = {"kl_obj_slab_kernel": 4 * full, "kl_fwd_kernel": 4 * full, "kl_obj_bwd_kernel": 8 * full, "kl_bwd_kernel": 8 * full}.get(name, 0)
        med = statistics.median(v)
        totals[lab] = totals.get(lab, 0.0) + med
        bw = f"{nbytes / 1e6:7.1f} {nbytes / med / 1e3:7.0f} {nbytes / med / 1e3 / 8000:9.1%}" if nbytes else f"{'-':>7s} {'-':>7s} {'-':>9s}"
        out.append(f"{lab:24s} {name:22s} {len(v):3d} {med:10.1f} {min(v):7.1f} {max(v):7.1f} {bw}")
    for lab, t in totals.items():
        out.append(f"{lab:24s} {'sum of medians':22s} {'':3s} {t:10.1f}")
    open(os.path.join(out_dir, "r20_kernels.txt"), "w").write("\n".join(out) + "\n")
    print("\n".join(out))


def steps(out_dir, K, rounds):
    import numpy as np
    import torch
    import bench
    from acvae_amd.trainer import TrainStep
    feats_host, caps, feat_lens, _ = bench.synthetic(1)
    g = torch.Generator().manual_seed(7)
    cap_lens = np.array(sorted([bench.L] + [int(x) for x in torch.randint(8, bench.L + 1, (bench.B - 1,), generator=g)], reverse=True))
    for b, n in enumerate(cap_lens):
        caps[b, n - 1] = 2
        caps[b, n:] = 0
    feats = feats_host.cuda()
    variants = {"default (Normal_kl_loss)": {}, "valid": dict(kl_reduction="valid"),
                "valid, free_bits 0.05 per dim": dict(kl_reduction="valid", free_bits=0.05),
                "valid, free_bits 8.0 per cell": dict(kl_reduction="valid", free_bits=8.0, free_bits_over="cell")}
    runs = {}
    for name, kw in variants.items():
        ts = TrainStep(bench.build_model().cuda().train(), bench.V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0, **kw)
        runs[name] = (ts, [])

    def step(ts):
        random.seed(0)
        return ts.step(feats, feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)

    for ts, _ in runs.values():
        for _ in range(8):
            step(ts)
    torch.cuda.synchronize()
    last = {}
    for _ in range(rounds):
        for name, (ts, v) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                last[name] = step(ts)
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) / K * 1e3)
    lines = [f"TrainStep.step, resident features, 32 clips x 1000 frames, captions of {cap_lens.min()}..{cap_lens.max()} tokens "
             f"({int((cap_lens - 1).sum())} of {len(cap_lens) * (cap_lens.max() - 1)} cells valid), {rounds} alternating rounds of {K} steps, ms per step:"]
    base = statistics.median(runs["default (Normal_kl_loss)"][1])
    for name, (ts, v) in runs.items():
        ts.synchronize()
        extra = "" if "gates_open" not in last[name] else f"  gates open {int(last[name]['gates_open'])}, kl {float(last[name]['kl']):.4f}, kl_raw {float(last[name]['kl_raw']):.4f}"
        lines.append(f"  {name:32s} median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  ({statistics.median(v) - base:+.3f} to the default){extra}")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "r20_steps.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_kl_objective_out")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-report", metavar="TRACE")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.kernel_report:
        kernel_report(a.kernel_report, a.out)
    elif a.kernels:
        kernels(a.out)
    else:
        steps(a.out, a.steps, a.rounds)
