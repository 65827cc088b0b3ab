#!/usr/bin/env python3
"""Measurements behind profiles/r19_likelihood.txt: scoring given captions on the device (acvae_amd/likelihood.py).

    python tools/bench_likelihood.py [--out DIR]
        one configs[4] batch (32 clips of 1000 frames x 5 captions of 22 tokens: 160 rows, V = 5000, E = 512) scored by
        score_captions against the host route (the same forward, logits and Gaussians downloaded, float64 torch on the CPU),
        alternating, and evaluate_likelihood with both modes per batch                                  -> DIR/r19_eval.txt
    rocprofv3 --kernel-trace -d TRACE -o t --output-format csv -- python tools/bench_likelihood.py --kernels [--out DIR]
        acvae_caption_terms against the two launches it replaces (acvae_row_logsoftmax_argmax + acvae_ls_ce_fwd, reduction
        0), alternating, at R = 160 and R = 32, on one buffer set ("warm": resident in the last-level cache) and on six in
        rotation ("cold"); writes the labels of its dispatches in order                        -> DIR/r19_kernel_labels.json
    python tools/bench_likelihood.py --kernel-report TRACE [--out DIR]
        reads the trace and the labels (no GPU)                                                     -> DIR/r19_kernels.txt
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(out_dir):
    import torch
    from acvae_amd import _lib
    T, V, E = 21, 5000, 512
    labels = []
    st = _lib.current_stream()

    def make(R, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.randn(R, T, V, device="cuda", generator=g) * 2
        tg = torch.randint(0, V, (R, T), device="cuda", generator=g)
        ga = [torch.randn(R, T, E, device="cuda", generator=g) for _ in range(4)]
        return x, tg, ga

    for R in (160, 32):
        sets = [make(R, 100 + i) for i in range(6)]
        lp = torch.empty(R, T, device="cuda")
        rk = torch.empty(R, T, dtype=torch.int32, device="cuda")
        kl = torch.empty(R, T, device="cuda")
        lse = torch.empty(R, T, device="cuda")
        rows = torch.empty(R, T, device="cuda")
        none4 = [None] * 4

        def new(s, with_kl, tag):
            x, tg, ga = s
            _lib.call("acvae_caption_terms", x, T * V, V, tg, T, None, *(ga if with_kl else none4), lp, rk, kl, R, T, V,
                      E if with_kl else 0, st)
            labels.append([tag, 1])

        def old(s, tag):
            x, tg, _ = s
            _lib.call("acvae_row_logsoftmax_argmax", x, T * V, V, None, None, lse, T, 1, R, T, V, st)
            _lib.call("acvae_ls_ce_fwd", x, T * V, V, tg, T, None, lse, 0.0, 0, rows, None, R, T, V, st)
            labels.append([tag, 2])

        for i in range(4):                                 # warm-up: code objects
            new(sets[0], True, "warmup"); old(sets[0], "warmup")
        torch.cuda.synchronize()
        for mode, n in (("warm", 1), ("cold", 6)):
            for i in range(36):
                s = sets[i % n]
                new(s, False, f"R{R}.{mode}.terms_logits_only")
                old(s, f"R{R}.{mode}.two_launch_route")
                new(s, True, f"R{R}.{mode}.terms_with_kl")
            torch.cuda.synchronize()
        # the same bits from both routes' logprob? (the new one is max-subtracted online, the old one in two passes)
        new(sets[0], False, "check"); old(sets[0], "check")
        torch.cuda.synchronize()
        print(f"R={R}: max |logprob_new + ce_row_old| = {float((lp + rows).abs().max()):.3e}")

    os.makedirs(out_dir, exist_ok=True)
    json.dump(labels, open(os.path.join(out_dir, "r19_kernel_labels.json"), "w"))
    print("calls labelled:", len(labels))


def kernel_report(trace_dir, out_dir):
    T, V, E = 21, 5000, 512
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace found under {trace_dir}")
    rows = list(csv.DictReader(open(paths[0])))
    mine = [r for r in rows if any(k in r["Kernel_Name"] for k in ("caption_terms_kernel", "row_stats_kernel", "ce_rows_kernel"))]
    mine.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = json.load(open(os.path.join(out_dir, "r19_kernel_labels.json")))
    calls = {}
    if len(mine) != sum(n for _, n in labels):
        sys.exit(f"{len(mine)} dispatches in the trace for {sum(n for _, n in labels)} labelled")
    i = 0
    for lab, n in labels:                                # (a label names one call and the number of its dispatches)
        us = sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[i:i + n])
        calls.setdefault(lab, []).append(us)
        i += n
    out = ["acvae_caption_terms against acvae_row_logsoftmax_argmax + acvae_ls_ce_fwd (reduction 0), T = 21, V = 5000, E = 512, fp32;",
           "kernel time from rocprofv3 --kernel-trace (sum of the route's kernels per call), 36 alternating calls per line;",
           "warm: one buffer set (67 MB of logits at R = 160: resident in the 256 MB last-level cache); cold: six sets in rotation.",
           "GB/s = the bytes the route must read once (logits, + the four Gaussians with KL) over the time; 8 TB/s is the HBM peak.",
           f"{'case':42s} {'n':>3s} {'median us':>10s} {'min':>8s} {'max':>8s} {'GB/s':>8s} {'of 8 TB/s':>9s}"]
    for lab, v in calls.items():
        if lab in ("warmup", "check"):
            continue
        R = int(lab.split(".")[0][1:])
        nbytes = R * T * V * 4 + (4 * R * T * E * 4 if lab.endswith("with_kl") else 0)
        med = statistics.median(v)
        gbs = nbytes / med / 1e3
        out.append(f"{lab:42s} {len(v):3d} {med:10.1f} {min(v):8.1f} {max(v):8.1f} {gbs:8.0f} {gbs / 8000:9.1%}")
    open(os.path.join(out_dir, "r19_kernels.txt"), "w").write("\n".join(out) + "\n")
    print("\n".join(out))


def end_to_end(out_dir):
    import numpy as np
    import torch
    import bench
    from acvae_amd import evaluate as EV, likelihood as lk
    B, C, T, L, V = 32, 5, 1000, 22, 5000
    model = bench.build_model().cuda().eval()
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, T, 64, generator=g)
    fl = np.full(B, T, dtype=np.int64)
    caps = torch.zeros(B * C, L)
    caps[:, 0] = 1; caps[:, -1] = 2
    caps[:, 1:-1] = torch.randint(4, V, (B * C, L - 2), generator=g).float()
    cl = np.full(B * C, L, dtype=np.int64)
    ci = np.repeat(np.arange(B), C)
    feats_d = feats.cuda()
    lines = []

    def device_route(z):
        rec = lk.score_captions(model, feats_d, fl, caps, cl, clip_index=ci, z=z, samples=1)
        return rec["nll"].cpu().numpy()                      # the download a caller makes: 160 float64

    def host_route(z):
        rows = lk.Rows(cl, ci, B, 1)
        with torch.no_grad():
            o = model(feats_d, fl.copy(), caps[torch.from_numpy(rows.pair)], rows.lens, ss_ratio=1.0,
                      dis_ratio=0 if z == "posterior" else 1, clip_index=rows.clip)
            x = o["logits"].cpu().double()
            ga = [o[k].cpu().double() for k in ("q_means", "q_logs", "p_means", "p_logs")]
        tg = caps[torch.from_numpy(rows.pair)][:, 1:].long()
        lp = torch.log_softmax(x, -1).gather(-1, tg.unsqueeze(-1)).squeeze(-1)
        rank = (x > x.gather(-1, tg.unsqueeze(-1))).sum(-1)
        kl = (ga[3] / 2 - ga[1] / 2 + (torch.exp(ga[1]) + (ga[0] - ga[2]) ** 2) / (2 * torch.exp(ga[3])) - .5).sum(-1)
        return (-lp.sum(1)).numpy(), rank, kl

    for z in ("posterior", "prior"):
        times = {"device": [], "host": []}
        for rep in range(7):
            for name, fn in (("device", device_route), ("host", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(z)
                torch.cuda.synchronize()
                if rep >= 2:                                 # two warm-up rounds
                    times[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in times.items():
            lines.append(f"score one batch (32 clips x 5 captions, z={z}), {name} route: median {np.median(v):.1f} ms "
                       f"(min {min(v):.1f}, max {max(v):.1f}, n={len(v)})")

    # evaluate_likelihood end to end: 2 batches, both modes
    voc = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(V - 4)]:
        voc.add_word(w)
    items = [(f"clip{i}", feats[i % B]) for i in range(2 * B)]
    key2caps = {f"clip{i}": [" ".join(f"w{int(t)}" for t in torch.randint(0, V - 4, (L - 2,), generator=g)) for _ in range(C)]
                for i in range(2 * B)}
    ts = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = EV.evaluate_likelihood(model, items, key2caps, voc, batch_size=B, z=("posterior", "prior"), samples=1)
        torch.cuda.synchronize()
        if rep >= 1:
            ts.append((time.perf_counter() - t0) * 1e3 / 2)
    lines.append(f"evaluate_likelihood, z=(posterior, prior), samples=1, per batch of 32 clips x 5 captions (one encoder pass, two "
               f"forwards; host tokenising and the result's formulas included): median {np.median(ts):.1f} ms (min {min(ts):.1f}, max {max(ts):.1f}, n={len(ts)})")
    lines.append(f"  (random weights: perplexity {res['prior']['perplexity']:.1f} at V = 5000, top1 {res['prior']['top1']:.4f})")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "r19_eval.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_likelihood_out")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-report", metavar="TRACE")
    a = ap.parse_args()
    if a.kernel_report:
        kernel_report(a.kernel_report, a.out)
    elif a.kernels:
        kernels(a.out)
    else:
        end_to_end(a.out)
