"""Ensemble rollouts at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20).

  python tools/bench_ensemble_rollout.py [--members 2] [--sample-n 5] [--reps 7] [--json out.json]
      ms per batch (median, min - max) of Ensemble.rollout "sample", Ensemble.rollout "greedy" and M back-to-back
      single-model rollouts (model.rollout_shared_encoder, "sample"), all with rng="device", alternating in one process so
      that all see the same machine.  Every timed call runs the encoders too and ends in a device synchronise.
  python tools/bench_ensemble_rollout.py --kernels --rows 160     a short run for rocprofv3 --kernel-trace --stats:
      rocprofv3 --kernel-trace --stats -d DIR -o k -- python tools/bench_ensemble_rollout.py --kernels --rows 160
      the fused acvae_ensemble_mix_sample launch against the two launches it replaces (acvae_ensemble_mix with `out`, then
      acvae_sample_next_word on the mixed row), V = 5000, M = 2 and 5, the same inputs, 50 launches of each.  The kernels'
      names carry M (ensemble_mix_sample_kernel<M>, ensemble_mix_kernel<M>); sample_rows_kernel's time is the mean over both M.
  python tools/bench_ensemble_rollout.py --bytes                  the kernels' algorithmic bytes per launch (no GPU)
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

B, T, V, E, MAXLEN = 32, 1000, 5000, 512, 20
KERNEL_MEMBERS = (2, 5)


def kernel_bytes(M, rows):
    """Algorithmic bytes per launch: the members' rows and (fused / draw) the noise row read once from HBM; the two-launch
    route also writes the mixed row and reads it back."""
    return {"fused": (M + 1) * rows * V * 4, "mix_with_out": (M + 1) * rows * V * 4, "sample_next_word": 2 * rows * V * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--sample-n", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rows", type=int, default=160)
    ap.add_argument("--bytes", action="store_true")
    args = ap.parse_args()
    if args.bytes:
        for rows in (160, 32):
            for M in KERNEL_MEMBERS:
                print(f"R={rows} M={M}: {kernel_bytes(M, rows)}")
        return
    import numpy as np
    import torch
    from acvae_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_rollout.py measures on the GPU: none found")

    if args.kernels:
        R, st = args.rows, _lib.current_stream()
        g = torch.Generator(device="cuda").manual_seed(1)
        noise = torch.empty(R, V, device="cuda").exponential_(1, generator=g)
        seqs = torch.zeros(R, MAXLEN, dtype=torch.long, device="cuda")
        lp, mixed = torch.empty(R, MAXLEN, device="cuda"), torch.empty(R, V, device="cuda")
        word, best = torch.empty(R, dtype=torch.long, device="cuda"), torch.empty(R, device="cuda")
        for M in KERNEL_MEMBERS:
            rows = [torch.randn(R, V, device="cuda", generator=g) * 2 for _ in range(M)]
            ld = np.full(M, V, np.int64)
            for _ in range(50):
                _lib.call("acvae_ensemble_mix_sample", rows, ld.ctypes.data, M, noise, V, 2, 1.0, None, 0, seqs, MAXLEN, lp,
                          MAXLEN, word, 2, 0, R, V, st)
                _lib.call("acvae_ensemble_mix", rows, ld.ctypes.data, M, None, mixed, V, None, None, 0, R, V, st)
                _lib.call("acvae_sample_next_word", mixed, V, 0, noise, V, 0, 2, 1.0, word, best, 1, 0, R, 1, V, st)
            torch.cuda.synchronize()
        return

    from acvae_amd.ensemble import Ensemble

    def member(seed):                                     # bench.build_model's architecture under another seed
        from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
        from acvae_amd.encoder import Cnn10
        from acvae_amd.vae_model import Hybrid_VAEModel
        torch.manual_seed(seed)
        dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0,
                                        num_layers=1, rnn_type="GRU", attn_size=E)
        return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                               prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().eval()

    M, n = args.members, args.sample_n
    models = [member(s) for s in range(1, M + 1)]
    ens = Ensemble(models)
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)
    runs = {
        "rollout_sample": lambda: ens.rollout(feats, fl.copy(), sample_n=n, method="sample", rng="device", max_length=MAXLEN),
        "rollout_greedy": lambda: ens.rollout(feats, fl.copy(), sample_n=n, method="greedy", max_length=MAXLEN),
        "single_model_rollouts": lambda: [m.rollout_shared_encoder(feats, fl.copy(), n, method="sample", rng="device",
                                                                   max_length=MAXLEN) for m in models],
    }

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in runs.values():                              # warm-up of every shape
        timed(fn); timed(fn)
    times = {k: [] for k in runs}
    for _ in range(args.reps):                            # alternating
        for k, fn in runs.items():
            times[k].append(timed(fn))
    record = dict(members=M, sample_n=n, clips=B, rows=B * n, reps=args.reps,
                  ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()})
    for k, v in times.items():
        print("M=%d sample_n=%d %-22s %.2f ms/batch (%.2f - %.2f)" % (M, n, k, statistics.median(v), min(v), max(v)), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape: {B} clips, T={T}, V={V}, E={E}, max_length {MAXLEN}, rng='device'; every "
                       "call runs the members' encoders and ends in a synchronise", "record": record}, fh, indent=1)


if __name__ == "__main__":
    main()
