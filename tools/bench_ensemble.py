"""Ensemble decoding at the configs[4] shape (32 clips, T = 1000, V = 5000, E = 512, max_length 20): Ensemble.forward, greedy
and beam 3, for M = 1, 2, 4 members (seeds of bench.py's model), beside M back-to-back single-model calls
(model(feats, feat_lens, method="beam", beam_size=3) resp. method="greedy") in the same process, the two alternating so that
both see the same machine.  Every timed call runs the members' encoders too and ends in a device synchronise.

  python tools/bench_ensemble.py [--reps 7] [--json out.json]     ms per batch (median, min - max) and captions/s
  python tools/bench_ensemble.py --trace                          a short run for rocprofv3 --kernel-trace --stats:
      rocprofv3 --kernel-trace --stats -d DIR -o ens -- python tools/bench_ensemble.py --trace
  python tools/bench_ensemble.py --mix-bytes                      the mix kernel's algorithmic bytes per launch (no GPU)
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
MEMBERS = (1, 2, 4)
METHODS = (("greedy", 1), ("beam", 3))


def mix_bytes(M, rows):
    """Algorithmic bytes of one acvae_ensemble_mix launch: M * R * V * 4 read plus R * V * 4 written (greedy writes no scores)."""
    return {"read": M * rows * V * 4, "written_beam": rows * V * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--mix-bytes", action="store_true")
    args = ap.parse_args()
    if args.mix_bytes:
        for M in MEMBERS:
            for method, beam in METHODS:
                print(f"M={M} {method}: rows {B * beam}, {mix_bytes(M, B * beam)}")
        return
    import numpy as np
    import torch
    from acvae_amd import _lib
    if os.environ.get("ACVAE_DEV_LIB"):      # this TOOL's hook: time another build of the library (tools/ab_build.py)
        _lib.use_library(os.environ["ACVAE_DEV_LIB"])
    from acvae_amd.ensemble import Ensemble
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py measures on the GPU: none found")

    def member(seed):                                     # bench.build_model's architecture under another seed
        from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
        from acvae_amd.encoder import Cnn10
        from acvae_amd.vae_model import Hybrid_VAEModel
        torch.manual_seed(seed)
        dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0,
                                        num_layers=1, rnn_type="GRU", attn_size=E)
        return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                               prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().eval()

    models = [member(s) for s in range(1, max(MEMBERS) + 1)]
    feats = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fl = np.full(B, T)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    records = []
    for M in MEMBERS:
        ens = Ensemble(models[:M])
        for method, beam in METHODS:
            kw = dict(method=method, beam_size=beam, max_length=MAXLEN)

            def run_ens():
                ens(feats, fl.copy(), **kw)

            def run_singles():
                for m in models[:M]:
                    m(feats, fl.copy(), **kw)
            run_ens(); run_singles()                      # warm-up of every shape
            if args.trace:
                for _ in range(3):
                    run_ens()
                torch.cuda.synchronize()
                continue
            te, ts = [], []
            for _ in range(args.reps):                    # alternating
                te.append(timed(run_ens)); ts.append(timed(run_singles))
            rec = dict(members=M, method=method, beam=beam, clips=B, rows=B * beam,
                       ensemble_ms=dict(median=statistics.median(te), min=min(te), max=max(te)),
                       singles_ms=dict(median=statistics.median(ts), min=min(ts), max=max(ts)),
                       ensemble_captions_per_s=B / statistics.median(te) * 1e3,
                       singles_captions_per_s=B * M / statistics.median(ts) * 1e3, mix_bytes=mix_bytes(M, B * beam))
            records.append(rec)
            print("M=%d %-6s beam %d: ensemble %.2f ms/batch (%.2f - %.2f) = %.0f captions/s | %d single-model calls %.2f ms "
                  "(%.2f - %.2f) = %.0f captions/s of one model each" % (
                      M, method, beam, rec["ensemble_ms"]["median"], min(te), max(te), rec["ensemble_captions_per_s"], M,
                      rec["singles_ms"]["median"], min(ts), max(ts), rec["singles_captions_per_s"]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"workload": f"configs[4] shape: {B} clips, T={T}, V={V}, E={E}, max_length {MAXLEN}; every call runs the "
                       "members' encoders and ends in a synchronise", "reps": args.reps, "records": records}, fh, indent=1)


if __name__ == "__main__":
    main()
