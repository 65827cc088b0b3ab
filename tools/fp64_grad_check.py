"""Encoder gradients of one full-size case of tests/test_fullsize_grads_gpu.py against the oracle run in float64.

    python tools/fp64_grad_check.py [CASE]          (CASE: a key of that file's CASES, default B16_T3000; needs an MI355X)

Runs the HIP training step (default launch path) and the fp32 oracle as the test does, then the oracle once more in float64
(weights, features and noise cast to double) under the HIP path's own ReLU decisions (and, for a scheduled-sampling case,
fed the HIP path's own words), and prints for every encoder tensor the
relative L2 distance of the fp32 oracle and of the HIP gradient from float64.  A per-tensor bound in the test's TOL_ENC_OF
rests on these numbers (the fp32 oracle's own distance from float64); re-check it after a change to the encoder kernels.

This tool is for full size.  At small shapes the same comparison is a test of the suite:
tests/test_encoder_composite_gpu.py holds every encoder tensor of Cnn10, Cnn14_16k and ResNet38 (training, evaluation mode,
no dropout, both convolution routes) to a margin over the fp32 reference's distance from float64 (tests/encoder_ref.py)."""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import acvae_oracle as O  # noqa: E402
import test_fullsize_grads_gpu as M  # noqa: E402


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).sum().sqrt() / b.pow(2).sum().sqrt())


def main(name):
    t0 = time.time()
    c = M._case(name)
    model, _ = M._hip(c, "default")
    masks = [m.cpu() for m in model.encoder.relu_masks()]
    hip = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if p.grad is not None}
    del model
    force = {i: m for i, m in enumerate(masks)}
    g32 = M._oracle_under(c)(force)
    rec = c["rec"]
    st64 = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in c["state"].items()}
    noise = dict(dropout=[m.clone() for m in rec["dropout"]], eps_q=rec["eps_q"].double(), eps_p=rec["eps_p"].double(),
                 relu_force=force, fed_words=c["fed"])      # a scheduled-sampling case: the HIP run's own words, as in the test
    torch.manual_seed(M.SEED); random.seed(M.SEED)
    g64 = M._patched(c["flags"], lambda: O.OracleTrainer(st64, M.V).step(
        c["feats"].double(), c["fl"].copy(), c["caps"].double(), c["cl"], c["ss"], c["dis"], noise=noise,
        apply_update=False))["grads"]
    bounds = M.TOL_ENC_OF.get(name, {})
    print(f"{name}: {time.time() - t0:.0f} s; relative L2 from the float64 oracle (test bound: 5e-4 unless listed)")
    print(f"{'tensor':40s} {'fp32 oracle':>12s} {'HIP':>10s} {'HIP - oracle':>13s} {'bound':>8s}")
    for k in g64:
        if k.startswith("encoder."):
            print(f"{k:40s} {rel(g32[k], g64[k]):12.2e} {rel(hip[k], g64[k]):10.2e} {rel(hip[k], g32[k]):13.2e} "
                  f"{bounds.get(k, 5e-4):8.1e}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "B16_T3000")
