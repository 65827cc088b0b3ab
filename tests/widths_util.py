"""The text side with widths that are NOT all equal: one builder that takes the embed width E, the decoder GRU's width H,
the attention width A and the posterior GRU's width Hq apart, and the named width sets every file uses
(test_text_widths_gpu.py, test_decode_persist_gpu.py, test_posterior_layers_gpu.py, test_scst_gpu.py, test_ensemble_gpu.py).

Which widths are free:
- training: A only.  mean_log_out = Linear(E, 2E) is fed the pooled GRU outputs (H == E), and the MSE pairs
  q_means_utt [N, 2 Hq] with p_means_utt [N, 2 E] (Hq == E);
- inference and differentiable rollouts (no utterance head): H and A;
- the posterior called on its own: Hq."""
import numpy as np

import acvae_oracle as O

# training: (E, A) with H = Hq = E; optional B, T, V (defaults B = 3, T = 64, V = 44)
TRAIN_SETS = {
    "E64_A32": dict(E=64, A=32),                         # A < E: the max(A, E) regions are sized by E
    "E64_A160": dict(E=64, A=160),                       # A > E: sized by A; persistent forward and BPTT both eligible
    "E128_A96": dict(E=128, A=96, B=5),                  # neither a power-of-two multiple of the other
    "E64_A72": dict(E=64, A=72),                         # A % 32 != 0: per-step paths only; vector attention (A % 4 == 0)
    "E64_A50": dict(E=64, A=50, B=4),                    # A % 4 != 0: the scalar attention path
    "E64_A160_T1056": dict(E=64, A=160, T=1056, B=2),    # S = 66: streamed attention, rc_splits = 2 (A-wide d qd shares)
    "E512_A256": dict(E=512, A=256, B=4, V=300),         # production E: ks_rb = 3, ks_pa = 2, A = 256 launch width
}
# sets meant for the persistent decode launches (forward and BPTT): A % 32 == 0
TRAIN_PERSISTENT = ("E64_A32", "E64_A160", "E128_A96", "E64_A160_T1056", "E512_A256")
# inference and rollouts: (E, H, A); in the last neither H nor A is a multiple of 32 and A % 4 != 0
INFER_SETS = [(64, 96, 160), (64, 32, 96), (128, 64, 64), (64, 40, 50)]
# the posterior alone: (E, Hq); the last runs per step (Hq % 32 != 0)
POSTERIOR_SETS = [(64, 64), (64, 32), (64, 96), (32, 160), (48, 40)]
ENSEMBLE_MEMBERS = [(64, 96, 160), (64, 32, 96)]


def make_state(V, E, H, A, Hq, encoder="Cnn10", proj_embed=None):
    return O.closed_form_state(O.state_shapes(V, E, H, A, Hq, 512 if encoder == "Cnn10" else 2048, encoder=encoder,
                                              proj_embed=proj_embed))


def build_model(V, E, H, A, Hq, state=None, encoder="Cnn10", dec_dropout=0.0, proj_embed=0):
    """Hybrid_VAEModel on the GPU with the four widths given apart (test_model_gpu.build_model passes one number for all)."""
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10, Cnn14_16k
    from acvae_amd.vae_model import Hybrid_VAEModel
    enc = Cnn10(64, 512) if encoder == "Cnn10" else Cnn14_16k(64, 2048)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=H, dropout=dec_dropout,
                                    num_layers=1, rnn_type="GRU", attn_size=A)
    if proj_embed:
        dec.load_word_embeddings(np.zeros((V, proj_embed), dtype=np.float32), tune=True, projection=True)
    m = Hybrid_VAEModel(enc, dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": Hq, "dropout": 0.0},
                        prior_model="PriorRNN", prior_args={"hidden_size": E, "dropout": 0.0})
    if state is not None:
        missing = m.load_state_dict({k: v.clone() for k, v in state.items()})
        assert not missing.missing_keys and not missing.unexpected_keys, missing
    assert (m.decoder.embed_size, m.decoder.model.hidden_size, m.decoder.attn.attn_size) == (E, H, A)
    return m.cuda()


def ragged_caps(B, L, V, generator, short_row=1):
    """[B, L] float captions <start> w .. <end> with lengths L, L - 1, .., one of them (row `short_row`) only <start><end>."""
    import torch
    lens = [max(2, L - b) for b in range(B)]
    if B > 1:
        lens[short_row] = 2
    lens = sorted(lens, reverse=True)
    caps = torch.zeros(B, L)
    for b, n in enumerate(lens):
        caps[b, 0] = 1; caps[b, n - 1] = 2
        if n > 2:
            caps[b, 1:n - 1] = torch.randint(4, V, (n - 2,), generator=generator).float()
    return caps, np.array(lens)


_PLAN_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "persist_plan.h"
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  int d[7];
  for (int k = 0; k < 7; ++k) d[k] = std::atoi(argv[k + 1]);
  const acvae::PdPlan f = acvae::decode_fwd_plan(d[0], d[1], d[2], d[3], d[4], d[5], true);
  const acvae::PbPlan b = acvae::decode_bwd_plan(d[0], d[1], d[2], d[3], d[4], d[5]);
  const acvae::PqPlan q = acvae::posterior_plan(d[0], d[1], d[6]);
  std::printf("%d %d %d %d %d %d %d %d %d %ld %d %d %d\n", (int)f.shape_ok, f.att_resident, f.n_d1, f.grid, (int)b.shape_ok, b.ks_rb,
              b.ks_pa, b.rc_splits, b.grid, b.dqd_part_floats, (int)q.shape_ok, q.grid, b.dv_rows);
  return 0;
}
"""
_plan_exe = []


def plans(N, Tc, S, E, H, A, Hq):
    """The plans of the persistent launches at these dims, read from acvae_amd/csrc/persist_plan.h itself through a small
    driver built with ROCm's host compiler (as tests/test_persist_plan_cpu.py does; that file's driver is a fixed sweep with its
    checks compiled in, this one answers for the dims it is given).  Built once per process in a directory that is removed
    when the process ends.  Returns a dict of the fields."""
    import atexit
    import os
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = "/opt/rocm/llvm/bin/clang++"
    if not _plan_exe:
        assert os.path.exists(cxx), f"{cxx} not found: the ROCm host compiler is needed to build the plan driver"
        d = tempfile.mkdtemp(prefix="acvae_plans_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, exe = os.path.join(d, "plans.cpp"), os.path.join(d, "plans")
        with open(src, "w") as fh:
            fh.write(_PLAN_DRIVER)
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "acvae_amd", "csrc"), src,
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        _plan_exe.append(exe)
    r = subprocess.run([_plan_exe[0]] + [str(int(x)) for x in (N, Tc, S, E, H, A, Hq)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    v = [int(x) for x in r.stdout.split()]
    keys = ("fwd_ok", "fwd_att_resident", "fwd_n_d1", "fwd_grid", "bwd_ok", "ks_rb", "ks_pa", "rc_splits", "bwd_grid",
            "dqd_part_floats", "post_ok", "post_grid", "dv_rows")
    return dict(zip(keys, v))


def train_dims(name, L=7):
    """(B, T, V, E, A, S, Tc) of a training width set: Cnn10 makes one memory frame of 16 feature frames; Tc = L - 1."""
    p = TRAIN_SETS[name]
    B, T, V = p.get("B", 3), p.get("T", 64), p.get("V", 44)
    return B, T, V, p["E"], p["A"], T // 16, L - 1
