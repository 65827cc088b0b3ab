"""CPU: the float64 reference of the decode composite (tests/decode_ref.py) and its yardstick, before any GPU is asked.

- its float32 run IS the oracle's text side: bit-equal to O.hybrid_forward on a small model with replayed noise, plain and
  with projected embeddings + embedding dropout + every step fed the prior's z;
- every case of tests/test_decode_composite_gpu.py: the pool margin is >= 1e-4, every r32 is finite and <= 1e-4 (so that
  max(1e-5, 8 r32) <= 8e-4 stays below the 2e-3 |ref| the whole-model check grads_match_oracle allows an element: the new
  bound is the tighter one on every tensor), and widths_util.plans says about the persistent launches what the case means;
- the bound is not vacuous: every MUTANT of the backward (one defect each, at the smallest case that can show it) is
  flagged on at least one tensor, while the float32 restatement of the same case stays within an eighth of the bound."""
import dataclasses
import math
import random

import pytest
import torch

import acvae_oracle as O
import decode_ref as R
import widths_util as W


@pytest.mark.parametrize("variant", ["plain", "proj_dropout_dis"])
def test_float32_run_is_the_oracles_text_side(variant):
    V, E, A, B, T, L = 44, 64, 32, 3, 64, 7
    hard = variant != "plain"
    state = W.make_state(V, E, E, A, E, proj_embed=24 if hard else None)
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(B, T, V, L, seed=5, ragged=True)
    torch.manual_seed(3); random.seed(3)
    rec = {}
    with torch.no_grad():
        want = O.hybrid_forward(state, feats, feat_lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=1 if hard else 0,
                                training=hard, record=rec, dec_dropout=0.3 if hard else 0.0)
    Tc = int(max(cap_lens)) - 1
    text = {k: v for k, v in state.items() if not k.startswith(("encoder.", "ln."))}     # audio_embeds is behind ln already
    with torch.no_grad():
        got = R.decode(text, want["audio_embeds"], want["audio_embeds_lens"], caps[:, :Tc].long(),
                       torch.as_tensor(cap_lens) - 1, want["q_z"], rec["eps_p"], [int(hard)] * Tc,
                       rec["dec_keep"] if hard else None, 0.3 if hard else 0.0, dtype=torch.float32)
    pairs = dict(logits="logits", outputs="outputs", p_means="p_means", p_logs="p_logs", p_z="p_z", p_means_utt="p_means_utt",
                 h="state")
    for mine, theirs in pairs.items():
        assert torch.equal(got[mine], want[theirs]), mine
    assert torch.equal(got["attn_w"], want["attn_weights"].transpose(1, 2)), "attn_w"
    assert torch.equal(got["hp"], want["hiddens_state"][0]) and torch.equal(got["cp"], want["hiddens_state"][1])
    assert torch.equal(got["lse"], torch.logsumexp(want["logits"], dim=-1))
    assert hard == (rec["dec_keep"] is not None)


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_case_is_reachable_and_takes_its_path(case):
    y = R.yardstick(case)
    margin = R.pool_margin(case)
    assert margin >= R.POOL_MARGIN, f"{case.name}: pool margin {margin:.2e}; choose another seed"
    worst = max(y, key=lambda k: y[k][1])
    print(f"{case.name}: pool margin {margin:.2e}, worst r32 {y[worst][1]:.2e} ({worst})")
    for k, (ref, r32) in y.items():
        assert math.isfinite(r32) and r32 <= 1e-4, (case.name, k, r32)
        assert bool(torch.isfinite(ref).all()), (case.name, k)
    names = set(y)
    assert {"fwd." + k for k in R.FWD if not (case.rollout and k == "p_means_utt")} <= names
    assert ("d_q_z" in names) == (not case.rollout) and "d_mem" in names
    # what is never reached is exactly zero in the reference
    d = R.inputs(case)
    dm = y["d_mem"][0]
    for n in range(case.N):
        assert float(dm[n, int(d["mem_lens"][n]):].abs().max() if int(d["mem_lens"][n]) < case.S else 0.0) == 0.0
    if not case.rollout:
        plan = W.plans(case.N, case.Tc, case.S, case.E, case.H, case.A, case.E)
        assert (plan["fwd_ok"] == 1 and plan["bwd_ok"] == 1) == case.persist_ok, (case.name, plan)
        assert case.persist_ok or case.path in ("per_step", "no_split", "defer_per_step"), case.name
        if case.S >= 64:               # S = 66 is past the streamed-attention threshold: two attention shares per clip
            assert plan["rc_splits"] == -(-case.S // 64) and (plan["dqd_part_floats"] > 0) == (case.S > 64), plan
    lens = d["lens1"].tolist()
    assert case.N == 1 or case.full or (min(lens) == 1 and max(lens) == case.Tc)
    assert case.N == 1 or (int(d["mem_lens"].min()) == 1 and int(d["mem_lens"].max()) == case.S)


SMALL = dict(N=2, Tc=2, S=2)
MUTANT_CASES = {
    "no_max_pool": R.Case("m", **SMALL, ups=("p_means_utt",)),
    "mean_over_Tc": R.Case("m", **SMALL, ups=("p_means_utt",)),                 # lens1 = [2, 1]: row 1 is divided by 2
    "embed_once": R.Case("m", N=2, Tc=1, S=2, words="same", ups=("logits",)),
    "mem_one_past": R.Case("m", **SMALL, ups=("logits",)),                      # mem_lens = [2, 1]
    "no_last_dh": R.Case("m", N=2, Tc=1, S=2, ups=("logits", "outputs")),
    "no_last_z": R.Case("m", **SMALL, ups=("p_means",)),
    "dis_z_to_q": R.Case("m", N=2, Tc=1, S=2, dis="all", ups=("logits",)),
    "no_keep_scale": R.Case("m", N=2, Tc=1, S=2, p=0.3, ups=("logits",)),
    "no_ln_bias": R.Case("m", N=2, Tc=1, S=2, ups=("logits",)),
}


def test_every_mutant_is_listed():
    assert set(MUTANT_CASES) == set(R.MUTANTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bound_flags_the_mutant(mutant):
    c = MUTANT_CASES[mutant]
    y = R.yardstick(c)
    d = R.inputs(c)
    words = R.fed_words(c, d["caps"])
    good = R._run(c, d, words, torch.float32)
    assert max(R.excess(good[k], ref, r32) for k, (ref, r32) in y.items()) <= 1.0 / R.FACTOR + 1e-12
    bad = R._run(c, d, words, torch.float64, mutant)
    over = {k: R.excess(bad[k], ref, r32) for k, (ref, r32) in y.items()}
    flagged = sorted(k for k, v in over.items() if v > 1.0)
    print(mutant, "flagged on", flagged)
    assert flagged, f"{mutant}: within the bound on every tensor (worst {max(over.values()):.3g})"
    assert all(not k.startswith("fwd.") for k in flagged), flagged               # a mutant changes the backward only


def test_measure_edges():
    z = torch.zeros(3)
    assert R.ratio(z, z) == 0.0 and R.ratio(z + 1e-30, z) == math.inf
    assert R.excess(z, z, 0.0) == 0.0 and R.excess(z + 1e-30, z, 0.0) == math.inf
    ref = torch.tensor([1.0, 0.0, -2.0])
    assert R.excess(torch.tensor([1.0, float("nan"), -2.0]), ref, 0.0) == math.inf
    rms = math.sqrt(5.0 / 3.0)
    assert abs(R.excess(ref + torch.tensor([0.0, 1e-5 * rms, 0.0]), ref, 0.0) - 1.0) < 1e-6
    c = dataclasses.replace(R.CASES[0], seed=9)
    assert c.ref_key() != R.CASES[0].ref_key() and R.CASES[0].ref_key() == R.CASES[1].ref_key()
