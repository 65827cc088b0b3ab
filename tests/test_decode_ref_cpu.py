"""CPU: the float64 reference of the decode composite (tests/decode_ref.py) and its yardstick, before any GPU is asked.

- its float32 run IS the oracle's text side: bit-equal to O.hybrid_forward on a small model with replayed noise, plain and
  with projected embeddings + embedding dropout + every step fed the prior's z;
- every case of tests/test_decode_composite_gpu.py: the pool margin is >= 1e-4, every r32 is finite and <= 1e-4 (so that
  max(1e-5, 8 r32) <= 8e-4 stays below the 2e-3 |ref| the whole-model check grads_match_oracle allows an element: the new
  bound is the tighter one on every tensor), and widths_util.plans says about the persistent launches what the case means;
- the bound is not vacuous: every MUTANT of the backward (one defect each, at the smallest case that can show it) is
  flagged on at least one tensor, while the float32 restatement of the same case stays within an eighth of the bound;
- the S > 64 cases cover the share layouts of the persistent BPTT's split attention role and both forward attention forms,
  and the two mistakes of a split attention backward (frames >= 64 left out of d qd; the softmax backward's sum taken per
  share) are flagged at every one of those cases."""
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
        if case.S >= 64:               # 64 frames per attention workgroup of the BPTT: S > 64 hands d qd over as shares
            assert plan["rc_splits"] == -(-case.S // R.SHARE) and (plan["dqd_part_floats"] > 0) == (case.S > 64), plan
            assert plan["dv_rows"] == case.N * plan["rc_splits"], plan
        if case.S > 64:
            assert case.att in ("resident", "streamed") or case.path == "per_step", case.name
            assert not case.att or plan["fwd_att_resident"] == int(case.att == "resident"), (case.name, plan)
            assert max(plan["fwd_grid"], plan["bwd_grid"]) <= 256, plan       # one workgroup per CU of an MI355X is enough
    lens = d["lens1"].tolist()
    assert case.N == 1 or case.full or (min(lens) == 1 and max(lens) == case.Tc)
    assert d["mem_lens"].tolist() == case.frames()
    assert case.N == 1 or (int(d["mem_lens"].min()) == 1 and int(d["mem_lens"].max()) == case.S)


def persistent_long():
    """The S > 64 cases whose backward is the persistent launch."""
    return [c for c in R.CASES if c.S > 64 and c.path in ("persist", "defer") and c.persist_ok and not c.rollout]


def test_long_clips_cover_the_share_layouts_and_both_attention_forms():
    cases = persistent_long()
    assert len(cases) >= 17
    fwd = {c.att for c in cases if c.ss == "all"}                    # (a mixed-sampling forward runs per step)
    assert fwd == {"resident", "streamed"}, fwd
    tails = {(-(-n // R.SHARE), n - (n - 1) // R.SHARE * R.SHARE) for c in cases for n in c.frames() if n > R.SHARE}
    assert {(2, 1), (2, 2), (2, 64), (3, 1), (3, 2), (3, 59)} <= tails, tails       # (shares, frames of the last share)
    # clips that leave one share or two of their workgroups fully masked, beside a clip that fills them
    assert any(c.S > 128 and any(n <= 64 for n in c.frames()) and any(64 < n <= 128 for n in c.frames()) for c in cases)
    # each per-step partner shares its reference with a persistent case
    keys = {c.ref_key() for c in cases}
    partners = [c for c in R.CASES if c.S > 64 and c.path == "per_step"]
    assert {c.S for c in partners} == {66, 130, 187} and all(c.ref_key() in keys for c in partners)
    assert any(c.A == 512 for c in cases) and any(c.E == 512 and c.A < 512 and c.S > 128 for c in cases)
    assert {c.Tc for c in cases} >= {1, 2, 3, 7} and {c.N for c in cases} >= {1, 32}


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
    "dqd_share0_only": R.Case("m", N=2, Tc=2, S=66, ups=("logits",)),           # mem_lens = [66, 1]: two frames in share 1
    "softmax_sum_per_share": R.Case("m", N=2, Tc=1, S=66, ups=("logits",)),
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


LONG_REFS = {}
for _c in persistent_long():
    LONG_REFS.setdefault(_c.ref_key(), _c)


@pytest.mark.parametrize("case", list(LONG_REFS.values()), ids=[c.name for c in LONG_REFS.values()])
@pytest.mark.parametrize("mutant", R.SPLIT_MUTANTS)
def test_the_bound_flags_a_wrong_split_attention_in_every_long_case(mutant, case):
    """The two mistakes a split attention backward can make, at every S > 64 case itself (one run per distinct reference;
    every such case has a clip of more than 64 frames).  One pair is the same function: with Tc = 1, d qd of the only step
    meets h_{-1} = 0 in the weight gradient and no earlier step in dh, so leaving frames out of it changes NOTHING - there
    the mutant must give the float64 reference back, and the case is in the list for the rows of dqd nobody writes."""
    c = case
    assert max(c.frames()) > R.SHARE
    y = R.yardstick(c)
    d = R.inputs(c)
    words = R.fed_words(c, d["caps"], None if c.ss == "all" else R.surrogate_words(c))
    bad = R._run(c, d, words, torch.float64, mutant)
    over = {k: R.excess(bad[k], ref, r32) for k, (ref, r32) in y.items()}
    flagged = sorted(k for k, v in over.items() if v > 1.0)
    print(c.name, mutant, "flagged on", flagged)
    assert all(not k.startswith("fwd.") for k in flagged), flagged
    if mutant == "dqd_share0_only" and c.Tc == 1:
        assert max(over.values()) <= 1e-6, over                     # (float64 rounding of the restated attention, no more)
        return
    assert flagged, f"{c.name} {mutant}: within the bound on every tensor (worst {max(over.values()):.3g})"


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
