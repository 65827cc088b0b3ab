"""CPU: the float64 reference of the fp32 encoders (tests/encoder_ref.py) and its yardstick, before any GPU is asked.

- every case of tests/test_encoder_composite_gpu.py is admissible: under the float64 run's own ReLU decisions the fp32
  reference's distance from it (alt) has a median over the gradient tensors of at most 5e-5, a tenth of
  parity_util.grads_match_oracle's tol_enc = 5e-4 (the criterion tests/test_shared_encoder_gpu.py uses for its seed), so
  MARGIN x the yardstick stays well inside today's bound on the typical tensor.  test_zz_admissibility_table prints median
  and max alt per case;
- the bound is not vacuous: each PLANT of tests/encoder_ref.py (one defect in the oracle's BatchNorm) is flagged - its worst
  ratio exceeds the family's MARGIN - while its plain relative L2 stays under today's 2e-4 on EVERY tensor, so no
  fp32-oracle test of the suite would have seen it; the clean fp32 reference of the same case has ratio <= 1 everywhere;
- the float64 reference of a training case is the same from two calls (its dropout masks are inputs, not draws)."""
import os
import statistics

import pytest
import torch

import encoder_ref as E

TABLE = {}
REFS = {}
for _c in E.CASES:
    REFS.setdefault(_c.ref_key(), _c)
REFS = list(REFS.values())


@pytest.fixture(autouse=True)
def threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.mark.parametrize("case", REFS, ids=[c.name for c in REFS])
def test_case_is_admissible(case):
    y = E.yardstick(case)
    grads = E.gradient_keys(y)
    alts = [y[k][1] for k in grads]
    med, top = statistics.median(alts), max(alts)
    TABLE[case.name] = (med, top, max(y, key=lambda k: y[k][1]))
    print(f"{case.name}: median alt {med:.2e}, max {top:.2e} over {len(grads)} gradient tensors")
    assert all(bool(torch.isfinite(ref).all()) and alt == alt for ref, alt in y.values()), case.name
    assert med <= E.ADMISSIBLE, f"{case.name}: median alt {med:.2e}; choose another B or seed"
    assert E.floor_of(y) == med
    head = E.HEAD[case.arch]
    assert {"audio_embeds", "audio_embeds_pooled", "bn0.weight", "bn0.bias"} <= set(y) and not any(k.startswith(head) for k in y)
    assert len(grads) == {"Cnn10": 26, "Cnn14_16k": 38, "ResNet38": 119}[case.arch]
    stats = [k for k in y if k.endswith(("running_mean", "running_var"))]
    assert len(stats) == (0 if case.mode == "eval" else {"Cnn10": 18, "Cnn14_16k": 26, "ResNet38": 80}[case.arch])
    assert tuple(y["audio_embeds"][0].shape) == (case.B, case.T // E.DIV[case.arch], E.WIDTH[case.arch])


def test_zz_admissibility_table():
    """Prints median and max alt per case (runs last, over whatever cases ran before it)."""
    for name, (med, top, worst) in TABLE.items():
        print(f"{name:30s} median {med:.2e}  max {top:.2e}  (largest alt of any tensor: {worst})")
    assert all(med <= E.ADMISSIBLE for med, _, _ in TABLE.values())


def test_case_table_covers_the_driver_branches():
    by = lambda arch, **kw: {(c.B, c.T) for c in E.CASES if c.arch == arch and all(getattr(c, k) == v for k, v in kw.items())}
    assert by("Cnn10", mode="train", route="default", hooked=False) == {(1, 16), (3, 47), (2, 96), (2, 250), (5, 40), (33, 16)}
    assert by("Cnn10", mode="eval", route="default") == by("Cnn10", mode="train_p0") == {(1, 16), (3, 47), (2, 96)}
    assert {(c.B, c.T, c.mode) for c in E.CASES if c.arch == "Cnn10" and c.route == "igemm"} == {(3, 47, "train"), (2, 96, "eval")}
    assert [(c.B, c.T, c.mode) for c in E.CASES if c.hooked] == [(2, 96, "train")]
    assert by("Cnn14_16k", mode="train", route="default") >= {(4, 64), (2, 95), (4, 128)}
    assert by("Cnn14_16k", mode="eval") >= {(4, 64), (2, 95), (4, 128)}
    assert {c.mode for c in E.CASES if c.arch == "Cnn14_16k" and c.T == 32} == {"train", "eval"}
    assert by("Cnn14_16k", route="igemm") == {(4, 64)}
    assert by("ResNet38", mode="train") == by("ResNet38", mode="eval") == {(2, 64), (3, 72)}
    # a case that is called another way shares its reference with a plain one
    keys = {c.ref_key() for c in E.CASES if c.route == "default" and not c.hooked}
    assert all(c.ref_key() in keys for c in E.CASES)


# The case each PLANT is shown at.  eval_eps: the evaluation-mode cases; the two conv_block1 plants: B = 2, T = 96, where that
# block's BatchNorm count is 12288 and 1 / count = 8e-5 lies under today's 2e-4.
PLANT_CASES = {"eval_eps": ("cnn10-B2_T96-eval", "cnn10-B3_T47-eval"), "no_bessel": ("cnn10-B2_T96-train",),
               "bwd_count": ("cnn10-B2_T96-train",)}


def test_every_plant_is_listed():
    assert set(PLANT_CASES) == set(E.PLANTS)


@pytest.mark.parametrize("plant,name", [(p, n) for p, names in PLANT_CASES.items() for n in names])
def test_the_bound_flags_the_plant_and_todays_does_not(plant, name):
    case = E.CASES[E.CASE_IDS.index(name)]
    y, zs = E.yardstick_z(case)
    masks = [z > 0 for z in zs]             # the float64 run's own decisions, for the clean and the planted fp32 run alike
    good = E.ratio(E.reference(case, masks, torch.float32), case, y=y)
    assert max(good.values()) <= 1.0 + 1e-9, max(good, key=good.get)      # (alt / max(alt, floor))
    with E.planted(plant):
        bad = E.reference(case, masks, torch.float32)
    ratios = E.ratio(bad, case, y=y)
    plain = {k: E.rel_l2(bad[k], ref) for k, (ref, _) in y.items()}
    flagged = sorted(k for k, r in ratios.items() if r > E.MARGIN[case.arch])
    worst, wp = max(ratios, key=ratios.get), max(plain, key=plain.get)
    print(f"{plant} at {name}: worst ratio {ratios[worst]:.1f} ({worst}), {len(flagged)} of {len(ratios)} tensors flagged; "
          f"largest plain relative L2 {plain[wp]:.2e} ({wp}), today's bound {E.TODAY[case.arch]:.0e}")
    assert flagged, f"{plant}: within {E.MARGIN[case.arch]} x the yardstick on every tensor (worst {ratios[worst]:.2f})"
    assert plain[wp] < E.TODAY[case.arch], f"{plant}: today's bound sees it already ({wp}: {plain[wp]:.2e})"
    if plant == "no_bessel":
        assert all(k.endswith("running_var") and k.startswith(E.PLANT_LAYER) for k in flagged), flagged
    else:                                                 # the forward is the clean one
        assert not any(k.startswith("audio_embeds") or k.endswith(("running_mean", "running_var")) for k in flagged), flagged


def test_float64_reference_is_reproducible():
    case = E.CASES[E.CASE_IDS.index("cnn10-B3_T47-train")]
    a, b = E.reference(case), E.reference(case)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert E.inputs(case)["masks"] is not None and len(E.inputs(case)["masks"]) == 6


def test_ratio_edges():
    case = E.CASES[E.CASE_IDS.index("cnn10-B1_T16-eval")]
    y = E.yardstick(case)
    exact = {k: ref for k, (ref, _) in y.items()}
    assert max(E.ratio(exact, case, y=y).values()) == 0.0
    k = min(E.gradient_keys(y), key=lambda n: y[n][1])    # the tightest tensor: held to the floor, not to its own alt
    assert y[k][1] < 0.5 * E.floor_of(y)
    off = dict(exact)
    off[k] = exact[k] * (1 + 2 * E.floor_of(y))
    assert abs(E.ratio(off, case, y=y)[k] - 2.0) < 1e-6
    with pytest.raises(AssertionError):
        E.ratio({kk: v for kk, v in exact.items() if kk != k}, case, y=y)
    assert E.CASES[E.CASE_IDS.index("cnn10-B2_T96-train-hooked")].ref_key() == E.CASES[E.CASE_IDS.index("cnn10-B2_T96-train")].ref_key()
