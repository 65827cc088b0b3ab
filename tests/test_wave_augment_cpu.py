"""CPU: the host half of augmenting batches formed from waveforms (acvae_amd/augment.py: Augment.draw_shape, AugmentPlan,
window_table / apply_plans' validation; acvae_amd/frontend.py: Augmented and the refusals around it).  draw_shape is held
against Augment.draw on the reference golden's configs, clips and seeds: the same record, the same cropped clip through
source_rows(), the same generator states."""
import random

import numpy as np
import pytest
import torch

from acvae_amd import _lib
from acvae_amd import augment as A
from acvae_amd import batch as B
from acvae_amd import evaluate as EV
from acvae_amd import frontend as FE
from conftest import load_golden
from test_augment_cpu import golden_augment, golden_clips, golden_configs


def cropped(clip, plan):
    """The clip after the plan's crops, before its final roll: the gather by source_rows() with that roll undone."""
    return np.roll(clip[plan.source_rows()], -plan.params.shift, axis=0)


def chain_by_hand(x, steps):
    """np.roll and slicing, one op at a time: steps are ("roll", shift) and ("crop", start, size)."""
    for st in steps:
        x = np.roll(x, st[1], axis=0) if st[0] == "roll" else x[st[1]:st[1] + st[2]]
    return x


def test_defines_are_visible():
    assert int(_lib._defs["ACVAE_AUG_MAX_WINDOWS"]) == A.MAX_WINDOWS == 4
    assert int(_lib._defs["ACVAE_AUG_WINDOW_TABLE_WIDTH"]) == A.WINDOW_TABLE_WIDTH == A.TABLE_WIDTH + 2 + 3 * A.MAX_WINDOWS == 49
    assert "acvae_augment_window" in _lib.PROTOS and len(_lib.PROTOS["acvae_augment_window"][1]) == 10


def test_draw_shape_makes_the_draws_of_draw_on_the_reference_configs():
    g = load_golden("augment_ref")
    cl = golden_clips(g)
    F = int(g["F"])
    seen = {"crop": 0, "no crop": 0, "fold": 0, "shift": 0, "time": 0, "freq": 0}
    for k, spec in golden_configs(g):
        seed = int(g[f"c{k}_seed"])
        random.seed(seed); np.random.seed(seed)
        aug = golden_augment(spec)
        drawn = [aug.draw(c) for c in cl]
        ends = random.random(), np.random.random()
        random.seed(seed); np.random.seed(seed)
        plans = [aug.draw_shape(len(c), F) for c in cl]
        assert (random.random(), np.random.random()) == ends, f"config {k} {spec}: the generators end in another state"
        for i, ((feat, rec), plan) in enumerate(zip(drawn, plans)):
            assert isinstance(plan, A.AugmentPlan) and not isinstance(plan, A.AugmentParams)
            assert plan.params == rec and plan.src_length == len(cl[i]), (k, i)
            assert plan.source_rows().dtype == np.int64
            assert np.array_equal(cropped(cl[i], plan), feat), f"config {k} {spec} clip {i}: another crop"
            has_crop = any(op[0] == "crop" for op in aug.ops)
            seen["crop"] += len(plan.windows) > 0
            seen["no crop"] += has_crop and not plan.windows and len(cl[i]) > 1000
            seen["fold"] += any(w[1] != 0 for w in plan.windows)
            seen["shift"] += rec.shift != 0
            seen["time"] += len(rec.time_masks)
            seen["freq"] += len(rec.freq_masks)
    assert all(seen.values()), seen          # a roll in front of a crop, a crop that fires, one that does not


def test_roll_in_front_of_a_crop_is_the_window_shift():
    x = np.arange(1200 * 4, dtype=np.float32).reshape(1200, 4)
    aug = A.Augment([A.Augment.roll(0, 10), A.Augment.crop(1000, 1.0)], timemask=False, freqmask=False)
    folded = 0
    for seed in range(20):
        random.seed(seed); np.random.seed(seed)
        feat, rec = aug.draw(x)
        ends = random.random(), np.random.random()
        random.seed(seed); np.random.seed(seed)
        plan = aug.draw_shape(1200, 4)
        assert (random.random(), np.random.random()) == ends
        assert plan.params == rec and len(plan.windows) == 1 and plan.windows[0][2] == 1200
        assert np.array_equal(x[plan.source_rows()], feat)
        folded += plan.windows[0][1] != 0
    assert folded


def test_chains_of_rolls_and_crops_against_numpy_step_by_step():
    x = np.arange(500 * 4, dtype=np.float32).reshape(500, 4)
    ops = [A.Augment.roll(0, 60), A.Augment.crop(300, 1.0), A.Augment.roll(0, 60), A.Augment.crop(120, 1.0),
           A.Augment.roll(5, 40)]
    aug = A.Augment(ops, timemask=False, freqmask=False)
    for seed in range(12):
        random.seed(seed); np.random.seed(seed)
        steps, L = [], 500
        for op in ops:                                       # the draws, restated
            if op[0] == "roll":
                steps.append(("roll", int(np.random.normal(op[1], op[2]))))
            else:
                random.random()
                steps.append(("crop", int(np.random.randint(0, L - op[1])), op[1]))
                L = op[1]
        random.random()
        random.seed(seed); np.random.seed(seed)
        plan = aug.draw_shape(500, 4)
        assert [w[2] for w in plan.windows] == [500, 300] and plan.params.length == 120
        assert all(0 <= w[1] < w[2] for w in plan.windows)
        assert np.array_equal(x[plan.source_rows()], chain_by_hand(x, steps)), seed
        feat, rec = aug_draw(aug, x, seed)
        assert rec == plan.params and np.array_equal(cropped(x, plan), feat)
    # four crops at the most
    A.Augment([A.Augment.crop(10, 1.0)] * A.MAX_WINDOWS)
    with pytest.raises(ValueError, match="crops"):
        A.Augment([A.Augment.crop(10, 1.0)] * (A.MAX_WINDOWS + 1))
    random.seed(0); np.random.seed(0)
    plan = A.Augment([A.Augment.crop(s, 1.0) for s in (400, 300, 200, 100)], p=0.0).draw_shape(500, 4)
    assert len(plan.windows) == 4 and plan.params.length == 100
    rows = plan.source_rows()
    assert np.array_equal(rows, np.arange(100) + sum(w[0] for w in plan.windows))


def aug_draw(aug, x, seed):
    random.seed(seed); np.random.seed(seed)
    return aug.draw(x)


def test_short_clip_raises_like_randrange():
    aug = A.Augment(p=1.0, T=30, freqmask=False)
    with pytest.raises(ValueError):
        for seed in range(50):
            random.seed(seed)
            aug.draw_shape(3, 64)


def test_nothing_drawn_is_the_identity_plan():
    random.seed(5); np.random.seed(5)
    fourth, first_np = [random.random() for _ in range(4)][3], np.random.random()
    random.seed(5); np.random.seed(5)
    aug = A.parse_augments([])
    for _ in range(3):
        plan = aug.draw_shape(50, 64)
        assert plan == A.AugmentPlan(50, [], A.AugmentParams(50))
        assert np.array_equal(plan.source_rows(), np.arange(50))
    assert random.random() == fourth and np.random.random() == first_np
    assert A.batch_params([None, None, None, (plan,), None, None]) is None        # never taken for a record column


def good_plan():
    return A.AugmentPlan(40, [(5, 3, 40), (2, 0, 20)], A.AugmentParams(10, 4, [(0, 3)], [(1, 2)]))


def test_window_table_layout():
    tab, out_lens = A.window_table([good_plan(), A.AugmentPlan(7, [], A.AugmentParams(7))], [40, 7], 41, 64)
    assert tab.shape == (2, A.WINDOW_TABLE_WIDTH) and tab.dtype == np.int32 and list(out_lens) == [10, 7]
    W = A.TABLE_WIDTH
    assert list(tab[0, :5]) == [4, 1, 1, 0, 3] and list(tab[0, W:W + 8]) == [10, 2, 5, 3, 40, 2, 0, 20]
    assert list(tab[1, W:W + 2]) == [7, 0] and not tab[1, W + 2:].any()
    # the leading columns are table()'s for the cropped clips
    assert np.array_equal(tab[:, :W], A.table([good_plan().params, A.AugmentParams(7)], [10, 7], 10, 64))


BAD_PLANS = {
    "source length": (lambda p: setattr(p, "src_length", 39), None),
    "window length": (lambda p: p.windows.__setitem__(0, (5, 3, 39)), None),
    "window beyond the unrolled clip": (lambda p: p.windows.__setitem__(1, (11, 0, 20)), None),
    "start outside": (lambda p: p.windows.__setitem__(0, (40, 3, 40)), None),
    "negative start": (lambda p: p.windows.__setitem__(0, (-1, 3, 40)), None),
    "shift outside": (lambda p: p.windows.__setitem__(0, (5, 40, 40)), None),
    "window larger than its clip": (lambda p: p.windows.__setitem__(1, (2, 0, 41)), None),
    "too many windows": (lambda p: p.windows.extend([(0, 0, 10)] * 3), None),
    "record longer than the last window's clip": (lambda p: setattr(p.params, "length", 21), None),
    "record length without windows": (None, lambda p: A.AugmentPlan(40, [], A.AugmentParams(39))),
    "final shift": (lambda p: setattr(p.params, "shift", 10), None),
    "time mask": (lambda p: setattr(p.params, "time_masks", [(3, 11)]), None),
    "freq mask": (lambda p: setattr(p.params, "freq_masks", [(60, 65)]), None),
    "too many masks": (lambda p: setattr(p.params, "freq_masks", [(0, 1)] * 9), None),
    "not a plan": (None, lambda p: p.params),
    "no record": (lambda p: setattr(p, "params", None), None),
}


@pytest.mark.parametrize("what", sorted(BAD_PLANS))
def test_apply_plans_validates_before_any_launch(what):
    """A CPU tensor: the ValueError of validation comes before the RuntimeError of a batch that is not on the device."""
    x = torch.zeros(1, 41, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_plans(x, [40], [good_plan()])                   # the good plan passes validation
    edit, swap = BAD_PLANS[what]
    plan = good_plan()
    if edit is not None:
        edit(plan)
    if swap is not None:
        plan = swap(plan)
    with pytest.raises(ValueError):
        A.apply_plans(x, [40], [plan])
    with pytest.raises(ValueError):
        A.window_table([plan], [40], 41, 64)


def test_apply_plans_validates_the_batch():
    p = good_plan()
    for x, lens, plans in [
        (torch.zeros(1, 41, 64), [40, 40], [p]),                                   # count
        (torch.zeros(1, 41, 64), [40], [p, p]),
        (torch.zeros(1, 39, 64), [40], [p]),                                       # longer than T
        (torch.zeros(1, 41, 62), [40], [p]),                                       # F % 4
        (torch.zeros(1, 41, A.MAX_F + 4), [40], [p]),
        (torch.zeros(1, 41, 64, dtype=torch.float64), [40], [p]),
        (torch.zeros(41, 64), [40], [p]),
    ]:
        with pytest.raises(ValueError):
            A.apply_plans(x, lens, plans)


def augmented():
    return FE.LogMel.panns_32k().augmented(A.parse_augments(["randomcrop", "timeroll", "timemask", "freqmask"]))


def test_augmented_is_a_front_end_for_training_only():
    fe = FE.LogMel.panns_32k()
    aug = A.parse_augments(["timeroll"])
    afe = fe.augmented(aug)
    assert isinstance(afe, FE.Augmented) and afe.frontend is fe and afe.augment is aug and afe.last_plans is None
    assert afe.sample_rate == 32000
    rs = fe.at_input_rate(44100).augmented(aug)
    assert isinstance(rs, FE.Augmented) and isinstance(rs.frontend, FE.Resampled) and rs.sample_rate == 44100
    pcm = torch.tensor([-32768, 16384], dtype=torch.int16)
    assert torch.equal(afe.to_float(pcm), fe.to_float(pcm))
    waves, lens = afe.check(np.zeros((2, 4000), np.float32), [4000, 3000])
    assert isinstance(waves, torch.Tensor) and list(lens) == [4000, 3000]
    with pytest.raises(ValueError):
        afe.check(np.zeros((2, 4000), np.float32), [4000, 100])                    # the inner front end's own check
    with pytest.raises(ValueError, match="spectrogram"):
        afe(torch.zeros(1, 4000), [4000], spectrogram=True)
    with pytest.raises(ValueError):
        FE.Augmented(afe, aug)
    with pytest.raises(ValueError):
        FE.Augmented(fe, [A.AugmentParams(3)])


def test_evaluation_refuses_an_augmented_front_end():
    from acvae_amd.ensemble import ensemble_evaluate
    afe = augmented()
    items = [("a", torch.zeros(4000))]
    with pytest.raises(ValueError, match="never augments"):
        EV.evaluate(None, items, None, frontend=afe)
    with pytest.raises(ValueError, match="never augments"):
        ensemble_evaluate([], items, None, frontend=afe)
    for mode in ("eval", "validation"):
        with pytest.raises(ValueError, match="never augments"):
            B.forward_batch(None, [["a"], torch.zeros(1, 4000), [4000]], mode, frontend=afe, method="greedy", beam_size=1)
    with pytest.raises(ValueError, match="never augments"):
        B.forward_batch_shared_encoder(None, [["a"], torch.zeros(1, 4000), [4000]], frontend=afe, method="greedy", beam_size=2)


def test_frontend_with_augment_records_stays_refused():
    from acvae_amd.trainer import TrainStep
    afe = augmented()
    records = [A.AugmentParams(13)]
    with pytest.raises(ValueError, match="augment"):
        TrainStep.step(None, torch.zeros(1, 4000), [4000], None, None, augment=records, frontend=afe)
    with pytest.raises(ValueError, match=r"augmented\("):
        FE.refuse_augment(records)
    batch = [torch.zeros(1, 4000), torch.zeros(1, 3), ["a"], tuple(records), [4000], [3]]
    for kw in ({}, {"augment": records}):
        with pytest.raises(ValueError, match="augment"):
            B.forward_batch(None, list(batch), "train", device="cpu", frontend=afe, **kw)
