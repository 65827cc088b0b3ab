"""CPU: the host half of the training-time augmentation (acvae_amd/augment.py) against the reference's own transforms
(tests/golden/augment_ref.npz, written by tools/make_augment_golden.py from datasets/augment.py): the same draws on
Python's `random` and numpy's global generator, and - through a numpy restatement of the device arithmetic - the same
outputs; parse_augments' refusals and warnings; the dataset's 4th field through collate_fn's sort."""
import json
import random
import warnings

import numpy as np
import pytest
import torch

from acvae_amd import augment as A
from acvae_amd import batch as B
from acvae_amd import dataset as D
from conftest import load_golden


def golden_clips(g):
    """tools/make_augment_golden.py:clips, restated."""
    rs = np.random.RandomState(int(g["clip_seed"]))
    F = int(g["F"])
    cl = [(np.round(rs.randn(int(L), F) * 4.0) / 4.0 - 4.0).astype(np.float32) for L in g["lengths"]]
    assert np.array_equal([c.astype(np.float64).sum() for c in cl], g["clip_sums"]), "clip recipe drifted"
    return cl


def golden_output(g, k, i, clip):
    """The reference's output for clip i of config k (tools/make_augment_golden.py:decode, restated): the clip rows it
    was taken from, with the stored values in the cells that differ."""
    out = clip[g[f"c{k}_src{i}"].astype(np.int64)].copy()
    exc = np.unpackbits(g[f"c{k}_exc{i}"])[:out.size].astype(bool).reshape(out.shape)
    out[exc] = g[f"c{k}_val{i}"]
    return out


def golden_augment(spec):
    if spec["kind"] == "spec_augment":
        return A.Augment(**spec["config"])
    return A.parse_augments(spec["config"])


def golden_configs(g):
    k = 0
    while f"c{k}_config" in g:
        yield k, json.loads(str(g[f"c{k}_config"]))
        k += 1


def restate(feat, rec):
    """The device arithmetic in numpy: np.roll by the shift, then each mask in order filled with the fp64 mean of the clip
    as it stands (rounded to fp32).  Returns the output and the boolean map of masked cells."""
    out = np.roll(np.asarray(feat, dtype=np.float32), rec.shift, axis=0).copy()
    masked = np.zeros(out.shape, dtype=bool)
    for a, b in rec.time_masks:
        out[a:b, :] = np.float32(out.astype(np.float64).mean())
        masked[a:b, :] = True
    for a, b in rec.freq_masks:
        out[:, a:b] = np.float32(out.astype(np.float64).mean())
        masked[:, a:b] = True
    return out, masked


def check_against_reference(got, ref, masked, what):
    """Outside the masks bit for bit; the fills within 1e-6 x the clip's RMS (the reference's means are numpy fp32
    pairwise sums)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[~masked], ref[~masked]), f"{what}: cells outside the masks differ"
    rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    err = np.abs(got[masked].astype(np.float64) - ref[masked].astype(np.float64))
    assert err.size == 0 or float(err.max()) <= 1e-6 * rms, f"{what}: fill error {float(err.max()):.3e} (rms {rms:.3e})"


def draw_golden(g, k, spec, cl):
    seed = int(g[f"c{k}_seed"])
    random.seed(seed)
    np.random.seed(seed)
    aug = golden_augment(spec)
    drawn = [aug.draw(c) for c in cl]
    return drawn, random.random(), np.random.random()


@pytest.fixture(scope="module")
def g():
    return load_golden("augment_ref")


def test_draws_and_outputs_match_the_reference(g):
    cl = golden_clips(g)
    seen = {"crop": 0, "fold": 0, "shift": 0, "time": 0, "freq": 0, "overlap": 0}
    for k, spec in golden_configs(g):
        drawn, nr, nn = draw_golden(g, k, spec, cl)
        assert nr == float(g[f"c{k}_next_random"]), f"config {k} {spec}: Python random state differs from the reference"
        assert nn == float(g[f"c{k}_next_np"]), f"config {k} {spec}: numpy random state differs from the reference"
        for i, (feat, rec) in enumerate(drawn):
            ref = golden_output(g, k, i, cl[i])
            assert rec.length == len(feat) == len(ref)
            got, masked = restate(feat, rec)
            check_against_reference(got, ref, masked, f"config {k} {spec} clip {i}")
            seen["crop"] += len(feat) < len(cl[i])
            seen["fold"] += len(feat) < len(cl[i]) and spec["config"][:1] == ["timeroll"]
            seen["shift"] += rec.shift != 0
            seen["time"] += len(rec.time_masks)
            seen["freq"] += len(rec.freq_masks)
            seen["overlap"] += int(masked.sum()) < sum((b - a) * feat.shape[1] for a, b in rec.time_masks) + \
                sum((b - a) * len(feat) for a, b in rec.freq_masks)
    assert all(seen.values()), seen          # the fixture exercises every path


def test_spec_augment_draws_p_for_every_clip():
    """Every switch off: spec_augment's wrapper still draws one random.random() per clip, and nothing else moves."""
    random.seed(5); np.random.seed(5)
    fourth, first_np = [random.random() for _ in range(4)][3], np.random.random()
    random.seed(5); np.random.seed(5)
    aug = A.parse_augments([])
    x = np.ones((50, 64), np.float32)
    for _ in range(3):
        feat, rec = aug.draw(x)
        assert feat is x and rec == A.AugmentParams(50)
    assert random.random() == fourth and np.random.random() == first_np


def test_roll_before_a_crop_is_folded_into_its_window():
    x = np.arange(1200 * 4, dtype=np.float32).reshape(1200, 4)
    aug = A.Augment([A.Augment.roll(0, 10), A.Augment.crop(1000, 1.0)], timemask=False, freqmask=False)
    for seed in range(20):
        random.seed(seed); np.random.seed(seed)
        shift = int(np.random.normal(0, 10))
        start = np.random.randint(0, 200)
        random.seed(seed); np.random.seed(seed)
        feat, rec = aug.draw(x)
        assert rec.shift == 0 and rec.length == 1000
        assert np.array_equal(feat, np.roll(x, shift, axis=0)[start:start + 1000])


def test_rolls_add_up_modulo_the_clip_length():
    x = np.arange(37 * 4, dtype=np.float32).reshape(37, 4)
    aug = A.Augment([A.Augment.roll(0, 30), A.Augment.crop(1000, 1.0), A.Augment.roll(0, 30)],
                    timemask=False, freqmask=False)
    random.seed(1); np.random.seed(1)
    s = int(np.random.normal(0, 30)) + int(np.random.normal(0, 30))
    random.seed(1); np.random.seed(1)
    feat, rec = aug.draw(x)
    assert feat is x and rec.shift == s % 37
    assert np.array_equal(restate(feat, rec)[0], np.roll(x, s, axis=0))


def test_parse_augments_refusals_and_warnings():
    with pytest.raises(NotImplementedError, match="torch.solve"):
        A.parse_augments(["timemask", "timewarp"])
    with pytest.raises(NotImplementedError, match="torch.solve"):
        A.Augment(timewarp=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        aug = A.parse_augments(["timemask", "mixup", "randomcrop", "specnoise", "timeroll"])
    assert sorted(str(x.message).split("'")[1] for x in w) == ["mixup", "specnoise"]
    assert aug.timemask and not aug.freqmask and [op[0] for op in aug.ops] == ["crop", "roll"]
    assert [op[0] for op in A.parse_augments(["timeroll", "randomcrop"]).ops] == ["roll", "crop"]
    A.Augment(num_timemask=8, num_freqmask=8)
    with pytest.raises(ValueError):
        A.Augment(num_timemask=9)
    with pytest.raises(ValueError):
        A.parse_augments(["freqmask"], num_freqmask=9)


def test_short_clip_raises_like_randrange():
    aug = A.Augment(p=1.0, T=30, freqmask=False)
    x = np.zeros((3, 64), np.float32)
    with pytest.raises(ValueError):
        for seed in range(50):
            random.seed(seed)
            aug.draw(x)


def test_table_validation():
    rec = A.AugmentParams(length=10, shift=3, time_masks=[(0, 4), (2, 10)], freq_masks=[(60, 64)])
    tab = A.table([rec], [10], 12, 64)
    assert tab.shape == (1, A.TABLE_WIDTH) and tab.dtype == np.int32
    assert list(tab[0, :7]) == [3, 2, 1, 0, 4, 2, 10] and list(tab[0, 3 + 2 * A.MAX_MASKS:][:2]) == [60, 64]
    bad = [
        ([rec], [11]),                                                             # record / length out of order
        ([rec, rec], [10]),                                                        # count
        ([A.AugmentParams(10, shift=10)], [10]),                                   # shift range
        ([A.AugmentParams(10, time_masks=[(5, 11)])], [10]),                       # mask beyond the clip
        ([A.AugmentParams(10, time_masks=[(5, 5)])], [10]),                        # empty mask
        ([A.AugmentParams(10, freq_masks=[(60, 65)])], [10]),                      # beyond F
        ([A.AugmentParams(10, freq_masks=[(0, 1)] * 9)], [10]),                    # too many
        ([A.AugmentParams(13)], [13]),                                             # longer than T
        ([(0, 1)], [10]),                                                          # not a record
    ]
    for params, lens in bad:
        with pytest.raises(ValueError):
            A.table(params, lens, 12, 64)


class _Voc:
    def __call__(self, w):
        return {"<start>": 1, "<end>": 2}.get(w, 3 + len(w))


def test_dataset_field_survives_collate_sort():
    info = [{"audio_id": f"a{i}", "captions": [{"tokens": " ".join(["w"] * (i % 4 + 1))}]} for i in range(6)]
    feats = {f"a{i}": np.full((40 + 300 * i, 64), float(i), np.float32) for i in range(6)}
    plain = D.CaptionDataset(feats, info, _Voc())
    assert len(plain[(0, 0)]) == 3
    ds = D.CaptionDataset(feats, info, _Voc(), augment=A.Augment([A.Augment.crop(1000, 1.0)], p=1.0, T=20, F=10))
    random.seed(3); np.random.seed(3)
    items = [ds[(i, 0)] for i in range(6)]
    batch = B.collate_fn([0, 1], 1)(list(items))
    assert len(batch) == 6 and isinstance(batch[3], tuple) and A.batch_params(batch) is batch[3]
    assert A.batch_params(B.collate_fn([0, 1], 1)([plain[(i, 0)] for i in range(6)])) is None
    for n, (key, rec) in enumerate(zip(batch[2], batch[3])):
        i = int(key[1:])
        assert rec is items[i][3] and rec.length == int(batch[-2][n]) == min(40 + 300 * i, 1000)
        assert bool((batch[0][n, :rec.length] == float(i)).all())
    assert list(batch[-1]) == sorted(batch[-1], reverse=True)
    A.table(batch[3], batch[-2], batch[0].shape[1], 64)
