"""CPU: one encoder pass shared by a clip's captions in the training step - what can be checked without a GPU: the two new
entry points (acvae_rows_gather / acvae_rows_fold) are exported and refuse bad arguments before any launch, the ABI version
is unchanged, the batch source (CaptionGroupSampler, CaptionGroupDataset, collate_groups) draws one item per clip with k
distinct captions and fetches every feature once, and ``clip_index`` is validated before any library call."""
import random

import numpy as np
import pytest
import torch

from acvae_amd import _lib, batch as B, dataset as DS
from acvae_amd.augment import Augment, AugmentParams


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.lib()
    assert "acvae_rows_gather" in _lib.PROTOS and "acvae_rows_fold" in _lib.PROTOS
    assert hasattr(lib, "acvae_rows_gather") and hasattr(lib, "acvae_rows_fold")
    assert lib.acvae_abi_version() == 3


def test_new_entry_points_refuse_null_pointers_and_bad_dimensions():
    lib = _lib.lib()
    f = torch.zeros(256)
    i64 = torch.zeros(64, dtype=torch.long)
    i32 = torch.zeros(64, dtype=torch.int32)
    p, q, r = f.data_ptr(), i64.data_ptr(), i32.data_ptr()       # host memory: every refusal below comes before any launch
    assert p % 16 == 0
    assert lib.acvae_rows_gather(None, None, None, 2, 4, 64, None) == -1
    assert lib.acvae_rows_fold(None, None, None, None, 2, 4, 64, None) == -1
    for args in ((None, q, p), (p, None, p), (p, q, None)):
        assert lib.acvae_rows_gather(*args, 2, 4, 64, None) == -1
    for args in ((None, r, r, p), (p, None, r, p), (p, r, None, p), (p, r, r, None)):
        assert lib.acvae_rows_fold(*args, 2, 4, 64, None) == -1
    for dims in ((2, 4, 62), (2, 4, 0), (2, 4, -4), (2, 0, 64), (2, -1, 64), (0, 4, 64), (-3, 4, 64)):    # (B, N, R)
        assert lib.acvae_rows_gather(p, q, p, *dims, None) == -1, dims
        assert lib.acvae_rows_fold(p, r, r, p, *dims, None) == -1, dims
    # a float pointer that is not 16-byte aligned: refused as well (ACVAE_EALIGN), still without a launch
    assert lib.acvae_rows_gather(p + 4, q, p, 2, 4, 64, None) == -2
    assert lib.acvae_rows_fold(p, r, r, p + 4, 2, 4, 64, None) == -2


# ---------------------------------------------------------------- the batch source
class _Voc:
    def __call__(self, w):
        return {"<start>": 1, "<end>": 2}.get(w, 3 + len(w))


class _Reader:
    """audio_id -> feature, counting the calls"""

    def __init__(self, lens):
        self.calls = []
        self.feats = {f"clip{n}": np.random.RandomState(n).randn(L, 8).astype(np.float32) for n, L in enumerate(lens)}

    def __call__(self, audio_id):
        self.calls.append(audio_id)
        return self.feats[audio_id]


def _info(ncaps):
    return [{"audio_id": f"clip{n}", "captions": [{"tokens": " ".join(["w" * (1 + (n + c) % 4)] * (1 + (2 * n + 3 * c) % 6))}
                                                  for c in range(k)]} for n, k in enumerate(ncaps)]


def test_group_sampler_visits_every_clip_once_with_k_distinct_captions():
    info = _info([5, 3, 4, 5, 3, 6])
    ds = DS.CaptionGroupDataset(_Reader([9] * 6), info, _Voc())
    assert len(ds) == 6
    for k in (1, 2, 3):
        sampler = DS.CaptionGroupSampler(ds, k, shuffle=True)
        assert len(sampler) == 6
        random.seed(7)
        epoch = list(sampler)
        assert sorted(a for a, _ in epoch) == list(range(6))
        for a, caps in epoch:
            assert len(caps) == k and len(set(caps)) == k and all(0 <= c < len(info[a]["captions"]) for c in caps)
        random.seed(7)
        assert list(sampler) == epoch                                  # a seeded epoch is repeatable
        assert any(list(sampler) != epoch for _ in range(4))           # ... and the next epochs draw again
    unshuffled = [a for a, _ in DS.CaptionGroupSampler(ds, 2)]
    assert unshuffled == list(range(6))
    assert [a for a, _ in DS.CaptionGroupSampler(ds, 3, audio_subset_indices=[4, 1])] == [4, 1]
    with pytest.raises(ValueError, match="fewer than caps_per_clip=4"):
        DS.CaptionGroupSampler(ds, 4)
    DS.CaptionGroupSampler(ds, 4, audio_subset_indices=[0, 2, 3, 5])   # the clips with too few captions are not in the subset
    with pytest.raises(ValueError, match="at least 1"):
        DS.CaptionGroupSampler(ds, 0)


def test_group_items_fetch_the_feature_once_and_collate_into_a_shared_batch():
    lens = [9, 12, 7]
    info = _info([4, 4, 4])
    reader = _Reader(lens)
    voc = _Voc()
    ds = DS.CaptionGroupDataset(reader, info, voc)
    picks = [(0, (2, 0, 3)), (1, (1, 3, 0)), (2, (0, 1, 2))]
    items = [ds[p] for p in picks]
    assert reader.calls == ["clip0", "clip1", "clip2"]                  # one fetch per clip, not one per caption
    for (a, cs), (feat, caps, key) in zip(picks, items):
        assert key == f"clip{a}" and torch.equal(feat, torch.from_numpy(reader.feats[key])) and len(caps) == 3
        for c, cap in zip(cs, caps):
            toks = info[a]["captions"][c]["tokens"].split()
            assert cap.tolist() == [1] + [voc(t) for t in toks] + [2]
    batch = B.collate_groups()(list(items))
    feats, caps, keys, clip_index, feat_lens, cap_lens = batch
    assert len(batch) == 6 and tuple(feats.shape) == (3, 12, 8) and feats.dtype == torch.float32
    assert list(feat_lens) == lens                                      # the clips keep the items' order
    assert tuple(caps.shape) == (9, int(max(cap_lens))) and len(cap_lens) == len(keys) == len(clip_index) == 9
    assert list(cap_lens) == sorted(cap_lens, reverse=True) and len(set(cap_lens)) > 1
    assert clip_index.dtype == np.int64 and np.array_equal(np.bincount(clip_index), [3, 3, 3])
    seen = {0: [], 1: [], 2: []}
    for r in range(9):
        c = int(clip_index[r])
        assert keys[r] == f"clip{c}"
        row = caps[r, :cap_lens[r]].long().tolist()
        assert not caps[r, cap_lens[r]:].any()
        seen[c].append(row)
        assert torch.equal(feats[c, :lens[c]], torch.from_numpy(reader.feats[keys[r]]))
    for c, item in enumerate(items):                                    # every caption of every clip arrived, with its clip
        assert sorted(seen[c]) == sorted(cap.tolist() for cap in item[1])
    # clips that carry different numbers of captions are refused
    with pytest.raises(ValueError, match="same number"):
        B.collate_groups()([items[0], (items[1][0], items[1][1][:2], items[1][2])])
    with pytest.raises(ValueError, match="same number"):
        B.collate_groups()([(items[0][0], [], items[0][2])])


def test_group_items_draw_the_augmentation_once_per_clip():
    reader = _Reader([40, 30])
    aug = Augment([Augment.crop(size=16, p=1.0), Augment.roll()], T=4, F=3, p=1.0)
    ds = DS.CaptionGroupDataset(reader, _info([3, 3]), _Voc(), augment=aug)
    random.seed(3); np.random.seed(3)
    items = [ds[(0, (0, 1, 2))], ds[(1, (2, 0, 1))]]
    assert reader.calls == ["clip0", "clip1"]
    random.seed(3); np.random.seed(3)
    want = [aug.draw(reader.feats[k]) for k in ("clip0", "clip1")]      # exactly one draw per clip, in item order
    for item, (feat, params) in zip(items, want):
        assert len(item) == 4 and isinstance(item[3], AugmentParams) and item[3] == params
        assert tuple(item[0].shape) == (16, 8) and np.array_equal(item[0].numpy(), feat)
    batch = B.collate_groups()(list(items))
    assert len(batch) == 7 and batch[3] == (items[0][3], items[1][3])    # the B clips' records, where batch_params looks
    from acvae_amd.augment import batch_params
    assert batch_params(batch) == batch[3]
    assert len(batch[4]) == 6 and list(batch[-2]) == [16, 16] and len(batch[-1]) == 6


# ---------------------------------------------------------------- clip_index validation (before any library call)
def _cpu_model(V=20, E=64):
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0, num_layers=1,
                                    rnn_type="GRU", attn_size=E)
    return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid",
                           posterior_args={"hidden_size": E, "dropout": 0.0}, prior_model="PriorRNN",
                           prior_args={"hidden_size": E, "dropout": 0.0})


def test_clip_rows_builds_the_lists_the_kernels_read():
    from acvae_amd.vae_model import clip_rows
    idx, offsets, rows, k = clip_rows([2, 0, 1, 1, 0, 2], 3, 6)
    assert idx.dtype == np.int64 and offsets.dtype == np.int32 and rows.dtype == np.int32 and k == 2
    assert idx.tolist() == [2, 0, 1, 1, 0, 2] and offsets.tolist() == [0, 2, 4, 6] and rows.tolist() == [1, 4, 2, 3, 0, 5]
    assert clip_rows(torch.tensor([1, 0]), 2, 2)[3] == 1
    assert clip_rows(np.array([0, 0, 0], dtype=np.int32), 1, 3)[1].tolist() == [0, 3]


@pytest.mark.parametrize("clip_index,why", [
    ([0, 1, 2, 0, 1], "one entry per caption row"),                    # N - 1 entries
    ([[0, 1, 2], [0, 1, 2]], "one entry per caption row"),             # not one-dimensional
    ([0, 1, 2, 0, 1, 3], r"must lie in \[0, 3\)"),
    ([0, 1, 2, 0, 1, -1], r"must lie in \[0, 3\)"),
    ([0.0, 1.0, 2.0, 0.0, 1.0, 2.0], "integer array"),
    ([True, False, True, False, True, False], "integer array"),
    ([0, 1, 2, 0, 1, 1], "equal multiplicities"),                      # clip 1 three times, clip 2 once
    ([0, 0, 0, 1, 1, 1], "equal multiplicities"),                      # clip 2 never
])
def test_model_refuses_a_bad_clip_index_before_any_library_call(clip_index, why):
    model = _cpu_model()
    feats = torch.zeros(3, 64, 64)                                     # CPU tensors: a library call would raise RuntimeError
    caps = torch.ones(6, 5)
    with pytest.raises(ValueError, match=why):
        model(feats, np.array([64, 64, 48]), caps, np.array([5, 5, 4, 4, 3, 3]), ss_ratio=1.0, dis_ratio=0,
              clip_index=np.asarray(clip_index))


def test_clip_index_belongs_to_the_training_forward_and_trainstep_passes_it_on():
    import inspect
    from acvae_amd.trainer import TrainStep
    model = _cpu_model()
    with pytest.raises(ValueError, match="training forward"):
        model(torch.zeros(3, 64, 64), np.array([64, 64, 48]), method="greedy", clip_index=[0, 1, 2])
    for fn in (TrainStep.step, TrainStep.forward_loss, B.forward_batch):
        assert inspect.signature(fn).parameters["clip_index"].default is None
    seen = {}

    class _Spy(torch.nn.Module):
        def forward(self, *a, **k):
            seen.update(k)
            raise KeyboardInterrupt

    ts = TrainStep.__new__(TrainStep)
    ts.model = _Spy()
    with pytest.raises(KeyboardInterrupt):
        ts.forward_loss(None, None, None, None, clip_index=[0, 0])
    assert seen["clip_index"] == [0, 0]
    seen.clear()
    with pytest.raises(KeyboardInterrupt):
        ts.forward_loss(None, None, None, None)
    assert "clip_index" not in seen                                     # the plain step calls the model as it always did
