"""Training-time augmentation of a config's ``augments`` list (``utils/train_util.py:92-114``, ``datasets/augment.py``):
``"randomcrop"``, ``"timeroll"``, ``"timemask"`` and ``"freqmask"``.

The work is split the way the package splits every training-time random draw: the host makes the reference's draws,
one for one and in the reference's order, on Python's ``random`` and numpy's global generator (``Augment.draw``, a few
dozen calls per clip whatever its length), and the arithmetic runs on the uploaded batch in one HIP kernel
(``apply`` -> ``acvae_spec_augment``) on the training step's stream.

How the transforms are split:
  * the crop is a host slice, so the lengths ``collate_fn`` pads with are already the cropped ones;
  * a roll that comes before a crop that fires is folded into the crop's (circular) window, a host copy of at most
    ``size`` rows;
  * every other roll is a device shift modulo the clip's own length (several rolls add up);
  * the masks of ``spec_augment`` (always last, as in the reference) are device work: each fills its region with the
    mean of the clip as it stands just before it.
"""
import random
import warnings
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_MASKS = int(_lib._defs["ACVAE_AUG_MAX_MASKS"])
TABLE_WIDTH = int(_lib._defs["ACVAE_AUG_TABLE_WIDTH"])
MAX_F = int(_lib._defs["ACVAE_AUG_MAX_F"])
assert TABLE_WIDTH == 3 + 4 * MAX_MASKS


@dataclass
class AugmentParams:
    """What ``Augment.draw`` decided for one clip, beyond the host crop: ``length`` is the clip's length after the crop,
    ``shift`` the device roll in [0, length), ``time_masks`` / ``freq_masks`` the non-empty ``[start, end)`` masks in the
    order the reference applies them."""
    length: int
    shift: int = 0
    time_masks: List[Tuple[int, int]] = field(default_factory=list)
    freq_masks: List[Tuple[int, int]] = field(default_factory=list)


def _masks(n_cells, width, num, masks):
    """datasets/augment.py time_mask / freq_mask (:30-62), draws only: ``width`` is the reference's T or F, ``n_cells``
    the clip's length or number of channels.  ``randrange`` raises ValueError where the clip is too short, as there."""
    for _ in range(num):
        t = random.randrange(0, width)
        start = random.randrange(0, n_cells - t)
        if t == 0:                                 # the reference returns here: no more masks of this kind
            return
        end = random.randrange(start, start + t)
        if end > start:                            # an empty mask writes nothing and changes no later mean
            masks.append((start, end))


class Augment:
    """The reference's transform list for one config: the crop and roll in list order (``ops``: ("crop", size, p) and
    ("roll", mean, std)), then ``spec_augment`` with the reference's keyword names and defaults.  ``timewarp`` is
    refused (see ``parse_augments``)."""

    def __init__(self, ops: Sequence[tuple] = (), timemask: bool = True, num_timemask: int = 2, freqmask: bool = True,
                 num_freqmask: int = 2, timewarp: bool = False, F: int = 15, W: int = 40, T: int = 30, p: float = 0.2):
        if timewarp:
            raise NotImplementedError(_TIMEWARP)
        for name, k in (("num_timemask", num_timemask), ("num_freqmask", num_freqmask)):
            if k > MAX_MASKS:
                raise ValueError(f"{name}={k}: at most {MAX_MASKS} masks of each kind")
        self.ops = []
        for op in ops:
            if op[0] not in ("crop", "roll") or len(op) != 3:
                raise ValueError(f"unknown augment op {op!r}")
            self.ops.append(tuple(op))
        self.timemask, self.num_timemask, self.freqmask, self.num_freqmask = timemask, num_timemask, freqmask, num_freqmask
        self.F, self.T, self.p = F, T, p

    @staticmethod
    def crop(size: int = 1000, p: float = 0.2):
        """datasets/augment.py random_crop's keywords and defaults."""
        return ("crop", size, p)

    @staticmethod
    def roll(mean: float = 0, std: float = 10):
        """datasets/augment.py time_roll's keywords and defaults."""
        return ("roll", mean, std)

    def draw(self, feature):
        """One clip ``[L, F]`` -> (the clip, possibly cropped, as a numpy array; its ``AugmentParams``).  Makes exactly the
        reference's draws in the reference's order."""
        feat = np.asarray(feature)
        shift = 0                                  # pending roll of `feat`
        for op in self.ops:
            L = feat.shape[0]
            if op[0] == "crop":                    # random_crop (:84-93)
                _, size, p = op
                if L <= size or random.random() > p:
                    continue
                start = np.random.randint(0, L - size)
                if shift % L == 0:
                    feat = feat[start:start + size]
                else:                              # roll(feat, shift)[start:start + size]: a circular window
                    feat = feat[(np.arange(start, start + size) - shift) % L]
                shift = 0
            else:                                  # time_roll (:95-103)
                _, mean, std = op
                shift += int(np.random.normal(mean, std))
        L = feat.shape[0]
        params = AugmentParams(length=L, shift=shift % L if L > 0 else 0)
        if random.random() < self.p:               # spec_augment's wrapper (:65-77) draws this for every clip
            if self.timemask and self.num_timemask > 0:
                _masks(L, self.T, self.num_timemask, params.time_masks)
            if self.freqmask and self.num_freqmask > 0:
                _masks(feat.shape[1], self.F, self.num_freqmask, params.freq_masks)
        return feat, params


_TIMEWARP = ("'timewarp' is not supported: the reference's datasets/augment.py time_warp calls sparse_image_warp, which "
             "needs torch.solve, removed from torch (it raises RuntimeError on current versions)")


def parse_augments(augment_list: Sequence[str], **spec_augment_kwargs) -> Augment:
    """utils/train_util.py:92-114: a config's ``augments`` list -> one ``Augment``.  ``"timemask"`` / ``"freqmask"`` switch
    on spec_augment's masks, ``"randomcrop"`` / ``"timeroll"`` add a crop / roll in list order, ``"timewarp"`` raises
    NotImplementedError, other names are ignored as in the reference, with a warning.  ``spec_augment_kwargs`` override
    spec_augment's other defaults (num_timemask, F, T, p, ...)."""
    kw = {"timemask": False, "freqmask": False, "timewarp": False}
    ops = []
    for name in augment_list:
        if name in ("timemask", "freqmask"):
            kw[name] = True
        elif name == "timewarp":
            raise NotImplementedError(_TIMEWARP)
        elif name == "randomcrop":
            ops.append(Augment.crop())
        elif name == "timeroll":
            ops.append(Augment.roll())
        else:
            warnings.warn(f"parse_augments: unknown augment {name!r} is ignored (as the reference ignores it)")
    kw.update(spec_augment_kwargs)
    return Augment(ops, **kw)


def table(params: Sequence[AugmentParams], feat_lens, T: int, F: int) -> np.ndarray:
    """Validate the records against the batch and build the kernel's int32 table [N, TABLE_WIDTH] (include/acvae_hip.h,
    acvae_spec_augment).  Raises ValueError on anything the kernel would have to clamp."""
    lens = np.asarray(feat_lens).reshape(-1)
    if len(params) != len(lens):
        raise ValueError(f"{len(params)} augment records for a batch of {len(lens)} clips")
    tab = np.zeros((len(lens), TABLE_WIDTH), dtype=np.int32)
    for n, (rec, L) in enumerate(zip(params, lens)):
        L = int(L)
        if not isinstance(rec, AugmentParams):
            raise ValueError(f"clip {n}: {type(rec).__name__} is not an AugmentParams")
        if not 0 <= L <= T:
            raise ValueError(f"clip {n}: length {L} outside [0, {T}]")
        if rec.length != L:
            raise ValueError(f"clip {n}: record drawn for length {rec.length}, batch length {L} (records out of order?)")
        if not (0 <= rec.shift < max(L, 1)):
            raise ValueError(f"clip {n}: shift {rec.shift} outside [0, {max(L, 1)})")
        for kind, masks, limit, col in (("time", rec.time_masks, L, 3), ("freq", rec.freq_masks, F, 3 + 2 * MAX_MASKS)):
            if len(masks) > MAX_MASKS:
                raise ValueError(f"clip {n}: {len(masks)} {kind} masks, at most {MAX_MASKS}")
            for k, (a, b) in enumerate(masks):
                if not (0 <= a < b <= limit):
                    raise ValueError(f"clip {n}: {kind} mask [{a}, {b}) outside [0, {limit})")
                tab[n, col + 2 * k], tab[n, col + 2 * k + 1] = a, b
        tab[n, 0], tab[n, 1], tab[n, 2] = rec.shift, len(rec.time_masks), len(rec.freq_masks)
    return tab


def apply(feats_d, feat_lens, params: Sequence[AugmentParams]):
    """The device half: the rolls and masks of ``params`` (one record per clip, in batch order) applied to the uploaded
    batch ``feats_d`` [N, T, F] (fp32, F % 4 == 0, F <= MAX_F) on the current stream.  Validates on the host first (ValueError, no
    launch).  Returns a new tensor; ``feats_d`` is not written."""
    _lib.require_cuda(feats_d)
    if feats_d.dim() != 3 or feats_d.dtype != torch.float32:
        raise ValueError(f"feats must be float32 [N, T, F], got {feats_d.dtype} {tuple(feats_d.shape)}")
    N, T, F = feats_d.shape
    if F % 4 != 0 or F > MAX_F:
        raise ValueError(f"feature dimension {F}: the kernel takes multiples of 4 up to {MAX_F}")
    if T * F >= 1 << 31:
        raise ValueError(f"clips of {T} x {F} cells: the kernel indexes a clip with 32-bit integers")
    tab = table(params, feat_lens, T, F)
    x = feats_d.contiguous()
    out = torch.empty_like(x)
    if N == 0:
        return out
    lens = np.asarray(feat_lens).reshape(-1).astype(np.int32)
    up = _lib.h2d(np.concatenate([lens, tab.reshape(-1)]), x.device)      # one upload: lengths, then the table
    _lib.call("acvae_spec_augment", x, out, up, up[N:], N, T, F, TABLE_WIDTH, _lib.current_stream())
    return out


def batch_params(batch):
    """The AugmentParams column of a collated training batch (``CaptionDataset(..., augment=...)``), or None."""
    if len(batch) >= 6 and isinstance(batch[3], (tuple, list)) and batch[3] and \
            all(isinstance(r, AugmentParams) for r in batch[3]):
        return batch[3]
    return None
