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

Clips that exist only on the device (features formed there from waveforms, ``acvae_amd.frontend.Augmented``) cannot be
sliced on the host.  Every draw depends on the clip's shape alone, so ``Augment.draw_shape(L, F)`` makes the same draws
without the clip and returns an ``AugmentPlan``: the crops that fired as circular windows (a pending roll folded into
each), then the ``AugmentParams`` of the cropped clip.  ``apply_plans`` -> ``acvae_augment_window`` performs the crop on
the device in front of the same rolls and masks, bit for bit what ``apply`` gives on the host-cropped clip.
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
MAX_WINDOWS = int(_lib._defs["ACVAE_AUG_MAX_WINDOWS"])
WINDOW_TABLE_WIDTH = int(_lib._defs["ACVAE_AUG_WINDOW_TABLE_WIDTH"])
assert TABLE_WIDTH == 3 + 4 * MAX_MASKS and WINDOW_TABLE_WIDTH == TABLE_WIDTH + 2 + 3 * MAX_WINDOWS


@dataclass
class AugmentParams:
    """What ``Augment.draw`` decided for one clip, beyond the host crop: ``length`` is the clip's length after the crop,
    ``shift`` the device roll in [0, length), ``time_masks`` / ``freq_masks`` the non-empty ``[start, end)`` masks in the
    order the reference applies them."""
    length: int
    shift: int = 0
    time_masks: List[Tuple[int, int]] = field(default_factory=list)
    freq_masks: List[Tuple[int, int]] = field(default_factory=list)


@dataclass
class AugmentPlan:
    """What ``Augment.draw_shape`` decided for one clip of ``src_length`` rows: ``windows``, one ``(start, shift, length)``
    per crop that fired, in order - ``length`` the clip's length in front of that crop, ``shift`` the roll pending in front
    of it (modulo ``length``), the crop keeping rows ``[start, start + size)`` of the rolled clip, circularly - and
    ``params``, the ``AugmentParams`` of the clip after the crops.  Not an ``AugmentParams``: ``batch_params`` never takes
    it for a record column."""
    src_length: int
    windows: List[Tuple[int, int, int]] = field(default_factory=list)
    params: AugmentParams = None

    def source_rows(self):
        """int64 ``[params.length]``: the input row each output row comes from, before the masks."""
        L = self.params.length
        if L <= 0:
            return np.zeros(0, dtype=np.int64)
        j = (np.arange(L, dtype=np.int64) - self.params.shift) % L
        for start, shift, length in reversed(self.windows):
            j = (start + j - shift) % length
        return j


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
        if sum(op[0] == "crop" for op in self.ops) > MAX_WINDOWS:
            raise ValueError(f"{sum(op[0] == 'crop' for op in self.ops)} crops: at most {MAX_WINDOWS}")
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

    def draw_shape(self, L: int, F: int) -> AugmentPlan:
        """``draw`` for a clip known by its shape ``(L, F)`` alone: exactly the calls ``draw`` makes on ``random`` and
        ``np.random``, in the same order (the ValueError of ``randrange`` on a clip that is too short included) -> the
        ``AugmentPlan`` whose crops the device performs (``apply_plans``)."""
        L, F = int(L), int(F)
        plan = AugmentPlan(src_length=L)
        shift = 0                                  # pending roll
        for op in self.ops:
            if op[0] == "crop":
                _, size, p = op
                if L <= size or random.random() > p:
                    continue
                start = np.random.randint(0, L - size)
                plan.windows.append((int(start), shift % L, L))
                L, shift = int(size), 0
            else:
                _, mean, std = op
                shift += int(np.random.normal(mean, std))
        plan.params = params = AugmentParams(length=L, shift=shift % L if L > 0 else 0)
        if random.random() < self.p:
            if self.timemask and self.num_timemask > 0:
                _masks(L, self.T, self.num_timemask, params.time_masks)
            if self.freqmask and self.num_freqmask > 0:
                _masks(F, self.F, self.num_freqmask, params.freq_masks)
        return plan


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


def window_table(plans: Sequence[AugmentPlan], src_lens, T: int, F: int):
    """Validate the plans against the batch of uncropped clips ``[N, T, F]`` and build the kernel's int32 table
    ``[N, WINDOW_TABLE_WIDTH]`` (include/acvae_hip.h, acvae_augment_window) -> ``(table, out_lens int64 [N])``.  Raises
    ValueError on anything the kernel would have to clamp."""
    lens = np.asarray(src_lens).reshape(-1)
    if len(plans) != len(lens):
        raise ValueError(f"{len(plans)} augment plans for a batch of {len(lens)} clips")
    out_lens = np.zeros(len(lens), dtype=np.int64)
    tab = np.zeros((len(lens), WINDOW_TABLE_WIDTH), dtype=np.int32)
    for n, (plan, L) in enumerate(zip(plans, lens)):
        L = int(L)
        if not isinstance(plan, AugmentPlan) or not isinstance(plan.params, AugmentParams):
            raise ValueError(f"clip {n}: {type(plan).__name__} is not an AugmentPlan with its AugmentParams")
        if not 0 <= L <= T:
            raise ValueError(f"clip {n}: length {L} outside [0, {T}]")
        if plan.src_length != L:
            raise ValueError(f"clip {n}: plan drawn for length {plan.src_length}, batch length {L} (plans out of order?)")
        if len(plan.windows) > MAX_WINDOWS:
            raise ValueError(f"clip {n}: {len(plan.windows)} windows, at most {MAX_WINDOWS}")
        sizes = [w[2] for w in plan.windows[1:]] + [plan.params.length]
        for k, ((start, shift, length), size) in enumerate(zip(plan.windows, sizes)):
            if length != L:
                raise ValueError(f"clip {n}: window {k} cut from a clip of {length} rows, the clip in front of it has {L}")
            if not 1 <= size <= length:
                raise ValueError(f"clip {n}: window {k} of {size} rows out of a clip of {length}")
            if not 0 <= start < length:
                raise ValueError(f"clip {n}: window {k} starts at {start}, outside [0, {length})")
            if not 0 <= shift < length:
                raise ValueError(f"clip {n}: window {k}: shift {shift} outside [0, {length})")
            if shift == 0 and start + size > length:
                raise ValueError(f"clip {n}: window {k} [{start}, {start + size}) beyond the unrolled clip's {length} rows")
            tab[n, TABLE_WIDTH + 2 + 3 * k:TABLE_WIDTH + 5 + 3 * k] = start, shift, length
            L = size
        if plan.params.length != L:
            raise ValueError(f"clip {n}: record drawn for length {plan.params.length}, the clip has {L} rows")
        out_lens[n] = L
        tab[n, TABLE_WIDTH], tab[n, TABLE_WIDTH + 1] = L, len(plan.windows)
    To = int(out_lens.max()) if len(out_lens) else 0
    tab[:, :TABLE_WIDTH] = table([p.params for p in plans], out_lens, To, F)
    return tab, out_lens


def apply_plans(feats_d, src_lens, plans: Sequence[AugmentPlan]):
    """The device half for clips that were never on the host: the crops, rolls and masks of ``plans`` (one ``AugmentPlan``
    per clip, in batch order) applied to the uncropped batch ``feats_d`` [N, T, F] (fp32, F % 4 == 0, F <= MAX_F) of
    ``src_lens`` rows on the current stream.  Validates on the host first (ValueError, no launch).  -> ``(out [N, To, F],
    out_lens np.int64 [N])`` with ``To = max(out_lens)``; rows behind a clip's own are zeros; ``feats_d`` is not written."""
    if not isinstance(feats_d, torch.Tensor) or feats_d.dim() != 3 or feats_d.dtype != torch.float32:
        raise ValueError(f"feats must be a float32 [N, T, F] tensor, got {getattr(feats_d, 'dtype', type(feats_d).__name__)} "
                         f"{tuple(getattr(feats_d, 'shape', ()))}")
    N, T, F = feats_d.shape
    if F % 4 != 0 or F > MAX_F:
        raise ValueError(f"feature dimension {F}: the kernel takes multiples of 4 up to {MAX_F}")
    if T * F >= 1 << 31:
        raise ValueError(f"clips of {T} x {F} cells: the kernel indexes a clip with 32-bit integers")
    tab, out_lens = window_table(plans, src_lens, T, F)
    _lib.require_cuda(feats_d)
    To = int(out_lens.max()) if N else 0
    x = feats_d.contiguous()
    out = torch.empty((N, To, F), dtype=x.dtype, device=x.device)
    if N == 0 or To == 0:
        return out, out_lens
    lens = np.asarray(src_lens).reshape(-1).astype(np.int32)
    up = _lib.h2d(np.concatenate([lens, tab.reshape(-1)]), x.device)      # one upload: lengths, then the table
    _lib.call("acvae_augment_window", x, out, up, up[N:], N, T, To, F, WINDOW_TABLE_WIDTH, _lib.current_stream())
    return out, out_lens


def batch_params(batch):
    """The AugmentParams column of a collated training batch (``CaptionDataset(..., augment=...)``), or None."""
    if len(batch) >= 6 and isinstance(batch[3], (tuple, list)) and batch[3] and \
            all(isinstance(r, AugmentParams) for r in batch[3]):
        return batch[3]
    return None
