"""Shared by the parameter-group GPU tests: the bound the fused one-group update is held to against torch.optim (a copy of
tests/test_optim_gpu.py's ``agree`` and its ``loose`` rule, kept here so that no test file imports another for it), the
clip coefficient as the kernels form it, and the layouts (slices, groups, chunk tables) the kernel tests run over."""
import ctypes

import numpy as np
import torch

from acvae_amd import optim

PAD = 8                                 # guard elements behind every buffer: must come back untouched
GUARD = 7.0


def coef_of(total_norm, gscale, max_norm):
    """The clip coefficient exactly as the kernels form it, in fp32."""
    c = np.float32(gscale)
    if max_norm > 0:
        r = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
        c = np.float32(c * min(r, np.float32(1.0)))
    return float(c)


def agree(got, ref, start, what, loose=None, loose_tol=0.0):
    """got / ref after three updates that started from `start`.  Each element is a chain of ~10 fp32 operations per step;
    torch and the kernel may round a few of them differently (torch's lerp / addcmul may fuse a multiply-add, its division
    by a scalar multiplies by the reciprocal).  A differing rounding costs at most one ulp (1.2e-7 relative) of the term
    it rounds, and no term exceeds the largest total change of the tensor, max|ref - start|.  Bound: 8 ulp of the element
    + 16 ulp of the largest change.  Elements flagged `loose` are held to `loose_tol` only."""
    got, ref, start = got.detach().cpu().double(), ref.detach().cpu().double(), start.detach().cpu().double()
    s = float((ref - start).abs().max())
    assert s > 0, f"{what}: the reference did not move"
    tol = 1e-6 * ref.abs() + 2e-6 * s
    if loose is not None:
        tol = torch.where(loose, torch.full_like(tol, loose_tol), tol)
    err = (got - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max err/tol {float((err / tol).max()):.2f}, max err {float(err.max()):.3e}"


def loose_elements(grad, param, weight_decay):
    """Adam with L2 decay: g' = coef*g + wd*p can cancel, and a one-ulp difference in g' moves the update g'/(|g'| + eps)
    by lr*eps*delta/|g'|^2, above the bound of `agree` once |g'| < ~3e-5.  Those elements are held to the bound of three
    steps, 3 * 10 * lr, and may be at most 0.1 % of the tensor (LOOSE_CAP); their moments to 1e-3 of the tensor's largest."""
    return (grad.double() + weight_decay * param.detach().double()).abs() < 3e-5


LOOSE_CAP = 1e-3


def padded(x, n):
    """x in a device buffer of n + PAD elements, the tail holding GUARD."""
    t = torch.full((n + PAD,), GUARD, device="cuda")
    t[:n].copy_(x)
    return t


def doubles(vals):
    vals = [float(v) for v in vals]
    return (ctypes.c_double * len(vals))(*vals)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    """Equality of the fp32 bit patterns (NaN payloads included)."""
    return torch.equal(bits(a), bits(b))


class Layout:
    """Slices of one flat buffer: padded sizes, each slice's group, and the chunk tables cut from them."""

    def __init__(self, sizes, group_of, chunk):
        self.sizes, self.group_of, self.chunk = list(sizes), list(group_of), int(chunk)
        self.n = sum(self.sizes)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    def table(self, skipped=(), first=()):
        return optim.chunk_table(self.sizes, self.group_of, skipped, first, self.chunk)

    def segments(self, skipped=(), first=()):
        return optim.group_segments(self.sizes, self.group_of, skipped, first)

    def mask(self, idx):
        """bool [n]: the elements of the slices `idx`."""
        m = torch.zeros(self.n, dtype=torch.bool)
        for i in idx:
            m[int(self.offs[i]):int(self.offs[i + 1])] = True
        return m

    def group_mask(self, k, skipped=()):
        return self.mask([i for i, g in enumerate(self.group_of) if g == k and i not in set(skipped)])


def group_hyper(k):
    """All-different hyperparameters of group k; group 0 has no weight decay (that branch of the kernel)."""
    return dict(lr=1e-3 * (1 + k), betas=(0.9 - 0.01 * k, 0.999 - 0.001 * k), eps=1e-8 * (1 + k), weight_decay=0.01 * k,
                momentum=0.9 - 0.02 * k)
