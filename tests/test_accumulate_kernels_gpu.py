"""GPU, C ABI: acvae_grad_accumulate bit for bit against fp32 addition, acvae_ema_step against the float64 evaluation of
torch's lerp rule, at sizes around the float4 body / scalar tail / block / grid-stride boundaries, with guard elements
behind every buffer; and what both refuse, with the outputs left as they were."""
import numpy as np
import pytest
import torch

from acvae_amd import _lib

pytestmark = pytest.mark.gpu
PAD, GUARD = 8, 7.0
CAP = int(_lib._defs["ACVAE_FLAT_BLOCKS_CAP"])
# one full trip of the grid-stride loop is CAP blocks x 256 threads x 4 elements; a few float4 and a scalar tail beyond it
N_SECOND_TRIP = CAP * 256 * 4 + 4 * 300 + 3
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, (1 << 20) + 3, N_SECOND_TRIP]
EINVAL, EALIGN = -1, -2

# (acc, grads) pairs with a result that a careless kernel gets wrong: signed zeros, infinities, NaN, denormals, cancellation
TINY = 1e-40                      # a denormal
MINN = 1.17549435e-38             # the smallest normal
PAIRS = [(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (float("inf"), 1.0), (float("inf"), float("-inf")),
         (float("-inf"), float("-inf")), (float("nan"), 1.0), (1.0, float("nan")), (TINY, TINY), (TINY, -TINY),
         (MINN, -TINY), (3 * TINY, -TINY), (1.5, -1.5), (1e30, -1e30), (3e38, 3e38), (-3e38, -3e38), (1.0, 2.0 ** -24),
         (1.0, 2.0 ** -24 + 2.0 ** -40), (-0.0, TINY)]


def padded(x):
    """x on the device with PAD guard elements behind it."""
    t = torch.full((x.numel() + PAD,), GUARD, device="cuda")
    t[:x.numel()].copy_(x)
    return t


def guards_ok(*bufs):
    return all(bool((b[-PAD:] == GUARD).all()) for b in bufs)


def inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    acc, grads = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    a = torch.tensor([p[0] for p in PAIRS], dtype=torch.float32)
    b = torch.tensor([p[1] for p in PAIRS], dtype=torch.float32)
    k = min(n, len(PAIRS))
    acc[:k], grads[:k] = a[:k], b[:k]                  # in the float4 body ...
    if n >= 4 * len(PAIRS):
        acc[-len(PAIRS):], grads[-len(PAIRS):] = a, b  # ... and up to the last element, the scalar tail included
    return acc, grads


def same_bits(got, ref):
    """NaN positions as masks, everything else on the int32 view."""
    got, ref = got.cpu(), ref.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    keep = ~nan
    assert torch.equal(got.view(torch.int32)[keep], ref.view(torch.int32)[keep])


@pytest.mark.parametrize("n", SIZES)
def test_accumulate_first_copies_and_never_reads_acc(n):
    _, grads = inputs(n, 11 + n % 97)
    acc_d = padded(torch.full((n,), float("nan")))
    g_d = padded(grads)
    _lib.call("acvae_grad_accumulate", acc_d, g_d, n, 1, _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_ok(acc_d, g_d)
    same_bits(acc_d[:n], grads)
    same_bits(g_d[:n], grads)


@pytest.mark.parametrize("n", SIZES)
def test_accumulate_adds_like_fp32(n):
    acc, grads = inputs(n, 23 + n % 89)
    ref = acc + grads                                  # torch's fp32 addition on the host: one IEEE addition per element
    if n >= len(PAIRS):
        assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any()) and bool((ref == 0).any())
        assert bool(((ref != 0) & (ref.abs() < MINN)).any()), "no denormal result among the planted pairs"
    acc_d, g_d = padded(acc), padded(grads)
    _lib.call("acvae_grad_accumulate", acc_d, g_d, n, 0, _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_ok(acc_d, g_d)
    same_bits(acc_d[:n], ref)
    same_bits(g_d[:n], grads)


def lerp64(ema, params, decay):
    """The kernel's two-branch expression in float64, with the fp32 weight the kernel uses."""
    w32 = np.float32(1.0 - decay)
    w = float(w32)
    e, p = ema.double(), params.double()
    return e + w * (p - e) if w32 < np.float32(0.5) else p - (p - e) * (1.0 - w)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.999, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_ema_step_against_float64(n, decay):
    g = torch.Generator().manual_seed(5 + n % 83)
    ema, params = torch.randn(n, generator=g), torch.randn(n, generator=g) * 2
    e_d, p_d = padded(ema), padded(params)
    _lib.call("acvae_ema_step", e_d, p_d, n, decay, _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_ok(e_d, p_d)
    assert torch.equal(p_d[:n].cpu(), params)
    got = e_d[:n].cpu()
    # three fp32 roundings (difference, product, sum) and a fourth for 1 - w in the second branch
    bound = 4 * 2.0 ** -24 * (ema.double().abs() + params.double().abs())
    err = (got.double() - lerp64(ema, params, decay)).abs()
    assert bool((err <= bound).all()), f"n={n} decay={decay}: max err/bound {float((err / bound).max()):.2f}"
    if decay == 1.0:
        assert torch.equal(got.view(torch.int32), ema.view(torch.int32)), "decay 1 must leave ema as it is"
    if decay == 0.0:
        assert torch.equal(got.view(torch.int32), params.view(torch.int32)), "decay 0 must copy params"


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
@pytest.mark.parametrize("n", [5, 1025, (1 << 20) + 3])
def test_ema_of_equal_buffers_is_exact(n, decay):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    e_d, p_d = padded(x), padded(x)
    _lib.call("acvae_ema_step", e_d, p_d, n, decay, _lib.current_stream())
    torch.cuda.synchronize()
    assert guards_ok(e_d, p_d)
    assert torch.equal(e_d[:n].cpu().view(torch.int32), x.view(torch.int32))


def test_refusals_leave_the_outputs_alone():
    """Each refused call returns its negative code before any launch: the poisoned outputs keep their bits."""
    n = 1024
    lib = _lib.lib()
    st = _lib.current_stream()
    POISON = -123.25
    out = torch.full((n + 16,), POISON, device="cuda")
    src = torch.ones(n + 16, device="cuda")
    both = torch.full((2 * n,), POISON, device="cuda")
    o, s = out.data_ptr(), src.data_ptr()
    assert o % 16 == 0 and s % 16 == 0
    acc = lambda *a: lib.acvae_grad_accumulate(*a)
    ema = lambda *a: lib.acvae_ema_step(*a)
    for first in (0, 1):
        assert acc(None, s, n, first, st) == EINVAL and acc(o, None, n, first, st) == EINVAL
        assert acc(o, s, 0, first, st) == EINVAL and acc(o, s, -4, first, st) == EINVAL
        assert acc(o + 4, s, n, first, st) == EALIGN and acc(o, s + 4, n, first, st) == EALIGN
        b = both.data_ptr()
        assert acc(b, b, n, first, st) == EINVAL                       # the same range
        assert acc(b, b + 16, n, first, st) == EINVAL                  # shifted by one float4
        assert acc(b + 4 * (n - 4), b, n, first, st) == EINVAL         # the last float4 of one on the first of the other
    assert ema(None, s, n, 0.9, st) == EINVAL and ema(o, None, n, 0.9, st) == EINVAL
    assert ema(o, s, 0, 0.9, st) == EINVAL
    assert ema(o + 4, s, n, 0.9, st) == EALIGN and ema(o, s + 4, n, 0.9, st) == EALIGN
    assert ema(both.data_ptr(), both.data_ptr() + 16, n, 0.9, st) == EINVAL
    assert ema(o, s, n, 1.5, st) == EINVAL and ema(o, s, n, -0.1, st) == EINVAL and ema(o, s, n, float("nan"), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((both == POISON).all()) and bool((src == 1).all())
    # adjacent ranges do not overlap: accepted
    b = both.data_ptr()
    assert acc(b, b + 4 * n, n, 1, st) == 0
    torch.cuda.synchronize()
    assert bool((both == POISON).all())
