"""GPU: the operand staging of the Winograd weight gradient (conv_wino.hip, wino_wgrad_body) at the smallest shapes at which
each branch of its addressing can go wrong, through acvae_conv3x3_wgrad_wino.

The staging loads the activation window through a buffer descriptor of the current clip (rows above / below the clip read as
zero in hardware), keeps the window's padding columns as slots zeroed once per LDS buffer, sends dead items to a dummy slot,
and takes the masked arm of the gradient DMA only in a stage that reaches below the clip.  What can go wrong, and the cases:

  * every stage shape: W = 4, 8, 16, 32, 64 (the _s1 .. _s4 instantiations; at W = 64 the padding column alternates with the
    stage's segment, i.e. with the LDS buffer);
  * image edges: H = 5, 6, 7, 9 (row above the clip, row below it, the half-empty last tile row on the masked DMA arm);
  * clip boundaries: N = 2, 3 - the row above clip 1 is the last row of clip 0 in memory;
  * channels (64, 64), (64, 128), (128, 64); with and without the BatchNorm + ReLU operand, signed scales and shifts of the
    order of 1 (relu(shift) at a padding position would be an error of the order of the result itself).

At those sizes the launch plan gives every workgroup ONE stage (N * spc <= Z), so only the prologue's staging is ever read.
`test_stage_ranges_cross_clips` therefore adds, per stage shape, a batch large enough that a workgroup runs `per` = 2 or 3
stages, with spc not a multiple of `per` (ranges cross clip boundaries inside the main loop, both buffer parities start a
range) and N * spc not a multiple of `per` (a ragged last range).  `test_reads_stay_inside_the_tensors` puts X and dY into
larger buffers filled with NaN.

Reference: the float64 weight gradient of conv2d(relu(x * scale + shift), w) (or of plain x) on the CPU, the ReLU decision
taken from the kernel's own fp32 expression.  Bound: the one tests/test_kernels_gpu.py holds this kernel to (restated below):
every element within 6 sigma of the rounding random walk of an fp32 chain of K = N H W terms, relative to max(|ref|, rms).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from acvae_amd import _lib
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu

CHANNELS = [(64, 64), (64, 128), (128, 64)]
HEIGHTS = [5, 6, 7, 9]
WIDTHS = [4, 8, 16, 32, 64]
PAD = 16384          # floats in front of and behind a tensor inside its NaN-filled buffer: 64 KB, 16-byte aligned


def chain_tol(K):
    """tests/test_kernels_gpu.py: |err| bound for an fp32 k-ordered chain of K terms with O(1) result: 6 sigma of the rounding
    random walk 2^-24 * sqrt(K) * rms, floor 1e-5."""
    return max(1e-5, 6 * 2.0 ** -24 * math.sqrt(K))


def assert_every_element(got, ref, K, what):
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    rms = float(ref.pow(2).mean().sqrt())
    tol = chain_tol(K) * torch.maximum(ref.abs(), torch.full_like(ref, rms))
    err = (got - ref).abs()
    bad = err > tol
    print(f"{what}: worst {float((err / tol).max()):.3f} x tol (|err| {float(err.max()):.3e}, rms {rms:.3e})")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, worst " \
                                f"{float((err / tol).max()):.2f} x tol (|err| {float(err.max()):.3e}, rms {rms:.3e})"


def make_case(N, H, W, Cin, Cout, act, seed):
    """NHWC fp32 operands and the float64 reference dW[co][ci][3][3]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    dy = torch.randn(N, H, W, Cout, generator=g) / math.sqrt(N * H * W)
    sc = sh = None
    if act:
        sign = torch.where(torch.rand(Cin, generator=g) < 0.5, -1.0, 1.0)
        sc = sign * (torch.rand(Cin, generator=g) + 0.5)
        sh = 0.75 + 0.5 * torch.randn(Cin, generator=g)           # mostly positive: relu(shift) ~ 1 where padding leaked
        xin = x * sc + sh                                          # fp32, the kernel's own expression
        xa = torch.where(xin > 0, xin.double(), torch.zeros((), dtype=torch.double))
    else:
        xa = x.double()
    xp = F.pad(xa, (0, 0, 1, 1, 1, 1))                             # [N][H + 2][W + 2][Cin]
    dyr = dy.double().reshape(-1, Cout).t().contiguous()
    ref = torch.empty(Cout, Cin, 3, 3, dtype=torch.double)
    for a in range(3):
        for b in range(3):
            ref[:, :, a, b] = dyr @ xp[:, a:a + H, b:b + W, :].reshape(-1, Cin)
    return x, dy, sc, sh, ref


def run_wgrad(xd, dyd, sc, sh, N, H, W, Cin, Cout):
    wsb = _lib.call("acvae_conv3x3_workspace_bytes", N, H, W, Cin, Cout)
    ws = guarded(wsb, 0xFF).view
    scd = None if sc is None else sc.cuda()
    shd = None if sh is None else sh.cuda()
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
    _lib.call("acvae_conv3x3_wgrad_wino", dyd, xd, scd, shd, dw, ws, wsb, N, H, W, Cin, Cout, _lib.current_stream())
    return dw


def check(N, H, W, Cin, Cout, act, seed):
    x, dy, sc, sh, ref = make_case(N, H, W, Cin, Cout, act, seed)
    dw = run_wgrad(x.cuda(), dy.cuda(), sc, sh, N, H, W, Cin, Cout)
    assert_every_element(dw, ref, N * H * W, f"wino wgrad {Cin}->{Cout} {N}x{H}x{W} act={int(act)}")


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("W", WIDTHS)
def test_edges_of_every_stage_shape(W, N):
    seed = 1000 * W + 100 * N
    for H in HEIGHTS:
        for (Cin, Cout) in CHANNELS:
            for act in (False, True):
                seed += 1
                check(N, H, W, Cin, Cout, act, seed)


# (N, H, W): with (Cin, Cout) = (128, 64) the plan splits K over Z = 128 workgroups.
#   W = 64: spc = 8,  total 272 -> per 3 (8 % 3 != 0, 272 % 3 != 0), ranges start in either segment
#   W = 32: spc = 5,  total 135 -> per 2
#   W = 16: spc = 3 (the last stage of a clip has one tile row of two), total 135 -> per 2
#   W = 8:  spc = 3 (one tile row of four in the last stage), total 135 -> per 2
#   W = 4:  spc = 3 (one tile row of eight), total 135 -> per 2
CROSSING = [(34, 7, 64), (27, 9, 32), (45, 9, 16), (45, 17, 8), (45, 33, 4)]


@pytest.mark.parametrize("N,H,W", CROSSING)
def test_stage_ranges_cross_clips(N, H, W):
    for act in (False, True):
        check(N, H, W, 128, 64, act, seed=7 * W + int(act))


def in_nan_buffer(t):
    """A device copy of `t` that is a view into a larger buffer, PAD NaN floats in front of it and behind it."""
    buf = torch.full((PAD + t.numel() + PAD,), float("nan"), device="cuda")
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


@pytest.mark.parametrize("N,H,W", [(3, 7, 64), (3, 5, 32), (2, 9, 16), (3, 7, 8), (2, 9, 4), (27, 9, 32), (34, 7, 64)])
def test_reads_stay_inside_the_tensors(N, H, W):
    """X and dY surrounded by NaN: a read outside the tensors that the descriptor (or the DMA mask) did not stop shows up as
    NaN in dW - 0 * NaN is NaN, so even a read that the transform weights with zero does.  That argument holds for dY in both
    halves and for X in the plain-operand half.  Under the BatchNorm + ReLU operand the clamp drops a NaN read from X (it
    becomes 0 or relu(shift), as v_max_f32 made it before), so there a stray X read can show only as an error against the
    bound; the addressing is the same in both halves, and the plain half is the one that pins it."""
    Cin, Cout = (128, 64) if N > 3 else (64, 64)
    for act in (False, True):
        x, dy, sc, sh, ref = make_case(N, H, W, Cin, Cout, act, seed=31 * W + H + int(act))
        xbuf, xd = in_nan_buffer(x)
        dybuf, dyd = in_nan_buffer(dy)
        dw = run_wgrad(xd, dyd, sc, sh, N, H, W, Cin, Cout)
        assert_every_element(dw, ref, N * H * W, f"wino wgrad in NaN {Cin}->{Cout} {N}x{H}x{W} act={int(act)}")
        assert bool(torch.isnan(xbuf[:PAD]).all()) and bool(torch.isnan(xbuf[-PAD:]).all())
        assert bool(torch.isnan(dybuf[:PAD]).all()) and bool(torch.isnan(dybuf[-PAD:]).all())
