"""GPU: the bf16-storage kernels that are not convolutions, one by one through the per-op C ABI, every element against
float64 on the same bf16 inputs - the bf16 twins of test_kernels_gpu.py's first-conv and BatchNorm tests:

  * acvae_conv1_first_fwd_bf16 (conv1_first_fwd<bf16>): the rounded output, this layer's BatchNorm from the rounded values
    and the running buffers (training), or from the running buffers alone (evaluation); acvae_conv1_first_bwd_bf16: dW1 and bn0's dgamma / dbeta from a bf16 dY;
  * acvae_bn_relu_pool_fwd_bf16 (bn_relu_pool / bn_relu_drop <bf16>) and acvae_bn_relu_bwd_bf16 (bn_bwd<bf16>: the
    reduction and the plain / pool / drop apply kernels), training and evaluation, explicit keep masks, odd H and W,
    C = 64 .. 2048 (the reduction works in chunks of 1024 channels), and sizes where the grid-stride loops run more than once.

A bf16 output must be the correctly rounded value of the float64 result: |got - ref| <= half a bf16 ulp of ref plus the fp32
chain bound test_kernels_gpu.py uses (so only a ref within fp32 error of a rounding midpoint may round the other way).  fp32
outputs keep the chain bound.  ReLU decisions come from the kernels' own fp32 expression y * scale + shift > 0 on both sides."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from acvae_amd import _lib
from test_kernels_gpu import S, assert_every_element, chain_tol, nhwc, ws_buf
from ws_guard import ws_guards  # noqa: F401  (autouse fixture: every guard of ws_buf intact after each test)

pytestmark = pytest.mark.gpu


def half_ulp_bf16(ref):
    """Half the spacing of bf16 values at |ref| (8 significant bits): ref = m * 2^e, m in [0.5, 1) -> 2^(e - 9); 0 where
    ref == 0, which bf16 holds exactly (a ReLU-clamped or dropped element must come out as 0)."""
    _, e = torch.frexp(ref)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def assert_rounded(got, ref, K, what):
    """got (bf16) is ref (float64) rounded to bf16, up to the fp32 chain bound of a K-term computation."""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rms = float(ref.pow(2).mean().sqrt())
    tol = half_ulp_bf16(ref) + chain_tol(K) * torch.maximum(ref.abs(), torch.full_like(ref, rms))
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, worst " \
                                f"{float((err / tol).max()):.2f} x tol (|err| {float(err.max()):.3e}, rms {rms:.3e})"
    return float((err / tol).max())


def test_half_ulp_bound_is_tight():
    """The bound itself: a correctly rounded value passes, one bf16 step off fails."""
    ref = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3
    ref[::7] = 0
    rounded = ref.float().bfloat16()
    assert_rounded(rounded, ref, 1, "rounded")
    up = (rounded.view(torch.int16) + 1).view(torch.bfloat16)                        # one bf16 step away from zero
    up[::7] = 0
    with pytest.raises(AssertionError):
        assert_rounded(up, ref, 1, "one step off")
    leaky = rounded.clone()                      # a zero that is not zero (a leaky ReLU slope of 1e-3, say) fails as well
    leaky[::7] = 1e-3
    with pytest.raises(AssertionError):
        assert_rounded(leaky, ref, 1, "not zero")


@pytest.mark.parametrize("N,Tt", [(3, 37), (2, 250), (5, 401)])
def test_first_conv_bf16_fwd_bwd_vs_fp64(N, Tt):
    """conv_block1.conv1 of the bf16 encoder: fp32 features through bn0's affine, fp32 weights on the VALU, the output rounded
    to bf16, its BatchNorm from the rounded output (batch statistics, running buffers with the unbiased variance); the
    backward from a bf16 dY (the stored gradient bn_bwd<bf16> writes).  Evaluation: BatchNorm from the running buffers."""
    Fm = 64
    g = torch.Generator().manual_seed(Tt)
    x = torch.randn(N, Tt, Fm, generator=g) * 1.7 + 0.4
    sc0, sh0 = torch.rand(Fm, generator=g) + 0.5, torch.randn(Fm, generator=g) * 0.2
    w1 = torch.randn(64, 1, 3, 3, generator=g) / 3
    g1, b1 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    rm0, rv0 = torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5
    dy = (torch.randn(N, 64, Tt, Fm, generator=g) / math.sqrt(N * Tt * Fm)).bfloat16()
    # bn0 = [4][64]: scale | shift | mean | invstd of the mel BatchNorm (the backward reads all four)
    mu0, var0 = x.double().mean((0, 1)), x.double().var((0, 1), unbiased=False)
    inv0 = 1 / torch.sqrt(var0 + 1e-5)
    bn0 = torch.stack([sc0, sh0, mu0.float(), inv0.float()]).contiguous()
    # fp64 reference on the kernel's fp32 operand x * scale0 + shift0
    xin = (x * sc0 + sh0).double().unsqueeze(1).requires_grad_(True)
    w1d = w1.double().requires_grad_(True)
    y = F.conv2d(xin, w1d, padding=1)
    y.backward(dy.double())
    wsb = _lib.call("acvae_conv3x3_workspace_bytes", N, Tt, Fm, 1, 64)
    ws = ws_buf(wsb)
    xd = x.cuda().contiguous()
    cnt = N * Tt * Fm
    for training in (1, 0):
        Y = torch.empty(N, Tt, Fm, 64, device="cuda", dtype=torch.bfloat16)
        rm, rv = rm0.cuda(), rv0.cuda()
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        bn1 = torch.empty(4, 64, device="cuda")
        _lib.call("acvae_conv1_first_fwd_bf16", xd, sc0.cuda(), sh0.cuda(), w1.cuda().contiguous(), Y, g1.cuda(), b1.cuda(),
                  rm, rv, nbt, training, bn1, ws, wsb, N, Tt, Fm, S())
        worst = assert_rounded(Y, nhwc(y.detach()), 9, f"first conv bf16 fwd {N}x{Tt} train={training}")
        ys = Y.float().cpu().double()                 # the statistics are those of the stored (rounded) tensor
        if training:
            mu, var = ys.mean((0, 1, 2)), ys.var((0, 1, 2), unbiased=False)
            rms = float(ys.pow(2).mean().sqrt())
            assert float((bn1[2].cpu().double() - mu).abs().max()) <= 1e-5 * rms
            np.testing.assert_allclose(rm.cpu().double(), 0.9 * rm0.double() + 0.1 * mu, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(rv.cpu().double(), 0.9 * rv0.double() + 0.1 * var * cnt / (cnt - 1), rtol=1e-5)
            assert int(nbt) == 1
        else:                                             # evaluation: the running buffers, left as they were
            mu, var = rm0.double(), rv0.double()
            np.testing.assert_allclose(bn1[2].cpu().double(), mu, rtol=1e-6, atol=1e-7)
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 0
        sc1 = g1.double() / torch.sqrt(var + 1e-5)
        np.testing.assert_allclose(bn1[3].cpu().double(), 1 / torch.sqrt(var + 1e-5), rtol=3e-5)
        np.testing.assert_allclose(bn1[0].cpu().double(), sc1, rtol=3e-5)
        np.testing.assert_allclose(bn1[1].cpu().double(), b1.double() - mu * sc1, rtol=3e-5,
                                   atol=3e-5 * float((mu * sc1).abs().max()))
    # backward: dW1 and bn0's dgamma / dbeta (xin = scale0 * x + shift0 with scale0 = gamma0 * invstd0: dbeta0 = sum dxin,
    # dgamma0 = sum dxin * xhat)
    dW1, dg0, db0 = torch.empty(64, 1, 3, 3, device="cuda"), torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    _lib.call("acvae_conv1_first_bwd_bf16", xd, bn0.cuda(), w1.cuda().contiguous(), nhwc(dy).cuda(), dW1, dg0, db0, ws, wsb,
              N, Tt, Fm, S())
    dxin = xin.grad.squeeze(1)
    xhat = (x.double() - mu0) * inv0
    assert_every_element(dW1, w1d.grad, N * Tt * Fm, "first conv bf16 dW")
    assert_every_element(db0, dxin.sum((0, 1)), N * Tt * 9, "bn0 dbeta (bf16 dY)")
    assert_every_element(dg0, (dxin * xhat).sum((0, 1)), N * Tt * 9, "bn0 dgamma (bf16 dY)")
    print(f"first conv bf16 {N}x{Tt}: worst output {worst:.2f} x its bound")


def bn_case(N, H, W, C, seed):
    """bf16 Y, and its BatchNorm [4][C] (scale | shift | mean | invstd, fp32) from float64 batch statistics."""
    g = torch.Generator().manual_seed(seed)
    Y = (torch.randn(N, C, H, W, generator=g) * (torch.rand(C, 1, 1, generator=g) + 0.5)
         + torch.randn(C, 1, 1, generator=g) * 0.5).bfloat16()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    yd = Y.double()
    mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    bn = torch.stack([scale, shift, mean.float(), invstd.float()]).contiguous()
    return g, Y, gamma, bn


# (N, H, W, C, pool): odd H / W, 64 .. 2048 channels; the last two run the element-wise grid-stride loops more than once
# (ew_grid caps a launch at 8192 x 256 threads of four channels each: > 2^21 channel quads, counted on the output of the
# pooling kernels - 4 x 65 x 33 x 256 for the last one)
BN_SHAPES = [(3, 9, 7, 64, 1), (2, 7, 5, 128, 1), (2, 5, 3, 256, 1), (3, 6, 4, 512, 1), (2, 5, 3, 1024, 1),
             (2, 5, 2, 2048, 0), (2, 3, 3, 2048, 0), (4, 65, 33, 1024, 0), (4, 130, 66, 1024, 1)]


@pytest.mark.parametrize("N,H,W,C,pool", BN_SHAPES, ids=[f"{n}x{h}x{w}x{c}-p{p}" for n, h, w, c, p in BN_SHAPES])
def test_bn_relu_pool_and_backward_bf16_vs_fp64(N, H, W, C, pool):
    g, Y, gamma, bn = bn_case(N, H, W, C, seed=N * 7 + H * 13 + C)
    sc, sh = bn[0], bn[1]
    mean, invstd = bn[2].double().view(1, -1, 1, 1), bn[3].double().view(1, -1, 1, 1)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    keep = torch.rand(N, C, Ho, Wo, generator=g) > 0.2
    keep_d = keep.to(torch.uint8).cuda().contiguous()
    Yg, bng = nhwc(Y).cuda(), bn.cuda()
    mask = (Y.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) > 0          # fp32, as the kernels evaluate it
    z = Y.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    a = torch.where(mask, z, torch.zeros((), dtype=torch.double))
    # forward: P = dropout(pool(relu(bn(Y)))), with and without dropout
    worst = 0.0
    for p_drop in (0.2, 0.0):
        P = torch.empty(N, Ho, Wo, C, device="cuda", dtype=torch.bfloat16)
        _lib.call("acvae_bn_relu_pool_fwd_bf16", Yg, bng, P, N, H, W, C, pool, p_drop, 0, 0, keep_d if p_drop else None, S())
        p_ref = F.avg_pool2d(a, 2) if pool else a
        if p_drop:
            p_ref = p_ref * keep.double() / 0.8
        worst = max(worst, assert_rounded(P, nhwc(p_ref), 4, f"bn_relu_pool bf16 C={C} pool={pool} p={p_drop}"))
    # backward through dropout (+ pool) - upstream 1 / 2 - and the plain upstream 0, training and evaluation mode
    dP = (torch.randn(N, C, Ho, Wo, generator=g)).bfloat16()
    dO0 = (torch.randn(N, C, H, W, generator=g)).bfloat16()
    wsb = _lib.call("acvae_bn_workspace_bytes", N, H, W, C)
    ws = ws_buf(wsb)
    cnt = N * H * W
    for upstream in (1 if pool else 2, 0):
        if upstream == 0:
            up = dO0.double()
        else:
            up = dP.double() * keep.double() / 0.8
            if pool:
                up = F.interpolate(up, scale_factor=2, mode="nearest") / 4
                up = F.pad(up, (0, W - 2 * Wo, 0, H - 2 * Ho))            # rows / columns behind the last window: no gradient
        gg = up * mask.double()                                             # the gradient at bn's output
        yhat = (Y.double() - mean) * invstd
        dbeta, dgamma = gg.sum((0, 2, 3)), (gg * yhat).sum((0, 2, 3))
        for training in (1, 0):
            if training:
                dy_ref = sc.double().view(1, -1, 1, 1) * (gg - dbeta.view(1, -1, 1, 1) / cnt
                                                         - yhat * dgamma.view(1, -1, 1, 1) / cnt)
            else:
                dy_ref = sc.double().view(1, -1, 1, 1) * gg
            dY = torch.empty(N, H, W, C, device="cuda", dtype=torch.bfloat16)
            dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            dO = nhwc(dO0 if upstream == 0 else dP).cuda()
            _lib.call("acvae_bn_relu_bwd_bf16", Yg, dO, upstream, bng, dg, db, dY, ws, wsb, N, H, W, C, training,
                      0.2 if upstream else 0.0, 0, 0, keep_d if upstream else None, S())
            what = f"C={C} {N}x{H}x{W} upstream={upstream} train={training}"
            assert_every_element(db, dbeta, cnt, "dbeta bf16 " + what)
            assert_every_element(dg, dgamma, cnt, "dgamma bf16 " + what)
            worst = max(worst, assert_rounded(dY, nhwc(dy_ref), 16, "dY bf16 " + what))
    print(f"bn bf16 {N}x{H}x{W}x{C} pool={pool}: worst bf16 output {worst:.2f} x its bound")
