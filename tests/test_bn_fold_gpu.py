"""GPU: the BatchNorm + ReLU backward folded into the kernel that consumes its output gives the same bits as the two-pass
sequence it replaces - acvae_bn_relu_bwd (its apply pass writes dY), then the consumer reading that dY.

  * acvae_conv1_first_bwd_bn against acvae_bn_relu_bwd (upstream 0) + acvae_conv1_first_bwd: bn1's dgamma / dbeta, dW1 and
    bn0's dgamma / dbeta, bit for bit, at the production shape (B = 32, T = 1000 and 3000), at a frame count that is not a
    multiple of the kernel's row block, in training and in evaluation mode.
The paths that keep the separate apply pass (the bf16 encoder, every other block) are run by the existing suites.
"""
import pytest
import torch

from acvae_amd import _lib

pytestmark = pytest.mark.gpu


def S():
    return _lib.current_stream()


def ws_buf(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")


def bn_consts(C, gen):
    """[4][C] scale | shift | mean | invstd, scale of both signs so that the ReLU passes and blocks in every channel"""
    scale = torch.randn(C, device="cuda", generator=gen)
    shift = 0.3 * torch.randn(C, device="cuda", generator=gen)
    mean = 0.1 * torch.randn(C, device="cuda", generator=gen)
    invstd = 0.5 + torch.rand(C, device="cuda", generator=gen)
    return torch.stack([scale, shift, mean, invstd]).contiguous()


@pytest.mark.parametrize("N,T,training", [(32, 1000, 1), (32, 1000, 0), (32, 3000, 1), (3, 37, 1), (3, 37, 0)])
def test_first_conv_bwd_with_bn1_folded_is_bit_identical(N, T, training):
    Fm = 64
    gen = torch.Generator(device="cuda").manual_seed(1000 * N + T + training)
    x = torch.randn(N, T, Fm, device="cuda", generator=gen)
    bn0 = bn_consts(Fm, gen)
    w1 = 0.3 * torch.randn(64, 1, 3, 3, device="cuda", generator=gen)
    Y1 = torch.randn(N, T, Fm, 64, device="cuda", generator=gen)
    dO = torch.randn(N, T, Fm, 64, device="cuda", generator=gen)
    bn1 = bn_consts(64, gen)
    wsb = _lib.call("acvae_conv3x3_workspace_bytes", N, T, Fm, 1, 64) + _lib.call("acvae_bn_workspace_bytes", N, T, Fm, 64)
    ws = ws_buf(wsb)
    out = lambda: [torch.full((64,), float("nan"), device="cuda") for _ in range(2)] + \
        [torch.full((64, 1, 3, 3), float("nan"), device="cuda")] + [torch.full((64,), float("nan"), device="cuda") for _ in range(2)]
    # two passes: bn1's backward writes dY, the first conv's backward reads it
    dg1, db1, dW1, dg0, db0 = out()
    dY = torch.empty_like(Y1)
    _lib.call("acvae_bn_relu_bwd", Y1, dO, 0, bn1, dg1, db1, dY, ws, wsb, N, T, Fm, 64, training, 0.0, 0, 0, None, S())
    _lib.call("acvae_conv1_first_bwd", x, bn0, w1, dY, dW1, dg0, db0, ws, wsb, N, T, Fm, S())
    del dY
    # folded: bn1's sums, then the first conv's backward forms dY itself as it gathers its operand
    fg1, fb1, fW1, fg0, fb0 = out()
    _lib.call("acvae_conv1_first_bwd_bn", x, bn0, w1, Y1, dO, bn1, fg1, fb1, fW1, fg0, fb0, ws, wsb, N, T, Fm, training, S())
    torch.cuda.synchronize()
    for name, a, b in (("bn1 dgamma", dg1, fg1), ("bn1 dbeta", db1, fb1), ("dW1", dW1, fW1), ("bn0 dgamma", dg0, fg0),
                       ("bn0 dbeta", db0, fb0)):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} differ, max |diff| {float((a - b).abs().max()):.3e}"

