"""GPU parity of the ResNet38 encoder (acvae_amd.encoder.ResNet38, ACVAE_ARCH_RESNET38): every new kernel alone against
fp64, the whole encoder's forward and every parameter gradient against an fp64 CPU restatement of the reference
(models/encoder.py:1014-1036, :1096-1167, :1169-1234) written here, reproducibility, dropout, the implicit-GEMM fallback,
and a TrainStep with the encoder inside Hybrid_VAEModel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from acvae_amd import _lib
from acvae_amd.encoder import ResNet38
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu
NULL = None


def close(a, b, rtol, atol, what=""):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    ok = err <= atol + rtol * b.abs()
    assert bool(ok.all()), f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e}), " \
                           f"{int((~ok).sum())}/{ok.numel()} out of tolerance"


def rel_l2(a, b):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).pow(2).sum().sqrt() / max(float(b.pow(2).sum().sqrt()), 1e-30))


# ------------------------------------------------------------------------------------------------ per-op kernels vs fp64
def nchw(x):
    return x.permute(0, 3, 1, 2)


def bn_pack(C, g):
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    mean = torch.randn(C, generator=g) * 0.2
    invstd = torch.rand(C, generator=g) + 0.5
    return torch.cat([scale, shift, mean, invstd]).float()


@pytest.mark.parametrize("N,H,W,C,ds", [(2, 7, 5, 64, True), (3, 4, 2, 128, False), (1, 9, 3, 512, True), (2, 6, 4, 256, False)])
@pytest.mark.parametrize("training", [1, 0])
def test_res_join_kernels_vs_fp64(N, H, W, C, ds, training):
    g = torch.Generator().manual_seed(H * 100 + C)
    y2 = torch.randn(N, H, W, C, generator=g)
    yd = torch.randn(N, H, W, C, generator=g) if ds else None
    x = torch.randn(N, H, W, C, generator=g)
    bn2, bnd = bn_pack(C, g), bn_pack(C, g)
    ident = (yd.double() * bnd[:C].double() + bnd[C:2 * C].double()) if ds else x.double()
    ref = torch.relu(y2.double() * bn2[:C].double() + bn2[C:2 * C].double() + ident)
    dev = lambda t: None if t is None else t.cuda().contiguous()
    out = torch.empty(N, H, W, C, device="cuda")
    _lib.call("acvae_res_join_fwd", dev(y2), dev(bn2), dev(yd), dev(bnd) if ds else NULL, NULL if ds else dev(x), out, N, H, W, C,
              _lib.current_stream())
    close(out, ref, 1e-6, 1e-6, "join fwd")
    dO = torch.randn(N, H, W, C, generator=g)
    G, dy2, dyd = (torch.empty(N, H, W, C, device="cuda") for _ in range(3))
    dg2, db2, dgd, dbd = (torch.empty(C, device="cuda") for _ in range(4))
    wsb = _lib.call("acvae_res_join_bwd_workspace_bytes", N, H, W, C)
    ws = guarded(wsb, 0xFF).view
    _lib.call("acvae_res_join_bwd", dev(dO), out, dev(y2), dev(bn2), dev(yd), dev(bnd) if ds else NULL, G, dy2, dyd if ds else NULL,
              dg2, db2, dgd if ds else NULL, dbd if ds else NULL, training, ws, wsb, N, H, W, C, _lib.current_stream())
    # fp64: the decisions the kernel took (out > 0 of its own output)
    gg = dO.double() * (out.cpu() > 0).double()
    close(G, gg, 0, 0, "G")
    M = N * H * W

    def bnb(y, pk):
        sc, mu, iv = pk[:C].double(), pk[2 * C:3 * C].double(), pk[3 * C:].double()
        yh = (y.double() - mu) * iv
        sg, sgy = gg.sum((0, 1, 2)), (gg * yh).sum((0, 1, 2))
        dy = sc * (gg - sg / M - yh * sgy / M) if training else sc * gg
        return dy, sg, sgy
    dy, sg, sgy = bnb(y2, bn2)
    close(db2, sg, 1e-5, 1e-4, "dbeta2"); close(dg2, sgy, 1e-5, 1e-4, "dgamma2"); close(dy2, dy, 1e-4, 1e-5, "dy2")
    if ds:
        dy, sg, sgy = bnb(yd, bnd)
        close(dbd, sg, 1e-5, 1e-4, "dbetad"); close(dgd, sgy, 1e-5, 1e-4, "dgammad"); close(dyd, dy, 1e-4, 1e-5, "dyd")


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 5, 3, 64, 128), (3, 16, 8, 128, 256), (1, 3, 2, 256, 512), (2, 31, 7, 64, 64)])
def test_conv1x1_kernels_vs_fp64(N, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(Cin + H)
    X = torch.randn(N, H, W, Cin, generator=g)
    Wt = torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1
    M = N * H * W
    ref = X.double().reshape(M, Cin) @ Wt.double().reshape(Cout, Cin).T
    Y = torch.empty(N, H, W, Cout, device="cuda")
    rows = _lib.lib().acvae_conv1x1_partials_rows(N, H, W)
    part = torch.empty(rows, 2, Cout, device="cuda")
    _lib.call("acvae_conv1x1_fwd", X.cuda(), Wt.cuda(), Y, part, N, H, W, Cin, Cout, _lib.current_stream())
    close(Y.reshape(M, Cout), ref, 1e-5, 1e-5, "conv1x1 fwd")
    close(part.double().sum(0)[0], ref.sum(0), 1e-5, 1e-3, "sum y")
    close(part.double().sum(0)[1], (ref * ref).sum(0), 1e-5, 1e-3, "sum y^2")
    dY = torch.randn(N, H, W, Cout, generator=g)
    base = torch.randn(N, H, W, Cin, generator=g)
    dX = base.cuda()
    _lib.call("acvae_conv1x1_dgrad", dY.cuda(), Wt.cuda(), dX, 1, N, H, W, Cin, Cout, _lib.current_stream())
    refx = base.double().reshape(M, Cin) + dY.double().reshape(M, Cout) @ Wt.double().reshape(Cout, Cin)
    close(dX.reshape(M, Cin), refx, 1e-5, 1e-5, "conv1x1 dgrad (+=)")
    wsb = _lib.call("acvae_conv1x1_wgrad_workspace_bytes", N, H, W, Cin, Cout)
    ws = guarded(wsb, 0xFF).view
    dW = torch.empty(Cout, Cin, 1, 1, device="cuda")
    _lib.call("acvae_conv1x1_wgrad", dY.cuda(), X.cuda(), dW, ws, wsb, N, H, W, Cin, Cout, _lib.current_stream())
    close(dW.reshape(Cout, Cin), dY.double().reshape(M, Cout).T @ X.double().reshape(M, Cin), 1e-5, 1e-4, "conv1x1 wgrad")


@pytest.mark.parametrize("N,H,W,C", [(2, 7, 5, 64), (1, 4, 2, 512), (3, 9, 9, 128), (2, 2, 3, 256)])
def test_avg_pool2_kernels_vs_fp64(N, H, W, C):
    g = torch.Generator().manual_seed(H * W + C)
    X = torch.randn(N, H, W, C, generator=g)
    Ho, Wo = H // 2, W // 2
    mask = torch.rand(N, C, Ho, Wo, generator=g) > 0.2
    P = torch.empty(N, Ho, Wo, C, device="cuda")
    _lib.call("acvae_avg_pool2_fwd", X.cuda(), P, N, H, W, C, 0.2, 0, 0, mask.to(torch.uint8).cuda(), _lib.current_stream())
    ref = F.avg_pool2d(nchw(X.double()), 2) * mask.double() / 0.8
    close(nchw(P), ref, 1e-6, 1e-6, "pool fwd")
    P0 = torch.empty_like(P)
    _lib.call("acvae_avg_pool2_fwd", X.cuda(), P0, N, H, W, C, 0.0, 0, 0, NULL, _lib.current_stream())
    close(nchw(P0), F.avg_pool2d(nchw(X.double()), 2), 1e-6, 1e-6, "pool fwd p=0")
    dP = torch.randn(N, Ho, Wo, C, generator=g)
    add = torch.randn(N, H, W, C, generator=g)
    dX = torch.empty(N, H, W, C, device="cuda")
    _lib.call("acvae_avg_pool2_bwd", dP.cuda(), add.cuda(), dX, N, H, W, C, 1, 0.2, 0, 0, mask.to(torch.uint8).cuda(),
              _lib.current_stream())
    xr = nchw(X.double()).requires_grad_(True)
    (F.avg_pool2d(xr, 2) * mask.double() / 0.8 * nchw(dP.double())).sum().backward()
    close(nchw(dX), xr.grad + nchw(add.double()), 1e-6, 1e-6, "pool bwd")
    dX1 = torch.empty(N, H, W, C, device="cuda")        # pool == 0: the identity sum of a basic block
    _lib.call("acvae_avg_pool2_bwd", add.cuda(), X.cuda(), dX1, N, H, W, C, 0, 0.0, 0, 0, NULL, _lib.current_stream())
    close(dX1, add.double() + X.double(), 1e-7, 1e-7, "grad add")


def test_new_kernels_use_no_scratch():
    from acvae_amd.build import resource_usage
    u = resource_usage()
    names = ["res_join", "conv1x1", "slab_sum", "avg_pool2", "positive_mask"]
    mine = {k: v for k, v in u.items() if any(n in k for n in names)}
    assert len(mine) >= 9, sorted(mine)
    assert all(v.get("scratch", 0) == 0 for v in mine.values()), {k: v.get("scratch") for k, v in mine.items()}


# ------------------------------------------------------------------------------------------------ fp64 restatement
P_SITE = [0.2] + [0.1] * 16 + [0.2, 0.2, 0.5, 0.5]


def make_state(seed, enc=None):
    """A non-degenerate state in the reference's layout: bn2.weight != 0, BN affines and running statistics spread."""
    torch.manual_seed(seed)
    enc = enc if enc is not None else ResNet38(64, 2048)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            if k.endswith(".weight") and v.dim() == 1:
                v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g))
            elif k.endswith(".bias") and not k.startswith("fc1"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_mean"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
    return enc


def ref_forward(st, feats, lens, training, masks, relu_force=None, probe=None):
    """fp64 restatement of ResNet38.forward; st: {name: tensor} (running buffers updated in place in training).  It runs at
    the state's dtype: tests/encoder_ref.py also evaluates it in fp32."""
    site = [0]

    def relu(z):
        if probe is not None:
            probe.append(z.detach().clone())
        i = site[0]; site[0] += 1
        if relu_force is not None:
            return z * relu_force[i].to(z.dtype)
        return torch.relu(z)

    def bn(x, p):
        return F.batch_norm(x, st[p + ".running_mean"], st[p + ".running_var"], st[p + ".weight"], st[p + ".bias"], training,
                            0.1, 1e-5)

    def drop(x, i):
        if not training:
            return x
        return x * masks[i].to(x.dtype) / (1.0 - P_SITE[i])

    def conv(x, p, pad=1):
        return F.conv2d(x, st[p], padding=pad)

    x = feats.to(st["bn0.weight"].dtype)[:, None]
    x = bn(x.transpose(1, 3), "bn0").transpose(1, 3)
    x = relu(bn(conv(x, "conv_block1.conv1.weight"), "conv_block1.bn1"))
    x = relu(bn(conv(x, "conv_block1.conv2.weight"), "conv_block1.bn2"))
    x = drop(F.avg_pool2d(x, 2), 0)
    k = 0
    for layer, n in enumerate((3, 4, 6, 3)):
        for i in range(n):
            p = f"resnet.layer{layer + 1}.{i}"
            ds = layer > 0 and i == 0
            out = F.avg_pool2d(x, 2) if ds else x
            out = drop(relu(bn(conv(out, p + ".conv1.weight"), p + ".bn1")), 1 + k)
            out = bn(conv(out, p + ".conv2.weight"), p + ".bn2")
            ident = bn(conv(F.avg_pool2d(x, 2), p + ".downsample.1.weight", 0), p + ".downsample.2") if ds else x
            x = relu(out + ident)
            k += 1
    x = drop(F.avg_pool2d(x, 2), 17)
    x = relu(bn(conv(x, "conv_block_after1.conv1.weight"), "conv_block_after1.bn1"))
    x = relu(bn(conv(x, "conv_block_after1.conv2.weight"), "conv_block_after1.bn2"))
    x = drop(x, 18)
    x = x.mean(3)
    pooled = drop(x.max(2)[0] + x.mean(2), 19)
    pooled = drop(torch.relu(F.linear(pooled, st["fc1.weight"], st["fc1.bias"])), 20)
    return {"audio_embeds": x.transpose(1, 2).contiguous(), "audio_embeds_pooled": pooled}


def ref_state(enc):
    st = {k: v.detach().cpu().double().clone() for k, v in enc.state_dict().items() if "num_batches" not in k}
    for k, v in st.items():
        if not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    return st


def random_masks(enc, N, T, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(s, generator=g) >= p for s, p in zip(enc.site_shapes(N, T)[1], P_SITE)]


def run_grads(enc, feats, lens, R, masks):
    enc.train()
    enc.keep_saved = True
    enc.dropout_masks = [m.to(torch.uint8) for m in masks]
    for p in enc.parameters():
        p.grad = None
    out = enc(feats.cuda(), lens)
    (out["audio_embeds"] * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out, {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("B,Tt,seed", [(2, 64, 1), (3, 72, 2), (2, 200, 3)])
def test_resnet38_forward_and_gradients_vs_fp64(B, Tt, seed):
    """Train mode with explicit dropout masks: outputs, running statistics and the lens mutation against fp64; then EVERY
    parameter gradient against autograd through the restatement evaluated under the HIP path's own ReLU decisions
    (tests/test_encoder_gpu.py::encoder_grads_vs_oracle explains the replay).  T = 72 and 200 put odd sizes in the stages
    (9 / 25 frames)."""
    enc = make_state(seed).cuda()
    g = torch.Generator().manual_seed(seed + 10)
    feats = torch.randn(B, Tt, 64, generator=g)
    R = torch.randn(B, Tt // 32, 2048, generator=g)
    lens = np.array([Tt] + [Tt - 7 * (i + 1) for i in range(B - 1)])
    masks = random_masks(enc, B, Tt, seed)
    st0 = ref_state(enc)
    probe = []
    with torch.no_grad():
        o0 = ref_forward(st0, feats, lens, True, masks, probe=probe)
    lens_in = lens.copy()
    out, grads = run_grads(enc, feats, lens_in, R, masks)
    assert (lens_in == lens // 32).all() and out["audio_embeds_lens_dev"].cpu().tolist() == (lens // 32).tolist()
    # 40 layers deep with batch statistics: fp32 against fp64 to 1e-3 relative (Cnn14's 6 ConvBlocks take 5e-4)
    close(out["audio_embeds"], o0["audio_embeds"], 1e-3, 1e-4, "audio_embeds")
    close(out["audio_embeds_pooled"], o0["audio_embeds_pooled"], 1e-3, 1e-4, "pooled")
    sd = enc.state_dict()
    for k in ["bn0.running_mean", "resnet.layer2.0.downsample.2.running_var", "resnet.layer4.2.bn2.running_mean",
              "conv_block_after1.bn2.running_var", "resnet.layer1.1.bn1.running_var"]:
        close(sd[k], st0[k], 1e-3, 1e-5, k)
    assert int(sd["resnet.layer3.0.bn2.num_batches_tracked"]) == 1
    relu = [m.cpu() for m in enc.relu_masks()]
    assert len(relu) == 36 == len(probe)
    zmax = 0.0
    for m, z in zip(relu, probe):
        d = m != (z > 0)
        if bool(d.any()):
            zmax = max(zmax, float(z[d].abs().max()))
    assert zmax < 1e-3, f"ReLU decisions differ from fp64 at |z| = {zmax:.2e}"
    st = ref_state(enc)
    o = ref_forward(st, feats, lens, True, masks, relu_force=relu)
    (o["audio_embeds"] * R.double()).sum().backward()
    worst, wk = 0.0, None
    n = 0
    for k, v in st.items():
        if k.startswith("fc1") or not v.requires_grad:
            assert k not in grads or not k.startswith("fc1")
            continue
        e = rel_l2(grads[k], v.grad)
        n += 1
        if e > worst:
            worst, wk = e, k
    assert n == 119 == len(grads)           # every BatchNorm affine and convolution weight; fc1 receives none
    print(f"worst gradient rel-L2 {worst:.2e} at {wk}")
    assert worst <= 1e-4, f"{wk}: relative L2 {worst:.2e}"     # measured 1.0-1.2e-5


def test_resnet38_eval_mode_vs_fp64():
    enc = make_state(7).cuda().eval()
    g = torch.Generator().manual_seed(17)
    feats = torch.randn(2, 96, 64, generator=g)
    st = ref_state(enc)
    with torch.no_grad():
        o = ref_forward(st, feats, [96, 90], False, None)
        out = enc(feats.cuda(), [96, 90])
    close(out["audio_embeds"], o["audio_embeds"], 1e-3, 1e-4, "eval audio_embeds")
    close(out["audio_embeds_pooled"], o["audio_embeds_pooled"], 1e-3, 1e-4, "eval pooled")
    assert int(enc.state_dict()["bn0.num_batches_tracked"]) == 0


def test_resnet38_backward_bit_reproducible():
    enc = make_state(4).cuda()
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(2, 72, 64, generator=g)
    R = torch.randn(2, 2, 2048, generator=g)
    masks = random_masks(enc, 2, 72, 4)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    _, g1 = run_grads(enc, feats, np.array([72, 60]), R, masks)
    enc.load_state_dict(sd)
    _, g2 = run_grads(enc, feats, np.array([72, 60]), R, masks)
    assert g1.keys() == g2.keys() and len(g1) == 119
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_resnet38_philox_dropout():
    enc = make_state(5).cuda().train()
    feats = torch.randn(2, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        a = enc(feats, [64, 64])["audio_embeds"]
        b = enc(feats, [64, 64])["audio_embeds"]
        assert not torch.equal(a, b)                         # fresh draws per call
        enc.p_block = enc.p_fc = 0.0
        c = enc(feats, [64, 64])["audio_embeds"]
        d = enc(feats, [64, 64])["audio_embeds"]
        assert torch.equal(c, d)                             # p = 0: deterministic
    # the expectation: a pool of raw activations with Philox dropout keeps the mean
    X = torch.rand(4, 64, 64, 128, device="cuda") + 1.0
    P = torch.empty(4, 32, 32, 128, device="cuda")
    _lib.call("acvae_avg_pool2_fwd", X, P, 4, 64, 64, 128, 0.2, 1234, 17, NULL, _lib.current_stream())
    ref = F.avg_pool2d(nchw(X), 2)
    kept = float((P != 0).float().mean())
    assert abs(kept - 0.8) < 0.01
    assert abs(float(P.mean() / ref.mean()) - 1.0) < 0.01


def test_resnet38_implicit_gemm_fallback_keeps_parity():
    """ACVAE_CONV_WINO=0 (read once per process, hence the child): every 3x3 layer on the implicit GEMM."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "forward_and_gradients_vs_fp64 and 72"], env=dict(os.environ, ACVAE_CONV_WINO="0"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ the model around it
def build_r38_model(V, E):
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.vae_model import Hybrid_VAEModel
    enc = make_state(11)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0, num_layers=1,
                                    rnn_type="GRU", attn_size=E)
    m = Hybrid_VAEModel(enc, dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E, "dropout": 0.0},
                        prior_model="PriorRNN", prior_args={"hidden_size": E, "dropout": 0.0})
    assert hasattr(m, "ln") and tuple(m.ln.weight.shape) == (E, 2048)
    return m.cuda()


def test_train_step_resnet38_matches_torch_adam_twin():
    import random
    import acvae_oracle as O
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import close as oclose
    V, E = 40, 512
    feats, caps, fl, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    m1 = build_r38_model(V, E).train()
    m3 = build_r38_model(V, E).train()
    m3.load_state_dict(m1.state_dict())
    for m in (m1, m3):
        m.encoder.p_block = m.encoder.p_fc = 0.0
    t1, t3 = TrainStep(m1, V), TrainStep(m3, V)
    deep = set(m1.encoder.conv_block_after1.parameters())
    assert t1.n_enc_deep == sum((p.numel() + 3) // 4 * 4 for p in deep)
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    for k in range(3):
        if k:
            with torch.no_grad():
                for a, b in zip(m1.parameters(), m3.parameters()):
                    b.copy_(a)
        torch.manual_seed(3 + k); random.seed(3 + k)
        t1.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
        torch.manual_seed(3 + k); random.seed(3 + k)
        for p in m3.parameters():
            p.grad = None
        loss, _, _ = t3.forward_loss(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], 1.0)
        opt.step()
        n = 0
        for (kk, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
            if b.grad is not None:
                oclose(b, a, 1e-5, 1e-6, what=f"step {k + 1} {kk}")
                n += 1
        assert n == 154                      # 119 encoder tensors (fc1 has no gradient here) + the text side's
    # checkpoint round trip
    import io
    buf = io.BytesIO()
    torch.save(m1.state_dict(), buf)
    buf.seek(0)
    m4 = build_r38_model(V, E)
    m4.load_state_dict(torch.load(buf))
    for (k, a), (_, b) in zip(m1.state_dict().items(), m4.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ g17: the reference itself
def ref_close(a, b, what):
    """Against the fp32 reference: both sides round through 40 layers (fp64 holds this path to 1e-3 / 1e-4 above, the
    reference's own error is of the same size), hence 1e-3 absolute on O(1) outputs, plus relative L2 <= 2e-4."""
    close(a, b, 1e-3, 1e-3, what)
    assert rel_l2(a, b) <= 2e-4, (what, rel_l2(a, b))


def test_g17_resnet38_matches_reference():
    """tests/golden/g17 (tools/make_resnet38_golden.py): the reference's ResNet38 on closed-form parameters, train mode
    with its 21 recorded dropout masks and eval mode, at (B, T) = (2, 64), (3, 96), (2, 200)."""
    import acvae_oracle as O
    from conftest import load_golden, unpack_masks
    g = load_golden("g17_resnet38_encoder")
    keys = [str(k) for k in g["keys"]]
    shapes = {k: tuple(int(x) for x in g["shapes"][i][:int(g["ndims"][i])]) for i, k in enumerate(keys)}
    state = O.closed_form_state(shapes)
    for ci in range(3):
        p = f"c{ci}_"
        feats = torch.from_numpy(g[p + "feats"])
        enc = ResNet38(64, 2048)
        enc.load_state_dict({k: v.clone() for k, v in state.items()})
        enc = enc.cuda().train()
        enc.dropout_masks = [m.to(torch.uint8) for m in unpack_masks(g, p)]
        assert len(enc.dropout_masks) == 21
        lens = g[p + "lens"].copy()
        with torch.no_grad():
            out = enc(feats.cuda(), lens)
        assert (lens == g[p + "lens_after"]).all()
        ref_close(out["audio_embeds"], g[p + "train_audio_embeds"], f"{p}train audio_embeds")
        ref_close(out["audio_embeds_pooled"], g[p + "train_pooled"], f"{p}train pooled")
        sd = enc.state_dict()
        for k in [n[len(p + "stat_"):] for n in g if n.startswith(p + "stat_")]:
            close(sd[k], g[p + "stat_" + k], 1e-3, 1e-5, k)
        assert int(sd["resnet.layer3.0.bn2.num_batches_tracked"]) == int(g[p + "nbt"])
        enc2 = ResNet38(64, 2048)
        enc2.load_state_dict({k: v.clone() for k, v in state.items()})
        enc2 = enc2.cuda().eval()
        with torch.no_grad():
            oe = enc2(feats.cuda(), g[p + "lens"].copy())
        ref_close(oe["audio_embeds"], g[p + "eval_audio_embeds"], f"{p}eval audio_embeds")
        ref_close(oe["audio_embeds_pooled"], g[p + "eval_pooled"], f"{p}eval pooled")
