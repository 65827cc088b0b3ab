"""Device-drawn dropout (the Philox branch of drop4 / drop_mul4 / dropout_keep) bit for bit against a host Philox.

Every other parity test passes an explicit keep-mask; every real training step draws on the device instead, and its backward
draws again, independently of its forward.  Here each kernel that draws is run twice - keep_mask = NULL, and the mask that
tests/philox_ref.py computes on the host from the stated rule - and the two runs must agree in every bit: forward outputs,
dY / dX, dgamma, dbeta, and at encoder level both outputs, every parameter gradient and every running statistic.  The
explicit-mask branch is held to fp64 by the other test files, so the equality carries that parity over to the branch that
trains.  Nothing here has a tolerance.  tests/test_philox_ref_cpu.py shows for each shape used here that a wrong counter,
order, index, word order, site, seed half or channel-chunk offset changes the host mask, i.e. fails these equalities.
"""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import philox_ref as R
from acvae_amd import _lib
from acvae_amd.encoder import Cnn10, Cnn14_16k, ResNet38, _PannsCnn

pytestmark = pytest.mark.gpu


def S():
    return _lib.current_stream()


def first_encoder_seed():
    """What _next_seed() returns first for _seed_base = SEED_BASE (the method itself, not a restatement)."""
    return _PannsCnn._next_seed(SimpleNamespace(_seed_base=R.SEED_BASE, _calls=0))


def draws():
    return [(seed, site, p) for seed in (R.SEED_HI, first_encoder_seed()) for site in R.SITES for p in R.PROBS]


@functools.lru_cache(maxsize=None)
def host_mask(seed, site, p, stored):
    """(keep-mask [N,C,H,W] uint8 as the keep_mask argument takes it, the same mask [N,H,W,C] bool) on the device."""
    N, H, W, C = stored
    m = R.keep_mask_nhwc(seed, site, p, stored)
    return (torch.from_numpy(np.ascontiguousarray(m.transpose(0, 3, 1, 2)).astype(np.uint8)).cuda(), torch.from_numpy(m).cuda())


def case_id(c):
    return "x".join(map(str, c[:4])) + f"-p{c[4]}"


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def inputs(case, dtype, seed=0):
    """Y = rand + 1 with bn = [1, 0, mean, invstd]: relu(bn(Y)) = Y > 0, so a zero output is a dropped one (bf16 too)."""
    N, H, W, C, pool = case
    g = torch.Generator().manual_seed(seed + 131 * H + C)
    Y = (torch.rand(N, H, W, C, generator=g) + 1.0).to(dtype).cuda()
    bn = torch.stack([torch.ones(C), torch.zeros(C), 1.5 + 0.1 * torch.randn(C, generator=g),
                      torch.rand(C, generator=g) + 0.5]).contiguous().cuda()
    Ns, Hs, Ws, _ = R.stored_shape(*case)
    dO = (torch.rand(Ns, Hs, Ws, C, generator=g) + 1.0).to(dtype).cuda()
    return Y, bn, dO


FWD = {"f32": ("acvae_bn_relu_pool_fwd", torch.float32), "bf16": ("acvae_bn_relu_pool_fwd_bf16", torch.bfloat16),
       "avg": ("acvae_avg_pool2_fwd", torch.float32)}


def forward(entry, case, Y, bn, p, seed, site, mask):
    N, H, W, C, pool = case
    name, dtype = FWD[entry]
    P = torch.full(R.stored_shape(*case), float("nan"), dtype=dtype, device="cuda")
    if entry == "avg":
        assert pool
        _lib.call(name, Y, P, N, H, W, C, p, seed, site, mask, S())
    else:
        _lib.call(name, Y, bn, P, N, H, W, C, pool, p, seed, site, mask, S())
    return P


def check_forward(entry, case, seed, site, p):
    Y, bn, _ = inputs(case, FWD[entry][1])
    mask, keep = host_mask(seed, site, p, R.stored_shape(*case))
    P = forward(entry, case, Y, bn, p, seed, site, None)
    assert bool(torch.isfinite(P).all())
    what = f"{entry} {case} seed {seed:#x} site {site} p {p}"
    differ = (P != 0) != keep
    assert not bool(differ.any()), f"{what}: {int(differ.sum())} of {keep.numel()} keep decisions differ from the host Philox"
    assert same_bits(P, forward(entry, case, Y, bn, p, seed, site, mask)), what
    return P, keep


# acvae_avg_pool2_fwd always pools: the pooled cases are its cases
FWD_CASES = [(entry, case) for entry in FWD for case in R.KERNEL_CASES if case[4] or entry != "avg"]


@pytest.mark.parametrize("entry,case", FWD_CASES, ids=[f"{e}-{case_id(c)}" for e, c in FWD_CASES])
def test_forward_draws_the_host_mask(entry, case):
    n = 0
    for seed, site, p in draws():
        _, keep = check_forward(entry, case, seed, site, p)
        n += keep.numel()
    print(f"{entry} {case}: {n} draws compared")


WRAP_CASES = [("f32", R.WRAP_SHAPES[0]), ("f32", R.WRAP_SHAPES[1]), ("avg", R.WRAP_SHAPES[1])]


@pytest.mark.parametrize("entry,case", WRAP_CASES, ids=[f"{e}-{case_id(c)}" for e, c in WRAP_CASES])
def test_forward_draws_the_host_mask_behind_one_pass_of_the_grid(entry, case):
    stored = R.stored_shape(*case)
    assert int(np.prod(stored)) // 4 > 8192 * 256
    _, keep = check_forward(entry, case, *R.WRAP_DRAW)
    print(f"{entry} {case}: {keep.numel()} draws compared")


# ------------------------------------------------------------------------------------------------ backward
def bn_backward(case, dtype, Y, bn, dO, upstream, training, p, seed, site, mask, ws, wsb):
    N, H, W, C, _ = case
    dY = torch.full((N, H, W, C), float("nan"), dtype=dtype, device="cuda")
    dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    _lib.call("acvae_bn_relu_bwd" + ("_bf16" if dtype == torch.bfloat16 else ""), Y, dO, upstream, bn, dg, db, dY, ws, wsb, N, H, W,
              C, training, p, seed, site, mask, S())
    return dY, dg, db


def check_bn_backward(case, dtype, seed, site, p, trainings=(1, 0)):
    """case = (N, H, W, C, pool): upstream 1 (dropout + pool) where pool, else 2 (dropout only)."""
    N, H, W, C, pool = case
    Y, bn, dO = inputs(case, dtype)
    mask, keep = host_mask(seed, site, p, R.stored_shape(*case))
    wsb = _lib.call("acvae_bn_workspace_bytes", N, H, W, C)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device="cuda")
    for training in trainings:
        a = bn_backward(case, dtype, Y, bn, dO, 1 if pool else 2, training, p, seed, site, None, ws, wsb)
        b = bn_backward(case, dtype, Y, bn, dO, 1 if pool else 2, training, p, seed, site, mask, ws, wsb)
        what = f"bn_relu_bwd {dtype} {case} training {training} seed {seed:#x} site {site} p {p}"
        for x, y, name in zip(a, b, ("dY", "dgamma", "dbeta")):
            assert bool(torch.isfinite(x).all()), (what, name)
            assert same_bits(x, y), f"{what}: {name} differs between the device draw and the host mask"
        if not training:       # evaluation-mode BatchNorm: dY = scale * g, non-zero exactly where the upstream element is kept
            dY = a[0]
            if pool:
                dY = dY[:, :2 * (H // 2), :2 * (W // 2)].reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4)
                assert bool(((dY != 0) == keep[..., None, None]).all()), what
                assert not bool(a[0][:, 2 * (H // 2):].any()) and not bool(a[0][:, :, 2 * (W // 2):].any()), what
            else:
                assert bool(((dY != 0) == keep).all()), what
    return keep.numel() * len(trainings)


@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=case_id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bn_relu_backward_redraws_its_forward_mask(dtype, case):
    n = sum(check_bn_backward(case, dtype, seed, site, p) for seed, site, p in draws())
    print(f"bn_relu_bwd {dtype} {case}: {n} draws compared")


def test_bn_relu_backward_redraws_its_forward_mask_behind_one_pass_of_the_grid():
    n = check_bn_backward(R.WRAP_SHAPES[1], torch.float32, *R.WRAP_DRAW, trainings=(1,))
    print(f"bn_relu_bwd {R.WRAP_SHAPES[1]}: {n} draws compared")


def avg_backward(case, dP, add, p, seed, site, mask):
    N, H, W, C, pool = case
    dX = torch.full((N, H, W, C), float("nan"), device="cuda")
    _lib.call("acvae_avg_pool2_bwd", dP, add, dX, N, H, W, C, pool, p, seed, site, mask, S())
    return dX


def check_avg_backward(case, seed, site, p):
    N, H, W, C, pool = case
    Y, _, dP = inputs(case, torch.float32, seed=1)
    mask, keep = host_mask(seed, site, p, R.stored_shape(*case))
    for add in (None, Y):
        a = avg_backward(case, dP, add, p, seed, site, None)
        what = f"avg_pool2_bwd {case} add {add is not None} seed {seed:#x} site {site} p {p}"
        assert bool(torch.isfinite(a).all()), what
        assert same_bits(a, avg_backward(case, dP, add, p, seed, site, mask)), what
        if add is None and not pool:
            assert bool(((a != 0) == keep).all()), what
    return 2 * keep.numel()


@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=case_id)
def test_avg_pool_backward_redraws_its_forward_mask(case):
    n = sum(check_avg_backward(case, seed, site, p) for seed, site, p in draws())
    print(f"avg_pool2_bwd {case}: {n} draws compared")


# ------------------------------------------------------------------------------------------------ the planted draw
@pytest.mark.parametrize("case", R.PLANT_CASES, ids=case_id)
def test_a_draw_exactly_at_p_is_kept_forward_and_backward(case):
    """Element 4 * PLANT_QUAD + PLANT_WORD of the stored tensor draws the 24-bit value 2^23 = 0.5 * 2^24: `>=` keeps it at
    p = 0.5 and `>` would drop it, in the forward and in each backward form."""
    N, H, W, C, pool = case
    seed, site, p = R.PLANT_SEED, R.PLANT_SITE, 0.5
    e = 4 * R.PLANT_QUAD + R.PLANT_WORD
    stored = R.stored_shape(*case)
    n, ho, wo, c = (int(i) for i in np.unravel_index(e, stored))
    for entry in ("f32", "bf16") + (("avg",) if pool else ()):
        P, keep = check_forward(entry, case, seed, site, p)
        assert bool(keep.reshape(-1)[e]) and float(P.reshape(-1)[e]) != 0.0, entry
    rows, cols = (slice(2 * ho, 2 * ho + 2), slice(2 * wo, 2 * wo + 2)) if pool else (slice(ho, ho + 1), slice(wo, wo + 1))
    for dtype in (torch.float32, torch.bfloat16):
        check_bn_backward(case, dtype, seed, site, p)
        Y, bn, dO = inputs(case, dtype)
        wsb = _lib.call("acvae_bn_workspace_bytes", N, H, W, C)
        ws = torch.empty(int(wsb), dtype=torch.uint8, device="cuda")
        dY, _, _ = bn_backward(case, dtype, Y, bn, dO, 1 if pool else 2, 0, p, seed, site, None, ws, wsb)
        assert bool((dY[n, rows, cols, c] != 0).all()), dtype
    check_avg_backward(case, seed, site, p)
    _, _, dP = inputs(case, torch.float32, seed=1)
    dX = avg_backward(case, dP, None, p, seed, site, None)
    assert bool((dX[n, rows, cols, c] != 0).all())


# ------------------------------------------------------------------------------------------------ encoders
ENCODERS = {"Cnn10": (Cnn10, 512, 80), "Cnn14_16k": (Cnn14_16k, 2048, 96), "ResNet38": (ResNet38, 2048, 72)}
N_CLIPS = 2


def make_encoder(name, dtype):
    """A non-degenerate state: BatchNorm affines and running statistics spread, ResNet38's bn2.weight away from its zero
    initialisation (a zero there would hide the residual branch, and its dropout sites, from both outputs)."""
    cls, width, _ = ENCODERS[name]
    torch.manual_seed(7)
    enc = cls(64, width)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            if k.endswith(".weight") and v.dim() == 1:
                v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g))
            elif k.endswith(".bias") and ("bn" in k or k.endswith(".2.bias")):          # BatchNorm biases (.2: downsample)
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_mean"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
    enc.compute_dtype = dtype
    enc._seed_base, enc._calls = R.ENCODER_SEED_BASE, 0
    return enc.cuda().train()


def record_seeds(enc):
    """Wrap the module's _next_seed: the list receives the seed of every forward."""
    seeds, inner = [], enc._next_seed

    def wrapped():
        seeds.append(inner())
        return seeds[-1]
    enc._next_seed = wrapped
    return seeds


def site_shapes(enc, name, T):
    """[N,C,H,W] of each block-level dropout site and [N,C] of the two head sites, in site order."""
    if name == "ResNet38":
        return enc.site_shapes(N_CLIPS, T)[1]
    chans, out, h, w = [64, 128, 256, 512, 1024, 2048], [], T, 64
    for b in range(enc.N_BLOCKS):
        if b < enc.N_BLOCKS - 1 or name == "Cnn10":          # Cnn14_16k's sixth block pools (1, 1)
            h, w = h // 2, w // 2
        out.append((N_CLIPS, chans[b], h, w))
    return out + [(N_CLIPS, enc.OUT_CHANNELS)] * 2


def site_probs(enc, name):
    """p of each site as the encoder driver passes it: p_block, half of it (in fp32) inside ResNet38's blocks, p_fc."""
    pb, pf = np.float32(enc.p_block), np.float32(enc.p_fc)
    if name == "ResNet38":
        probs = [pb] + [np.float32(0.5) * pb] * 16 + [pb, pb, pf, pf]
    else:
        probs = [pb] * enc.N_BLOCKS + [pf, pf]
    assert [np.float32(p) for p in R.ENCODER_SITE_PROBS[name]] == probs
    return probs


def host_masks(enc, name, T, seed):
    shapes, probs = site_shapes(enc, name, T), site_probs(enc, name)
    assert len(shapes) == len(probs) == enc._n_dropout_sites() == (21 if name == "ResNet38" else enc.N_BLOCKS + 2)
    masks = [R.keep_mask_nchw(seed, site, p, s) if len(s) == 4 else R.keep_mask_rows(seed, site, p, s)
             for site, (s, p) in enumerate(zip(shapes, probs))]
    return [torch.from_numpy(m) for m in masks], sum(m.size for m in masks)


def batch(T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N_CLIPS, T, 64, generator=g).cuda(), g


def weights(enc):
    """The parameters the encoder's autograd node differentiates (the pooled head's output carries no gradient)."""
    mine = {id(p) for p in enc._weights()}
    return {k: p for k, p in enc.named_parameters() if id(p) in mine}


def assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if not same_bits(a[k].float(), b[k].float())]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ between the device draw and the host's masks: {bad[:8]}"


ENCODER_CASES = [("Cnn10", "f32"), ("Cnn10", "bf16"), ("Cnn14_16k", "f32"), ("Cnn14_16k", "bf16"), ("ResNet38", "f32")]


@pytest.mark.parametrize("name,dtype", ENCODER_CASES, ids=[f"{n}-{d}" for n, d in ENCODER_CASES])
def test_encoder_step_with_device_dropout_equals_its_host_mask_twin(name, dtype):
    T = ENCODERS[name][2]
    enc_a = make_encoder(name, dtype)
    enc_b = copy.deepcopy(enc_a)
    seeds = record_seeds(enc_a)
    feats, g = batch(T, 3)

    def step(enc):
        out = enc(feats, [T] * N_CLIPS)
        ae, pooled = out["audio_embeds"], out["audio_embeds_pooled"]
        Rw = torch.randn(ae.shape, generator=torch.Generator().manual_seed(5)).cuda()
        (ae * Rw).sum().backward()
        return ({"audio_embeds": ae.detach(), "audio_embeds_pooled": pooled.detach()},
                {k: p.grad for k, p in weights(enc).items() if p.grad is not None}, dict(enc.named_buffers()))

    out_a, grads_a, stats_a = step(enc_a)                      # run A: dropout_masks = None, drawn on the device
    assert len(seeds) == 1 and seeds[0] >> 32
    enc_b.dropout_masks, n = host_masks(enc_b, name, T, seeds[0])
    out_b, grads_b, stats_b = step(enc_b)                      # run B: the host's masks
    assert bool(torch.isfinite(out_a["audio_embeds"]).all()) and bool((out_a["audio_embeds_pooled"] == 0).any())
    assert_same(out_a, out_b, f"{name} {dtype} outputs")
    assert_same(grads_a, grads_b, f"{name} {dtype} gradients")
    assert_same(stats_a, stats_b, f"{name} {dtype} running statistics")
    assert len(grads_a) == len(enc_a._weights()) and all(bool(g_.abs().sum() > 0) for g_ in grads_a.values())
    print(f"{name} {dtype}: {n} draws compared over {len(enc_b.dropout_masks)} sites, seed {seeds[0]:#x}")


def test_interleaved_backwards_use_the_seed_of_their_own_forward():
    """forward 1, forward 2, backward 2, backward 1 on one Cnn10: each call equals its explicit-mask twin built from the seed
    of call 1 and call 2 respectively."""
    name, T = "Cnn10", ENCODERS["Cnn10"][2]
    enc_a = make_encoder(name, "f32")
    enc_b = copy.deepcopy(enc_a)
    seeds = record_seeds(enc_a)
    x1, x2 = batch(T, 21)[0], batch(T, 22)[0]
    r1, r2 = (torch.randn(N_CLIPS, T // 16, 512, generator=torch.Generator().manual_seed(s)).cuda() for s in (31, 32))

    def run(enc, masks_of_call):
        outs = []
        for call, x in enumerate((x1, x2)):
            enc.dropout_masks = masks_of_call(call)
            outs.append(enc(x, [T] * N_CLIPS))
        w = weights(enc)
        g2 = torch.autograd.grad((outs[1]["audio_embeds"] * r2).sum(), list(w.values()))
        g1 = torch.autograd.grad((outs[0]["audio_embeds"] * r1).sum(), list(w.values()))
        return ([{k: o[k].detach() for k in ("audio_embeds", "audio_embeds_pooled")} for o in outs],
                [dict(zip(w, g1)), dict(zip(w, g2))], dict(enc.named_buffers()))

    outs_a, grads_a, stats_a = run(enc_a, lambda call: None)
    assert len(seeds) == 2 and seeds[0] != seeds[1]
    outs_b, grads_b, stats_b = run(enc_b, lambda call: host_masks(enc_b, name, T, seeds[call])[0])
    for call in (0, 1):
        assert_same(outs_a[call], outs_b[call], f"call {call + 1} outputs")
        assert_same(grads_a[call], grads_b[call], f"call {call + 1} gradients")
    assert_same(stats_a, stats_b, "running statistics")
    assert not torch.equal(outs_a[0]["audio_embeds_pooled"] == 0, outs_a[1]["audio_embeds_pooled"] == 0)
