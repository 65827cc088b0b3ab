"""The fp32 audio encoders (acvae_encoder_fwd / acvae_encoder_bwd_hooked: Cnn10, Cnn14_16k, ResNet38) restated on the CPU at any
dtype, and the yardstick the float64 run gives the HIP path - the encoder's twin of tests/decode_ref.py.  Nothing from the
HIP path enters this file but the ReLU decisions a caller hands in.

inputs()     what a Case feeds: features randn * 1.5 + 0.3, the upstream R of the loss (audio_embeds * R).sum(), dropout
             masks drawn by the oracle (Cnn10 / Cnn14_16k: torch.manual_seed(5), as tests/test_encoder_gpu.py draws them;
             ResNet38: test_resnet38_gpu.random_masks) and the state: closed form for Cnn10 / Cnn14_16k,
             test_resnet38_gpu.make_state for ResNet38.
reference()  O.cnn10_forward (ResNet38: test_resnet38_gpu.ref_forward) at `dtype` under given ReLU decisions (None: its own
             z > 0) and the backward of (audio_embeds * R).sum(): audio_embeds, audio_embeds_pooled, every parameter gradient
             and, in training, the batch's part of every running statistic (running - 0.9 old: the old value would hide it).
yardstick()  {tensor: (float64 value, alt)}: alt is the relative L2 of the fp32 reference from the float64 one under the SAME
             decisions - how far a correct fp32 evaluation in another summation order is from the truth.
ratio()      per tensor rel_l2(got, float64) / max(alt, floor); floor is the median alt over the case's gradient tensors, so
             that the tightest tensors (bn0.*, alt near 5e-8: one BatchNorm from the input) do not demand more than fp32
             gives.  The floor comes from the reference alone.

A tensor passes when its ratio is at most the family's MARGIN.  tests/test_encoder_ref_cpu.py shows that every Case is
admissible (median alt <= 5e-5) and that the bound flags the PLANTS below, each of which today's fixed bounds (2e-4 Cnn10,
5e-4 Cnn14_16k, relative L2) let through.

PLANTS are deliberately wrong variants of the oracle (one defect each), entered with `planted(name)`:
  eval_eps       BatchNorm's epsilon 2e-5 instead of 1e-5 in the evaluation-mode backward, every layer
  no_bessel      conv_block1's running_var takes the biased batch variance (no n / (n - 1)) in training
  bwd_count      conv_block1's BatchNorm backward divides its two sums by count - 1 instead of count in training
The last two sit in conv_block1 only: its count is B T 64 (12288 at B = 2, T = 96), so the defect is 8e-5 of the tensor; in
the last block (count B T / 8 ... B T / 16) the same defect is 1e-2 and today's bounds see it."""
import contextlib
import dataclasses
import functools
import statistics

import torch
import torch.nn.functional as F

import acvae_oracle as O

ARCHS = ("Cnn10", "Cnn14_16k", "ResNet38")
DIV = {"Cnn10": 16, "Cnn14_16k": 32, "ResNet38": 32}
WIDTH = {"Cnn10": 512, "Cnn14_16k": 2048, "ResNet38": 2048}
HEAD = {"Cnn10": "embed_pooled", "Cnn14_16k": "fc1", "ResNet38": "fc1"}
# Every tensor within MARGIN x the fp32 reference's distance from the float64 one.  tests/test_bf16_oracle_gpu.py's values for
# this comparison are 4.0 / 8.0 / 8.0; measured on the MI355X the fp32 HIP path's worst ratios are 5.03 (Cnn10), 8.06
# (Cnn14_16k) and 5.51 (ResNet38), so the first two are raised, to 1.6 and 1.5 times the measured worst.  The cause is
# rounding: an MFMA convolution adds its K = 9 Cin products (576 .. 18432) in ONE k-ordered chain, a random walk of
# 2^-24 sqrt(K) (tests/test_kernels_gpu.py chain_tol), while the CPU library behind the yardstick adds them in 16 or more
# interleaved partial sums (vector lanes x K blocks), sqrt(16) = 4 times less; the yardstick is the lucky one of two correct
# fp32 evaluations, more so the larger K (Cnn14_16k).  Measured for it (tests/test_encoder_composite_gpu.py): every tensor over
# 4.0 / 8.0 is a gradient behind the deep convolutions, 3e-6 .. 8e-6 from float64 in Cnn10 and 1.0e-5 in Cnn14_16k's
# evaluation mode - under chain_tol's 1e-5 floor for ONE kernel - and 5.7e-5 where BatchNorm over 16 values amplifies a
# yardstick of 7e-6; the Winograd and implicit-GEMM routes of the same case are equally far from float64 and as far from
# each other as two independent errors (d(a, b) = 0.8 .. 1.1 hypot(d(a, f64), d(b, f64))), and the tensors both routes compute
# with the same kernels are bit-equal between them and pass at 4.0: no part of the distance is shared glue.
MARGIN = {"Cnn10": 8.0, "Cnn14_16k": 12.0, "ResNet38": 8.0}
# |z| of the float64 replay below which a ReLU decision may differ (tests/test_encoder_gpu.py, tests/test_resnet38_gpu.py)
FLIP_ZONE = {"Cnn10": 1e-4, "Cnn14_16k": 1e-3, "ResNet38": 1e-3}
TODAY = {"Cnn10": 2e-4, "Cnn14_16k": 5e-4, "ResNet38": 1e-4}       # the fixed relative-L2 bounds of the fp32-oracle tests
ADMISSIBLE = 5e-5                   # median alt over the gradients: a tenth of grads_match_oracle's tol_enc = 5e-4
PLANTS = ("eval_eps", "no_bessel", "bwd_count")
PLANT_LAYER = "conv_block1."


@dataclasses.dataclass(frozen=True)
class Case:
    """One shape / mode of an encoder.  `route` and `hooked` say how the GPU test calls the HIP path; they do not enter the
    reference."""
    name: str
    arch: str
    B: int
    T: int
    mode: str = "train"               # train (explicit dropout masks) | train_p0 (p_block = p_fc = 0) | eval
    route: str = "default"            # default | igemm (ACVAE_CONV_WINO=0: every 3x3 layer on the implicit GEMM)
    hooked: bool = False              # _grad_ready_cb set: acvae_encoder_bwd_hooked with a block_done callback
    seed: int = 1

    def __post_init__(self):
        assert self.arch in ARCHS and self.mode in ("train", "train_p0", "eval") and self.route in ("default", "igemm")
        assert self.T >= DIV[self.arch] and self.B >= 1 and (self.arch != "ResNet38" or self.mode != "train_p0")

    @property
    def training(self):
        return self.mode != "eval"

    def ref_key(self):
        return dataclasses.replace(self, name="", route="default", hooked=False)


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).pow(2).sum().sqrt() / max(float(b.pow(2).sum().sqrt()), 1e-300))


# ---------------------------------------------------------------------------------------------------------- the inputs
def _r38():
    import test_resnet38_gpu as R38         # (imports the package, touches no device)
    return R38


@functools.lru_cache(maxsize=2)
def _r38_enc(seed):
    """The ResNet38 module (on the CPU) in the non-degenerate state of tests/test_resnet38_gpu.py."""
    return _r38().make_state(seed)


@functools.lru_cache(maxsize=None)
def _cnn_state(arch):
    if arch == "Cnn10":
        shapes = O.state_shapes(10)
    else:
        shapes = O.state_shapes(10, enc_embed=2048, encoder="Cnn14_16k")
    return O.closed_form_state({k: v for k, v in shapes.items() if k.startswith("encoder.")})


def state_of(case):
    """The encoder's state, fp32, keyed as its state dict (no "encoder." prefix).  Shared between calls: do not write to it."""
    if case.arch == "ResNet38":
        return {k: v.detach() for k, v in _r38_enc(case.seed).state_dict().items()}
    return {k[len("encoder."):]: v for k, v in _cnn_state(case.arch).items()}


def inputs(case):
    return _inputs(case.ref_key())


@functools.lru_cache(maxsize=4)
def _inputs(case):
    """dict(state, feats [B,T,64], R [B,T//div,C], lens, masks): masks is the list of keep masks in forward order for `train`,
    None otherwise.  Cached and shared: do not write to it."""
    g = torch.Generator().manual_seed(case.seed)
    feats = torch.randn(case.B, case.T, 64, generator=g) * 1.5 + 0.3
    R = torch.randn(case.B, case.T // DIV[case.arch], WIDTH[case.arch], generator=g)
    lens = [case.T] * case.B
    state = state_of(case)
    masks = None
    if case.mode == "train" and case.arch == "ResNet38":
        masks = _r38().random_masks(_r38_enc(case.seed), case.B, case.T, case.seed)
    elif case.mode == "train":
        masks = []
        torch.manual_seed(5)
        with torch.no_grad():
            O.cnn10_forward({"encoder." + k: v.clone() for k, v in state.items()}, feats, list(lens), True, None, masks)
    return dict(state=state, feats=feats, R=R, lens=lens, masks=masks)


# ---------------------------------------------------------------------------------------------------------- the reference
@contextlib.contextmanager
def _no_dropout():
    """O.cnn10_forward's dropout probabilities are the reference's constants; p_block = p_fc = 0 is the identity."""
    orig = O._dropout
    O._dropout = lambda x, p, training, masks, record: x
    try:
        yield
    finally:
        O._dropout = orig


def reference(case, relu_masks=None, dtype=torch.float64, probe=None):
    """-> {tensor: value at `dtype`}.  relu_masks: one bool tensor [N,C,H,W] per ReLU site in forward order, or None for the
    run's own z > 0.  probe (a list) receives every site's pre-activation."""
    d = inputs(case)
    st0, training = d["state"], case.training
    feats, R = d["feats"].to(dtype), d["R"].to(dtype)
    masks = [m.clone() for m in d["masks"]] if d["masks"] is not None else None
    force = None if relu_masks is None else {i: m for i, m in enumerate(relu_masks)}
    head = HEAD[case.arch]
    st = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in st0.items()}
    leaves = [k for k, v in st.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))]
    for k in leaves:
        st[k].requires_grad_(True)
    if case.arch == "ResNet38":
        fst = {k: v for k, v in st.items() if "num_batches" not in k}
        o = _r38().ref_forward(fst, feats, d["lens"], training, masks, relu_force=force, probe=probe)
    else:
        pst = {"encoder." + k: v for k, v in st.items()}
        with (_no_dropout() if case.mode == "train_p0" else contextlib.nullcontext()):
            o = O.cnn10_forward(pst, feats, list(d["lens"]), training, masks, None, relu_probe=probe, relu_force=force)
    (o["audio_embeds"] * R).sum().backward()
    out = {"audio_embeds": o["audio_embeds"].detach(), "audio_embeds_pooled": o["audio_embeds_pooled"].detach()}
    for k in leaves:
        if k.startswith(head + "."):
            assert st[k].grad is None, k           # the pooled head is not on the way to audio_embeds
            continue
        out[k] = st[k].grad
    for k, v in st.items():
        if k.endswith(("running_mean", "running_var")):
            if training:
                out[k] = v.detach().double() - 0.9 * st0[k].double()      # (in float64 at either dtype: the stored value is judged)
            else:
                assert torch.equal(v, st0[k].to(dtype)), k
    return out


def gradient_keys(y):
    return [k for k in y if not k.startswith("audio_embeds") and not k.endswith(("running_mean", "running_var"))]


def yardstick_z(case, relu_masks=None):
    """({tensor: (float64 value, alt)}, the float64 run's pre-activations per ReLU site).  relu_masks None: the float64 run's
    own decisions, which the fp32 run is then held to as well."""
    z = []
    r64 = reference(case, relu_masks, torch.float64, probe=z)
    masks = [v > 0 for v in z] if relu_masks is None else relu_masks
    r32 = reference(case, masks, torch.float32)
    assert set(r32) == set(r64)
    return {k: (v, rel_l2(r32[k], v)) for k, v in r64.items()}, z


@functools.lru_cache(maxsize=3)          # (a Cnn14_16k or ResNet38 entry holds 0.6 GB of float64 gradients)
def _yardstick(key):
    return yardstick_z(key)[0]


def yardstick(case, relu_masks=None):
    """{tensor: (float64 value, alt)}; with the reference's own decisions it is cached per Case."""
    if relu_masks is None:
        return _yardstick(case.ref_key())
    return yardstick_z(case, relu_masks)[0]


def floor_of(y):
    """The median alt over the gradient tensors."""
    return statistics.median(y[k][1] for k in gradient_keys(y))


def ratio(got, case, relu_masks=None, y=None):
    """{tensor: rel_l2(got, float64) / max(alt, floor)} over every tensor of the yardstick (y: one already computed for these
    decisions).  A tensor missing from `got` is an error."""
    y = yardstick(case, relu_masks) if y is None else y
    assert set(got) == set(y), sorted(set(got) ^ set(y))
    floor = floor_of(y)
    return {k: rel_l2(got[k], ref) / max(alt, floor) for k, (ref, alt) in y.items()}


# ---------------------------------------------------------------------------------------------------------- planted errors
class _BnCountMinus1(torch.autograd.Function):
    """Training BatchNorm whose backward takes its two means over count - 1."""

    @staticmethod
    def forward(ctx, x, w, b, y):
        mean = x.mean((0, 2, 3), keepdim=True)
        invstd = (x.var((0, 2, 3), unbiased=False, keepdim=True) + 1e-5).rsqrt()
        ctx.save_for_backward((x - mean) * invstd, invstd, w)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        xhat, invstd, w = ctx.saved_tensors
        m = xhat.numel() // xhat.shape[1] - 1
        sg, sgx = g.sum((0, 2, 3), keepdim=True), (g * xhat).sum((0, 2, 3), keepdim=True)
        dx = w.view(1, -1, 1, 1) * invstd * (g - sg / m - xhat * sgx / m)
        return dx, sgx.flatten(), sg.flatten(), None


@contextlib.contextmanager
def planted(name):
    """Run the oracle (O.cnn10_forward) with one PLANT in its BatchNorm."""
    assert name in PLANTS, name
    orig = O._bn

    def bn(state, p, x, training):
        rv = state[p + ".running_var"]
        old = rv.clone()
        y = orig(state, p, x, training)
        here = p[len("encoder."):].startswith(PLANT_LAYER)
        if name == "eval_eps" and not training:
            bad = F.batch_norm(x, state[p + ".running_mean"], rv, state[p + ".weight"], state[p + ".bias"], False, 0.1, 2e-5)
            return y.detach() + bad - bad.detach()              # the forward's value, the wrong epsilon's gradient
        if name == "no_bessel" and training and here:
            rv.data.copy_(0.9 * old + 0.1 * x.detach().var((0, 2, 3), unbiased=False))     # (.data: autograd saved the buffer)
        if name == "bwd_count" and training and here:
            return _BnCountMinus1.apply(x, state[p + ".weight"], state[p + ".bias"], y.detach())
        return y
    O._bn = bn
    try:
        yield
    finally:
        O._bn = orig


# ---------------------------------------------------------------------------------------------------------- the cases
def _c(arch, B, T, mode="train", **kw):
    tag = {"Cnn10": "cnn10", "Cnn14_16k": "cnn14", "ResNet38": "r38"}[arch]
    name = f"{tag}-B{B}_T{T}-{mode}" + ("-igemm" if kw.get("route") == "igemm" else "") + ("-hooked" if kw.get("hooked") else "")
    return Case(name, arch, B, T, mode, **kw)


# The smallest shapes at which each branch of the driver (csrc/encoder.hip) can go wrong.  Seeds: the first that
# tests/test_encoder_ref_cpu.py admits (median alt <= 5e-5), found with the reference alone.
CASES = [
    # Cnn10 (time / 16).  T = 16: one output frame, block 4 at H = 2; T = 47: odd heights 47 / 23 / 11 / 5 in front of every pool;
    # T = 250: 250 / 125 / 62 / 31; B = 5, T = 40: heights 5 and W < 4 beside them; B = 33, T = 16: a 128-pixel tile of block 4
    # (H = 2, W = 8) spans eight clips
    _c("Cnn10", 1, 16), _c("Cnn10", 3, 47), _c("Cnn10", 2, 96), _c("Cnn10", 2, 250), _c("Cnn10", 5, 40), _c("Cnn10", 33, 16),
    # evaluation mode: running statistics in both directions, the data gradient's filter images built at backward time, the
    # first conv's folded BatchNorm backward with running statistics
    _c("Cnn10", 1, 16, "eval"), _c("Cnn10", 3, 47, "eval"), _c("Cnn10", 2, 96, "eval"),
    # p_block = p_fc = 0 in training.  B = 1, T = 16 normalises block 4 over 16 values: seed 1 has median alt 6.1e-5 (not
    # admissible), seeds 2 .. 6 have 3.8e-5, 1.6e-4, 2.4e-5, 6.5e-5, 4.5e-5; seed 4, the smallest
    _c("Cnn10", 1, 16, "train_p0", seed=4), _c("Cnn10", 3, 47, "train_p0"), _c("Cnn10", 2, 96, "train_p0"),
    _c("Cnn10", 3, 47, route="igemm"), _c("Cnn10", 2, 96, "eval", route="igemm"),
    _c("Cnn10", 2, 96, hooked=True),
    # Cnn14_16k (time / 32).  T = 95: 95 / 47 / 23 / 11 / 5, block 6 at H = 2; T = 32: block 6 at H = 1, W = 2 (implicit GEMM
    # beside Winograd layers).  In training B = 3, T = 32 normalises over 6 values (median alt 2.2e-4: not admissible); B = 8 does.
    _c("Cnn14_16k", 4, 64), _c("Cnn14_16k", 2, 95), _c("Cnn14_16k", 4, 128),
    _c("Cnn14_16k", 4, 64, "eval"), _c("Cnn14_16k", 2, 95, "eval"), _c("Cnn14_16k", 4, 128, "eval"),
    _c("Cnn14_16k", 3, 32, "eval"), _c("Cnn14_16k", 8, 32),
    _c("Cnn14_16k", 4, 64, route="igemm"),
    # ResNet38 (time / 32): T = 72 puts 9 frames (odd) in front of the stride-2 pool of layer 3
    _c("ResNet38", 2, 64), _c("ResNet38", 3, 72), _c("ResNet38", 2, 64, "eval"), _c("ResNet38", 3, 72, "eval"),
]
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
