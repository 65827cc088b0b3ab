"""GPU: the fused Adam(amsgrad) / AdamW / SGD updates against torch.optim, and TrainStep driven through its
torch.optim.Optimizer façade: end to end against a torch-optimiser twin, under LR schedulers, across checkpoints, with a
parameter that has no gradient, and with the default (Adam) path unchanged."""
import io
import random
import warnings

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from test_model_gpu import build_model, close

pytestmark = pytest.mark.gpu
V, E = 40, 64
N = (1 << 20) + 3                       # not a multiple of four: the scalar tail runs
PAD = 8                                 # guard elements behind every buffer: must come back untouched


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
    it rounds, and no term exceeds the largest total change of the tensor, max|ref - start| (moments and buffers are sums
    of a few scaled gradients; a parameter's update is a few lr); where terms cancel, the element itself can be far
    smaller than that.  Bound: 8 ulp of the element (the parameter's own roundings, three steps) + 16 ulp of the largest
    change.  A wrong formula (bias correction, decay, dampening, nesterov term, first-step rule) moves elements by
    percent of the change, orders of magnitude above this.  Elements flagged `loose` are held to `loose_tol` only."""
    got, ref, start = got.detach().cpu().double(), ref.detach().cpu().double(), start.detach().cpu().double()
    s = float((ref - start).abs().max())
    assert s > 0, f"{what}: the reference did not move"
    tol = 1e-6 * ref.abs() + 2e-6 * s
    if loose is not None:
        tol = torch.where(loose, torch.full_like(tol, loose_tol), tol)
    err = (got - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max err/tol {float((err / tol).max()):.2f}, max err {float(err.max()):.3e}"


KERNEL_CASES = [
    ("Adam", dict(weight_decay=0.05, amsgrad=False)),
    ("Adam", dict(weight_decay=0.05, amsgrad=True)),
    ("AdamW", dict(weight_decay=0.01, amsgrad=False)),
    ("AdamW", dict(weight_decay=0.1, amsgrad=True)),
    ("SGD", dict()),
    ("SGD", dict(momentum=0.9, dampening=0.3)),
    ("SGD", dict(momentum=0.9, nesterov=True)),
    ("SGD", dict(momentum=0.8, weight_decay=0.05)),
]


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("name, opts", KERNEL_CASES, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in o.items())}"
                                                         for n, o in KERNEL_CASES])
def test_kernel_matches_torch_optim(name, opts, clip):
    """Three updates with different gradients, grad_scale 0.5, the clip coefficient from the device-side norm (active:
    max_norm well below the norm; inactive: far above); torch.optim.<X>(foreach=False) on CPU fp32 copies gets its
    gradient scaled by the same fp32 coefficient."""
    gen = torch.Generator().manual_seed(7)
    lr = 1e-3 if name != "SGD" else 1e-2
    p0 = torch.randn(N, generator=gen)
    grads = [torch.randn(N, generator=gen) * s for s in (1.0, 0.3, 2.0)]
    gscale = 0.5
    max_norm = 100.0 if clip else 1e6            # 0.5 * ||g|| is ~150..1000
    adam = name != "SGD"
    mom = opts.get("momentum", 0.0)

    def padded(x):
        t = torch.full((N + PAD,), 7.0, device="cuda")
        t[:N].copy_(x)
        return t
    p = padded(p0)
    st = [padded(torch.zeros(N)) for _ in range(3)]
    partials = torch.empty(_lib.call("acvae_grad_norm_partials"), device="cuda")
    tn = torch.zeros(1, device="cuda")
    ref = torch.nn.Parameter(p0.clone())
    opt = getattr(torch.optim, name)([ref], lr=lr, foreach=False, **opts)
    s = _lib.current_stream()
    # Adam with L2 decay: g' = coef*g + wd*p can cancel, and a one-ulp difference delta in g' (an ulp of its terms, ~1e-8,
    # not of the small result) moves the update g'/(|g'| + eps) by lr*eps*delta/|g'|^2, above the bound of `agree` once
    # |g'| < ~3e-5.  Those elements (a few hundred of the million) are held to the bound of three steps, 3 * 10 * lr, and
    # may be at most 0.1 % of the tensor; their moments, which see that parameter again through wd*p, to 1e-3 of the
    # tensor's largest value.
    loose = torch.zeros(N, dtype=torch.bool)
    for k, g in enumerate(grads):
        gd = padded(g)
        _lib.call("acvae_grad_norm", gd, N, gscale, partials, tn, s)
        if adam:
            _lib.call("acvae_adamw_step", p, gd, st[0], st[1], st[2] if opts["amsgrad"] else None, N, lr, 0.9, 0.999, 1e-8,
                      opts["weight_decay"], int(name == "AdamW"), int(opts["amsgrad"]), k + 1, gscale, max_norm, tn, s)
        else:
            _lib.call("acvae_sgd_step", p, gd, st[0] if mom else None, N, lr, mom, opts.get("dampening", 0.0),
                      opts.get("weight_decay", 0.0), int(opts.get("nesterov", False)), int(k == 0), gscale, max_norm, tn, s)
        c = coef_of(float(tn.item()), gscale, max_norm)
        assert (c < gscale) == clip, (c, float(tn.item()))
        ref.grad = g * torch.tensor(c, dtype=torch.float32)
        if adam and name == "Adam":
            gp = ref.grad.double() + opts["weight_decay"] * ref.detach().double()
            loose |= gp.abs() < 3e-5
        opt.step()
    torch.cuda.synchronize()
    for t in [p] + st:
        assert bool((t[N:] == 7.0).all()), "a kernel wrote past the end of its buffer"
    assert int(loose.sum()) <= N // 1000, int(loose.sum())
    agree(p[:N], ref.detach(), p0, "param", loose, 30 * lr)
    so = opt.state[ref]
    if adam:
        for i, key in enumerate(("exp_avg", "exp_avg_sq", "max_exp_avg_sq")[:3 if opts["amsgrad"] else 2]):
            agree(st[i][:N], so[key], torch.zeros(N), key, loose, 1e-3 * float(so[key].abs().max()))
    elif mom:
        agree(st[0][:N], so["momentum_buffer"], torch.zeros(N), "momentum_buffer")
    else:
        assert bool((st[0] == torch.cat([torch.zeros(N), torch.full((PAD,), 7.0)]).cuda()).all())   # plain SGD: no state


# ---------------------------------------------------------------------------------------------------- TrainStep
def _state():
    return O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))


_BATCH = {}


def _batch():
    if not _BATCH:
        _BATCH["b"] = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    return _BATCH["b"]


def fresh(state=None, **kw):
    from acvae_amd.trainer import TrainStep
    m = build_model(V, E, _state() if state is None else state).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V, **kw)


def one(ts, seed=3):
    feats, caps, fl, cl = _batch()
    torch.manual_seed(seed); random.seed(seed)
    return ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)


def twin_step(t3, m3, opt, seed=3, max_norm=1.0):
    """The reference's loop body on a twin: forward_loss -> backward -> clip_grad_norm_ -> the torch optimiser."""
    feats, caps, fl, cl = _batch()
    torch.manual_seed(seed); random.seed(seed)
    for p in m3.parameters():
        p.grad = None
    loss, _, _ = t3.forward_loss(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    loss.backward()
    torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], max_norm)
    opt.step()


def compare_params(m1, m3, what):
    n = 0
    for (k, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
        if b.grad is not None:
            close(b, a, 1e-5, 1e-6, what=f"{what} {k}")
            n += 1
    assert n > 10


def sync_params(src, dst):
    """Start the next step of both runs from the same parameters: the HIP forward/backward is deterministic, so both then
    see bit-identical gradients and only the optimiser arithmetic differs (a one-ulp difference in a parameter could
    otherwise flip a ReLU decision upstream and move a whole encoder gradient by ~1 %)."""
    with torch.no_grad():
        for a, b in zip(src.parameters(), dst.parameters()):
            b.copy_(a)


TWIN_CASES = [
    ("AdamW", {"weight_decay": 0.05, "amsgrad": True}),
    ("AdamW", {}),
    ("SGD", {"momentum": 0.9, "nesterov": True, "weight_decay": 1e-3, "lr": 1e-2}),
]


@pytest.mark.parametrize("name, args", TWIN_CASES, ids=["AdamW-amsgrad", "AdamW", "SGD-nesterov"])
def test_train_step_matches_torch_optimizer_twin(name, args):
    m1, t1 = fresh(optimizer=name, optimizer_args=args)
    m3, t3 = fresh()
    opt = getattr(torch.optim, name)([p for p in m3.parameters() if p.requires_grad], **{"lr": 5e-4, **args})
    assert t1.optimizer.param_groups[0]["weight_decay"] == opt.param_groups[0]["weight_decay"]
    for k in range(2):
        if k:
            sync_params(m1, m3)
        before = [p.detach().clone() for p in m1.parameters()]
        one(t1, seed=3 + k)
        twin_step(t3, m3, opt, seed=3 + k)
        compare_params(m1, m3, f"{name} step {k + 1}")
        assert any(not torch.equal(a, b) for a, b in zip(before, m1.parameters()))


def test_lr_schedulers_drive_the_fused_update():
    """LambdaLR, ExponentialLR and ReduceLROnPlateau over ts.optimizer give the parameters of a run that sets ts.lr by hand
    to the same values before each step, bit for bit, and see optimizer.step() called (no order warning)."""
    from torch.optim import lr_scheduler as S
    m_a, t_a = fresh(optimizer="AdamW")
    m_b, t_b = fresh(optimizer="AdamW")
    scheds = [S.LambdaLR(t_a.optimizer, lambda e: 1.0 / (1 + e)), S.ExponentialLR(t_a.optimizer, gamma=0.5)]
    lrs = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for k in range(3):
            lrs.append(t_a.lr)
            one(t_a, seed=3 + k)
            for s in scheds:
                s.step()
    assert not [x for x in w if "optimizer.step()" in str(x.message)], [str(x.message) for x in w]
    assert lrs[0] == 5e-4 and lrs[2] < lrs[1] < lrs[0]
    plateau = S.ReduceLROnPlateau(t_a.optimizer, mode="min", factor=0.1, patience=0)
    plateau.step(1.0)
    lr_before = t_a.optimizer.param_groups[0]["lr"]
    plateau.step(2.0)                                                  # worse: lr drops by 10x
    assert t_a.optimizer.param_groups[0]["lr"] == pytest.approx(lr_before * 0.1, rel=1e-12)
    lrs.append(t_a.lr)
    one(t_a, seed=6)
    for k, lr in enumerate(lrs):
        t_b.lr = lr
        one(t_b, seed=3 + k)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m_a.named_parameters(), m_b.named_parameters()):
        assert torch.equal(a, b), k


def test_one_cycle_cycles_sgd_momentum_like_torch():
    """OneCycleLR(cycle_momentum=True) over an SGD TrainStep matches torch SGD + OneCycleLR for three steps: lr and
    momentum are read from the param group on every step."""
    from torch.optim.lr_scheduler import OneCycleLR
    args = {"momentum": 0.9, "lr": 1e-2}
    m1, t1 = fresh(optimizer="SGD", optimizer_args=args)
    m3, t3 = fresh()
    opt = torch.optim.SGD([p for p in m3.parameters() if p.requires_grad], **args)
    kw = dict(max_lr=5e-2, total_steps=6, base_momentum=0.7, max_momentum=0.95, cycle_momentum=True)
    s1, s3 = OneCycleLR(t1.optimizer, **kw), OneCycleLR(opt, **kw)
    moms = []
    for k in range(3):
        if k:
            sync_params(m1, m3)
        moms.append(t1.optimizer.param_groups[0]["momentum"])
        assert moms[-1] == opt.param_groups[0]["momentum"] and t1.lr == opt.param_groups[0]["lr"]
        one(t1, seed=3 + k)
        twin_step(t3, m3, opt, seed=3 + k)
        s1.step(); s3.step()
        compare_params(m1, m3, f"OneCycle SGD step {k + 1}")
        for p1, p3 in zip(m1.parameters(), m3.parameters()):
            if p3.grad is not None:
                off = t1._offsets()[p1]
                close(t1.momentum_buffer[off:off + p1.numel()].view_as(p1), opt.state[p3]["momentum_buffer"], 1e-5, 1e-6,
                      what="momentum_buffer")
    assert len(set(moms)) >= 2, moms


@pytest.mark.parametrize("name, args", [("SGD", {"momentum": 0.9, "dampening": 0.1, "lr": 1e-2}),
                                        ("AdamW", {"amsgrad": True, "weight_decay": 0.05})], ids=["SGD", "AdamW-amsgrad"])
def test_checkpoint_round_trip_and_torch_compat(name, args):
    """{"model", "optimizer": ts.optimizer.state_dict()} resumes bit for bit, and loads into the torch class over the
    restored model, which then takes the same next step."""
    m1, t1 = fresh(optimizer=name, optimizer_args=args)
    one(t1)
    buf = io.BytesIO()
    torch.save({"model": m1.state_dict(), "optimizer": t1.optimizer.state_dict()}, buf)
    one(t1, seed=4)
    ck = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    keys = set(getattr(torch.optim, name)([torch.zeros(1, requires_grad=True)]).defaults) | {"params"}
    assert set(ck["optimizer"]["param_groups"][0]) == keys
    st0 = next(iter(ck["optimizer"]["state"].values()))
    assert set(st0) == ({"momentum_buffer"} if name == "SGD" else {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"})
    m2, t2 = fresh(optimizer=name, optimizer_args=args)
    m2.load_state_dict(ck["model"])
    t2.optimizer.load_state_dict(ck["optimizer"])
    one(t2, seed=4)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    m3, t3 = fresh()
    m3.load_state_dict(ck["model"])
    opt = getattr(torch.optim, name)([p for p in m3.parameters() if p.requires_grad], lr=1.0)
    opt.load_state_dict(ck["optimizer"])
    twin_step(t3, m3, opt, seed=4)
    compare_params(m1, m3, f"torch {name} vs fused")


def test_sgd_momentum_leaves_parameters_without_gradient_alone():
    """torch.optim.SGD gives a parameter whose .grad is None no buffer and no update; at its first gradient the buffer
    starts from that gradient itself (no dampening), while the others apply momentum*buf + (1-dampening)*g."""
    m, ts = fresh(optimizer="SGD", optimizer_args={"momentum": 0.9, "dampening": 0.5, "lr": 1e-2})
    victim = m.decoder.attn.v
    other = m.decoder.classifier.bias
    orig = ts._check_grad_aliasing
    drop = [True]

    def drop_then_check():
        if drop[0]:
            victim.grad = None                      # as if this parameter had not taken part in the step
        return orig()
    ts._check_grad_aliasing = drop_then_check
    offs = ts._offsets()
    v_before = victim.detach().clone()
    one(ts)
    torch.cuda.synchronize()
    assert torch.equal(victim.detach(), v_before), "a parameter without gradient was moved"
    assert victim not in ts._sgd_started and other in ts._sgd_started
    ov, oo = offs[victim], offs[other]
    assert not bool(ts.momentum_buffer[ov:ov + victim.numel()].any()), "it got a buffer"
    idx = {id(p): i for i, p in enumerate(m.parameters())}
    assert idx[id(victim)] not in ts.optimizer.state_dict()["state"]
    o_buf1 = ts.momentum_buffer[oo:oo + other.numel()].clone()
    drop[0] = False
    one(ts, seed=4)
    torch.cuda.synchronize()
    c = coef_of(float(ts.total_norm.item()), 1.0, 1.0)
    gv = victim.grad.detach() * torch.tensor(c, dtype=torch.float32, device="cuda")
    go = other.grad.detach() * torch.tensor(c, dtype=torch.float32, device="cuda")
    close(ts.momentum_buffer[ov:ov + victim.numel()].view_as(victim), gv, 1e-6, 1e-12, what="first buffer = gradient")
    close(victim.detach(), v_before - 1e-2 * gv, 1e-6, 1e-9, what="victim moved by -lr*g")
    close(ts.momentum_buffer[oo:oo + other.numel()], 0.9 * o_buf1 + 0.5 * go.reshape(-1), 1e-6, 1e-12,
          what="later buffer = momentum*buf + (1-dampening)*g")
    assert victim in ts._sgd_started


def test_default_optimizer_is_unchanged_adam():
    """TrainStep(model, V) and TrainStep(model, V, optimizer="Adam") are the same fused Adam, bit for bit, with the same
    state and nothing more; calling optimizer.step() outside TrainStep.step raises."""
    from acvae_amd.optim import FlatOptimizer
    m1, t1 = fresh()
    m2, t2 = fresh(optimizer="Adam")
    assert isinstance(t1.optimizer, torch.optim.Optimizer) and isinstance(t1.optimizer, FlatOptimizer)
    assert t1.max_exp_avg_sq is None and t1.momentum_buffer is None
    assert (t1.lr, t1.betas, t1.eps, t1.weight_decay) == (5e-4, (0.9, 0.999), 1e-8, 0)
    for k in range(2):
        one(t1, seed=3 + k)
        one(t2, seed=3 + k)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k
    assert torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    with pytest.raises(RuntimeError, match="TrainStep.step"):
        t1.optimizer.step()
    m3, t3 = fresh(optimizer="SGD")
    assert t3.exp_avg is None and t3.exp_avg_sq is None and t3.momentum_buffer is None
