"""GPU: TrainStep(accum_steps=, ema_decay=, ema_warmup=) on the golden-size model: the defaults unchanged, the exact identity
k x (the same micro-batch) == one plain step, micro-steps that leave the model alone while flat_acc holds the running sum,
the applied update against a torch twin, flush(), LR schedulers, scst_step, and the weight EMA with its context manager and
checkpoint."""
import random
import warnings

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd.trainer import TrainStep, ema_decay_at
from scst_util import StubScorer, text_side
from test_model_gpu import build_model, close

pytestmark = pytest.mark.gpu
V, E = 40, 64
_CACHE = {}


def _state():
    return O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))


def batch(seed=1, B=3):
    if (seed, B) not in _CACHE:
        _CACHE[seed, B] = O.synthetic_batch(B, 64, V, 7, seed=seed, ragged=True)
    return _CACHE[seed, B]


THREE = [(1, 3), (2, 2), (5, 3)]          # (seed, B) of three different micro-batches, one of them B = 2


def fresh(**kw):
    m = build_model(V, E, _state()).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V, **kw)


def seed_all(seed):
    torch.manual_seed(seed); random.seed(seed)


def micro(ts, b=(1, 3), seed=3):
    feats, caps, fl, cl = batch(*b)
    seed_all(seed)
    return ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)


def twin_grads(t2, m2, b, seed):
    """forward_loss + backward on the twin; the gradients as CLONES (they are views of a buffer the next backward
    overwrites), .grad set back to None.  -> [clone or None per parameter]"""
    feats, caps, fl, cl = batch(*b)
    seed_all(seed)
    for p in m2.parameters():
        p.grad = None
    loss, _, _ = t2.forward_loss(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    loss.backward()
    out = [None if p.grad is None else p.grad.detach().clone() for p in m2.parameters()]
    for p in m2.parameters():
        p.grad = None
    return out


def flat_of(ts, model, per_param):
    """Per-parameter tensors (None: zeros) laid out as ts's flat buffers are."""
    flat = torch.zeros_like(ts.flat_g)
    offs = ts._offsets()
    for p, g in zip(model.parameters(), per_param):
        if g is not None and p in offs:
            flat[offs[p]:offs[p] + p.numel()].copy_(g.reshape(-1))
    return flat


def sync_params(src, dst):
    with torch.no_grad():
        for a, b in zip(src.parameters(), dst.parameters()):
            b.copy_(a)


def state_of(ts):
    return {k: v.clone() for k, v in ts._state_buffers().items()}


def bits(t):
    return t.detach().clone()


# ---------------------------------------------------------------------------------------------------- 1. defaults
def test_defaults_change_nothing():
    m1, t1 = fresh()
    m2, t2 = fresh(accum_steps=1, ema_decay=None)
    for t in (t1, t2):
        assert t.flat_acc is None and t.flat_ema is None and t.micro_count == 0
        assert set(t.state_dict()) == {"step", "exp_avg", "exp_avg_sq"}
        assert t.flush() is None
    for k in range(2):
        p1, p2 = micro(t1, seed=3 + k), micro(t2, seed=3 + k)
        assert torch.equal(p1["loss"], p2["loss"]) and torch.equal(p1["grad_norm"], p2["grad_norm"])
        assert set(p1) == set(p2) == {"ce", "kl", "mse", "loss", "grad_norm"}
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k
    assert torch.equal(t1.flat_p, t2.flat_p) and t1.step_count == t2.step_count == 2
    with pytest.raises(RuntimeError, match="ema_decay"):
        with t1.ema_weights():
            pass


# ---------------------------------------------------------------------------------------------------- 2. the exact identity
IDENTITY = [("Adam", {}), ("AdamW", {"weight_decay": 0.05, "amsgrad": True}),
            ("SGD", {"momentum": 0.9, "nesterov": True, "lr": 1e-2})]


@pytest.mark.parametrize("name, args", IDENTITY, ids=["Adam", "AdamW-amsgrad", "SGD-nesterov"])
def test_k_times_the_same_micro_batch_is_one_plain_step(name, args):
    """g + g (+ g + g) and the factors 1/2, 1/4 are exact in fp32, so the norm, the clip coefficient and every element of the
    update come out identical: parameters and optimiser state bit for bit."""
    m0, t0 = fresh(optimizer=name, optimizer_args=args)
    p0 = micro(t0)
    torch.cuda.synchronize()
    g = t0.flat_g[:t0.n_active].cpu()
    nz = g[g != 0].abs()
    # the identity needs 4 g and g / 4 exact: nothing within a factor 4 of overflow, nothing in the denormals
    assert nz.numel() > 0.5 * g.numel() and bool(torch.isfinite(g).all())
    assert float(nz.max()) < float(torch.finfo(torch.float32).max) / 4 and float(nz.min()) >= float(torch.finfo(torch.float32).tiny)
    for k in (2, 4):
        m, t = fresh(optimizer=name, optimizer_args=args, accum_steps=k)
        for j in range(k):
            parts = micro(t)
            assert parts["applied"] == (j == k - 1) and t.micro_count == (j + 1) % k
            assert torch.equal(parts["loss"], p0["loss"])
        torch.cuda.synchronize()
        assert t.step_count == 1
        assert torch.equal(parts["grad_norm"], p0["grad_norm"]), (k, float(parts["grad_norm"]), float(p0["grad_norm"]))
        for (key, a), (_, b) in zip(m.named_parameters(), m0.named_parameters()):
            assert torch.equal(a, b), (k, key)
        assert torch.equal(t.flat_p, t0.flat_p)
        s, s0 = t._state_buffers(), t0._state_buffers()
        assert set(s) == set(s0) and len(s) == {"Adam": 2, "AdamW": 3, "SGD": 1}[name]
        for key in s:
            assert torch.equal(s[key], s0[key]), (k, key)
            assert bool(s[key].any())


# ---------------------------------------------------------------------------------------------------- 3. micro-steps
def test_micro_steps_leave_the_model_alone_and_flat_acc_is_the_running_sum():
    k = 3
    m1, t1 = fresh(accum_steps=k)
    m2, t2 = fresh()
    for j, b in enumerate(THREE):                      # a first window, so that the optimiser state is not all zeros
        assert micro(t1, b, seed=3 + j)["applied"] == (j == k - 1)
    sync_params(m1, m2)
    torch.cuda.synchronize()
    assert t1.step_count == 1 and t1.micro_count == 0
    flat_p, state = bits(t1.flat_p), state_of(t1)
    assert all(bool(v.any()) for v in state.values())
    n = t1.n_active
    running = None
    for j, b in enumerate(THREE[:k - 1]):
        parts = micro(t1, b, seed=13 + j)
        g = flat_of(t2, m2, twin_grads(t2, m2, b, seed=13 + j))   # (t2 lays its buffers out as t1 does)
        running = g if running is None else running + g            # summed here, in micro-step order, not by autograd
        torch.cuda.synchronize()
        assert parts["applied"] is False and "grad_norm" not in parts and {"loss", "ce", "kl", "mse"} <= set(parts)
        assert t1.micro_count == j + 1 and t1.step_count == 1
        assert torch.equal(t1.flat_p, flat_p), f"micro-step {j + 1} moved the parameters"
        for key, v in state.items():
            assert torch.equal(t1._state_buffers()[key], v), (j, key)
        assert bool(running[:n].any())
        assert torch.equal(t1.flat_acc[:n].view(torch.int32), running[:n].view(torch.int32)), f"flat_acc after micro-step {j + 1}"
    assert not torch.equal(t1.flat_acc[:n], t1.flat_g[:n])


# ---------------------------------------------------------------------------------------------------- 4. torch twin
@pytest.mark.parametrize("name, args", [("Adam", {}), ("SGD", {"momentum": 0.9, "lr": 1e-2})], ids=["Adam", "SGD-momentum"])
def test_applied_update_against_a_torch_twin(name, args):
    k = 3
    m1, t1 = fresh(optimizer=name, optimizer_args=args, accum_steps=k)
    m3, t3 = fresh()
    opt = getattr(torch.optim, name)([p for p in m3.parameters() if p.requires_grad], **{"lr": 5e-4, **args})
    for window in range(2):
        if window:
            sync_params(m1, m3)
        before = bits(t1.flat_p)
        total = None
        for j, b in enumerate(THREE):
            seed = 3 + 10 * window + j
            parts = micro(t1, b, seed)
            gs = twin_grads(t3, m3, b, seed)
            total = gs if total is None else [a if c is None else (c if a is None else a + c) for a, c in zip(total, gs)]
        assert parts["applied"] is True
        for p, g in zip(m3.parameters(), total):
            p.grad = None if g is None else g / k
        with_grad = [p for p in m3.parameters() if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(with_grad, 1.0)
        opt.step()
        torch.cuda.synchronize()
        assert abs(float(parts["grad_norm"]) - float(norm)) <= 1e-5 * float(norm), (float(parts["grad_norm"]), float(norm))
        assert len(with_grad) > 10
        for (key, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
            if b.grad is not None:
                close(a, b, 1e-5, 1e-6, what=f"{name} window {window + 1} {key}")
        assert not torch.equal(t1.flat_p, before) and t1.step_count == window + 1


# ---------------------------------------------------------------------------------------------------- 5. flush
def test_flush_applies_a_partial_window():
    m_a, t_a = fresh(accum_steps=3)
    m_b, t_b = fresh(accum_steps=2)
    start = bits(t_a.flat_p)
    assert t_a.flush() is None                         # empty: nothing happens
    assert torch.equal(t_a.flat_p, start) and t_a.step_count == 0 and t_a.micro_count == 0
    for j, b in enumerate(THREE[:2]):
        pa, pb = micro(t_a, b, seed=3 + j), micro(t_b, b, seed=3 + j)
    assert pa["applied"] is False and pb["applied"] is True and t_a.micro_count == 2
    assert torch.equal(t_a.flat_p, start)
    out = t_a.flush()
    torch.cuda.synchronize()
    assert out["applied"] is True and torch.equal(out["grad_norm"], pb["grad_norm"])
    assert t_a.micro_count == 0 and t_a.step_count == 1
    assert torch.equal(t_a.flat_p, t_b.flat_p) and not torch.equal(t_a.flat_p, start)
    for key, v in t_a._state_buffers().items():
        assert torch.equal(v, t_b._state_buffers()[key]), key
    after = bits(t_a.flat_p)
    assert t_a.flush() is None and torch.equal(t_a.flat_p, after) and t_a.step_count == 1


# ---------------------------------------------------------------------------------------------------- 6. LR schedulers
def test_lr_scheduler_steps_once_per_applied_update():
    from torch.optim.lr_scheduler import LambdaLR
    m, ts = fresh(accum_steps=2)
    sched = LambdaLR(ts.optimizer, lambda e: 1.0 / (1 + e))
    lrs = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for j in range(4):
            lrs.append(ts.lr)
            if micro(ts, THREE[j % 3], seed=3 + j)["applied"]:
                sched.step()
    lrs.append(ts.lr)
    assert not [x for x in w if "optimizer.step()" in str(x.message)], [str(x.message) for x in w]
    assert lrs == pytest.approx([5e-4, 5e-4, 2.5e-4, 2.5e-4, 5e-4 / 3], rel=1e-12)
    assert ts.step_count == 2


# ---------------------------------------------------------------------------------------------------- 7. scst_step
def test_scst_step_accumulates():
    feats, _, fl, _ = batch()
    vocab, keys, key2refs = text_side(V, 3, 1)
    sc, f = StubScorer(), feats.cuda()

    def scst(ts):
        seed_all(3)
        return ts.scst_step(f, fl.copy(), keys, key2refs, vocab, sc, max_length=10)
    m0, t0 = fresh()
    p0 = scst(t0)
    m, t = fresh(accum_steps=2)
    start, state = bits(t.flat_p), state_of(t)
    p1 = scst(t)
    torch.cuda.synchronize()
    assert p1["applied"] is False and "grad_norm" not in p1 and torch.equal(p1["sampled_seqs"], p0["sampled_seqs"])
    assert torch.equal(t.flat_p, start) and t.step_count == 0
    for key, v in state.items():
        assert torch.equal(t._state_buffers()[key], v), key
    p2 = scst(t)
    torch.cuda.synchronize()
    assert p2["applied"] is True and torch.equal(p2["loss"], p0["loss"]) and torch.equal(p2["grad_norm"], p0["grad_norm"])
    assert torch.equal(t.flat_p, t0.flat_p) and not torch.equal(t.flat_p, start)
    for key, v in t._state_buffers().items():
        assert torch.equal(v, t0._state_buffers()[key]), key
    # the posterior got no gradient in either micro-step: left alone, with no optimiser state, as by the plain step
    offs = t._offsets()
    for key, p in m.named_parameters():
        if key.startswith(("qnet.", "mean_log_out.")):
            o = offs[p]
            assert torch.equal(p.detach().reshape(-1), start[o:o + p.numel()]), key
            assert not bool(t.exp_avg[o:o + p.numel()].any()), key
    t.synchronize()


# ---------------------------------------------------------------------------------------------------- 8. EMA
def lerp64(e, p, decay):
    w32 = np.float32(1.0 - decay)
    w = float(w32)
    return e + w * (p - e) if w32 < np.float32(0.5) else p - (p - e) * (1.0 - w)


@pytest.mark.parametrize("decay, warmup", [(0.5, False), (0.999, False), (0.999, True)], ids=["0.5", "0.999", "0.999-warmup"])
def test_ema_follows_the_float64_recurrence(decay, warmup):
    m, ts = fresh(ema_decay=decay, ema_warmup=warmup)
    assert torch.equal(ts.flat_ema, ts.flat_p) and ts.flat_ema.data_ptr() != ts.flat_p.data_ptr()
    assert set(ts.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "ema", "ema_updates"}
    e64 = ts.flat_p.cpu().double()
    bound = torch.zeros_like(e64)
    for t in range(3):
        prev = bits(ts.flat_ema)
        parts = micro(ts, THREE[t], seed=3 + t)
        assert "applied" not in parts
        torch.cuda.synchronize()
        p = ts.flat_p.cpu().double()
        d_t = ema_decay_at(decay, t, warmup)
        assert d_t == (min(decay, (1 + t) / (10 + t)) if warmup else decay)
        bound += 4 * 2.0 ** -24 * (prev.cpu().double().abs() + p.abs())       # this step's roundings; a lerp passes earlier error on at most once
        e64 = lerp64(e64, p, d_t)
        err = (ts.flat_ema.cpu().double() - e64).abs()
        assert bool((err <= bound).all()), f"update {t + 1}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp_min(1e-300)).max()):.2f}"
        assert not torch.equal(ts.flat_ema, prev) and not torch.equal(ts.flat_ema, ts.flat_p)
    assert ts.ema_updates == 3


def test_ema_moves_only_on_applied_updates():
    m, ts = fresh(accum_steps=2, ema_decay=0.9)
    assert set(ts.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "ema", "ema_updates", "micro_count"}
    for window in range(2):
        prev = bits(ts.flat_ema)
        assert micro(ts, THREE[0], seed=3 + window)["applied"] is False
        torch.cuda.synchronize()
        assert torch.equal(ts.flat_ema, prev) and ts.ema_updates == window
        assert micro(ts, THREE[1], seed=5 + window)["applied"] is True
        torch.cuda.synchronize()
        assert not torch.equal(ts.flat_ema, prev) and ts.ema_updates == window + 1


class StepCall:
    """One call of the step API (prior + decoder, a held encoder memory), as a validation loop's search makes it."""

    def __init__(self):
        g = torch.Generator().manual_seed(2)
        N, S = 5, 9
        self.mem = torch.randn(N, S, E, generator=g).cuda()
        self.lens = torch.tensor([9, 7, 4, 2, 1])
        self.word = torch.randint(0, V, (N, 1), generator=g)
        self.h, self.hp, self.cp = (torch.randn(1, N, E, generator=g).cuda() for _ in range(3))
        self.lz, self.eps = torch.randn(N, E, generator=g).cuda(), torch.randn(N, E, generator=g)

    def __call__(self, m):
        was = m.training
        m.eval()
        with torch.no_grad():
            p = m.pnet(self.word, self.mem, (self.hp, self.cp), self.lz, self.lens, eps=self.eps)
            d = m.decoder(word=self.word, state=self.h, enc_mem=self.mem, enc_mem_lens=self.lens, z=p["z"])
        torch.cuda.synchronize()
        m.train(was)
        return {"z": p["z"].clone(), "logits": d["logits"].clone(), "weights": d["weights"].clone()}


def greedy(m):
    feats, _, fl, _ = batch()
    was = m.training
    m.eval()
    seed_all(7)                                        # the prior's noise
    with torch.no_grad():
        out = m(feats.cuda(), fl.copy(), method="greedy", max_length=8)
    torch.cuda.synchronize()
    m.train(was)
    return out["logits"].clone()


def test_ema_weights_context_and_checkpoint():
    m, ts = fresh(ema_decay=0.5)
    for t in range(2):
        micro(ts, THREE[t], seed=3 + t)
    torch.cuda.synchronize()
    live, ema = bits(ts.flat_p), bits(ts.flat_ema)
    assert not torch.equal(live, ema)
    call = StepCall()
    outside, g_outside = call(m), greedy(m)            # fills the per-weight caches for the held memory
    assert m._encproj_cache
    sd_ema = ts.ema_state_dict()
    assert list(sd_ema) == list(m.state_dict())
    # a fresh model loaded from the averaged state dict: what the context must compute
    m_ref = build_model(V, E, {k: v.cpu() for k, v in sd_ema.items()})
    want, g_want = call(m_ref), greedy(m_ref)
    with ts.ema_weights() as inside_model:
        assert inside_model is m and torch.equal(ts.flat_p, ema) and torch.equal(ts.flat_ema, live)
        sd = m.state_dict()
        named = dict(m.named_parameters())
        for k, v in sd.items():
            assert torch.equal(v, sd_ema[k]), k         # the averaged parameters, the live buffers
            if k in named:
                assert v.data_ptr() == named[k].data_ptr()
        inside, g_inside = call(m), greedy(m)
        for k in inside:
            assert torch.equal(inside[k], want[k]), f"step API inside ema_weights(): {k} (a stale per-weight cache?)"
        assert torch.equal(g_inside, g_want)
        assert not torch.equal(inside["weights"], outside["weights"]) and not torch.equal(g_inside, g_outside)
        for refused in (lambda: micro(ts), lambda: ts.flush(),
                        lambda: ts.scst_step(None, None, None, None, None, StubScorer())):
            with pytest.raises(RuntimeError, match="ema_weights"):
                refused()
    assert torch.equal(ts.flat_p, live) and torch.equal(ts.flat_ema, ema)
    again = call(m)
    for k in again:
        assert torch.equal(again[k], outside[k]), f"step API after ema_weights(): {k}"
    with pytest.raises(KeyError):
        with ts.ema_weights():
            call(m)
            raise KeyError("the body raised")
    assert torch.equal(ts.flat_p, live) and torch.equal(ts.flat_ema, ema) and not ts._in_ema
    micro(ts, THREE[2], seed=9)                         # training goes on
    # checkpoint: ema_state_dict -> load_ema_state_dict on a fresh object
    m2, t2 = fresh(ema_decay=0.5)
    assert not torch.equal(t2.flat_ema, ema)
    t2.load_ema_state_dict({k: v.cpu() for k, v in sd_ema.items()})
    offs = t2._offsets()
    inflat = torch.zeros_like(ema, dtype=torch.bool)
    for p in m2.parameters():
        if p in offs:
            inflat[offs[p]:offs[p] + p.numel()] = True
    assert torch.equal(t2.flat_ema.view(torch.int32)[inflat], ema.view(torch.int32)[inflat])
    assert torch.equal(t2.flat_ema, ema)                # (the alignment padding between parameters is zero in both)
