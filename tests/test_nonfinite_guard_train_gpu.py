"""GPU: TrainStep(nonfinite="skip") on the golden-size model.  Clean batches equal the unguarded grouped path bit for bit; a
bad batch ([good, BAD, good]) leaves parameters, optimiser state, EMA, BatchNorm statistics and the bias-correction count as
a run that never saw it; windows, flush(), max_skips, checkpoints, schedulers and scst_step.

Feeding NaN / inf features is safe on this path by reading the kernels: no kernel of step() turns a float comparison into an
address.  The encoder's convolutions, BatchNorm and average pools are arithmetic only, its pooled head takes a value maximum
(time_pool_kernel: fmaxf), the posterior's pool_fwd_kernel starts its arg-max at 0 and moves it only to t < len, the attention
and the losses take value maxima and index with the caption's own integers.  The rollouts of scst_step are different
(row_stats_kernel's arg-max of an all-NaN row is no word index), so the scst case here is a clean batch only."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import guard_util as GU
import param_groups_util as U
from acvae_amd import optim
from acvae_amd.trainer import TrainStep
from scst_util import StubScorer, text_side
from test_model_gpu import build_model
from test_optim_gpu import compare_params, sync_params

pytestmark = pytest.mark.gpu
V, E = 40, 64
_CACHE = {}
GOOD1, GOOD2, GOOD3, BADSRC = (1, 3), (2, 2), (5, 3), (7, 3)     # (seed, B) of the micro-batches


def _state():
    if "state" not in _CACHE:
        _CACHE["state"] = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    return {k: v.clone() for k, v in _CACHE["state"].items()}


def batch(b):
    if b not in _CACHE:
        _CACHE[b] = O.synthetic_batch(b[1], 64, V, 7, seed=b[0], ragged=True)
    return _CACHE[b]


def fresh(groups=None, **kw):
    m = build_model(V, E, _state()).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    if groups is not None:
        kw["param_groups"] = groups(m)
    return m, TrainStep(m, V, **kw)


def halves(m):
    enc = list(m.encoder.parameters())
    ids = {id(p) for p in enc}
    return [{"params": enc}, {"params": [p for p in m.parameters() if id(p) not in ids]}]


def step(ts, b, seed=3, bad=None):
    """One step() on batch b; bad: None, "nan" (one NaN feature) or "inf" (+inf in one clip)."""
    feats, caps, fl, cl = batch(b)
    f = feats.clone()
    if bad == "nan":
        f[1, 5, 9] = float("nan")
    elif bad == "inf":
        f[0, 3, :4] = float("inf")
    torch.manual_seed(seed); random.seed(seed)
    return ts.step(f.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)


def snap(ts):
    """Clones of everything the contract names."""
    torch.cuda.synchronize()
    out = {"flat_p": ts.flat_p.clone(), "flat_buf": ts.flat_buf.clone()}
    out.update({k: v.clone() for k, v in ts._state_buffers().items()})
    if ts.flat_ema is not None:
        out["flat_ema"] = ts.flat_ema.clone()
    return out


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert U.same_bits(a[k], b[k]), f"{what}: {k} differs"


def assert_finite(s, what):
    for k, v in s.items():
        assert bool(torch.isfinite(v).all()), f"{what}: {k} is not finite"


# ---------------------------------------------------------------------------------------------------- clean runs
CLEAN = [("AdamW", {"weight_decay": 0.05}), ("AdamW", {"weight_decay": 0.05, "amsgrad": True}), ("SGD", {"lr": 1e-2})]


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip-one-group", "clip-two-groups"])
@pytest.mark.parametrize("name, args", CLEAN, ids=["AdamW", "AdamW-amsgrad", "SGD"])
def test_clean_batches_equal_the_unguarded_grouped_path(name, args, clip):
    """Three clean batches.  The twin has no guard and is on the grouped path through two groups with identical
    hyperparameters.  Without clipping the guarded run has ONE group (its one-group chunk table cuts the buffer elsewhere,
    which moves the norm's last bits but nothing else); with clipping both have the same two groups, so the norm and the clip
    coefficient are bit-equal too."""
    common = dict(optimizer=name, optimizer_args=args, max_grad_norm=clip, ema_decay=0.9, ema_warmup=True)
    m_g, t_g = fresh(groups=None if clip is None else halves, nonfinite="skip", **common)
    m_t, t_t = fresh(groups=halves, **common)
    assert t_t._guard is None and not hasattr(t_t, "_buf_snapshot")
    for k, b in enumerate((GOOD1, GOOD2, GOOD3)):
        pg, pt = step(t_g, b, 3 + k), step(t_t, b, 3 + k)
        assert U.same_bits(pg["loss"], pt["loss"])
        assert int(pg["update_ok"].item()) == 1 and "update_ok" not in pt
        if clip is not None:
            assert U.same_bits(pg["grad_norm"], pt["grad_norm"])
            assert U.same_bits(pg["grad_norm_groups"], pt["grad_norm_groups"])
        else:
            assert bool(torch.isfinite(pg["grad_norm"]).all()) and float(pg["grad_norm"]) > 0     # computed for the decision
        assert_same(snap(t_g), snap(t_t), f"{name} step {k + 1}")
    assert t_g.guard_counts() == {"applied": 3, "skipped": 0, "streak": 0}
    assert GU.read_record(t_g._guard)["ema_updates"] == 3
    t_g.synchronize()


def test_plain_adam_agrees_with_the_default():
    """Plain Adam's default path is the older acvae_adam_step, whose operation order differs from opt_elem's: held to the
    bound tests/test_param_groups_train_gpu.py holds that pair to (compare_params, parameters synchronised between steps)."""
    m_g, t_g = fresh(nonfinite="skip", max_grad_norm=None)
    m_d, t_d = fresh(max_grad_norm=None)
    for k in range(2):
        if k:
            sync_params(m_g, m_d)
        pg, pd = step(t_g, GOOD1, 3 + k), step(t_d, GOOD1, 3 + k)
        assert U.same_bits(pg["loss"], pd["loss"])
        compare_params(m_g, m_d, f"plain Adam step {k + 1}")


# ---------------------------------------------------------------------------------------------------- skips
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_a_bad_batch_is_skipped_and_leaves_no_trace(bad):
    """[good1, BAD, good2] against a twin fed [good1, good2]: everything the contract names, bit for bit, after each of the
    twin's steps.  Without the guard the model is NaN after step 2 for good."""
    kw = dict(optimizer="AdamW", optimizer_args={"weight_decay": 0.05}, ema_decay=0.9, ema_warmup=True, nonfinite="skip")
    m1, t1 = fresh(**kw)
    m2, t2 = fresh(**kw)
    p1, p2 = step(t1, GOOD1, 3), step(t2, GOOD1, 3)
    assert int(p1["update_ok"].item()) == 1
    after1 = snap(t1)
    assert_same(after1, snap(t2), "after good1")
    pb = step(t1, BADSRC, 4, bad=bad)
    assert int(pb["update_ok"].item()) == 0
    # which route the skip took (a ReLU may turn NaN activations into zeros: then only the witness sees the statistics)
    print(f"BAD ({bad}): loss finite {bool(torch.isfinite(pb['loss']).all())}, norm finite "
          f"{bool(torch.isfinite(pb['grad_norm']).all())}, flat_buf finite after the restore "
          f"{bool(torch.isfinite(t1.flat_buf).all())}")
    assert_same(snap(t1), after1, f"after BAD ({bad})")
    assert t1.guard_counts() == {"applied": 1, "skipped": 1, "streak": 1}
    p1, p2 = step(t1, GOOD2, 5), step(t2, GOOD2, 5)
    assert int(p1["update_ok"].item()) == 1
    assert U.same_bits(p1["loss"], p2["loss"]) and U.same_bits(p1["grad_norm"], p2["grad_norm"])
    s1 = snap(t1)
    assert_same(s1, snap(t2), "after good2")
    assert_finite(s1, "after good2")
    assert not U.same_bits(s1["flat_p"], after1["flat_p"])
    assert t1.guard_counts() == {"applied": 2, "skipped": 1, "streak": 0}
    assert t2.guard_counts() == {"applied": 2, "skipped": 0, "streak": 0}
    r1, r2 = GU.read_record(t1._guard), GU.read_record(t2._guard)
    assert r1["ema_updates"] == r2["ema_updates"] == 2
    assert np.array_equal(r1["step_size"], r2["step_size"]) and np.array_equal(r1["bc2_sqrt"], r2["bc2_sqrt"])
    assert t1.step_count == 3 and t2.step_count == 2          # attempts
    t1.synchronize()


def test_nan_statistics_with_finite_gradients_are_witnessed():
    """The quiet hole: a BatchNorm running statistic turns NaN while the gradients stay finite.  Planted between the forward
    and the update (in front of the witness launch): the norm is finite, the witness alone makes the step a skip, and the
    buffers come back bit for bit."""
    m, ts = fresh(nonfinite="skip", ema_decay=0.5)
    step(ts, GOOD1, 3)
    before = snap(ts)
    witness = ts._guard_witness

    def planted(loss):
        ts.flat_buf[ts.flat_buf.numel() // 2] = float("nan")
        witness(loss)
    ts._guard_witness = planted
    parts = step(ts, GOOD2, 4)
    ts._guard_witness = witness
    assert int(parts["update_ok"].item()) == 0
    assert bool(torch.isfinite(parts["grad_norm"]).all()) and bool(torch.isfinite(parts["loss"]).all())
    assert_same(snap(ts), before, "after the planted NaN")
    assert ts.guard_counts() == {"applied": 1, "skipped": 1, "streak": 1}
    parts = step(ts, GOOD2, 4)
    assert int(parts["update_ok"].item()) == 1
    assert_finite(snap(ts), "after the next good step")


def test_a_bad_micro_step_drops_the_whole_window_and_flush_likewise():
    kw = dict(accum_steps=2, ema_decay=0.9, nonfinite="skip")
    m1, t1 = fresh(**kw)
    m2, t2 = fresh(**kw)
    start = snap(t1)
    assert step(t1, GOOD1, 3)["applied"] is False
    parts = step(t1, BADSRC, 4, bad="nan")
    assert parts["applied"] is True and int(parts["update_ok"].item()) == 0
    assert_same(snap(t1), start, "after the dropped window")   # BatchNorm statistics of BOTH micro-steps taken back
    for k, b in enumerate((GOOD2, GOOD3)):
        pa, pb = step(t1, b, 5 + k), step(t2, b, 5 + k)
    assert pa["applied"] is True and int(pa["update_ok"].item()) == 1
    assert U.same_bits(pa["grad_norm"], pb["grad_norm"])
    good = snap(t1)
    assert_same(good, snap(t2), "after the good window")
    assert not U.same_bits(good["flat_p"], start["flat_p"])
    # a bad micro-step first (the NaN stays in flat_acc), flush() on the half window
    assert step(t1, BADSRC, 7, bad="inf")["applied"] is False
    assert t1.micro_count == 1
    out = t1.flush()
    assert out["applied"] is True
    assert_same(snap(t1), good, "after flush() on a bad half window")
    assert t1.guard_counts() == {"applied": 1, "skipped": 2, "streak": 1}
    assert t1.micro_count == 0 and t1.step_count == 3
    t1.synchronize()


def test_max_skips_raises_with_the_counts():
    m, ts = fresh(nonfinite="skip", max_skips=2)
    step(ts, GOOD1, 3)
    good = snap(ts)
    with pytest.raises(RuntimeError, match=r"max_skips=2.*applied 1, skipped 3, streak 3"):
        for k in range(3):
            step(ts, BADSRC, 4 + k, bad="nan")
        ts.synchronize()
    assert_same(snap(ts), good, "after three skipped steps")
    assert_finite(good, "the last applied update")
    # within the limit nothing raises
    m, ts = fresh(nonfinite="skip", max_skips=2)
    for k in range(2):
        step(ts, BADSRC, 4 + k, bad="nan")
    step(ts, GOOD1, 3)
    ts.synchronize()
    assert ts.guard_counts() == {"applied": 1, "skipped": 2, "streak": 0}


# ---------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_stores_the_applied_count_and_resumes_bit_for_bit():
    m1, t1 = fresh(nonfinite="skip", optimizer="AdamW")
    step(t1, GOOD1, 3)
    step(t1, BADSRC, 4, bad="nan")
    sd = t1.optimizer_state_dict()
    assert sd["state"] and all(float(st["step"]) == 1.0 for st in sd["state"].values())
    assert float(sd["state"][min(sd["state"])]["step"]) == 1.0 and t1.step_count == 2
    model_sd = {k: v.clone() for k, v in m1.state_dict().items()}
    m2, t2 = fresh(nonfinite="skip", optimizer="AdamW")
    m2.load_state_dict(model_sd)
    t2.load_optimizer_state_dict(sd)
    assert t2.guard_counts() == {"applied": 1, "skipped": 0, "streak": 0}
    assert_same(snap(t1), snap(t2), "after loading")
    step(t1, GOOD2, 5), step(t2, GOOD2, 5)
    assert_same(snap(t1), snap(t2), "the step after the checkpoint")
    # a checkpoint from an unguarded run into a guarded one, and back
    m3, t3 = fresh(groups=halves, optimizer="AdamW")
    m4, t4 = fresh(groups=halves, optimizer="AdamW", nonfinite="skip")
    for k in range(2):
        step(t3, GOOD1, 3 + k)
    m4.load_state_dict({k: v.clone() for k, v in m3.state_dict().items()})
    t4.load_optimizer_state_dict(t3.optimizer_state_dict())
    assert t4.guard_counts()["applied"] == 2
    step(t3, GOOD2, 5), step(t4, GOOD2, 5)
    assert_same(snap(t3), snap(t4), "unguarded checkpoint, guarded resume")
    m5, t5 = fresh(groups=halves, optimizer="AdamW")
    m5.load_state_dict({k: v.clone() for k, v in m4.state_dict().items()})
    t5.load_optimizer_state_dict(t4.optimizer_state_dict())
    assert t5.step_count == 3
    step(t3, GOOD3, 6), step(t5, GOOD3, 6)
    assert_same(snap(t3), snap(t5), "guarded checkpoint, unguarded resume")


# ---------------------------------------------------------------------------------------------------- schedulers
def test_scheduler_counts_attempts_and_bias_correction_counts_applied_updates():
    """split_params groups under LambdaLR with one skip in the middle: update k runs at the learning rate of attempt k with
    the bias correction of the applied updates before it, the rule TrainStep documents (torch.amp leaves the scheduler to
    the caller in the same way)."""
    from torch.optim.lr_scheduler import LambdaLR
    m = build_model(V, E, _state()).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    ts = TrainStep(m, V, optimizer="AdamW", param_groups=optim.split_params(m, encoder_lr=1e-4), nonfinite="skip")
    G = len(ts.optimizer.param_groups)
    assert G == 4
    base = [g["lr"] for g in ts.optimizer.param_groups]
    lam = lambda e: 1.0 / (1 + e)
    sched = LambdaLR(ts.optimizer, [lam] * G)
    oks = []
    for k, (b, bad) in enumerate([(GOOD1, None), (BADSRC, "nan"), (GOOD2, None)]):
        lrs = [g["lr"] for g in ts.optimizer.param_groups]
        assert lrs == pytest.approx([x * lam(k) for x in base], rel=1e-12)        # the lr of attempt k + 1
        oks.append(int(step(ts, b, 3 + k, bad=bad)["update_ok"].item()))
        sched.step()
    assert oks == [1, 0, 1]
    counts = ts.guard_counts()
    assert counts == {"applied": 2, "skipped": 1, "streak": 0} and sched.last_epoch == 3 == ts.step_count
    rec = GU.read_record(ts._guard)
    for k, g in enumerate(ts.optimizer.param_groups):
        want = GU.host_scalars(base[k] * lam(2), g["betas"][0], g["betas"][1], 2)       # attempt 3's lr, t = 2 applied
        assert rec["step_size"][k] == want[0] and rec["bc2_sqrt"][k] == want[1], (k, rec["step_size"][k], want)
        assert want[0] != GU.host_scalars(base[k] * lam(2), g["betas"][0], g["betas"][1], 3)[0]


# ---------------------------------------------------------------------------------------------------- scst_step
def test_scst_step_with_the_guard_equals_the_grouped_twin():
    feats, _, fl, _ = batch(GOOD1)
    vocab, keys, key2refs = text_side(V, 3, 1)
    f = feats.cuda()
    m_g, t_g = fresh(nonfinite="skip", optimizer="AdamW", max_grad_norm=None)
    m_t, t_t = fresh(groups=halves, optimizer="AdamW", max_grad_norm=None)
    outs = []
    for ts in (t_g, t_t):
        torch.manual_seed(3); random.seed(3)
        outs.append(ts.scst_step(f, fl.copy(), keys, key2refs, vocab, StubScorer(), max_length=10))
    assert int(outs[0]["update_ok"].item()) == 1
    assert torch.equal(outs[0]["sampled_seqs"], outs[1]["sampled_seqs"]) and U.same_bits(outs[0]["loss"], outs[1]["loss"])
    assert_same(snap(t_g), snap(t_t), "scst_step")
    assert t_g.guard_counts() == {"applied": 1, "skipped": 0, "streak": 0}
    t_g.synchronize()
