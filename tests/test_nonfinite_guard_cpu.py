"""No GPU: the numpy twin of the guard's record (tests/guard_util.py) against a brute-force recomputation from the whole
history, four mutants of the twin that the comparison must catch, what TrainStep(nonfinite=, max_skips=) refuses before
anything is built, the header's declarations, and the checkpoint's ``step`` on a stub TrainStep over CPU tensors."""
import ctypes
import re

import numpy as np
import pytest
import torch

import guard_util as GU
from acvae_amd import _lib, trainer


sequence = GU.sequence


def run_twin(seq, kind, ema, warmup, mutant=None):
    """The twin over ``seq``; after every decision its record against the brute-force one.  -> first mismatch or None."""
    tw, history = GU.GuardTwin(mutant), []
    for calls, norm, lr, b1, b2 in seq:
        for loss, buf in calls:
            tw.witness(loss, buf)
        bad = any(GU.nonfinite(l) or GU.nonfinite(b) for l, b in calls)
        history.append((bad, norm, lr, b1, b2))
        tw.decide(norm, kind, lr, b1, b2, ema, warmup)
        want = GU.brute_force(history, kind, ema, warmup)
        for k, v in tw.fields().items():
            if v != want[k]:
                return f"decision {len(history)}: {k} {v} != {want[k]}"
        for k in ("step_size", "bc2_sqrt"):
            if not np.array_equal(getattr(tw, k).view(np.int32), want[k].view(np.int32)):
                return f"decision {len(history)}: {k}"
        if np.float32(tw.ema_w).view(np.int32) != np.float32(want["ema_w"]).view(np.int32):
            return f"decision {len(history)}: ema_w"
    return None


@pytest.mark.parametrize("kind, ema, warmup", [(GU.ADAM, 0.999, True), (GU.ADAM, 0.9, False), (GU.ADAM, -1.0, False),
                                               (GU.SGD, 0.5, True)])
def test_twin_equals_the_brute_force_record(kind, ema, warmup):
    for seed in range(4):
        seq = sequence(seed)
        oks = sum(1 for c, n, *_ in seq if np.isfinite(n) and not any(GU.nonfinite(l) or GU.nonfinite(b) for l, b in c))
        assert 10 < oks < len(seq) - 10                      # both kinds of decision, often
        assert run_twin(seq, kind, ema, warmup) is None


@pytest.mark.parametrize("mutant", ["t_before", "streak_kept", "flag_kept", "ema_on_skip"])
def test_mutants_are_caught(mutant):
    """t taken before the increment, streak not reset, window_bad not cleared, ema_updates moved on a skip."""
    assert run_twin(sequence(0), GU.ADAM, 0.999, True) is None
    assert run_twin(sequence(0), GU.ADAM, 0.999, True, mutant=mutant) is not None


def test_witness_is_an_or_and_finite_extremes_set_nothing():
    tw = GU.GuardTwin()
    fmax = np.finfo(np.float32).max
    tw.witness(np.float32(0.0), np.float32([0.0, -0.0, 1e-45, -1e-45, fmax, -fmax]))
    assert tw.window_bad == 0
    tw.witness(np.float32(1.0), np.float32([np.inf]))
    tw.witness(np.float32(1.0), np.float32([1.0]))
    assert tw.window_bad == 1
    assert tw.decide(np.float32(1.0), GU.SGD, [0.1]) == 0 and tw.window_bad == 0 and tw.streak == 1
    assert tw.decide(np.float32(1.0), GU.SGD, [0.1]) == 1 and tw.streak == 0 and tw.applied == 1
    dst, snap = np.ones(5, np.float32), np.zeros(5, np.float32)
    tw.restore(dst, snap)
    assert dst.all()
    tw.decide(np.float32(np.nan), GU.SGD, [0.1])
    tw.restore(dst, snap)
    assert not dst.any()


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.fixture
def no_library(monkeypatch):
    def used(*a, **k):
        raise AssertionError("the library was reached before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", used)
    monkeypatch.setattr(_lib, "call", used)
    monkeypatch.setattr(_lib, "require_cuda", used)


@pytest.mark.parametrize("kw, match", [
    (dict(nonfinite="raise"), "nonfinite"),
    (dict(nonfinite=True), "nonfinite"),
    (dict(nonfinite="Skip"), "nonfinite"),
    (dict(nonfinite="skip", max_skips=0), "max_skips"),
    (dict(nonfinite="skip", max_skips=-3), "max_skips"),
    (dict(nonfinite="skip", max_skips=2.0), "max_skips"),
    (dict(nonfinite="skip", max_skips=True), "max_skips"),
    (dict(nonfinite="skip", max_skips="5"), "max_skips"),
    (dict(max_skips=5), "nonfinite"),
    (dict(max_skips=None), "nonfinite"),
    (dict(nonfinite="skip", optimizer="SGD", optimizer_args={"momentum": 0.9}), "momentum"),
    (dict(nonfinite="skip", optimizer="SGD", optimizer_args={"momentum": 0.9, "nesterov": True}), "host"),
])
def test_constructor_refuses_before_anything_is_built(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        trainer.TrainStep(None, 40, **kw)


def test_check_guard_accepts_and_refuses():
    trainer.check_guard(None)
    trainer.check_guard("skip")
    trainer.check_guard("skip", 1)
    trainer.check_guard("skip", np.int64(7))
    trainer.check_guard("skip", None)
    trainer.check_guard("skip", 50, "SGD", [{"momentum": 0}])
    trainer.check_guard("skip", 50, "Adam", [{"betas": (0.9, 0.999)}])
    trainer.check_guard(None, optimizer="SGD", groups=[{"momentum": 0.9}])      # no guard: momentum is fine
    with pytest.raises(ValueError, match="momentum"):
        trainer.check_guard("skip", 50, "SGD", [{"momentum": 0}, {"momentum": 0.5}])
    assert trainer.DEFAULT_MAX_SKIPS == 50


# ---------------------------------------------------------------------------------------------------- header
def test_header_declares_and_library_exports_the_guard():
    P, I, L, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_float
    want = {
        "acvae_guard_witness": [("loss", P), ("buf", P), ("n_buf", L), ("record", P), ("stream", P)],
        "acvae_guard_decide": [("record", P), ("total_norm", P), ("kind", I), ("n_groups", I), ("lr", P), ("beta1", P),
                               ("beta2", P), ("ema_decay", D), ("ema_warmup", I), ("stream", P)],
        "acvae_ema_step_guarded": [("ema", P), ("params", P), ("n", L), ("record", P), ("stream", P)],
        "acvae_guard_restore": [("dst", P), ("snapshot", P), ("n", L), ("record", P), ("stream", P)],
    }
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in want.items():
        ret, got = _lib.PROTOS[name]
        assert ret is I and got == args, (name, got)
    for name in list(want) + ["acvae_adamw_groups_step_guarded", "acvae_sgd_groups_step_guarded"]:
        assert name in _lib.PROTOS and hasattr(so, name), name
    # the guarded steps are the grouped ones without `step` (SGD: without the momentum arguments), plus the record
    plain = [a for a, _ in _lib.PROTOS["acvae_adamw_groups_step"][1]]
    guarded = [a for a, _ in _lib.PROTOS["acvae_adamw_groups_step_guarded"][1]]
    assert guarded == [a for a in plain if a not in ("step", "stream")] + ["record", "stream"]
    src = open(_lib.HEADER).read()
    assert int(re.search(r"#define\s+ACVAE_ABI_VERSION\s+(\d+)", src).group(1)) == 3
    assert int(re.search(r"#define\s+ACVAE_GUARD_RECORD_BYTES\s+(\d+)", src).group(1)) == trainer.GUARD_RECORD_BYTES \
        == 4 * GU.RECORD_WORDS
    # the struct of the header, laid out by the C compiler's rules, is the layout the tests and the trainer read
    class Rec(ctypes.Structure):
        _fields_ = [("applied", L), ("skipped", L), ("streak", L), ("ema_updates", L), ("ok", ctypes.c_int32),
                    ("window_bad", ctypes.c_int32), ("step_size", F * 8), ("bc2_sqrt", F * 8), ("ema_w", F),
                    ("reserved", ctypes.c_int32)]
    assert ctypes.sizeof(Rec) == trainer.GUARD_RECORD_BYTES
    assert (Rec.ok.offset, Rec.window_bad.offset, Rec.step_size.offset, Rec.bc2_sqrt.offset, Rec.ema_w.offset) == \
        (32, 36, 40, 72, 104)
    assert trainer._GUARD_OK * 4 == Rec.ok.offset and trainer._GUARD_WINDOW_BAD * 4 == Rec.window_bad.offset


# ---------------------------------------------------------------------------------------------------- checkpoint on a stub
def stub(guard, applied, attempts):
    """A TrainStep that was never constructed: the attributes optimizer_state_dict / load_optimizer_state_dict read, over
    CPU tensors (building a real one needs a GPU)."""
    ps = [torch.nn.Parameter(torch.arange(6.0).reshape(2, 3)), torch.nn.Parameter(torch.ones(5))]
    ts = trainer.TrainStep.__new__(trainer.TrainStep)
    ts.order, ts.never, ts._group_lists = ps, set(), [ps]
    ts.optimizer_name, ts.step_count, ts._sgd_started = "Adam", attempts, set()
    total = sum((p.numel() + 3) // 4 * 4 for p in ps)
    ts.exp_avg, ts.exp_avg_sq, ts.max_exp_avg_sq, ts.momentum_buffer = torch.rand(total), torch.rand(total), None, None

    class Opt:
        param_groups = [dict(torch.optim.Adam([torch.zeros(1)]).defaults, params=ps)]
    ts.optimizer = Opt()
    ts.flat_ema, ts.accum_steps = None, 1
    ts._guard = None
    if guard:
        ts._guard = torch.zeros(GU.RECORD_WORDS, dtype=torch.int32)
        ts._guard_counters = ts._guard[:8].view(torch.int64)
        ts._guard_counters[0] = applied
        ts._guard_counters[1] = attempts - applied
        ts._guard_counters[2] = 3
    return ts


def test_checkpoint_step_is_the_applied_count():
    g = stub(True, applied=4, attempts=6)
    sd = g.optimizer_state_dict()
    assert [float(st["step"]) for st in sd["state"].values()] == [4.0, 4.0]
    # a guarded checkpoint into a guarded and into an unguarded TrainStep
    for guard in (True, False):
        t = stub(guard, applied=0, attempts=0)
        assert t.optimizer_state_dict()["state"] == {}            # nothing applied yet: no state, as torch
        t.load_optimizer_state_dict(sd)
        assert t.step_count == 4 and t._applied_count() == 4
        back = t.optimizer_state_dict()["state"]
        for i, st in sd["state"].items():                           # (the alignment padding between slices is not state)
            assert torch.equal(back[i]["exp_avg"], st["exp_avg"]) and torch.equal(back[i]["exp_avg_sq"], st["exp_avg_sq"])
        if guard:
            assert GU.read_record(t._guard)["applied"] == 4 and GU.read_record(t._guard)["streak"] == 0
        assert float(t.optimizer_state_dict()["state"][0]["step"]) == 4.0
    # an unguarded checkpoint (step = the host's count) into a guarded one
    u = stub(False, applied=7, attempts=7)
    t = stub(True, applied=1, attempts=2)
    t.load_optimizer_state_dict(u.optimizer_state_dict())
    assert GU.read_record(t._guard)["applied"] == 7 and t.step_count == 7
    assert t.state_dict()["step"] == 7
