"""CPU: the float64 yardstick of the KL objective (tests/kl_objective_util.py) against torch autograd and a brute-force
loop, the mutants it must flag, every refusal of KLObjective / TrainStep's keywords in front of any library call, and
kl_weight_cyclical at hand-computed points."""
import math

import numpy as np
import pytest
import torch

import kl_objective_util as K
from text_ref import D as F64, ratio

SHAPE = (3, 5, 6)
LENS = [5, 2, 0]


def _lam(ref, over):
    vals = ref["dims"] if over == "dim" else ref["s_c"][ref["mask"]]
    return K.place_lam(vals)[0]


def _modes():
    return [pytest.param(red, fb, over, id=f"{red}-{fb}-{over}") for red, fb, over in K.MODES] + \
        [pytest.param(red, None, "cell", id=f"{red}-None-cell") for red in ("all", "valid")]


def _torch_value(ts, lens, red, lam, over):
    """The same formula with torch.clamp / torch.where, for autograd."""
    mu_q, lv_q, mu_p, lv_p = ts
    R, T, E = mu_q.shape
    k = lv_p / 2. - lv_q / 2. + (torch.exp(lv_q) + (mu_q - mu_p) ** 2.) / (2. * torch.exp(lv_p)) - .5
    mask = K.cell_mask(lens, R, T, red)
    Dv = int(mask.sum())
    kS = torch.where(mask[:, :, None], k, torch.zeros_like(k))
    if lam is None:
        return kS.sum() / Dv
    if over == "dim":
        return torch.clamp(kS.sum((0, 1)) / Dv, min=lam).sum()
    return torch.where(mask, torch.clamp(kS.sum(-1), min=lam), torch.zeros(R, T, dtype=k.dtype)).sum() / Dv


@pytest.mark.parametrize("red,fb,over", _modes())
def test_yardstick_gradient_is_autograd_of_the_formula(red, fb, over):
    ts = [t.to(F64) for t in K.case(*SHAPE, seed=3)[:4]]
    base = K.objective(*ts, LENS, red, None, over)
    lam = None if fb is None else _lam(base, over)
    ref = K.objective(*ts, LENS, red, lam, over)
    if lam is not None:                     # the case exercises the gate: some open, some closed
        g = ref["gates"] if over == "dim" else ref["gates"][ref["mask"]]
        assert 0 < int(g.sum()) < g.numel()
    leaves = [t.clone().requires_grad_(True) for t in ts]
    val = _torch_value(leaves, LENS, red, lam, over)
    (val * 1.7).backward()
    assert abs(float(val.detach()) - float(ref["value"])) <= 1e-14 * max(1.0, abs(float(val.detach())))
    for got, leaf in zip(K.gradients(*ts, ref, g=1.7), leaves):
        assert ratio(got, leaf.grad, 1e-13 * (1 + leaf.grad.abs())) <= 1.0
        if red == "valid":                  # exact zeros outside S
            assert float(got[~ref["mask"]].abs().max()) == 0.0


@pytest.mark.parametrize("red,fb,over", _modes())
def test_yardstick_against_a_brute_force_loop(red, fb, over):
    ts = [t.to(F64) for t in K.case(*SHAPE, seed=4)[:4]]
    mu_q, lv_q, mu_p, lv_p = ts
    R, T, E = SHAPE
    lam = None if fb is None else _lam(K.objective(*ts, LENS, red, None, over), over)
    ref = K.objective(*ts, LENS, red, lam, over)
    cells = [(r, t) for r in range(R) for t in range(T) if red == "all" or t < LENS[r]]
    Dn = len(cells)
    k = {}
    for r, t in cells:
        for e in range(E):
            a, b, c, d = (float(x[r, t, e]) for x in ts)
            k[r, t, e] = d / 2 - b / 2 + (math.exp(b) + (a - c) ** 2) / (2 * math.exp(d)) - .5
    m = [sum(k[r, t, e] for r, t in cells) / Dn for e in range(E)]
    s = {c: sum(k[c + (e,)] for e in range(E)) for c in cells}
    if lam is None:
        val, n_open = sum(m), (E if over == "dim" else Dn)
    elif over == "dim":
        val, n_open = sum(max(x, lam) for x in m), sum(x > lam for x in m)
    else:
        val, n_open = sum(max(x, lam) for x in s.values()) / Dn, sum(x > lam for x in s.values())
    steps = [sum(s[r, t] for r in range(R) if (r, t) in s) / max(1, sum((r, t) in s for r in range(R))) for t in range(T)]
    assert ref["D"] == Dn and ref["gates_open"] == n_open
    assert abs(float(ref["value"]) - val) <= 1e-13 * max(1.0, abs(val))
    assert abs(float(ref["raw"]) - sum(m)) <= 1e-13 * max(1.0, abs(sum(m)))
    assert ratio(ref["dims"], torch.tensor(m, dtype=F64), 1e-13) <= 1.0
    assert ratio(ref["steps"], torch.tensor(steps, dtype=F64), 1e-13) <= 1.0


def _planted():
    """(inputs, lens) with dimension 1 at q == p in every cell (m_e exactly 0: the tie of lam = 0.0) and a NaN and an inf
    in padded cells."""
    mu_q, lv_q, mu_p, lv_p, _ = K.case(*SHAPE, seed=5)
    mu_p[:, :, 1] = mu_q[:, :, 1]
    lv_p[:, :, 1] = lv_q[:, :, 1]
    mu_q[1, 3, 0] = float("nan")
    lv_p[2, 0, 2] = float("inf")
    return (mu_q, lv_q, mu_p, lv_p), LENS


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_yardstick_flags_the_mutants(mutant):
    ts, lens = _planted()
    over = "dim"
    clean = [torch.where(K.cell_mask(lens, *SHAPE[:2], "valid")[:, :, None], t, torch.zeros_like(t)) for t in ts]
    lam = 0.0 if mutant == "gate_not_strict" else _lam(K.objective(*clean, lens, "valid", None, over), over)
    ref = K.objective(*ts, lens, "valid", lam, over)
    assert bool(torch.isfinite(ref["value"])) and float(ref["dims"][1]) == 0.0
    tol = K.forward_tols(*ts, ref)
    mut = K.objective(*ts, lens, "valid", lam, over, mutant=mutant)
    if mutant == "gate_not_strict":         # the tie: closed for the yardstick (and a zero gradient), open for the mutant
        assert not bool(ref["gates"][1]) and bool(mut["gates"][1])
        assert mut["gates_open"] == ref["gates_open"] + 1
        return
    if mutant in ("padded_times_zero", "mask_ignored"):
        assert not bool(torch.isfinite(mut["value"]))      # the padded NaN leaked
        return
    assert ratio(mut["value"], ref["value"], 100 * tol["value"]) > 1.0, mutant
    if mutant == "clamp_other_axis":
        assert not torch.equal(mut["gate_full"], ref["gate_full"])


def test_padded_values_change_nothing_and_a_valid_nan_does():
    ts, lens = _planted()
    clean = [torch.where(K.cell_mask(lens, *SHAPE[:2], "valid")[:, :, None], t, torch.zeros_like(t)) for t in ts]
    for fb, over in ((None, "dim"), (0.05, "dim"), (0.05, "cell")):
        a, b = K.objective(*ts, lens, "valid", fb, over), K.objective(*clean, lens, "valid", fb, over)
        for key in ("value", "raw", "dims", "steps", "s_c", "gate_full"):
            assert torch.equal(a[key], b[key]), (fb, over, key)
        for x, y in zip(K.gradients(*ts, a), K.gradients(*clean, b)):
            assert torch.equal(x, y)
        bad = [t.clone() for t in ts]
        bad[0][0, 1, 0] = float("nan")      # a cell of S
        assert math.isnan(float(K.objective(*bad, lens, "valid", fb, over)["value"]))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture
def no_library(monkeypatch):
    from acvae_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched before the refusal")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "h2d", touched)


def test_refusals_come_before_any_library_call(no_library):
    from acvae_amd.train_util import KLObjective
    for kw in (dict(reduction="mean"), dict(reduction=None), dict(free_bits_over="row"), dict(free_bits=-0.1),
               dict(free_bits=float("nan")), dict(free_bits=float("inf")), dict(free_bits=True), dict(free_bits=False),
               dict(free_bits="0.1"), dict(free_bits=np.bool_(True))):
        with pytest.raises(ValueError):
            KLObjective(**kw)
    KLObjective(free_bits=0.0), KLObjective(free_bits=0), KLObjective(free_bits=np.float32(.5))       # legal
    g = [torch.zeros(2, 3, 4) for _ in range(4)]
    valid = KLObjective("valid")
    with pytest.raises(ValueError):
        KLObjective()(g[0], g[1], g[2], torch.zeros(2, 3, 5))          # shapes differ
    with pytest.raises(ValueError):
        KLObjective()(g[0][0], g[1][0], g[2][0], g[3][0])              # not [R, T, E]
    with pytest.raises(ValueError):
        valid(*g)                                                      # lens1 missing
    for lens in ([3, 3, 3], [3], [4, 1], [-1, 2], [[3, 2]], [1.5, 2.0]):
        with pytest.raises(ValueError):
            valid(*g, lens1=np.array(lens))
    with pytest.raises(ValueError):
        valid(*g, lens1=torch.tensor([3, 4]))                          # a host tensor is a host array
    with pytest.raises(ValueError):
        valid(*g, lens1=[0, 0])                                        # D == 0
    with pytest.raises(ValueError):
        valid(*g, lens1=[3, 1], divisor=5)                             # a divisor that is not the sum


def test_trainstep_refuses_bad_keywords_before_it_builds_anything(no_library):
    from acvae_amd.trainer import TrainStep
    for kw in (dict(kl_reduction="token"), dict(free_bits=-1.0), dict(free_bits=True), dict(free_bits_over="batch")):
        with pytest.raises(ValueError):
            TrainStep(None, 10, **kw)


# ------------------------------------------------------------------------------------------------ the schedule
def test_kl_weight_cyclical_at_hand_computed_points():
    from acvae_amd.trainer import kl_weight_cyclical as w
    assert w(0, 100) == 0.0                                 # cycle start
    assert w(25, 100) == 0.5                                # half way up the ramp of 50 steps
    assert w(50, 100) == 1.0                                # end of the ramp
    assert w(75, 100) == 1.0 and w(99, 100) == 1.0          # plateau
    assert w(100, 100) == 0.0 and w(125, 100) == 0.5 and w(260, 100) == 1.0      # second and third cycle
    assert w(10, 40, ratio=0.25, beta=2.0) == 2.0 and w(5, 40, ratio=0.25, beta=2.0) == 1.0
    assert w(50, 100, ratio=1) == 0.5 and w(99, 100, ratio=1) == pytest.approx(0.99) and w(100, 100, ratio=1) == 0.0
    assert w(0, 100, floor=0.2) == 0.2 and w(25, 100, floor=0.2) == pytest.approx(0.6) and w(50, 100, floor=0.2) == 1.0
    assert w(25, 100, beta=0.5, floor=0.1) == pytest.approx(0.3)
    assert all(isinstance(w(s, 7), float) for s in range(15))
    for bad in (dict(step=-1, cycle_steps=10), dict(step=0, cycle_steps=0), dict(step=0, cycle_steps=10, ratio=0.0),
                dict(step=0, cycle_steps=10, ratio=1.5)):
        with pytest.raises(ValueError):
            w(**bad)
