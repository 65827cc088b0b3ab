"""GPU: TrainStep(param_groups=) on the golden-size model: against the default TrainStep where the arithmetic is the same,
against a torch optimiser over the same groups, under a per-group scheduler, across checkpoints, and together with
accumulation and the weight EMA."""
import io

import numpy as np
import pytest
import torch

import param_groups_util as U
from acvae_amd import _lib, optim
from test_optim_gpu import V, compare_params, fresh, one, sync_params, twin_step

pytestmark = pytest.mark.gpu


def halves(m):
    enc = list(m.encoder.parameters())
    ids = {id(p) for p in enc}
    return enc, [p for p in m.parameters() if id(p) not in ids]


def two_groups(m, a=None, b=None):
    enc, rest = halves(m)
    return [{"params": enc, **(a or {})}, {"params": rest, **(b or {})}]


def assert_same_params(m_a, m_b):
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m_a.named_parameters(), m_b.named_parameters()):
        assert U.same_bits(a, b), k


def test_two_groups_construct():
    """TrainStep has no param_groups keyword without this feature (TypeError)."""
    m, ts = fresh(optimizer="AdamW", param_groups=None)
    assert len(ts.optimizer.param_groups) == 1
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import _state, build_model, E
    m = build_model(V, E, _state()).train()
    ts = TrainStep(m, V, param_groups=two_groups(m, {"lr": 1e-4}))
    assert [g["lr"] for g in ts.optimizer.param_groups] == [1e-4, 5e-4]
    assert ts.group_norms.shape == (2,)
    with pytest.raises(ValueError, match="after construction"):
        ts.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, device="cuda"))]})


def fresh_groups(make, **kw):
    """fresh() with param_groups built from the model by `make`."""
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import _state, build_model, E
    m = build_model(V, E, _state()).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V, param_groups=make(m), **kw)


@pytest.mark.parametrize("name, args", [("AdamW", {}), ("AdamW", {"amsgrad": True, "weight_decay": 0.05}),
                                        ("SGD", {"momentum": 0.9, "lr": 1e-2})], ids=["AdamW", "AdamW-amsgrad", "SGD-momentum"])
def test_identical_groups_equal_the_default_bit_for_bit(name, args):
    """Two groups with the same hyperparameters, no clipping, against TrainStep without param_groups: loss and every
    parameter over two steps.  The optimisers are those whose one-group update runs the element arithmetic the grouped
    kernel shares (opt_elem); plain Adam's one-group path is the older acvae_adam_step, whose operation order differs, and
    is held to the torch bound below instead."""
    m_a, t_a = fresh_groups(two_groups, optimizer=name, optimizer_args=args, max_grad_norm=None)
    m_b, t_b = fresh(optimizer=name, optimizer_args=args, max_grad_norm=None)
    for k in range(2):
        pa, pb = one(t_a, seed=3 + k), one(t_b, seed=3 + k)
        assert U.same_bits(pa["loss"], pb["loss"])
        assert "grad_norm_groups" not in pa
    assert_same_params(m_a, m_b)
    for a, b in zip(t_a._state_buffers().values(), t_b._state_buffers().values()):
        assert U.same_bits(a, b)


def test_identical_groups_under_plain_adam_agree_with_the_default():
    """The default optimiser (Adam through acvae_adam_step) against two identical groups (opt_elem): the same update in
    another operation order, held to the bound the one-group update is held to against torch (compare_params)."""
    m_a, t_a = fresh_groups(two_groups, max_grad_norm=None)
    m_b, t_b = fresh(max_grad_norm=None)
    for k in range(2):
        if k:
            sync_params(m_a, m_b)
        pa, pb = one(t_a, seed=3 + k), one(t_b, seed=3 + k)
        assert U.same_bits(pa["loss"], pb["loss"])
        compare_params(m_a, m_b, f"plain Adam step {k + 1}")


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD"])
def test_one_explicit_group_takes_the_old_launches(name):
    """One group over everything, with clipping: the one-group entries, hence bit-equal to the default, plain Adam included."""
    args = {"momentum": 0.9, "lr": 1e-2} if name == "SGD" else {}
    m_a, t_a = fresh_groups(lambda m: [{"params": list(m.parameters())}], optimizer=name, optimizer_args=args)
    m_b, t_b = fresh(optimizer=name, optimizer_args=args)
    assert t_a.group_norms is None and t_a.lr == t_b.lr
    for k in range(2):
        pa, pb = one(t_a, seed=3 + k), one(t_b, seed=3 + k)
        assert U.same_bits(pa["loss"], pb["loss"]) and U.same_bits(pa["grad_norm"], pb["grad_norm"])
        assert "grad_norm_groups" not in pa
    assert_same_params(m_a, m_b)


def torch_groups(groups_of_ts, m1, m3):
    """The groups of a TrainStep over m1 rebuilt over the twin m3 (same parameter positions, same overrides)."""
    pos = {id(p): i for i, p in enumerate(m1.parameters())}
    p3 = list(m3.parameters())
    return [{**{k: v for k, v in g.items() if k != "params"}, "params": [p3[pos[id(p)]] for p in g["params"]]}
            for g in groups_of_ts]


TWIN_CASES = {
    "AdamW-split_params": ("AdamW", {}, lambda m: optim.split_params(m, encoder_lr=5e-5)),
    "Adam-betas-eps": ("Adam", {}, lambda m: two_groups(m, {"betas": (0.8, 0.99), "eps": 1e-6}, {"betas": (0.95, 0.999)})),
    "SGD-nesterov": ("SGD", {"momentum": 0.9, "nesterov": True, "lr": 1e-2, "weight_decay": 1e-3},
                     lambda m: two_groups(m, {"momentum": 0.9}, {"momentum": 0.8})),
}


@pytest.mark.parametrize("case", list(TWIN_CASES))
def test_groups_match_a_torch_optimizer_over_the_same_groups(case):
    name, args, make = TWIN_CASES[case]
    m1, t1 = fresh_groups(make, optimizer=name, optimizer_args=args)
    m3, t3 = fresh()
    given = make(m1)
    opt = getattr(torch.optim, name)(torch_groups(given, m1, m3), **{"lr": 5e-4, **args})
    assert len(t1.optimizer.param_groups) == len(opt.param_groups) >= 2
    for g1, g3 in zip(t1.optimizer.param_groups, opt.param_groups):
        for k in optim.PER_GROUP[name]:
            assert g1[k] == g3[k], k
    for k in range(2):
        if k:
            sync_params(m1, m3)
        before = [p.detach().clone() for p in m1.parameters()]
        one(t1, seed=3 + k)
        twin_step(t3, m3, opt, seed=3 + k)
        compare_params(m1, m3, f"{case} step {k + 1}")
        assert any(not torch.equal(a, b) for a, b in zip(before, m1.parameters()))


def test_a_group_with_lr_zero_keeps_its_bits_while_its_moments_move():
    m, ts = fresh_groups(lambda m: two_groups(m, {"lr": 0.0, "weight_decay": 0.0}))
    enc, rest = halves(m)
    before = {id(p): p.detach().clone() for p in m.parameters()}
    one(ts)
    torch.cuda.synchronize()
    offs = ts._offsets()
    head = m.encoder._head()
    moved_avg = 0
    for p in enc:
        assert U.same_bits(p, before[id(p)]), "a parameter of the lr = 0 group moved"
        if p is not head.weight and p is not head.bias:
            moved_avg += int(ts.exp_avg[offs[p]:offs[p] + p.numel()].ne(0).any())
    assert moved_avg > 10, "exp_avg of the lr = 0 group did not move"
    assert sum(int(not torch.equal(p, before[id(p)])) for p in rest) > 10


def test_grad_norm_groups():
    m, ts = fresh_groups(lambda m: optim.split_params(m, encoder_lr=5e-5), optimizer="AdamW")
    parts = one(ts)
    torch.cuda.synchronize()
    gn, total = parts["grad_norm_groups"].cpu().double(), float(parts["grad_norm"])
    G = len(ts.optimizer.param_groups)
    assert gn.shape == (G,) and G == 4
    chunk = int(_lib.call("acvae_opt_chunk_elems"))
    bound = (chunk / 256 + 16) * 2.0 ** -24 + 2 * 2.0 ** -23          # on the sum of squares; + the output's fp32 rounding
    for k, g in enumerate(ts.optimizer.param_groups):
        want = sum(float(ts.views[p].double().pow(2).sum()) for p in g["params"] if p in ts.views and p not in ts.never)
        assert want > 0
        assert abs(float(gn[k]) ** 2 - want) <= bound * want, (k, float(gn[k]) ** 2, want)
    root = np.float32(np.sqrt(float((gn ** 2).sum())))
    assert abs(float(root) - total) <= 2 * float(np.spacing(np.float32(total))), (float(root), total)


def test_lambda_lr_per_group_equals_setting_the_lrs_by_hand():
    from torch.optim.lr_scheduler import LambdaLR
    make = lambda m: two_groups(m, {"lr": 1e-4})
    m_a, t_a = fresh_groups(make, optimizer="AdamW")
    m_b, t_b = fresh_groups(make, optimizer="AdamW")
    f0, f1 = (lambda e: 1.0 / (1 + e)), (lambda e: 0.5 ** e)
    sched = LambdaLR(t_a.optimizer, [f0, f1])
    seen = []
    for k in range(3):
        seen.append([g["lr"] for g in t_a.optimizer.param_groups])
        one(t_a, seed=3 + k)
        sched.step()
    assert seen[0] == [1e-4, 5e-4] and seen[2][0] < seen[1][0] < seen[0][0] and seen[2][1] < seen[1][1] < seen[0][1]
    assert seen[2][0] / seen[0][0] != seen[2][1] / seen[0][1]
    for k, lrs in enumerate(seen):
        for g, lr in zip(t_b.optimizer.param_groups, lrs):
            g["lr"] = lr
        one(t_b, seed=3 + k)
    assert_same_params(m_a, m_b)


def test_checkpoint_round_trip_torch_compat_and_refusal():
    make = lambda m: optim.split_params(m, encoder_lr=5e-5)
    args = {"weight_decay": 0.05}
    m1, t1 = fresh_groups(make, optimizer="AdamW", optimizer_args=args)
    one(t1)
    buf = io.BytesIO()
    torch.save({"model": m1.state_dict(), "optimizer": t1.optimizer.state_dict()}, buf)
    one(t1, seed=4)
    ck = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    groups = ck["optimizer"]["param_groups"]
    assert len(groups) == 4 and [g["lr"] for g in groups] == [5e-5, 5e-5, 5e-4, 5e-4]
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0, 0.05, 0.0]
    ids = [i for g in groups for i in g["params"]]
    assert ids == list(range(len(ids))) and [len(g["params"]) for g in groups] == [len(g["params"]) for g in make(m1)]
    # resume into a fresh TrainStep: the same next step, bit for bit
    m2, t2 = fresh_groups(make, optimizer="AdamW", optimizer_args=args)
    m2.load_state_dict(ck["model"])
    t2.optimizer.load_state_dict(ck["optimizer"])
    one(t2, seed=4)
    assert_same_params(m1, m2)
    # torch.optim.AdamW over the same groups loads it and takes the same next step
    m3, t3 = fresh()
    m3.load_state_dict(ck["model"])
    opt = torch.optim.AdamW(torch_groups(make(m3), m3, m3), lr=1.0)
    opt.load_state_dict(ck["optimizer"])
    assert [g["lr"] for g in opt.param_groups] == [5e-5, 5e-5, 5e-4, 5e-4]
    twin_step(t3, m3, opt, seed=4)
    compare_params(m1, m3, "torch AdamW over the same groups vs fused")
    # another number of groups, or other sizes, is refused
    m4, t4 = fresh_groups(two_groups, optimizer="AdamW", optimizer_args=args)
    with pytest.raises(ValueError, match="4 param group"):
        t4.optimizer.load_state_dict(ck["optimizer"])
    m5, t5 = fresh(optimizer="AdamW", optimizer_args=args)
    with pytest.raises(ValueError, match="param group"):
        t5.optimizer.load_state_dict(ck["optimizer"])
    bad = {"state": ck["optimizer"]["state"], "param_groups": [dict(g) for g in groups]}
    bad["param_groups"][0]["params"] = bad["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="group 0"):
        t2.optimizer.load_state_dict(bad)


def test_accumulation_of_the_same_batch_twice_equals_one_grouped_step():
    """g + g over two micro-steps, scaled by 1/2, is g exactly: the grouped norm and update read flat_acc."""
    make = lambda m: optim.split_params(m, encoder_lr=5e-5)
    m_a, t_a = fresh_groups(make, optimizer="AdamW", accum_steps=2)
    m_b, t_b = fresh_groups(make, optimizer="AdamW")
    p1 = one(t_a)
    assert p1["applied"] is False and "grad_norm_groups" not in p1
    # BatchNorm running statistics moved in the first micro-step; the batch statistics, hence the gradients, do not depend on them
    p2 = one(t_a)
    pb = one(t_b)
    assert p2["applied"] is True
    torch.cuda.synchronize()
    assert U.same_bits(p2["grad_norm"], pb["grad_norm"]) and U.same_bits(p2["grad_norm_groups"], pb["grad_norm_groups"])
    assert_same_params(m_a, m_b)
    one(t_a, seed=4)
    out = t_a.flush()
    assert out["applied"] and out["grad_norm_groups"].shape == (4,)


def test_ema_follows_its_recurrence_on_the_grouped_parameters():
    m, ts = fresh_groups(lambda m: two_groups(m, {"lr": 1e-4}), optimizer="AdamW", ema_decay=0.9)
    ema = ts.flat_p.detach().cpu().double()
    bound = torch.zeros_like(ema)
    w = float(np.float32(1.0 - 0.9))                    # the kernel's weight: 1 - decay formed in double, rounded once
    for k in range(3):
        prev = ts.flat_ema.detach().cpu().double()
        one(ts, seed=3 + k)
        torch.cuda.synchronize()
        p = ts.flat_p.detach().cpu().double()
        # this step's fp32 roundings (the bound tests/test_accumulate_train_gpu.py holds the one-group EMA to); a lerp
        # passes earlier error on at most once
        bound += 4 * 2.0 ** -24 * (prev.abs() + p.abs())
        ema = ema + w * (p - ema)
        err = (ts.flat_ema.cpu().double() - ema).abs()
        assert bool((err <= bound).all()), f"update {k + 1}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.2f}"
    assert float((ts.flat_ema - ts.flat_p).abs().max()) > 0 and ts.ema_updates == 3


def test_single_group_views_raise_with_two_groups():
    m, ts = fresh_groups(two_groups)
    for key in ("lr", "betas", "eps", "weight_decay"):
        with pytest.raises(ValueError, match="optimizer.param_groups"):
            getattr(ts, key)
        with pytest.raises(ValueError, match="optimizer.param_groups"):
            setattr(ts, key, 1e-3)
