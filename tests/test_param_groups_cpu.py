"""No GPU: the chunk table of the grouped optimiser launches against a brute-force per-element map, what
TrainStep(param_groups=) refuses before anything is built and before any library call, split_params on a small module, and
the new entry points in the header and in the built library."""
import ctypes
import itertools
import re

import numpy as np
import pytest
import torch

from acvae_amd import _lib, optim, trainer

CHUNK = 64                                       # a small chunk keeps the brute-force maps tiny; the rule has no other constant
SIZES = [4, CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 8]


def element_map(sizes, group_of, skipped, first):
    """Per element: the group (or -1 where nothing may touch it), the `first` flag, and the index of its parameter."""
    g = np.concatenate([np.full(s, -1 if i in skipped else k) for i, (s, k) in enumerate(zip(sizes, group_of))])
    f = np.concatenate([np.full(s, i in first and i not in skipped) for i, s in enumerate(sizes)])
    return g, f


def check_table(sizes, group_of, skipped=(), first=(), chunk=CHUNK):
    skipped, first = set(skipped), set(first)
    t = optim.chunk_table(sizes, group_of, skipped, first, chunk)
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 3 and t.flags["C_CONTIGUOUS"]
    want_g, want_f = element_map(sizes, group_of, skipped, first)
    cover = np.zeros(sum(sizes), dtype=np.int64)
    got_g = np.full(sum(sizes), -1)
    got_f = np.zeros(sum(sizes), dtype=bool)
    last_end = 0
    for start4, len4, tag in t:
        a, n = 4 * int(start4), 4 * int(len4)
        assert 0 < n <= chunk and a >= last_end and a + n <= sum(sizes), (a, n)
        last_end = a + n
        assert tag & ~(optim.CHUNK_FIRST | (optim.MAX_GROUPS - 1)) == 0, tag
        cover[a:a + n] += 1
        got_g[a:a + n] = tag & (optim.CHUNK_FIRST - 1)
        got_f[a:a + n] = bool(tag & optim.CHUNK_FIRST)
    assert np.array_equal(cover, (want_g >= 0).astype(np.int64)), "every element of every segment exactly once, no other"
    assert np.array_equal(got_g, want_g), "a chunk crosses into a parameter of another group"
    assert np.array_equal(got_f[want_g >= 0], want_f[want_g >= 0]), "first bits do not follow the started set"
    # as few chunks as the rule allows: every segment costs ceil(len / chunk)
    segs = optim.group_segments(sizes, group_of, skipped, first)
    assert len(t) == sum(-(-(b - a) // chunk) for a, b, _, _ in segs)
    return t, segs


PATTERNS = {
    "alternating": lambda n: [i % 2 for i in range(n)],
    "one-group": lambda n: [0] * n,
    "eight-groups": lambda n: [i % 8 for i in range(n)],
    "pairs": lambda n: [(i // 2) % 3 for i in range(n)],
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_chunk_table_covers_every_segment_once(pattern):
    for sizes in list(itertools.permutations(SIZES, 5))[::7] + [SIZES * 2, [4] * 20]:
        sizes = list(sizes)
        check_table(sizes, PATTERNS[pattern](len(sizes)))


def test_chunk_table_one_group_is_one_segment_and_adjacent_parameters_merge():
    t, segs = check_table(SIZES, [0] * 5)
    assert segs == [(0, sum(SIZES), 0, False)]
    assert len(t) == -(-sum(SIZES) // CHUNK)
    _, segs = check_table(SIZES, [0, 0, 1, 1, 0])
    assert [s[2] for s in segs] == [0, 1, 0]


@pytest.mark.parametrize("skipped", [{0}, {2}, {4}, {0, 2, 4}, {1, 2}, {0, 1, 2, 3}], ids=str)
def test_skipped_parameters_are_uncovered(skipped):
    """At the start, between two parameters of the same group (which then form two segments), and at the end."""
    for groups in ([0] * 5, [0, 1, 0, 1, 0], [1, 1, 1, 0, 0]):
        _, segs = check_table(SIZES, groups, skipped)
    _, segs = check_table(SIZES, [0] * 5, {2})
    assert len(segs) == 2 and segs[0][1] == 4 + CHUNK - 4 and segs[1][0] == segs[0][1] + CHUNK


def test_first_bits_follow_the_started_set():
    for first in ({0}, {1, 2}, {0, 1, 2, 3, 4}, {4}, set()):
        t, segs = check_table(SIZES, [0, 0, 1, 1, 1], first=first)
        check_table(SIZES, [0] * 5, skipped={1}, first=first)
    _, segs = check_table(SIZES, [0] * 5, first={1, 2})
    assert [(s[3]) for s in segs] == [False, True, False]            # one group, three segments: `first` splits a run


def test_all_skipped_is_an_empty_table():
    t = optim.chunk_table(SIZES, [0] * 5, set(range(5)), (), CHUNK)
    assert t.shape == (0, 3) and t.dtype == np.int32


@pytest.mark.parametrize("kw, match", [
    (dict(sizes=[4, 6]), "multiple of 4"),
    (dict(sizes=[4, 0]), "multiple of 4"),
    (dict(sizes=[4, -4]), "multiple of 4"),
    (dict(group_of=[0, 8]), "group 8"),
    (dict(group_of=[0, -1]), "group -1"),
    (dict(group_of=[0]), "sizes"),
    (dict(chunk=6), "chunk"),
    (dict(chunk=0), "chunk"),
    (dict(chunk=-8), "chunk"),
    (dict(skipped=[2]), "skipped"),
    (dict(first=[-1]), "first"),
    (dict(sizes=[1 << 32, 1 << 32]), "int32"),
])
def test_chunk_table_refuses_what_the_kernel_would_clamp(kw, match):
    args = dict(sizes=[4, 8], group_of=[0, 1], skipped=(), first=(), chunk=8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        optim.chunk_table(**args)


# ---------------------------------------------------------------------------------------------------- refusals
class _Enc(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 2, 3)
        self.bn = torch.nn.BatchNorm2d(2)
        self.fc1 = torch.nn.Linear(2, 3)

    def _head(self):
        return self.fc1


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = _Enc()
        self.emb = torch.nn.Embedding(5, 4)
        self.out = torch.nn.Linear(4, 5)
        self.ln = torch.nn.LayerNorm(4)
        self.frozen = torch.nn.Parameter(torch.zeros(3), requires_grad=False)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure of the test, not a ValueError."""
    def used(*a, **k):
        raise AssertionError("the library was reached before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", used)
    monkeypatch.setattr(_lib, "call", used)
    monkeypatch.setattr(_lib, "require_cuda", used)


def _halves(m):
    enc = list(m.encoder.parameters())
    ids = {id(p) for p in enc}
    return enc, [p for p in m.parameters() if id(p) not in ids]


def _refusals():
    m = _Model()
    enc, rest = _halves(m)
    two = lambda a=None, b=None: [{"params": enc, **(a or {})}, {"params": rest, **(b or {})}]
    return m, [
        ("Adam", {}, [], "1..8 groups"),
        ("Adam", {}, [{"params": [p]} for p in list(m.parameters())[:9]], "1..8 groups"),
        ("Adam", {}, {"params": enc}, "list of dicts"),
        ("Adam", {}, [{"lr": 1e-3}], "group 0.*params"),
        ("Adam", {}, [{"params": enc}, {"params": rest[:-1]}], "in no group"),
        ("Adam", {}, [{"params": enc}, {"params": rest + enc[:1]}], "group 1.*already in group 0"),
        ("Adam", {}, [{"params": enc + enc[:1]}, {"params": rest}], "group 0.*already in group 0"),
        ("Adam", {}, [{"params": [torch.zeros(2)]}], "group 0.*Parameter"),
        ("Adam", {}, two(b={"amsgrad": True}), "group 1.*amsgrad"),
        ("AdamW", {"amsgrad": True}, two(a={"amsgrad": False}), "group 0.*amsgrad"),
        ("Adam", {}, two(b={"decoupled_weight_decay": True}), "group 1.*decoupled_weight_decay"),
        ("Adam", {}, two(a={"maximize": True}), "group 0.*maximize"),
        ("Adam", {}, two(a={"foreach": True}), "group 0.*foreach"),
        ("SGD", {"momentum": 0.9}, two(b={"nesterov": True}), "group 1.*nesterov"),
        ("SGD", {"momentum": 0.9}, two(b={"dampening": 0.1}), "group 1.*dampening"),
        ("SGD", {"momentum": 0.9}, two(b={"momentum": 0.0}), "momentum is zero in some"),
        ("SGD", {}, two(a={"momentum": 0.5}), "momentum is zero in some"),
        ("SGD", {"momentum": 0.9, "nesterov": True}, two(a={"momentum": 0.0}), "group 0"),
        ("Adam", {}, two(a={"momentum": 0.9}), "group 0.*'momentum' is not an option"),
        ("SGD", {}, two(b={"betas": (0.9, 0.99)}), "group 1.*'betas' is not an option"),
        ("Adam", {}, two(b={"learning_rate": 1.0}), "group 1.*'learning_rate'"),
        ("Adam", {}, two(a={"lr": -1.0}), "group 0.*learning rate"),
        ("Adam", {}, two(b={"betas": (0.9, 1.5)}), "group 1.*beta"),
        ("AdamW", {}, two(b={"eps": -1e-8}), "group 1.*epsilon"),
        ("SGD", {}, two(a={"weight_decay": -0.1}), "group 0.*weight_decay"),
    ]


_M, _CASES = _refusals()


@pytest.mark.parametrize("name, args, groups, match", _CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(_CASES)])
def test_constructor_refuses_before_anything_is_built(no_library, name, args, groups, match):
    with pytest.raises(ValueError, match=match):
        trainer.TrainStep(_M, 5, optimizer=name, optimizer_args=args, param_groups=groups)


def test_refusals_need_no_model(no_library):
    """What does not depend on the model's parameters is refused for TrainStep(None, ...) as well."""
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    for groups, match in (([], "1..8"), ([{"params": [p]}, {"params": [p]}], "already in group 0"),
                          ([{"params": [p]}, {"params": [q], "amsgrad": True}], "amsgrad"),
                          ([{"params": [p], "nope": 1}], "'nope'")):
        with pytest.raises(ValueError, match=match):
            trainer.TrainStep(None, 40, param_groups=groups)
    with pytest.raises(ValueError, match="param group"):            # the one-group refusal of optimizer_args stands
        trainer.TrainStep(None, 40, optimizer_args={"params": [p]})


def test_accepted_groups_resolve_to_full_dicts():
    m = _Model()
    enc, rest = _halves(m)
    base = optim.resolve("AdamW", {"weight_decay": 0.05}, lr=1e-3)
    # frozen parameters may be listed, the pooled head may be listed or left out, equal structural values may be named
    groups = optim.resolve_groups("AdamW", base, [{"params": enc, "lr": 1e-4, "amsgrad": False},
                                                  {"params": iter(rest), "betas": [0.8, 0.9], "weight_decay": 0.0}])
    assert [g["lr"] for g in groups] == [1e-4, 1e-3] and [g["weight_decay"] for g in groups] == [0.05, 0.0]
    assert groups[1]["betas"] == (0.8, 0.9) and groups[0]["betas"] == (0.9, 0.999)
    assert set(groups[0]) == set(base) | {"params"}
    trainable = [p for p in m.parameters() if p.requires_grad]
    optim.check_coverage(groups, trainable)
    head = m.encoder._head()
    no_head = [{"params": [p for p in enc if p is not head.weight and p is not head.bias]}, {"params": rest}]
    optim.check_coverage(optim.resolve_groups("AdamW", base, no_head), trainable, (head.weight, head.bias))
    with pytest.raises(ValueError, match="in no group"):
        optim.check_coverage(optim.resolve_groups("AdamW", base, no_head), trainable)
    opt = optim.FlatOptimizer(None, groups, "AdamW", base)
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["lr"] == 1e-4
    with pytest.raises(ValueError, match="after construction"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))]})
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5, lambda e: 2.0])
    assert [g["lr"] for g in opt.param_groups] == [0.5e-4, 2e-3] and sched.base_lrs == [1e-4, 1e-3]
    opt.param_groups[1]["amsgrad"] = True                           # a structural option changed in one group: every step checks
    with pytest.raises(ValueError, match="group 1.*amsgrad"):
        optim.check_groups("AdamW", opt.param_groups)


def test_split_params():
    m = _Model()
    groups = optim.split_params(m, encoder_lr=5e-5)
    enc_ids = {id(p) for p in m.encoder.parameters()}
    assert len(groups) == 4
    want = [(True, False), (True, True), (False, False), (False, True)]
    for g, (in_enc, small) in zip(groups, want):
        assert g["params"] and all((id(p) in enc_ids) == in_enc and (p.ndim <= 1) == small for p in g["params"])
        assert ("lr" in g) == in_enc and (g.get("lr") == 5e-5 or not in_enc)
        assert ("weight_decay" in g) == small and (g.get("weight_decay") == 0.0 or not small)
        assert set(g) <= {"params", "lr", "weight_decay"}
    listed = [id(p) for g in groups for p in g["params"]]
    assert len(listed) == len(set(listed)) and set(listed) == {id(p) for p in m.parameters() if p.requires_grad}
    assert id(m.encoder.bn.weight) in {id(p) for p in groups[1]["params"]}       # a BatchNorm scale: no decay
    assert id(m.ln.weight) in {id(p) for p in groups[3]["params"]}               # a LayerNorm scale: no decay
    plain = optim.split_params(m, no_decay=False)
    assert all(set(g) == {"params"} for g in plain) and len(plain) == 4
    for p in m.encoder.parameters():
        if p.ndim <= 1:
            p.requires_grad_(False)
    assert len(optim.split_params(m)) == 3                                       # an empty group is dropped
    full = optim.resolve_groups("AdamW", optim.resolve("AdamW", None, lr=5e-4), optim.split_params(m, encoder_lr=5e-5))
    assert [g["lr"] for g in full] == [5e-5, 5e-4, 5e-4] and [g["weight_decay"] for g in full] == [1e-2, 1e-2, 0.0]


def test_header_declares_and_library_exports_the_grouped_entries():
    P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    want = {
        "acvae_opt_chunk_elems": (L, []),
        "acvae_grad_norm_groups": (I, [("grads", P), ("chunks", P), ("n_chunks", I), ("n_groups", I), ("grad_scale", F),
                                       ("partials", P), ("group_norms", P), ("total_norm", P), ("stream", P)]),
        "acvae_adamw_groups_step": (I, [("params", P), ("grads", P), ("exp_avg", P), ("exp_avg_sq", P), ("max_exp_avg_sq", P),
                                        ("n", L), ("chunks", P), ("n_chunks", I), ("n_groups", I), ("lr", P), ("beta1", P),
                                        ("beta2", P), ("eps", P), ("weight_decay", P), ("decoupled", I), ("amsgrad", I),
                                        ("step", L), ("grad_scale", F), ("max_grad_norm", F), ("total_norm", P), ("stream", P)]),
        "acvae_sgd_groups_step": (I, [("params", P), ("grads", P), ("momentum_buffer", P), ("n", L), ("chunks", P),
                                      ("n_chunks", I), ("n_groups", I), ("lr", P), ("momentum", P), ("weight_decay", P),
                                      ("dampening", D), ("nesterov", I), ("grad_scale", F), ("max_grad_norm", F),
                                      ("total_norm", P), ("stream", P)]),
    }
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in want.items():
        assert name in _lib.PROTOS, name
        got_ret, got = _lib.PROTOS[name]
        assert got_ret is ret and got == args, (name, got)
        assert hasattr(so, name), f"{name} is declared but not exported"
    src = open(_lib.HEADER).read()
    assert int(re.search(r"#define\s+ACVAE_ABI_VERSION\s+(\d+)", src).group(1)) == 3
    assert int(re.search(r"#define\s+ACVAE_OPT_MAX_GROUPS\s+(\d+)", src).group(1)) == optim.MAX_GROUPS == 8
    assert int(re.search(r"#define\s+ACVAE_OPT_CHUNK_FIRST\s+(\d+)", src).group(1)) == optim.CHUNK_FIRST
    so.acvae_opt_chunk_elems.restype = ctypes.c_int64
    chunk = so.acvae_opt_chunk_elems()                               # a host constant: no device is touched
    assert chunk > 0 and chunk % 4 == 0
