"""GPU, through the C ABI: the non-finite guard's entries.  The witness's flag for NaN / inf at every position class, the
decision's record against the numpy twin (tests/guard_util.py) with the fp32 scalars EQUAL to the host-formed ones, the guarded
grouped update bit for bit against the unguarded one (applied) and against the untouched buffers (skipped), the guarded EMA and
the restore in both decisions, and every refusal."""
import numpy as np
import pytest
import torch

import guard_util as GU
import param_groups_util as U
from acvae_amd import _lib

pytestmark = pytest.mark.gpu
PAD, GUARD = U.PAD, U.GUARD
GSCALE = 0.5
EINVAL, EALIGN = -1, -2
FMAX = float(np.finfo(np.float32).max)


def chunk():
    return int(_lib.call("acvae_opt_chunk_elems"))


def stream():
    return _lib.current_stream()


def new_record(applied=0, skipped=0, streak=0, ema_updates=0, ok=0, window_bad=0):
    rec = torch.zeros(GU.RECORD_WORDS, dtype=torch.int32)
    rec[:8].view(torch.int64).copy_(torch.tensor([applied, skipped, streak, ema_updates]))
    rec[8], rec[9] = ok, window_bad
    return rec.cuda()


def scalar(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def decide(rec, norm, kind=GU.SGD, lr=(0.1,), b1=None, b2=None, ema=-1.0, warmup=False):
    """norm: a float or a device scalar."""
    tn = norm if torch.is_tensor(norm) else scalar(norm)
    _lib.call("acvae_guard_decide", rec, tn, kind, len(lr), U.doubles(lr), None if b1 is None else U.doubles(b1),
              None if b2 is None else U.doubles(b2), float(ema), int(warmup), stream())


# ---------------------------------------------------------------------------------------------------- witness
WITNESS_SIZES = [1, 3, 4, 5, 255, 256, 257, 3841]
BAD_VALUES = [float("nan"), float("inf"), float("-inf")]


def witness_flag(loss, buf, n, rec=None):
    """One call on a fresh (or the given) record; -> the record read back.  Everything but window_bad must be as it was."""
    rec = new_record(applied=3, skipped=2, streak=1, ema_updates=5, ok=1) if rec is None else rec
    before = GU.read_record(rec)
    _lib.call("acvae_guard_witness", loss, buf, n, rec, stream())
    after = GU.read_record(rec)
    for k, v in before.items():
        if k != "window_bad":
            assert np.array_equal(v, after[k]), f"the witness moved {k}"
    return after["window_bad"]


@pytest.mark.parametrize("n", WITNESS_SIZES)
def test_witness_flag_is_exact(n):
    gen = torch.Generator().manual_seed(n)
    clean = torch.randn(n, generator=gen)
    good_loss = scalar(1.5)
    # finite extremes set nothing: +-0, denormals, +-FLT_MAX
    edge = clean.clone()
    for i, v in enumerate([0.0, -0.0, 1e-45, -1e-45, 1e-39, FMAX, -FMAX][:n]):
        edge[i] = v
    buf = U.padded(edge, n)
    buf[n:] = float("nan")                                # behind the n_buf elements: not the witness's business
    assert witness_flag(good_loss, buf, n) == 0
    assert witness_flag(None, buf, n) == 0               # no loss to look at
    positions = sorted({0, n - 1, min(n - 1, (n // 2) | 1)})
    for pos in positions:
        for bad in BAD_VALUES:
            x = clean.clone()
            x[pos] = bad
            b = U.padded(x, n)
            assert witness_flag(good_loss, b, n) == 1, (n, pos, bad)
            assert bool((b[n:] == GUARD).all())
    # the element just behind n_buf is not read as part of the buffer
    x = U.padded(clean, n)
    x[n] = float("inf")
    assert witness_flag(good_loss, x, n) == 0


def test_witness_loss_alone_and_the_or():
    buf = U.padded(torch.ones(37), 37)
    for bad in BAD_VALUES:
        assert witness_flag(scalar(bad), buf, 37) == 1
        assert witness_flag(scalar(bad), None, 0) == 1   # no buffers at all (a model without BatchNorm)
    for fine in (0.0, -0.0, 1e-45, FMAX, -FMAX):
        assert witness_flag(scalar(fine), None, 0) == 0
    assert witness_flag(None, None, 0) == 0
    # an OR: once set, a clean call leaves it set; the decision clears it
    rec = new_record()
    assert witness_flag(scalar(1.0), buf, 37, rec) == 0
    assert witness_flag(scalar(float("nan")), buf, 37, rec) == 1
    assert witness_flag(scalar(1.0), buf, 37, rec) == 1
    decide(rec, 1.0)
    r = GU.read_record(rec)
    assert (r["ok"], r["window_bad"], r["skipped"], r["streak"], r["applied"]) == (0, 0, 1, 1, 0)
    assert witness_flag(scalar(1.0), buf, 37, rec) == 0


# ---------------------------------------------------------------------------------------------------- decide
@pytest.mark.parametrize("kind, ema, warmup", [(GU.ADAM, 0.999, True), (GU.ADAM, -1.0, False), (GU.SGD, 0.9, False)],
                         ids=["adam-ema-warmup", "adam", "sgd-ema"])
@pytest.mark.parametrize("G", [1, 2, 8])
def test_decide_equals_the_twin(G, kind, ema, warmup):
    """About 40 decisions, the betas and learning rates changing twice on the way; every integer of the record and the bits
    of every fp32 scalar after every decision.  The scalars are the host-formed ones (guard_util.host_scalars is the
    arithmetic of acvae_adamw_groups_step): EQUAL, not close."""
    seq = GU.sequence(100 + G, n=42, groups=G)
    tw, rec = GU.GuardTwin(), new_record()
    snaps = []
    for calls, norm, lr, b1, b2 in seq:
        for loss, buf in calls:
            tw.witness(loss, buf)
            b = torch.from_numpy(buf).cuda() if buf.size else None
            _lib.call("acvae_guard_witness", scalar(float(loss)), b, int(buf.size), rec, stream())
        tw.decide(norm, kind, lr, b1, b2, ema, warmup)
        decide(rec, float(norm), kind, lr, b1, b2, ema, warmup)
        snaps.append((rec.clone(), tw.fields(), tw.step_size.copy(), tw.bc2_sqrt.copy(), np.float32(tw.ema_w)))
    torch.cuda.synchronize()
    assert 5 < tw.applied < 37 and tw.skipped == 42 - tw.applied
    for i, (r, fields, ss, bc, w) in enumerate(snaps):
        got = GU.read_record(r)
        for k, v in fields.items():
            assert got[k] == v, f"decision {i + 1}: {k} {got[k]} != {v}"
        assert np.array_equal(got["step_size"].view(np.int32), ss.view(np.int32)), (i, got["step_size"], ss)
        assert np.array_equal(got["bc2_sqrt"].view(np.int32), bc.view(np.int32)), (i, got["bc2_sqrt"], bc)
        assert np.float32(got["ema_w"]).view(np.int32) == w.view(np.int32), (i, got["ema_w"], w)
        assert got["reserved"] == 0
    if kind == GU.SGD:
        assert not got["step_size"].any() and not got["bc2_sqrt"].any()
    if ema < 0:
        assert got["ema_updates"] == 0 and got["ema_w"] == 0


def test_decide_at_large_counts():
    """applied far into a run (beta^t underflows to the limit 1 - 0) and the int64 counters past 2^32."""
    rec = new_record(applied=(1 << 33) + 5, skipped=(1 << 32) + 1, streak=0, ema_updates=(1 << 33))
    decide(rec, 2.0, GU.ADAM, [1e-3], [0.9], [0.999], 0.999, True)
    decide(rec, float("inf"), GU.ADAM, [1e-3], [0.9], [0.999], 0.999, True)
    got = GU.read_record(rec)
    assert (got["applied"], got["skipped"], got["streak"], got["ema_updates"], got["ok"]) == \
        ((1 << 33) + 6, (1 << 32) + 2, 1, (1 << 33) + 1, 0)
    assert got["step_size"][0] == np.float32(1e-3) and got["bc2_sqrt"][0] == np.float32(1.0)
    assert got["ema_w"] == GU.host_ema_w(0.999, 1 << 33, True)


# ---------------------------------------------------------------------------------------------------- guarded update
KINDS = {
    "Adam": dict(adam=True, decoupled=0, amsgrad=0),
    "AdamW": dict(adam=True, decoupled=1, amsgrad=0),
    "AdamW-amsgrad": dict(adam=True, decoupled=1, amsgrad=1),
    "SGD": dict(adam=False),
}


def edge_layout(G):
    """Chunks of 1, 3, 4 and 5 float4s and of a chunk -1 / +0 / +1 float4, twice, the groups in turn; slice 5 is never
    covered (a NaN-filled gap between segments)."""
    c = chunk()
    sizes = [4, 12, 16, 20, c - 4, c, c + 4] * 2
    return U.Layout(sizes, [i % G for i in range(len(sizes))], c)


NEVER = 5


def run_update(L, G, kind, guarded, clip=True, holes=(NEVER,), start_step=3, steps=2, seed=11):
    """``steps`` updates from the same start.  guarded: decide on a record that holds applied = start_step - 1, then the
    guarded entry; otherwise the unguarded entry with step = start_step, start_step + 1, ...  Both read the same norm."""
    K = KINDS[kind]
    gen = torch.Generator().manual_seed(seed)
    n = L.n
    hole = L.mask(holes)
    nan = torch.full((n,), float("nan"))
    p0 = torch.where(hole, nan, torch.randn(n, generator=gen))
    p = U.padded(p0, n)
    st = [U.padded(torch.where(hole, nan, torch.rand(n, generator=gen) * 0.1), n) for _ in range(3)]
    tn, gn = torch.zeros(1, device="cuda"), torch.zeros(G, device="cuda")
    hy = [U.group_hyper(k) for k in range(G)]
    lr, wd = U.doubles(h["lr"] for h in hy), U.doubles(h["weight_decay"] for h in hy)
    b1, b2 = U.doubles(h["betas"][0] for h in hy), U.doubles(h["betas"][1] for h in hy)
    eps = U.doubles(h["eps"] for h in hy)
    rec = new_record(applied=start_step - 1)
    table = torch.from_numpy(L.table(holes)).cuda()
    nc = table.shape[0]
    partials = torch.empty(nc, device="cuda")
    max_norm = None
    for k in range(steps):
        gd = U.padded(torch.where(hole, nan, torch.randn(n, generator=gen) * (1.0 + k)), n)
        _lib.call("acvae_grad_norm_groups", gd, table, nc, G, GSCALE, partials, gn, tn, stream())
        if max_norm is None:
            max_norm = 0.5 * float(tn.item()) if clip else 0.0
        if guarded:
            _lib.call("acvae_guard_decide", rec, tn, GU.ADAM if K["adam"] else GU.SGD, G, lr, b1, b2, -1.0, 0, stream())
            if K["adam"]:
                _lib.call("acvae_adamw_groups_step_guarded", p, gd, st[0], st[1], st[2] if K["amsgrad"] else None, n, table,
                          nc, G, lr, b1, b2, eps, wd, K["decoupled"], K["amsgrad"], GSCALE, max_norm, tn, rec, stream())
            else:
                _lib.call("acvae_sgd_groups_step_guarded", p, gd, n, table, nc, G, lr, wd, GSCALE, max_norm, tn, rec,
                          stream())
        elif K["adam"]:
            _lib.call("acvae_adamw_groups_step", p, gd, st[0], st[1], st[2] if K["amsgrad"] else None, n, table, nc, G, lr,
                      b1, b2, eps, wd, K["decoupled"], K["amsgrad"], start_step + k, GSCALE, max_norm, tn, stream())
        else:
            _lib.call("acvae_sgd_groups_step", p, gd, None, n, table, nc, G, lr, U.doubles([0.0] * G), wd, 0.0, 0, GSCALE,
                      max_norm, tn, stream())
    torch.cuda.synchronize()
    return [p] + st, p0, rec


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("kind", list(KINDS))
def test_guarded_update_applied_equals_the_unguarded_bit_for_bit(kind, G, clip):
    L = edge_layout(G)
    got, p0, rec = run_update(L, G, kind, True, clip)
    want, _, _ = run_update(L, G, kind, False, clip)
    r = GU.read_record(rec)
    assert (r["applied"], r["skipped"], r["ok"]) == (4, 0, 1)
    hole = L.mask([NEVER])
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool((a[L.n:] == GUARD).all()), "a kernel wrote past the end of its buffer"
        assert U.same_bits(a, b), f"buffer {i} differs from the unguarded entry"
        assert U.same_bits(a[:L.n].cpu()[hole], torch.full((int(hole.sum()),), float("nan"))), f"buffer {i}: the gap moved"
    moved = ~hole & (got[0][:L.n].cpu() != p0)
    assert int(moved.sum()) > 0.99 * int((~hole).sum()), "the update did not move the parameters"


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_guarded_update_with_more_chunks_than_workgroups(kind):
    L = U.Layout([4] * 6000, [i % 2 for i in range(6000)], chunk())
    assert L.table().shape[0] == 6000 > 4096
    got, p0, _ = run_update(L, 2, kind, True, holes=())
    want, _, _ = run_update(L, 2, kind, False, holes=())
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool((a[L.n:] == GUARD).all()) and U.same_bits(a, b), i
    assert int((got[0][:L.n].cpu() != p0).sum()) > 0.99 * L.n


@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("kind", list(KINDS))
def test_guarded_update_skipped_touches_nothing(kind, G):
    """The gradient buffer is full of NaN, so the norm is NaN and the decision is a skip: every buffer keeps its bits."""
    K = KINDS[kind]
    L = edge_layout(G)
    n = L.n
    gen = torch.Generator().manual_seed(3)
    start = [torch.randn(n, generator=gen) for _ in range(4)]
    bufs = [U.padded(x, n) for x in start]
    gd = U.padded(torch.full((n,), float("nan")), n)
    table = torch.from_numpy(L.table()).cuda()
    nc = table.shape[0]
    tn, gn, partials = torch.zeros(1, device="cuda"), torch.zeros(G, device="cuda"), torch.empty(nc, device="cuda")
    hy = [U.group_hyper(k) for k in range(G)]
    lr, wd = U.doubles(h["lr"] for h in hy), U.doubles(h["weight_decay"] for h in hy)
    b1, b2 = U.doubles(h["betas"][0] for h in hy), U.doubles(h["betas"][1] for h in hy)
    rec = new_record(applied=2)
    decide(rec, 1.0, GU.ADAM, [h["lr"] for h in hy], [h["betas"][0] for h in hy], [h["betas"][1] for h in hy])   # scalars of t = 3
    before = GU.read_record(rec)
    _lib.call("acvae_grad_norm_groups", gd, table, nc, G, GSCALE, partials, gn, tn, stream())
    _lib.call("acvae_guard_decide", rec, tn, GU.ADAM if K["adam"] else GU.SGD, G, lr, b1, b2, -1.0, 0, stream())
    if K["adam"]:
        _lib.call("acvae_adamw_groups_step_guarded", bufs[0], gd, bufs[1], bufs[2], bufs[3] if K["amsgrad"] else None, n,
                  table, nc, G, lr, b1, b2, U.doubles(h["eps"] for h in hy), wd, K["decoupled"], K["amsgrad"], GSCALE, 1.0,
                  tn, rec, stream())
    else:
        _lib.call("acvae_sgd_groups_step_guarded", bufs[0], gd, n, table, nc, G, lr, wd, GSCALE, 1.0, tn, rec, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(tn).all())
    r = GU.read_record(rec)
    assert (r["ok"], r["applied"], r["skipped"], r["streak"]) == (0, 3, 1, 1)
    assert np.array_equal(r["step_size"], before["step_size"]) and np.array_equal(r["bc2_sqrt"], before["bc2_sqrt"])
    for i, (b, x) in enumerate(zip(bufs, start)):
        assert U.same_bits(b[:n], x), f"buffer {i} moved on a skipped update"
        assert bool((b[n:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------- EMA and restore
def flat_sizes():
    c = chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, (1 << 20) + 3]


@pytest.mark.parametrize("decay, updates, warmup", [(0.999, 5000, True), (0.999, 0, True), (0.3, 7, False)],
                         ids=["warm-w-small", "warm-w-large", "w-large"])
def test_guarded_ema_both_decisions(decay, updates, warmup):
    """Applied: bit-equal to acvae_ema_step with the host-formed decay (both branches of the lerp).  Skipped: untouched."""
    from acvae_amd.trainer import ema_decay_at
    for n in flat_sizes():
        gen = torch.Generator().manual_seed(n)
        e0, p0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        for ok in (1, 0):
            rec = new_record(ema_updates=updates)
            decide(rec, 1.0 if ok else float("nan"), GU.SGD, [0.1], ema=decay, warmup=warmup)
            e, p = U.padded(e0, n), U.padded(p0, n)
            _lib.call("acvae_ema_step_guarded", e, p, n, rec, stream())
            want = U.padded(e0, n)
            if ok:
                _lib.call("acvae_ema_step", want, p, n, ema_decay_at(decay, updates, warmup), stream())
            torch.cuda.synchronize()
            assert GU.read_record(rec)["ema_updates"] == updates + ok
            assert U.same_bits(e, want), (n, ok)
            assert U.same_bits(p[:n], p0) and bool((e[n:] == GUARD).all())
            assert ok == int(not U.same_bits(e[:n], e0))


def test_restore_both_decisions():
    for n in flat_sizes():
        gen = torch.Generator().manual_seed(n)
        d0, s0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        s0[0], d0[n - 1] = float("nan"), float("inf")    # bits are copied, whatever they are
        for ok in (1, 0):
            rec = new_record()
            decide(rec, 1.0 if ok else float("inf"))
            d, s = U.padded(d0, n), U.padded(s0, n)
            _lib.call("acvae_guard_restore", d, s, n, rec, stream())
            torch.cuda.synchronize()
            assert U.same_bits(d[:n], d0 if ok else s0), (n, ok)
            assert U.same_bits(s[:n], s0) and bool((d[n:] == GUARD).all()) and bool((s[n:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------- refusals
def _raw(name, *args):
    fn = getattr(_lib.lib(), name)
    return fn(*[_lib._conv(a) for a in args])


def _args(name):
    L = U.Layout([16, 32], [0, 1], chunk())
    t = torch.from_numpy(L.table()).cuda()
    buf = lambda: torch.zeros(L.n + 4, device="cuda")
    two = lambda v: U.doubles([v, v])
    rec = torch.zeros(GU.RECORD_WORDS + 4, dtype=torch.int32, device="cuda")
    if name == "acvae_guard_witness":
        return dict(loss=buf(), buf=buf(), n_buf=L.n, record=rec, stream=stream())
    if name == "acvae_guard_decide":
        return dict(record=rec, total_norm=buf(), kind=0, n_groups=2, lr=two(1e-3), beta1=two(0.9), beta2=two(0.999),
                    ema_decay=0.5, ema_warmup=0, stream=stream())
    if name == "acvae_adamw_groups_step_guarded":
        return dict(params=buf(), grads=buf(), exp_avg=buf(), exp_avg_sq=buf(), max_exp_avg_sq=buf(), n=L.n, chunks=t,
                    n_chunks=t.shape[0], n_groups=2, lr=two(1e-3), beta1=two(0.9), beta2=two(0.999), eps=two(1e-8),
                    weight_decay=two(0.0), decoupled=0, amsgrad=1, grad_scale=1.0, max_grad_norm=0.0, total_norm=None,
                    record=rec, stream=stream())
    if name == "acvae_sgd_groups_step_guarded":
        return dict(params=buf(), grads=buf(), n=L.n, chunks=t, n_chunks=t.shape[0], n_groups=2, lr=two(1e-2),
                    weight_decay=two(0.0), grad_scale=1.0, max_grad_norm=0.0, total_norm=None, record=rec, stream=stream())
    if name == "acvae_ema_step_guarded":
        return dict(ema=buf(), params=buf(), n=L.n, record=rec, stream=stream())
    return dict(dst=buf(), snapshot=buf(), n=L.n, record=rec, stream=stream())


NULLS = lambda *keys: [(dict([(k, None)]), EINVAL) for k in keys]
SHIFTS = lambda *keys: [(dict([(k, "shift")]), EALIGN) for k in keys]
CODES = {
    "acvae_guard_witness": NULLS("record") + [(dict(n_buf=-1), EINVAL), (dict(buf=None), EINVAL)] + SHIFTS("record", "buf")
    + [(dict(loss=None), 0), (dict(buf=None, n_buf=0), 0), (dict(n_buf=0), 0), (dict(), 0)],
    "acvae_guard_decide": NULLS("record", "total_norm", "lr", "beta1", "beta2")
    + [(dict(kind=2), EINVAL), (dict(kind=-1), EINVAL), (dict(n_groups=0), EINVAL), (dict(n_groups=9), EINVAL),
       (dict(ema_decay=1.5), EINVAL), (dict(ema_decay=float("nan")), EINVAL)] + SHIFTS("record")
    + [(dict(kind=1, beta1=None, beta2=None), 0), (dict(ema_decay=-1.0), 0), (dict(ema_decay=1.0), 0), (dict(), 0)],
    "acvae_adamw_groups_step_guarded": NULLS("params", "grads", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "chunks", "lr",
                                             "beta1", "beta2", "eps", "weight_decay", "record")
    + [(dict(n=0), EINVAL), (dict(n_groups=0), EINVAL), (dict(n_groups=9), EINVAL), (dict(n_chunks=0), EINVAL)]
    + SHIFTS("params", "grads", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "chunks", "record")
    + [(dict(max_exp_avg_sq=None, amsgrad=0), 0), (dict(), 0)],
    "acvae_sgd_groups_step_guarded": NULLS("params", "grads", "chunks", "lr", "weight_decay", "record")
    + [(dict(n=0), EINVAL), (dict(n_groups=0), EINVAL), (dict(n_groups=9), EINVAL), (dict(n_chunks=0), EINVAL)]
    + SHIFTS("params", "grads", "chunks", "record") + [(dict(), 0)],
    "acvae_ema_step_guarded": NULLS("ema", "params", "record") + [(dict(n=0), EINVAL), (dict(params="alias"), EINVAL)]
    + SHIFTS("ema", "params", "record") + [(dict(), 0)],
    "acvae_guard_restore": NULLS("dst", "snapshot", "record") + [(dict(n=-4), EINVAL), (dict(snapshot="alias"), EINVAL)]
    + SHIFTS("dst", "snapshot", "record") + [(dict(), 0)],
}
_ids = lambda x: ("-".join(f"{k}={v}" for k, v in x.items()) or "valid") if isinstance(x, dict) else str(x)


@pytest.mark.parametrize("name, change, code", [(n, c, k) for n, cases in CODES.items() for c, k in cases], ids=_ids)
def test_return_codes(name, change, code):
    args = _args(name)
    first = next(iter(args))
    for k, v in change.items():
        if v == "shift":
            args[k] = args[k][1:]
        elif v == "alias":
            args[k] = args[first][4:]                    # shares bytes with the first buffer
        else:
            args[k] = v
    assert _raw(name, *args.values()) == code
    torch.cuda.synchronize()
