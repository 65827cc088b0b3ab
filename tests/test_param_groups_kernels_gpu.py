"""GPU, through the C ABI: the grouped update against the one-group entries launched segment by segment (bit for bit), against
torch.optim with real param groups, the grouped norm against float64, and the refusals of the three entries."""
import ctypes

import numpy as np
import pytest
import torch

import param_groups_util as U
from acvae_amd import _lib, optim

pytestmark = pytest.mark.gpu
PAD, GUARD = U.PAD, U.GUARD
GSCALE = 0.5


def chunk():
    return int(_lib.call("acvae_opt_chunk_elems"))


def edge_sizes():
    c = chunk()
    return [4, c - 4, c, c + 4, 2 * c + 8]


def edge_layout(G):
    """The five edge sizes twice and two small slices, groups in turn; slice 6 never has a gradient (NaN-filled), slice 3
    gets its first gradient at the second step."""
    sizes = edge_sizes() * 2 + [12, 4]
    return U.Layout(sizes, [i % G for i in range(len(sizes))], chunk())


NEVER, LATE = 6, 3


def many_layout():
    """More chunks than the grouped launches have workgroups (4096), in a buffer of 24 k elements."""
    return U.Layout([4] * 6000, [i % 2 for i in range(6000)], chunk())


KINDS = {
    "Adam": dict(adam=True, decoupled=0, amsgrad=0),
    "AdamW": dict(adam=True, decoupled=1, amsgrad=0),
    "Adam-amsgrad": dict(adam=True, decoupled=0, amsgrad=1),
    "AdamW-amsgrad": dict(adam=True, decoupled=1, amsgrad=1),
    "SGD": dict(adam=False, momentum=False, dampening=0.0, nesterov=0),
    "SGD-momentum-dampening": dict(adam=False, momentum=True, dampening=0.3, nesterov=0),
    "SGD-nesterov": dict(adam=False, momentum=True, dampening=0.0, nesterov=1),
}


def run_steps(L, G, kind, clip, grouped, schedule, holes=(), seed=11):
    """Three updates.  schedule[k] = (skipped, first) of step k.  grouped: one acvae_*_groups_step per step; otherwise the
    one-group entry on every segment's slice with that group's hyperparameters.  Both read the same total_norm tensor,
    written by acvae_grad_norm_groups.  The slices `holes` (never covered) hold NaN in every buffer.  Returns the buffers
    [params, state0, state1, state2], the initial parameters, the gradients and each step's fp32 clip coefficient."""
    K = KINDS[kind]
    gen = torch.Generator().manual_seed(seed)
    n = L.n
    hole = L.mask(holes)
    nan = torch.full((n,), float("nan"))
    p0 = torch.where(hole, nan, torch.randn(n, generator=gen))
    grads = [torch.where(hole, nan, torch.randn(n, generator=gen) * s) for s in (1.0, 0.7, 2.0)]
    p = U.padded(p0, n)
    st = [U.padded(torch.where(hole, nan, torch.zeros(n)), n) for _ in range(3)]
    tn = torch.zeros(1, device="cuda")
    gn = torch.zeros(G, device="cuda")
    hy = [U.group_hyper(k) for k in range(G)]
    s = _lib.current_stream()
    max_norm, coefs = None, []
    for k, (skipped, first) in enumerate(schedule):
        gd = U.padded(grads[k], n)
        table = torch.from_numpy(L.table(skipped, first if K.get("momentum") else ())).cuda()
        partials = torch.empty(table.shape[0], device="cuda")
        _lib.call("acvae_grad_norm_groups", gd, table, table.shape[0], G, GSCALE, partials, gn, tn, s)
        if max_norm is None:
            max_norm = 0.5 * float(tn.item()) if clip else 1e6      # the later gradients are 0.7 and 2 times as large
        if grouped:
            if K["adam"]:
                _lib.call("acvae_adamw_groups_step", p, gd, st[0], st[1], st[2] if K["amsgrad"] else None, n, table,
                          table.shape[0], G, U.doubles(h["lr"] for h in hy), U.doubles(h["betas"][0] for h in hy),
                          U.doubles(h["betas"][1] for h in hy), U.doubles(h["eps"] for h in hy),
                          U.doubles(h["weight_decay"] for h in hy), K["decoupled"], K["amsgrad"], k + 1, GSCALE, max_norm,
                          tn, s)
            else:
                _lib.call("acvae_sgd_groups_step", p, gd, st[0] if K["momentum"] else None, n, table, table.shape[0], G,
                          U.doubles(h["lr"] for h in hy), U.doubles(h["momentum"] if K["momentum"] else 0.0 for h in hy),
                          U.doubles(h["weight_decay"] for h in hy), K["dampening"], K["nesterov"], GSCALE, max_norm, tn, s)
        else:
            for a, b, g, f in L.segments(skipped, first if K.get("momentum") else ()):
                h = hy[g]
                if K["adam"]:
                    _lib.call("acvae_adamw_step", p[a:b], gd[a:b], st[0][a:b], st[1][a:b], st[2][a:b] if K["amsgrad"] else None,
                              b - a, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], K["decoupled"],
                              K["amsgrad"], k + 1, GSCALE, max_norm, tn, s)
                else:
                    _lib.call("acvae_sgd_step", p[a:b], gd[a:b], st[0][a:b] if K["momentum"] else None, b - a, h["lr"],
                              h["momentum"] if K["momentum"] else 0.0, K["dampening"], h["weight_decay"], K["nesterov"],
                              int(f), GSCALE, max_norm, tn, s)
        c = U.coef_of(float(tn.item()), GSCALE, max_norm)
        assert (c < GSCALE) == clip, (c, float(tn.item()))
        coefs.append(c)
    torch.cuda.synchronize()
    return [p] + st, p0, grads, coefs


def edge_schedule(L):
    everyone = set(range(len(L.sizes)))
    return [({NEVER, LATE}, everyone), ({NEVER}, {NEVER, LATE}), ({NEVER}, {NEVER})]


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("kind", list(KINDS))
def test_grouped_step_equals_the_one_group_entries_bit_for_bit(kind, G, clip):
    """Parameters and every state buffer, over three steps, the guards behind the buffers and the NaN-filled gap (a slice
    that no chunk covers) included.  SGD-nesterov's second step has chunks with and without the `first` bit."""
    L = edge_layout(G)
    got, p0, _, _ = run_steps(L, G, kind, clip, True, edge_schedule(L), holes=[NEVER])
    want, _, _, _ = run_steps(L, G, kind, clip, False, edge_schedule(L), holes=[NEVER])
    hole = L.mask([NEVER])
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool((a[L.n:] == GUARD).all()) and bool((b[L.n:] == GUARD).all()), "a kernel wrote past the end of its buffer"
        assert U.same_bits(a, b), f"buffer {i} differs from the one-group launches"
        assert bool(torch.isnan(a[:L.n].cpu()[hole]).all()), f"buffer {i}: the gap was written"
        assert U.same_bits(a[:L.n].cpu()[hole], torch.full((int(hole.sum()),), float("nan"))), f"buffer {i}: gap bits moved"
    moved = ~hole & (got[0][:L.n].cpu() != p0)
    assert int(moved.sum()) > 0.99 * int((~hole).sum()), "the update did not move the parameters"
    assert not bool(torch.isnan(got[0][:L.n].cpu()[~hole]).any())


@pytest.mark.parametrize("kind", ["AdamW", "SGD-nesterov"])
def test_more_chunks_than_workgroups(kind):
    L = many_layout()
    assert L.table().shape[0] == 6000 > 4096
    late = set(range(0, 6000, 3))
    sched = [(late, set(range(6000))), ((), late), ((), ())]
    got, p0, _, _ = run_steps(L, 2, kind, True, True, sched)
    want, _, _, _ = run_steps(L, 2, kind, True, False, sched)
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool((a[L.n:] == GUARD).all()), "a kernel wrote past the end of its buffer"
        assert U.same_bits(a, b), f"buffer {i} differs from the one-group launches"
    # (an element whose lr * g is below half an ulp of the parameter keeps its bits under SGD)
    assert int((got[0][:L.n].cpu() != p0).sum()) > 0.99 * L.n


TORCH_CASES = [("Adam", dict(weight_decay=None)), ("AdamW", dict(weight_decay=None)),
               ("SGD", dict(momentum=None, nesterov=True))]


@pytest.mark.parametrize("name, opts", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_grouped_step_matches_torch_optim_with_param_groups(name, opts):
    """Three updates, G = 3 groups with all-different hyperparameters, clip active, against torch.optim.<X>(foreach=False)
    over real param groups on CPU fp32 copies, whose gradients are scaled by the same fp32 coefficient.  The bound and the
    loose rule are those the one-group kernels are held to (param_groups_util.agree).  With seed 11 the reference alone
    (torch on the CPU, the coefficient from a float64 norm) flags 14 / 33 / 47 / 86 loose elements at chunk sizes 4096 / 8192 /
    16384 / 32768, against caps of 41 / 82 / 164 / 328, and moves the parameters by 9.0e-3."""
    G = 3
    L = edge_layout(G)
    kind = {"Adam": "Adam", "AdamW": "AdamW", "SGD": "SGD-nesterov"}[name]
    sched = [((), set(range(len(L.sizes))))] + [((), ())] * 2
    got, p0, grads, coefs = run_steps(L, G, kind, True, True, sched)
    hy = [U.group_hyper(k) for k in range(G)]
    refs = [torch.nn.Parameter(p0[int(L.offs[i]):int(L.offs[i + 1])].clone()) for i in range(len(L.sizes))]
    groups = []
    for k in range(G):
        g = {"params": [r for i, r in enumerate(refs) if L.group_of[i] == k], "lr": hy[k]["lr"],
             "weight_decay": hy[k]["weight_decay"]}
        if name == "SGD":
            g["momentum"] = hy[k]["momentum"]
        else:
            g["betas"], g["eps"] = hy[k]["betas"], hy[k]["eps"]
        groups.append(g)
    opt = getattr(torch.optim, name)(groups, foreach=False, **({"nesterov": True, "momentum": 0.9} if name == "SGD" else {}))
    loose = torch.zeros(L.n, dtype=torch.bool)
    for k, g in enumerate(grads):
        c = torch.tensor(coefs[k], dtype=torch.float32)      # the fp32 coefficient the kernels formed from the device's norm
        for i, r in enumerate(refs):
            r.grad = g[int(L.offs[i]):int(L.offs[i + 1])] * c
            if name == "Adam":
                loose[int(L.offs[i]):int(L.offs[i + 1])] |= U.loose_elements(r.grad, r, hy[L.group_of[i]]["weight_decay"])
        opt.step()
    assert int(loose.sum()) <= U.LOOSE_CAP * L.n, int(loose.sum())
    lr_max = max(h["lr"] for h in hy)
    ref_p = torch.cat([r.detach() for r in refs])
    U.agree(got[0][:L.n], ref_p, p0, "param", loose, 30 * lr_max)
    keys = ("momentum_buffer",) if name == "SGD" else ("exp_avg", "exp_avg_sq")
    for j, key in enumerate(keys):
        ref_s = torch.cat([opt.state[r][key] for r in refs])
        U.agree(got[1 + j][:L.n], ref_s, torch.zeros(L.n), key, loose if name == "Adam" else None,
                1e-3 * float(ref_s.abs().max()))


# ---------------------------------------------------------------------------------------------------- the grouped norm
def norm_groups(L, g, G, gscale=1.0, table=None, poison=True):
    table = torch.from_numpy(L.table() if table is None else table).cuda()
    nc = table.shape[0]
    partials = torch.full((nc + PAD,), float("nan") if poison else 0.0, device="cuda")
    partials[nc:] = GUARD
    gn = torch.full((G + PAD,), GUARD, device="cuda")
    tn = torch.full((1 + PAD,), GUARD, device="cuda")
    _lib.call("acvae_grad_norm_groups", U.padded(g, L.n), table, nc, G, gscale, partials, gn, tn, _lib.current_stream())
    torch.cuda.synchronize()
    assert bool((partials[nc:] == GUARD).all()) and bool((gn[G:] == GUARD).all()) and bool((tn[1:] == GUARD).all())
    return gn[:G].cpu(), tn[:1].cpu(), partials[:nc].cpu()


def norm_bound():
    """Relative, on the sum of squares: a lane's fp32 chain over one chunk plus the block tree, for non-negative terms."""
    return (chunk() / 256 + 16) * 2.0 ** -24


WORST = {}


@pytest.mark.parametrize("G", [1, 2, 8])
def test_grouped_norm_against_float64(G):
    L = edge_layout(G)
    g = torch.randn(L.n, generator=torch.Generator().manual_seed(5)) * 3.0
    gn, tn, partials = norm_groups(L, g, G, GSCALE)
    gn2, tn2, partials2 = norm_groups(L, g, G, GSCALE)
    assert U.same_bits(gn, gn2) and U.same_bits(tn, tn2) and U.same_bits(partials, partials2), "two runs differ"
    g64 = g.double().numpy()
    sums = [float((g64[L.group_mask(k).numpy()] ** 2).sum()) for k in range(G)]
    ulp = 2.0 ** -23                                   # the output's own fp32 rounding (and that of sqrt * scale): 1 ulp
    for k in range(G):
        got = (float(gn[k]) / GSCALE) ** 2
        rel = abs(got - sums[k]) / sums[k]
        WORST[G] = max(WORST.get(G, 0.0), rel / (norm_bound() + 2 * ulp))
        print(f"G={G} group {k}: sum of squares rel err {rel:.3e}, bound {norm_bound() + 2 * ulp:.3e}")
        assert rel <= norm_bound() + 2 * ulp, (k, rel)
    rel = abs((float(tn[0]) / GSCALE) ** 2 - sum(sums)) / sum(sums)
    print(f"G={G} total: sum of squares rel err {rel:.3e}; worst ratio to the bound {max(WORST[G], rel / (norm_bound() + 2 * ulp)):.3f}")
    assert rel <= norm_bound() + 2 * ulp, rel
    # a table with a skipped slice: its elements (NaN here) reach nothing
    gg = g.clone()
    gg[L.mask([NEVER])] = float("nan")
    gn3, tn3, _ = norm_groups(L, gg, G, GSCALE, L.table({NEVER}))
    for k in range(G):
        want = float((g64[L.group_mask(k, {NEVER}).numpy()] ** 2).sum())
        assert abs((float(gn3[k]) / GSCALE) ** 2 - want) <= (norm_bound() + 2 * ulp) * want
    assert bool(torch.isfinite(tn3).all())


def test_grouped_norm_of_zero_gradients_is_exactly_zero():
    L = edge_layout(2)
    gn, tn, partials = norm_groups(L, torch.zeros(L.n), 2, GSCALE)
    assert bool((gn == 0).all()) and float(tn[0]) == 0.0 and bool((partials == 0).all())
    assert U.same_bits(gn, torch.zeros(2)) and U.same_bits(tn, torch.zeros(1))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient_stays_in_its_group(bad):
    G = 8
    L = edge_layout(G)
    g = torch.randn(L.n, generator=torch.Generator().manual_seed(6))
    clean, _, _ = norm_groups(L, g, G)
    victim = 4                                          # a slice of group 4, larger than two chunks
    g[int(L.offs[victim]) + chunk() + 5] = bad
    gn, tn, _ = norm_groups(L, g, G)
    check = torch.isnan if bad != bad else torch.isinf
    assert bool(check(gn[L.group_of[victim]])) and bool(check(tn[0]))
    others = [k for k in range(G) if k != L.group_of[victim]]
    assert bool(torch.isfinite(gn[others]).all())
    assert U.same_bits(gn[others], clean[others]), "another group's norm moved"


# ---------------------------------------------------------------------------------------------------- return codes
def _raw(name, *args):
    fn = getattr(_lib.lib(), name)
    return fn(*[_lib._conv(a) for a in args])


def _norm_args():
    L = edge_layout(2)
    t = torch.from_numpy(L.table()).cuda()
    return dict(grads=torch.zeros(L.n + 4, device="cuda"), chunks=t, n_chunks=t.shape[0], n_groups=2, grad_scale=1.0,
                partials=torch.zeros(t.shape[0], device="cuda"), group_norms=torch.zeros(2, device="cuda"),
                total_norm=torch.zeros(1, device="cuda"), stream=_lib.current_stream()), L


EINVAL, EALIGN = -1, -2


@pytest.mark.parametrize("change, code", [
    (dict(grads=None), EINVAL), (dict(chunks=None), EINVAL), (dict(partials=None), EINVAL), (dict(group_norms=None), EINVAL),
    (dict(total_norm=None), EINVAL), (dict(n_groups=0), EINVAL), (dict(n_groups=9), EINVAL), (dict(n_chunks=0), EINVAL),
    (dict(n_chunks=-1), EINVAL), (dict(grads="shift"), EALIGN), (dict(chunks="shift"), EALIGN), (dict(), 0)],
    ids=lambda x: ("-".join(f"{k}={v}" for k, v in x.items()) or "valid") if isinstance(x, dict) else str(x))
def test_norm_return_codes(change, code):
    args, _ = _norm_args()
    for k, v in change.items():
        args[k] = args[k][1:] if v == "shift" else v
    assert _raw("acvae_grad_norm_groups", *args.values()) == code
    torch.cuda.synchronize()


def _step_args(adam):
    L = edge_layout(2)
    t = torch.from_numpy(L.table()).cuda()
    buf = lambda: torch.zeros(L.n + 4, device="cuda")
    two = lambda v: U.doubles([v, v])
    if adam:
        return dict(params=buf(), grads=buf(), exp_avg=buf(), exp_avg_sq=buf(), max_exp_avg_sq=buf(), n=L.n, chunks=t,
                    n_chunks=t.shape[0], n_groups=2, lr=two(1e-3), beta1=two(0.9), beta2=two(0.999), eps=two(1e-8),
                    weight_decay=two(0.0), decoupled=0, amsgrad=1, step=1, grad_scale=1.0, max_grad_norm=0.0,
                    total_norm=None, stream=_lib.current_stream())
    return dict(params=buf(), grads=buf(), momentum_buffer=buf(), n=L.n, chunks=t, n_chunks=t.shape[0], n_groups=2,
                lr=two(1e-2), momentum=two(0.9), weight_decay=two(0.0), dampening=0.0, nesterov=0, grad_scale=1.0,
                max_grad_norm=0.0, total_norm=None, stream=_lib.current_stream())


ADAM_CODES = [(dict(params=None), EINVAL), (dict(grads=None), EINVAL), (dict(exp_avg=None), EINVAL),
              (dict(exp_avg_sq=None), EINVAL), (dict(max_exp_avg_sq=None), EINVAL), (dict(chunks=None), EINVAL),
              (dict(lr=None), EINVAL), (dict(beta1=None), EINVAL), (dict(beta2=None), EINVAL), (dict(eps=None), EINVAL),
              (dict(weight_decay=None), EINVAL), (dict(n=0), EINVAL), (dict(step=0), EINVAL), (dict(n_groups=0), EINVAL),
              (dict(n_groups=9), EINVAL), (dict(n_chunks=0), EINVAL), (dict(params="shift"), EALIGN),
              (dict(grads="shift"), EALIGN), (dict(exp_avg="shift"), EALIGN), (dict(exp_avg_sq="shift"), EALIGN),
              (dict(max_exp_avg_sq="shift"), EALIGN), (dict(chunks="shift"), EALIGN),
              (dict(max_exp_avg_sq=None, amsgrad=0), 0), (dict(), 0)]
SGD_CODES = [(dict(params=None), EINVAL), (dict(grads=None), EINVAL), (dict(momentum_buffer=None), EINVAL),
             (dict(chunks=None), EINVAL), (dict(lr=None), EINVAL), (dict(momentum=None), EINVAL),
             (dict(weight_decay=None), EINVAL), (dict(n=0), EINVAL), (dict(n_groups=0), EINVAL), (dict(n_groups=9), EINVAL),
             (dict(n_chunks=0), EINVAL), (dict(momentum="mixed"), EINVAL), (dict(nesterov=1, dampening=0.5), EINVAL),
             (dict(nesterov=1, momentum="zero"), EINVAL), (dict(params="shift"), EALIGN), (dict(grads="shift"), EALIGN),
             (dict(momentum_buffer="shift"), EALIGN), (dict(chunks="shift"), EALIGN),
             (dict(momentum_buffer=None, momentum="zero"), 0), (dict(), 0)]
_ids = lambda x: ("-".join(f"{k}={v}" for k, v in x.items()) or "valid") if isinstance(x, dict) else str(x)


def _apply(args, change):
    for k, v in change.items():
        if v == "shift":
            args[k] = args[k][1:]
        elif v == "mixed":
            args[k] = U.doubles([0.9, 0.0])
        elif v == "zero":
            args[k] = U.doubles([0.0, 0.0])
        else:
            args[k] = v
    return args


@pytest.mark.parametrize("change, code", ADAM_CODES, ids=_ids)
def test_adamw_groups_return_codes(change, code):
    args = _apply(_step_args(True), change)
    assert _raw("acvae_adamw_groups_step", *args.values()) == code
    torch.cuda.synchronize()


@pytest.mark.parametrize("change, code", SGD_CODES, ids=_ids)
def test_sgd_groups_return_codes(change, code):
    args = _apply(_step_args(False), change)
    assert _raw("acvae_sgd_groups_step", *args.values()) == code
    torch.cuda.synchronize()


def test_a_bad_table_is_never_followed():
    """Chunks that leave [0, n), name a group >= n_groups, carry unknown bits or a length above the chunk size: skipped or
    cut, and nothing outside the chunks' valid part is written.  (The host's chunk_table refuses to build such rows.)"""
    c = chunk()
    n = 4 * c
    rows = np.array([[0, 4, 0],                          # good: elements [0, 16)
                     [8, 4, 2],                          # group 2 of 2: skipped
                     [-4, 8, 0],                         # negative start: skipped
                     [16, 0, 0], [16, -3, 1],            # no length: skipped
                     [20, 4, 1 | 1024],                  # unknown bits: skipped
                     [24, 4, -1],                        # negative tag: skipped
                     [c // 2, 2 * c, 1],                 # longer than a chunk: cut to c elements
                     [n // 4 - 2, 8, 1],                 # runs over n: cut at n
                     [n // 4 + 8, 4, 0]], dtype=np.int32)   # wholly behind n: skipped
    table = torch.from_numpy(rows).cuda()
    touched = torch.zeros(n, dtype=torch.bool)
    touched[0:16] = True
    touched[2 * c:3 * c] = True
    touched[n - 8:] = True
    big = 64                                            # guard behind n wide enough for the rows that point there
    p = torch.full((n + big,), 1.0, device="cuda")
    g = torch.full((n + big,), 1.0, device="cuda")
    m = torch.zeros(n + big, device="cuda")
    v = torch.zeros(n + big, device="cuda")
    two = lambda x: U.doubles([x, x])
    _lib.call("acvae_adamw_groups_step", p, g, m, v, None, n, table, rows.shape[0], 2, two(1e-2), two(0.9), two(0.999),
              two(1e-8), two(0.0), 0, 0, 1, 1.0, 0.0, None, _lib.current_stream())
    torch.cuda.synchronize()
    for t, start in ((p, 1.0), (m, 0.0), (v, 0.0)):
        moved = (t != start).cpu()
        assert torch.equal(moved[:n], touched), (int(moved[:n].sum()), int(touched.sum()))
        assert not bool(moved[n:].any()), "written behind n"
    buf = torch.zeros(n + big, device="cuda")
    _lib.call("acvae_sgd_groups_step", p, g, buf, n, table, rows.shape[0], 2, two(1e-2), two(0.9), two(0.0), 0.0, 0, 1.0,
              0.0, None, _lib.current_stream())
    torch.cuda.synchronize()
    moved = (buf != 0).cpu()
    assert torch.equal(moved[:n], touched) and not bool(moved[n:].any())
