"""GPU: the KL objective (csrc/kl_objective.hip) through the C ABI and through acvae_amd.train_util.KLObjective, against
the float64 yardstick of tests/kl_objective_util.py at the smallest shapes that reach each edge of the kernels: one cell,
E not a multiple of 4 (scalar loads), E of more than one pass of 256 columns (260, 257, 512), cell counts one below, at and one
above the slab of ACVAE_KL_OBJECTIVE_SLAB cells, more than one slab, T beyond the longest caption, a row of length 0, all
rows at T.

Bounds: the kernels evaluate the terms and every sum in float64 and round each output to fp32 once, so the forward bound
is the store's half-ulp plus float64 evaluation terms (kl_objective_util.forward_tols); the gradients are fp32 and held to
text_ref.kl_bwd_tol, with exact zeros demanded where the gate is closed or the cell lies outside S.  Gates: lam sits at the
midpoint of the widest gap in the middle half of the yardstick's own sorted m_e / s_c; the half-gap must exceed 100 x the bound
of those values, and then every gate must match."""
import pytest
import torch

import kl_objective_util as K
import text_ref as TR
from acvae_amd import _lib
from acvae_amd.train_util import KLObjective
from text_ref import D as F64, compare
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu

S = _lib.current_stream
SLAB = int(_lib._defs["ACVAE_KL_OBJECTIVE_SLAB"])
EWORKSPACE, EINVAL = -4, -1

SHAPES = [(1, 1, 1), (2, 3, 5), (3, 5, 64), (5, 13, 260), (3, 5, 512), (2, 2, 257),
          (1, SLAB - 1, 12), (1, SLAB, 12), (SLAB + 1, 1, 12), (3, SLAB, 6)]


def lens_variants(R, T):
    """name -> lens1: ragged with the longest row at T and (R > 1) a row of 0; every row at T; every row short of T."""
    g = torch.Generator().manual_seed(R * 131 + T)
    ragged = torch.randint(0, T + 1, (R,), generator=g)
    ragged[0] = T
    if R > 1:
        ragged[R - 1] = 0
    out = {"ragged": ragged, "full": torch.full((R,), T)}
    if T > 1:
        short = torch.randint(0, T, (R,), generator=g)
        short[0] = T - 1
        out["short"] = short                            # T larger than max(lens1)
    return out


def scratch_bytes(R, T, E):
    return _lib.call("acvae_kl_objective_scratch_bytes", R, T, E)


def run_fwd(dev_ts, lens_d, Dv, lam, over, scratch=None, fill=0xFF):
    """One forward through the C ABI into guarded, prefilled outputs -> dict of host tensors (+ "gates_d" for the backward)."""
    R, T, E = dev_ts[0].shape
    free = lam is not None
    cellw = over == "cell"
    nbytes = scratch_bytes(R, T, E)
    if scratch is None:
        scratch = guarded(nbytes, fill, what="scratch")
    h = {k: guarded(n, 0xFF, what=k) for k, n in (("kl", 4), ("raw", 4), ("dims", 4 * E), ("steps", 4 * T), ("open", 4),
                                                  ("gates", (R * T if cellw else E) if free else 0))}
    f32 = lambda k: h[k].view.view(torch.float32)
    _lib.call("acvae_kl_objective_fwd", *dev_ts, lens_d, Dv, int(free), int(cellw), lam if free else 0.0, f32("kl"), f32("raw"),
              f32("dims"), f32("steps"), h["open"].view.view(torch.int32), h["gates"].view if free else None, scratch.view, nbytes,
              R, T, E, S())
    out = {"value": f32("kl").cpu()[0], "raw": f32("raw").cpu()[0], "dims": f32("dims").cpu(), "steps": f32("steps").cpu(),
           "gates_open": int(h["open"].view.view(torch.int32).cpu()[0]), "gates_d": h["gates"].view if free else None}
    out["gates"] = None if not free else out["gates_d"].cpu().bool().view((R, T) if cellw else (E,))
    return out


def run_bwd(dev_ts, lens_d, Dv, over, gates_d, g=1.0, want=(True,) * 4):
    R, T, E = dev_ts[0].shape
    hs = [guarded(R * T * E * 4, 0xFF, what=f"grad{i}") if w else None for i, w in enumerate(want)]
    outs = [None if x is None else x.view.view(torch.float32).view(R, T, E) for x in hs]
    _lib.call("acvae_kl_objective_bwd", *dev_ts, lens_d, Dv, int(over == "cell"), gates_d, torch.tensor([g], device="cuda"), *outs,
              R, T, E, S())
    return [None if o is None else o.cpu() for o in outs]


def placed(ref0, tol0, over):
    """lam from the yardstick's own unclamped values, with the half-gap asserted against the bound of those values."""
    vals, bound = (ref0["dims"], tol0["m_e"]) if over == "dim" else (ref0["s_c"][ref0["mask"]], tol0["s_c"][ref0["mask"]])
    lam, half = K.place_lam(vals)
    assert half > 100 * float(bound.max()), (over, half, float(bound.max()))
    return lam


def check_mode(tag, ts, dev_ts, lens, red, fb, over, worst):
    R, T, E = ts[0].shape
    lens_d = lens.cuda() if red == "valid" else None
    ref0 = K.objective(*ts, lens, red, None, over)
    tol0 = K.forward_tols(*ts, ref0)
    lam = None if fb is None else placed(ref0, tol0, over)
    ref = K.objective(*ts, lens, red, lam, over)
    tol = K.forward_tols(*ts, ref)
    got = run_fwd(dev_ts, lens_d, ref["D"], lam, over)
    what = f"{tag} {red} {fb} {over}"
    for key in ("value", "raw", "dims", "steps"):
        compare(got[key], ref[key], tol[key], f"{key} {what}", worst)
    assert got["gates_open"] == ref["gates_open"], what
    if lam is not None:
        assert torch.equal(got["gates"], ref["gates"]), (what, int((got["gates"] != ref["gates"]).sum()))
    g = 0.7
    grads = run_bwd(dev_ts, lens_d, ref["D"], over, got["gates_d"], g)
    for name, a, b, t in zip(("dmu_q", "dlv_q", "dmu_p", "dlv_p"), grads, K.gradients(*ts, ref, g), K.gradient_tols(*ts, ref, g)):
        compare(a, b, t, f"{name} {what}", worst)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_the_yardstick(shape):
    R, T, E = shape
    worst = {}
    for name, lens in lens_variants(R, T).items():
        *ts, _ = K.case(R, T, E, seed=R + T + E)
        dev_ts = [t.cuda() for t in ts]
        for red, fb, over in K.MODES:
            if red == "all" and name != "ragged":
                continue                                # (lens1 plays no part)
            check_mode(name, ts, dev_ts, lens, red, fb, over, worst)
    print(f"{shape}: worst error / tolerance {({k: round(v, 3) for k, v in worst.items()})}")


def test_module_value_diagnostics_and_autograd():
    R, T, E = 5, 13, 260
    *ts, lens = K.case(R, T, E, seed=2)
    for red, fb, over in K.MODES:
        ref0 = K.objective(*ts, lens, red, None, over)
        lam = None if fb is None else placed(ref0, K.forward_tols(*ts, ref0), over)
        ref = K.objective(*ts, lens, red, lam, over)
        tol = K.forward_tols(*ts, ref)
        leaves = [t.cuda().requires_grad_(True) for t in ts]
        mod = KLObjective(red, lam, over)
        for lens_arg, kw in ((lens.numpy(), {}), (lens.cuda(), {"divisor": ref["D"]}), (lens.cuda(), {})):
            val = mod(*leaves, lens1=lens_arg if red == "valid" else None, **(kw if red == "valid" else {}))
            assert val.shape == () and val.requires_grad
            compare(val.detach(), ref["value"], tol["value"], f"value {red} {fb} {over}")
            last = mod.last
            assert set(last) == {"kl_raw", "kl_dims", "kl_steps", "gates_open"} and all(v.is_cuda for v in last.values())
            assert not any(v.requires_grad for v in last.values())
            compare(last["kl_raw"], ref["raw"], tol["raw"], "kl_raw")
            compare(last["kl_dims"], ref["dims"], tol["dims"], "kl_dims")
            compare(last["kl_steps"], ref["steps"], tol["steps"], "kl_steps")
            assert int(last["gates_open"]) == ref["gates_open"] and last["gates_open"].dtype == torch.int32
        (val * 0.7).backward()
        for leaf, b, t in zip(leaves, K.gradients(*ts, ref, 0.7), K.gradient_tols(*ts, ref, 0.7)):
            compare(leaf.grad, b, t, f"grad {red} {fb} {over}")
    # only the posterior asks for a gradient: the other two outputs are not written
    leaves = [t.cuda().requires_grad_(i < 2) for i, t in enumerate(ts)]
    KLObjective("valid")(*leaves, lens1=lens.numpy()).backward()
    assert leaves[0].grad is not None and leaves[2].grad is None and leaves[3].grad is None
    # bf16 inputs are widened, not refused
    v16 = KLObjective("valid")(*[t.cuda().bfloat16() for t in ts], lens1=lens.numpy())
    assert v16.dtype == torch.float32 and bool(torch.isfinite(v16))


def test_tie_at_lam_zero_is_closed_with_an_exact_zero_gradient():
    R, T, E = 3, 5, 64
    *ts, lens = K.case(R, T, E, seed=6)
    for e in (0, 17, 63):
        ts[2][:, :, e] = ts[0][:, :, e]
        ts[3][:, :, e] = ts[1][:, :, e]
    dev_ts = [t.cuda() for t in ts]
    for red in ("all", "valid"):
        lens_d = lens.cuda() if red == "valid" else None
        ref = K.objective(*ts, lens, red, 0.0, "dim")
        got = run_fwd(dev_ts, lens_d, ref["D"], 0.0, "dim")
        for e in (0, 17, 63):
            assert float(got["dims"][e]) == 0.0 and not bool(got["gates"][e])
        assert torch.equal(got["gates"], ref["gates"]) and got["gates_open"] == E - 3
        for gr in run_bwd(dev_ts, lens_d, ref["D"], "dim", got["gates_d"]):
            assert float(gr[:, :, [0, 17, 63]].abs().max()) == 0.0
            assert not bool(gr[:, :, [0, 17, 63]].contiguous().view(torch.int32).any())   # +0 bits, not -0 or NaN
        # free_bits None differs from the clamp at 0.0 only in what it reports here, but it is another code path
        none = run_fwd(dev_ts, lens_d, ref["D"], None, "dim")
        assert none["gates_open"] == E and float(none["dims"][17]) == 0.0


def _same(a, b):
    for key in ("value", "raw", "dims", "steps"):
        assert torch.equal(a[key].view(-1).view(torch.int32), b[key].view(-1).view(torch.int32)), key
    assert a["gates_open"] == b["gates_open"]
    assert (a["gates"] is None and b["gates"] is None) or torch.equal(a["gates"], b["gates"])


@pytest.mark.parametrize("fb,over", [(None, "dim"), (0.02, "dim"), (0.5, "cell")])
def test_padded_nan_and_inf_change_no_bit_and_a_valid_nan_gives_nan(fb, over):
    R, T, E = 5, 13, 260
    *ts, lens = K.case(R, T, E, seed=7)
    pad = ~K.cell_mask(lens, R, T, "valid")
    assert int(pad.sum()) > 3
    dirty = [t.clone() for t in ts]
    for i, t in enumerate(dirty):
        t[pad] = [float("nan"), float("inf"), float("-inf"), float("nan")][i]
    Dv = int(lens.sum())
    lens_d = lens.cuda()
    a = run_fwd([t.cuda() for t in ts], lens_d, Dv, fb, over)
    b = run_fwd([t.cuda() for t in dirty], lens_d, Dv, fb, over)
    _same(a, b)
    assert bool(torch.isfinite(b["value"]))
    ga = run_bwd([t.cuda() for t in ts], lens_d, Dv, over, a["gates_d"])
    gb = run_bwd([t.cuda() for t in dirty], lens_d, Dv, over, b["gates_d"])
    for x, y in zip(ga, gb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(y[pad], torch.zeros_like(y[pad]))
    bad = [t.clone() for t in ts]
    bad[1][0, 0, 3] = float("nan")                      # row 0 is T long: a cell of S
    c = run_fwd([t.cuda() for t in bad], lens_d, Dv, fb, over)
    assert bool(torch.isnan(c["value"])) and bool(torch.isnan(c["raw"]))


@pytest.mark.parametrize("fb,over", [(None, "dim"), (0.02, "dim"), (0.5, "cell")])
def test_scratch_contents_do_not_matter_and_two_runs_agree(fb, over):
    R, T, E = 5, 13, 260
    *ts, lens = K.case(R, T, E, seed=8)
    dev_ts = [t.cuda() for t in ts]
    Dv, lens_d = int(lens.sum()), lens.cuda()
    base = run_fwd(dev_ts, lens_d, Dv, fb, over, fill=0x00)
    _same(base, run_fwd(dev_ts, lens_d, Dv, fb, over, fill=0x00))                   # two runs
    _same(base, run_fwd(dev_ts, lens_d, Dv, fb, over, fill=0xFF))                   # 0xFF: NaN as float64 too
    nan = guarded(scratch_bytes(R, T, E), 0, what="scratch")
    nan.view.view(torch.float64).fill_(float("nan"))
    _same(base, run_fwd(dev_ts, lens_d, Dv, fb, over, scratch=nan))
    used = guarded(scratch_bytes(R, T, E), 0, what="scratch")
    *other, _ = K.case(R, T, E, seed=9)
    run_fwd([t.cuda() * 3 for t in other], None, R * T, 0.1, "cell", scratch=used)   # a previous call's contents
    _same(base, run_fwd(dev_ts, lens_d, Dv, fb, over, scratch=used))


def test_all_without_free_bits_is_gauss_kl_fwd():
    R, T, E = 5, 13, 260
    *ts, lens = K.case(R, T, E, seed=10)
    dev_ts = [t.cuda() for t in ts]
    got = run_fwd(dev_ts, None, R * T, None, "dim")
    nparts = _lib.call("acvae_kl_partials", R * T * E)
    part, out = torch.empty(nparts, device="cuda"), torch.empty(1, device="cuda")
    _lib.call("acvae_gauss_kl_fwd", *dev_ts, part, out, R * T, E, S())
    ref = K.objective(*ts, lens, "all")
    bound = TR.kl_fwd_tol(*ts, R * T, nparts) + K.forward_tols(*ts, ref)["value"]
    compare(got["value"], out.cpu()[0].to(F64), bound, "objective against acvae_gauss_kl_fwd")
    compare(got["value"], ref["value"], K.forward_tols(*ts, ref)["value"], "objective against the yardstick")


def test_valid_without_free_bits_is_the_sum_of_caption_terms():
    from acvae_amd.likelihood import caption_terms
    R, T, E, V = 5, 13, 260, 11
    *ts, lens = K.case(R, T, E, seed=11)
    dev_ts = [t.cuda() for t in ts]
    Dv, lens_d = int(lens.sum()), lens.cuda()
    got = run_fwd(dev_ts, lens_d, Dv, None, "dim")
    g = torch.Generator().manual_seed(1)
    output = dict(zip(("q_means", "q_logs", "p_means", "p_logs"), dev_ts), logits=torch.randn(R, T, V, generator=g).cuda())
    terms = caption_terms(output, torch.randint(0, V, (R, T), generator=g).cuda(), lens_d)
    ref = K.objective(*ts, lens, "valid")
    tol = K.forward_tols(*ts, ref)
    # caption_terms rounds each cell's s_c to fp32 before its float64 row sums: U |s_c| per cell on top of the bound
    cell_round = TR.U * ref["s_c"].abs()
    compare(got["value"].to(F64) * Dv, terms["kl"].sum().cpu(), Dv * tol["value"] + cell_round.sum() + tol["s_c"].sum(),
            "D x objective against sum of caption_terms kl")
    n_t = ref["mask"].sum(0).clamp_min(1)
    col = terms["kl_steps"].cpu().to(F64).sum(0) / n_t
    compare(got["steps"], col, tol["steps"] + (cell_round.sum(0) + tol["s_c"].sum(0)) / n_t + TR.U * col.abs(),
            "kl_steps against caption_terms' column means")


def test_short_scratch_bad_arguments_and_misaligned_bases():
    R, T, E = 3, 5, 64
    *ts, lens = K.case(R, T, E, seed=12)
    dev_ts = [t.cuda() for t in ts]
    Dv, lens_d = int(lens.sum()), lens.cuda()
    lib = _lib.lib()
    need = scratch_bytes(R, T, E)
    nslab = -(-R * T // SLAB)
    assert need == 8 * (nslab * E + R * T + E)
    assert scratch_bytes(0, T, E) == 0 and scratch_bytes(R, T, 0) == 0
    outs = {k: guarded(n, 0xFF, what=k) for k, n in (("kl", 4), ("raw", 4), ("dims", 4 * E), ("steps", 4 * T), ("open", 4),
                                                     ("gates", E), ("scratch", need))}
    ptr = lambda x: None if x is None else x.data_ptr()

    def fwd(ts_=dev_ts, lens_=lens_d, D_=Dv, free=1, cellw=0, lam=0.1, nbytes=need, R_=R, T_=T, E_=E, drop=None):
        o = {k: (None if k == drop else h) for k, h in outs.items()}
        return lib.acvae_kl_objective_fwd(*[ptr(t) for t in ts_], ptr(lens_), D_, free, cellw, lam, ptr(o["kl"]), ptr(o["raw"]),
                                          ptr(o["dims"]), ptr(o["steps"]), ptr(o["open"]), ptr(o["gates"]), ptr(o["scratch"]),
                                          nbytes, R_, T_, E_, S())

    assert fwd(nbytes=need - 1) == EWORKSPACE
    for bad in (dict(R_=0), dict(T_=0), dict(E_=0), dict(D_=0), dict(D_=R * T + 1), dict(lens_=None, D_=Dv), dict(lam=-0.5),
                dict(lam=float("nan")), dict(lam=float("inf")), dict(drop="kl"), dict(drop="dims"), dict(drop="gates"),
                dict(drop="scratch"), dict(ts_=[dev_ts[0], None, dev_ts[2], dev_ts[3]]), dict(R_=2 ** 16, T_=2 ** 15)):
        assert fwd(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    for k, h in outs.items():                           # nothing was written by any refused call
        assert bool((h.view == 0xFF).all()), k
    assert fwd(free=0, lam=float("nan"), drop="gates") == 0          # lam and gates are not looked at without free bits
    g1 = torch.ones(1, device="cuda")
    d = [torch.empty(R, T, E, device="cuda") for _ in range(4)]
    bwd = lambda **kw: lib.acvae_kl_objective_bwd(*[ptr(t) for t in kw.get("ts_", dev_ts)], ptr(lens_d), kw.get("D_", Dv), 0, None,
                                                  ptr(kw.get("g", g1)), *[ptr(x) for x in kw.get("d", d)], kw.get("R_", R), T, E, S())
    assert bwd(R_=0) == EINVAL and bwd(D_=0) == EINVAL and bwd(g=None) == EINVAL
    assert bwd(ts_=[None] + dev_ts[1:]) == EINVAL and bwd(d=[None] * 4) == 0 and bwd() == 0

    # a base that is not 16-byte aligned takes the scalar loads: the same bits as the aligned copy, forward and backward
    for fb, over in ((None, "dim"), (0.05, "dim"), (0.3, "cell")):
        aligned = run_fwd(dev_ts, lens_d, Dv, fb, over)
        ga = run_bwd(dev_ts, lens_d, Dv, over, aligned["gates_d"])
        for which in range(4):
            shifted = list(dev_ts)
            buf = torch.empty(R * T * E + 1, device="cuda")
            shifted[which] = buf[1:].view(R, T, E).copy_(dev_ts[which])
            assert shifted[which].data_ptr() % 16 == 4
            off = run_fwd(shifted, lens_d, Dv, fb, over)
            _same(aligned, off)
            for x, y in zip(ga, run_bwd(shifted, lens_d, Dv, over, off["gates_d"])):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_any_subset_of_the_four_gradients_and_no_scratch_memory():
    R, T, E = 2, 3, 5
    *ts, lens = K.case(R, T, E, seed=13)
    dev_ts = [t.cuda() for t in ts]
    Dv, lens_d = int(lens.sum()), lens.cuda()
    full = run_bwd(dev_ts, lens_d, Dv, "dim", None, 1.3)
    for want in ((True, False, False, False), (False, True, False, True), (False, False, True, False)):
        part = run_bwd(dev_ts, lens_d, Dv, "dim", None, 1.3, want)
        for w, a, b in zip(want, part, full):
            assert (a is None) == (not w) and (a is None or torch.equal(a, b))
    from acvae_amd.build import resource_usage
    mine = {k: v for k, v in resource_usage().items() if "kl_obj_" in k}
    assert len(mine) == 6, sorted(mine)                 # slab and bwd in two forms each, finish, scalar
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vgprs"] <= 128, (k, u)
