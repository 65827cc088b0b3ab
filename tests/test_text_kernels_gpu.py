"""The text side's kernels ONE BY ONE through the per-op C ABI (acvae_attn_fwd / acvae_attn_bwd, the loss kernels,
acvae_gru_step / acvae_lstm_step / acvae_bigru_seq) against the fp64 references of tests/text_ref.py, EVERY element under the
rounding bound derived there (tests/test_text_ref_cpu.py shows the bound reachable and not vacuous), at the shapes where
the kernels branch.  Outputs and fully written workspaces start as NaN, accumulators start from random values, the
surroundings of strided outputs hold a sentinel that must survive.  The branch a case reaches is named in its id."""
import functools

import pytest
import torch

import text_ref as R
from acvae_amd import _lib
from text_ref import D
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = 777.0
WORST = {}


def S():
    return _lib.current_stream()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def nan_ws(nbytes):
    """Exactly `nbytes` between guards (tests/ws_guard.py), every float a NaN."""
    assert nbytes > 0, nbytes
    return guarded(nbytes, 0xFF).view


def check(got, ref, tol, what):
    return R.compare(got, ref, tol, what, WORST)


def lens_key(lens):
    return tuple(sorted(lens.items())) if lens else None


@functools.lru_cache(maxsize=None)
def fwd_case(N, Tq, S_, A, E, lk=None):
    """Operands, fp64 reference and bounds of one attention case: computed once, shared, never modified."""
    c = R.attn_case(N, Tq, S_, A, E, lens=dict(lk) if lk else None)
    _, w, ctx = R.attn_fwd(c["q"], c["p"], c["enc"], c["v"], c["lens"])
    tw, tc = R.attn_fwd_tol(c["q"], c["p"], c["enc"], c["v"], c["lens"])
    c.update(w=w, ctx=ctx, tw=tw, tc=tc, dev={k: c[k].cuda() for k in ("q", "p", "enc", "v", "dctx", "lens")})
    return c


def attn_fwd_call(c, N, Tq, S_, A, E, ws, flags):
    d = c["dev"]
    ctx, w = nans(N, Tq, E), nans(N, Tq, S_)
    _lib.call("acvae_attn_fwd", d["q"], Tq * A, A, d["p"], d["enc"], d["lens"], d["v"], ctx, Tq * E, E, w, Tq * S_, S_, N, Tq,
              S_, A, E, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), S(), flags)
    return ctx, w


# ------------------------------------------------------------------------------------------------ attention forward
@pytest.mark.parametrize("N,Tq,S_,A,E,lens,what", R.ATTN_FWD_CASES, ids=[f"{c[:5]} {c[6]}" for c in R.ATTN_FWD_CASES])
def test_attn_fwd_one_workgroup_form(N, Tq, S_, A, E, lens, what):
    """attn_fwd_kernel (no workspace, and again with a workspace under ACVAE_FLAG_NO_ATTN_SPLIT: the same bits): weights and
    ctx against fp64; masked weights exactly 0 (their bound is 0), a len == 0 row uniform."""
    c = fwd_case(N, Tq, S_, A, E, lens_key(lens))
    ctx, w = attn_fwd_call(c, N, Tq, S_, A, E, None, 0)
    # the declared size (0 where the shape never splits: a non-null pointer to no bytes), counters poisoned too: with
    # ACVAE_FLAG_NO_ATTN_SPLIT the call does not touch the workspace
    wsb = _lib.call("acvae_attn_fwd_workspace_bytes", N, Tq, S_, A, E)
    ws = guarded(wsb, 0xFF)
    ctx2, w2 = attn_fwd_call(c, N, Tq, S_, A, E, ws, _lib.FLAG_NO_ATTN_SPLIT)
    assert bool((ws.view == 0xFF).all())
    check(w, c["w"], c["tw"], f"attn_fwd.weights {what}")
    check(ctx, c["ctx"], c["tc"], f"attn_fwd.ctx {what}")
    assert torch.equal(w, w2) and torch.equal(ctx, ctx2)
    for n in range(N):
        ln = int(c["lens"][n])
        if 0 < ln < S_:
            assert float(w[n, :, ln:].abs().max()) == 0.0


def test_attn_fwd_strided_ctx_and_step_slices():
    """The decoder's calling convention on the one-workgroup form: ctx into the middle third of [N,3E] rows, q and weights as
    step-t slices of [N,Tc,.] buffers; everything around the outputs keeps its sentinel."""
    N, Tq, S_, A, E = R.ATTN_STRIDED_FWD
    Tc, t = 3, 1
    c = fwd_case(N, Tq, S_, A, E)
    d = c["dev"]
    qb = torch.full((N, Tc, A), SENT, device="cuda"); qb[:, t] = d["q"][:, 0]
    wb = torch.full((N, Tc, S_), SENT, device="cuda"); wb[:, t] = NAN
    cb = torch.full((N, 3 * E), SENT, device="cuda"); cb[:, E:2 * E] = NAN
    _lib.call("acvae_attn_fwd", qb.data_ptr() + 4 * t * A, Tc * A, A, d["p"], d["enc"], d["lens"], d["v"], cb.data_ptr() + 4 * E,
              3 * E, E, wb.data_ptr() + 4 * t * S_, Tc * S_, S_, N, 1, S_, A, E, None, 0, S(), 0)
    check(wb[:, t:t + 1], c["w"], c["tw"], "attn_fwd.weights step slice")
    check(cb[:, None, E:2 * E], c["ctx"], c["tc"], "attn_fwd.ctx middle third of [N,3E]")
    assert bool((wb[:, [0, 2]] == SENT).all()) and bool((cb[:, :E] == SENT).all()) and bool((cb[:, 2 * E:] == SENT).all())


@pytest.mark.parametrize("N,Tq,S_,A,E,strided,what", R.ATTN_SPLIT_CASES, ids=[f"{c[:5]} {c[6]}" for c in R.ATTN_SPLIT_CASES])
def test_attn_fwd_split_form_against_fp64(N, Tq, S_, A, E, strided, what):
    """attn_fwd_split_kernel (workspace given) against fp64, not against the other kernel."""
    c = fwd_case(N, Tq, S_, A, E)
    d = c["dev"]
    wsb = _lib.call("acvae_attn_fwd_workspace_bytes", N, Tq, S_, A, E)
    assert wsb > 1024
    ws = guarded(wsb, 0xFF).view                         # include/acvae_hip.h: the caller zeroes the first 1024 bytes (the
    ws[:1024] = 0                                        # arrival counters), ONCE; the partials behind them hold NaN
    ld = 3 * E if strided else E
    cb = torch.full((N, Tq, ld), SENT, device="cuda"); cb[..., (E if strided else 0):(2 * E if strided else E)] = NAN
    w = nans(N, Tq, S_)
    _lib.call("acvae_attn_fwd", d["q"], Tq * A, A, d["p"], d["enc"], d["lens"], d["v"], cb.data_ptr() + (4 * E if strided else 0),
              Tq * ld, ld, w, Tq * S_, S_, N, Tq, S_, A, E, ws, wsb, S(), 0)
    check(w, c["w"], c["tw"], f"attn_fwd_split.weights {what}")
    check(cb[..., E:2 * E] if strided else cb, c["ctx"], c["tc"], f"attn_fwd_split.ctx {what}")
    if strided:
        assert bool((cb[..., :E] == SENT).all()) and bool((cb[..., 2 * E:] == SENT).all())
    assert int(ws[:1024].view(torch.int32).abs().max()) == 0


# ------------------------------------------------------------------------------------------------ attention backward
def bwd_bases(N, S_, A, E, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in ((N, S_, A), (N, S_, E), (N, A))]


def attn_bwd_call(c, w32, base, N, Tq, S_, A, E):
    d = c["dev"]
    dq = nans(N, Tq, A)
    dP, dH, dv = (b.cuda() for b in base)
    wsb = _lib.call("acvae_attn_bwd_workspace_bytes", N, Tq, S_, A)
    ws = nan_ws(wsb)
    _lib.call("acvae_attn_bwd", d["dctx"], Tq * E, E, d["q"], Tq * A, A, d["p"], d["enc"], d["lens"], d["v"], w32, Tq * S_, S_,
              dq, Tq * A, A, dP, dH, dv, ws, wsb, N, Tq, S_, A, E, S())
    return dq, dP, dH, dv


@pytest.mark.parametrize("N,Tq,S_,A,E,lens,what", R.ATTN_BWD_CASES, ids=[f"{c[:5]} {c[6]}" for c in R.ATTN_BWD_CASES])
def test_attn_bwd_against_fp64(N, Tq, S_, A, E, lens, what):
    """dq (overwritten: starts NaN), dencproj / denc / dv (+= onto random values) against fp64; the weights are the fp64
    weights rounded, so the forward kernel plays no part.  Two calls are bit-identical (no atomics)."""
    c = fwd_case(N, Tq, S_, A, E, lens_key(lens))
    ref = R.attn_bwd(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"])
    base = bwd_bases(N, S_, A, E)
    tols = R.attn_bwd_tol(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"], *base)
    w32 = c["w"].float().cuda()
    got = attn_bwd_call(c, w32, base, N, Tq, S_, A, E)
    again = attn_bwd_call(c, w32, base, N, Tq, S_, A, E)
    want = [ref[0]] + [b.to(D) + r for b, r in zip(base, ref[1:])]
    for gt, wt, tl, name in zip(got, want, tols, ("dq", "dencproj", "denc", "dv")):
        check(gt, wt, tl, f"attn_bwd.{name} {what}")
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_attn_bwd_decoder_convention_accumulates_over_steps():
    """Tq = 1, dc_sn = E, dc_sj = 0, q / dq / weights step-t slices of [N,Tc,.] buffers, called for t = Tc-1 .. 0 into ONE
    dencproj / denc / dv that start from random values: result - start = the fp64 sum over the steps; dq is overwritten."""
    N, Tc, S_, A, E = R.ATTN_BWD_DECODER
    c = fwd_case(N, Tc, S_, A, E)
    d = c["dev"]
    ref = R.attn_bwd(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"])
    base = bwd_bases(N, S_, A, E)
    tols = R.attn_bwd_tol(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"], *base, steps=Tc)
    wb = c["w"].float().cuda()                                            # [N,Tc,S]
    dq = nans(N, Tc, A)
    dP, dH, dv = (b.cuda() for b in base)
    wsb = _lib.call("acvae_attn_bwd_workspace_bytes", N, 1, S_, A)
    ws = nan_ws(wsb)
    for t in range(Tc - 1, -1, -1):
        dc = d["dctx"][:, t].contiguous()                                 # [N,E]
        _lib.call("acvae_attn_bwd", dc, E, 0, d["q"].data_ptr() + 4 * t * A, Tc * A, A, d["p"], d["enc"], d["lens"], d["v"],
                  wb.data_ptr() + 4 * t * S_, Tc * S_, S_, dq.data_ptr() + 4 * t * A, Tc * A, A, dP, dH, dv, ws, wsb, N, 1, S_, A,
                  E, S())
    check(dq, ref[0], tols[0], "attn_bwd.dq decoder convention")
    for gt, b, r, tl, name in zip((dP, dH, dv), base, ref[1:], tols[1:], ("dencproj", "denc", "dv")):
        check(gt.cpu().to(D) - b.to(D), r, tl, f"attn_bwd.{name} decoder convention")


def test_attn_bwd_prior_convention_dctx_inside_3E_rows():
    """Tq = Tc in one call, dctx the middle third of a [N,Tc,3E] buffer, A = E."""
    N, Tc, S_, A, E = R.ATTN_BWD_PRIOR
    c = fwd_case(N, Tc, S_, A, E)
    d = c["dev"]
    ref = R.attn_bwd(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"])
    base = bwd_bases(N, S_, A, E)
    tols = R.attn_bwd_tol(c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"], *base)
    big = nans(N, Tc, 3 * E); big[..., E:2 * E] = d["dctx"]
    dq = nans(N, Tc, A)
    dP, dH, dv = (b.cuda() for b in base)
    wsb = _lib.call("acvae_attn_bwd_workspace_bytes", N, Tc, S_, A)
    ws = nan_ws(wsb)
    _lib.call("acvae_attn_bwd", big.data_ptr() + 4 * E, Tc * 3 * E, 3 * E, d["q"], Tc * A, A, d["p"], d["enc"], d["lens"], d["v"],
              c["w"].float().cuda(), Tc * S_, S_, dq, Tc * A, A, dP, dH, dv, ws, wsb, N, Tc, S_, A, E, S())
    want = [ref[0]] + [b.to(D) + r for b, r in zip(base, ref[1:])]
    for gt, wt, tl, name in zip((dq, dP, dH, dv), want, tols, ("dq", "dencproj", "denc", "dv")):
        check(gt, wt, tl, f"attn_bwd.{name} prior convention")


def test_attn_bwd_refusals():
    """S = 8193 and A = 2049 are UNSUPPORTED, a workspace one byte short is EWORKSPACE; nothing is launched."""
    t = torch.zeros(64, device="cuda")
    ln = torch.ones(2, dtype=torch.long, device="cuda")
    def call(N, Tq, S_, A, E, wsb):
        _lib.call("acvae_attn_bwd", t, Tq * E, E, t, Tq * A, A, t, t, ln, t, t, Tq * S_, S_, t, Tq * A, A, t, t, t, t, wsb, N, Tq, S_,
                  A, E, S())
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        call(1, 1, 8193, 4, 4, 1 << 30)
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        call(1, 1, 2, 2049, 4, 1 << 30)
    with pytest.raises(RuntimeError, match="EWORKSPACE"):
        call(1, 1, 2, 4, 4, _lib.call("acvae_attn_bwd_workspace_bytes", 1, 1, 2, 4) - 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("n", R.LOSS_SIZES, ids=lambda n: f"n={n}" + (" scalar tail" if n % 4 else "") +
                         (" past the 1024-block cap: second grid-stride pass" if n > 1024 * 1024 else ""))
def test_kl_and_mse_against_fp64(n):
    mu1, lv1, mu2, lv2 = R.kl_case(n)
    rows = 3 if n % 3 == 0 else 1
    E = n // rows
    nparts = _lib.call("acvae_kl_partials", n)
    assert nparts == min(1024, (n + 1023) // 1024)
    dv = [t.cuda() for t in (mu1, lv1, mu2, lv2)]
    part, out = nans(nparts), nans(1)
    _lib.call("acvae_gauss_kl_fwd", *dv, part, out, rows, E, S())
    check(out[0], R.kl_fwd(mu1, lv1, mu2, lv2, rows), R.kl_fwd_tol(mu1, lv1, mu2, lv2, rows, nparts), "kl_fwd")
    refs, tols = R.kl_bwd(mu1, lv1, mu2, lv2, 0.7, rows), R.kl_bwd_tol(mu1, lv1, mu2, lv2, 0.7, rows)
    g = torch.tensor([0.7], device="cuda")
    masks = [(1, 1, 1, 1)] + ([(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)] if n == 1025 else [])
    for m in masks:                                      # each output pointer null in turn
        outs = [nans(n) if k else None for k in m]
        _lib.call("acvae_gauss_kl_bwd", *dv, g, *outs, rows, E, S())
        for o, r, tl in zip(outs, refs, tols):
            if o is not None:
                check(o, r, tl, "kl_bwd")
    a, b = mu1 * 3, mu2
    part, out = nans(nparts), nans(1)
    _lib.call("acvae_mse_fwd", a.cuda(), b.cuda(), part, out, n, S())
    check(out[0], R.mse_fwd(a, b), R.mse_fwd_tol(a, b, nparts), "mse_fwd")


def test_kl_fwd_refuses_a_misaligned_pointer():
    t = torch.zeros(64, device="cuda")
    with pytest.raises(RuntimeError, match="EALIGN"):
        _lib.call("acvae_gauss_kl_fwd", t.data_ptr() + 4, t, t, t, t, t, 1, 8, S())
    torch.cuda.synchronize()


def test_reparam_past_the_grid_cap_strided_and_null_inputs():
    """513 x 512 elements (past the 1024-block cap of 262 144: the grid-stride loops take a second pass), `ml`, `z2` and `dml`
    with padded rows; dz, dmean_ext and dlog_ext null in turn."""
    rows, E = R.REPARAM_SHAPE
    g = torch.Generator().manual_seed(2)
    mean, logv, eps, dz, dm, dl = (torch.randn(rows, E, generator=g) for _ in range(6))
    logv = logv * 2
    ld = 2 * E + 4
    ml = nans(rows, ld); ml[:, :E] = mean.cuda(); ml[:, E:2 * E] = logv.cuda()
    epd = eps.cuda()
    om, ol, oz = nans(rows, E), nans(rows, E), nans(rows, E)
    z2 = torch.full((rows, 3 * E), SENT, device="cuda"); z2[:, 2 * E:] = NAN
    _lib.call("acvae_reparam_fwd", ml, ld, epd, E, om, ol, oz, E, z2.data_ptr() + 4 * 2 * E, 3 * E, rows, E, S())
    assert torch.equal(om.cpu(), mean) and torch.equal(ol.cpu(), logv)
    check(oz, R.reparam_fwd(mean, logv, eps), R.reparam_fwd_tol(mean, logv, eps), "reparam_fwd.z")
    assert torch.equal(z2[:, 2 * E:], oz) and bool((z2[:, :2 * E] == SENT).all())
    dzd, dmd, dld = dz.cuda(), dm.cuda(), dl.cuda()
    for args, dargs in (((dz, dm, dl), (dzd, dmd, dld)), ((None, dm, dl), (None, dmd, dld)), ((dz, None, dl), (dzd, None, dld)),
                        ((dz, dm, None), (dzd, dmd, None))):
        dml = torch.full((rows, ld), SENT, device="cuda"); dml[:, :2 * E] = NAN
        _lib.call("acvae_reparam_bwd", dargs[0], E, dargs[1], dargs[2], E, ol, E, epd, E, dml, ld, rows, E, S())
        (rm, rl), (tm, tl) = R.reparam_bwd(*args, logv, eps), R.reparam_bwd_tol(*args, logv, eps)
        check(dml[:, :E], rm, tm, "reparam_bwd.dmean")
        check(dml[:, E:2 * E], rl, tl, "reparam_bwd.dlogvar")
        assert bool((dml[:, 2 * E:] == SENT).all())


@pytest.mark.parametrize("V", R.CE_V)
@pytest.mark.parametrize("smooth", R.CE_SMOOTH)
@pytest.mark.parametrize("lens_kind", R.CE_LENS)
def test_ce_forward_backward_against_fp64(V, smooth, lens_kind):
    """acvae_ls_ce_fwd (rows, mean flag, sum) and acvae_ls_ce_bwd (reduction 0 with grad_rows, 1, 2): logits with a padded row
    stride whose pad is NaN, padded tg_sn, targets 0 and V - 1, lens1 None / containing 0 / T / T + 3; masked rows exactly 0.
    Once with the row kernel's lse (itself checked against fp64) and once with the fp64 lse rounded to fp32."""
    buf, tgb, lens1 = R.ce_case(V, lens_kind)
    N, T = buf.shape[:2]
    x, tg = buf[..., :V], tgb[:, :T]
    ldt = V + 3
    xb, tgd = buf.cuda(), tgb.cuda()
    l1 = None if lens1 is None else lens1.cuda()
    lse_k = nans(N, T)
    _lib.call("acvae_row_logsoftmax_argmax", xb, T * ldt, ldt, None, None, lse_k, T, 1, N, T, V, S())
    lse64 = torch.logsumexp(x.to(D), -1)
    check(lse_k, lse64, R.lse_tol(x), "row_lse")
    rows_ref, mean_ref, sum_ref = R.ce_fwd(x, tg, lens1, smooth)
    gr = torch.linspace(0.5, 1.5, N * T).view(N, T)
    g1 = torch.tensor([1.7], device="cuda")
    for lse, d_l, tag in ((lse_k, R.lse_tol(x), "kernel lse"), (lse64.float().cuda(), R.lse_tol(x, rounded_only=True), "fp64 lse rounded")):
        trows, tmean, tsum = R.ce_fwd_tol(x, tg, lens1, smooth, d_l)
        for red, ref, tol in ((0, None, None), (1, mean_ref, tmean), (2, sum_ref, tsum)):
            rows, out = nans(N, T), nans(1)
            _lib.call("acvae_ls_ce_fwd", xb, T * ldt, ldt, tgd, T + 2, l1, lse, smooth, red, rows, out, N, T, V, S())
            check(rows, rows_ref, trows, f"ce_fwd.rows {tag}")
            if red:
                check(out[0], ref, tol, f"ce_fwd.{'mean' if red == 1 else 'sum'} {tag}")
        for red, g in ((0, gr), (1, 1.7), (2, 1.7)):
            dl = torch.full((N, T, ldt), SENT, device="cuda"); dl[..., :V] = NAN
            _lib.call("acvae_ls_ce_bwd", xb, T * ldt, ldt, tgd, T + 2, l1, lse, smooth, red, None if red == 0 else g1,
                      gr.cuda() if red == 0 else None, dl, N, T, V, S())
            check(dl[..., :V], R.ce_bwd(x, tg, lens1, smooth, red, g), R.ce_bwd_tol(x, tg, lens1, smooth, red, g, d_l),
                  f"ce_bwd.reduction{red} {tag}")
            assert bool((dl[..., V:] == SENT).all())


def test_ce_refuses_a_one_word_vocabulary():
    """V = 1: s / (V - 1) has no value, and a one-word softmax no gradient; forward and backward refuse with EINVAL for any
    smoothing."""
    x, lse, rows, out = (torch.zeros(4, device="cuda") for _ in range(4))
    tg = torch.zeros(4, dtype=torch.long, device="cuda")
    for smooth in (0.1, 0.0):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_ls_ce_fwd", x, 2, 1, tg, 2, None, lse, smooth, 1, rows, out, 2, 2, 1, S())
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_ls_ce_bwd", x, 2, 1, tg, 2, None, lse, smooth, 1, out, None, rows, 2, 2, 1, S())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ recurrent cells
@pytest.mark.parametrize("N,I,H", R.RNN_STEP_CASES)
def test_gru_lstm_step_against_fp64(N, I, H):
    g = torch.Generator().manual_seed(N + I)
    x, h, c = torch.randn(N, I, generator=g), torch.randn(N, H, generator=g) * .5, torch.randn(N, H, generator=g)
    wsb = _lib.call("acvae_rnn_workspace_bytes", N, 1, I, H)
    ws = nan_ws(wsb)
    _, gw = R.rnn_weights("gru", I, H)
    ho = nans(N, H)
    _lib.call("acvae_gru_step", x.cuda(), h.cuda(), *(t.cuda() for t in gw), ho, ws, wsb, N, I, H, S())
    check(ho, R.gru_cell(x, h, *gw), R.gru_cell_tol(x, h, *gw), "gru_step.h")
    _, lw = R.rnn_weights("lstm", I, H)
    ho, co = nans(N, H), nans(N, H)
    _lib.call("acvae_lstm_step", x.cuda(), h.cuda(), c.cuda(), *(t.cuda() for t in lw), ho, co, ws, wsb, N, I, H, S())
    rh, rc = R.lstm_cell(x, h, c, *lw)
    th, tc = R.lstm_cell_tol(x, h, c, *lw)
    check(ho, rh, th, "lstm_step.h"); check(co, rc, tc, "lstm_step.c")


@pytest.mark.parametrize("n,Tc,E,H,lens", R.BIGRU_CASES, ids=lambda x: str(x))
def test_bigru_seq_against_fp64_packed_bigru(n, Tc, E, H, lens):
    """Unsorted lengths containing 1 and Tc; `hidden` at t >= len is exactly 0 (its bound is 0); the pads of X hold random
    values that must not be read into any state."""
    from acvae_amd.encoder import ptr_table
    X = torch.randn(n, Tc, E, generator=torch.Generator().manual_seed(n + Tc))
    _, w = R.rnn_weights("gru", E, H, bidirectional=True)
    ref, tol = R.bigru(X, lens, w, want_tol=True)
    wd = [t.cuda().contiguous() for t in w]
    wsb = _lib.call("acvae_rnn_workspace_bytes", n, Tc, E, H)
    ws = nan_ws(wsb)
    hidden = nans(n, Tc, 2 * H)
    _lib.call("acvae_bigru_seq", X.cuda(), torch.tensor(lens).cuda(), ptr_table(wd), hidden, ws, wsb, n, Tc, E, H, S())
    check(hidden, ref, tol, "bigru_seq.hidden")


def test_zz_worst_ratio_per_op_and_tensor():
    """Runs last in this file: prints (-s) the worst measured err / tol per op and tensor against fp64."""
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
