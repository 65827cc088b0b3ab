"""GPU: scoring given captions on the device (csrc/likelihood.hip, acvae_amd/likelihood.py, evaluate_likelihood).

The kernels alone, through the C ABI, against tests/likelihood_util.py (float64, from the definitions) at the smallest
shapes where they can go wrong; then the front on the small models of the other tests: against the yardstick applied to the
model's own forward under the same noise, against the existing unsmoothed loss, against the oracle, and end to end.

Oracle margin (test_score_captions_against_the_oracle): a caption's nll / kl may lie MARGIN = 4 (the project's usual
multiple, tests/test_bf16_oracle_gpu.py) times as far from the float64 oracle as the fp32 oracle's own value does, the fp32
oracle's distance taken per caption and no smaller than its mean over the case's captions (a single caption's fp32 error can
be zero by chance).  The fp32 oracle evaluates the caption's numbers in its own arithmetic, fp32 log-softmax, KL terms and
sums included.  The test prints the ratios; measured worst: nll 2.84 (posterior) and 1.76 (prior), kl 1.27.
"""
import json
import random
import types

import numpy as np
import pytest
import torch

import acvae_oracle as O
import likelihood_util as LU
import text_ref as R
from acvae_amd import _lib, likelihood as lk
from acvae_amd import evaluate as EV
from test_model_gpu import build_model
from test_sched_sampling_gpu import _caps
from text_ref import D
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu

S = _lib.current_stream
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ the kernels alone
def gauss_case(N, T, E, seed=0):
    """text_ref.kl_case's values, every cell carrying the extreme pair (lv1 = 8, lv2 = -8) in its first and last element."""
    mu1, lv1, mu2, lv2 = (t.view(N, T, E).clone() for t in R.kl_case(N * T * E, seed))
    for i in (0, E - 1):
        lv1[..., i] = 8.0
        lv2[..., i] = -8.0
    return mu1, lv1, mu2, lv2


def out_buffers(N, T):
    """logprob / kl prefilled with NaN, rank with -1, each between guard words."""
    h = [guarded(N * T * 4, 0xFF, what=w) for w in ("logprob", "rank", "kl")]
    return h[0].view.view(torch.float32).view(N, T), h[1].view.view(torch.int32).view(N, T), h[2].view.view(torch.float32).view(N, T)


def run_terms(xb, ld_n, ld_t, tgb, tg_sn, lens1, gauss, N, T, V):
    """-> (logprob, rank, kl) on the host and the five sums of acvae_caption_sums over those cells."""
    lp, rk, kl = out_buffers(N, T)
    l1 = None if lens1 is None else lens1.cuda()
    gd = [None] * 4 if gauss is None else [g.cuda().contiguous() for g in gauss]
    E = 0 if gauss is None else gauss[0].shape[-1]
    _lib.call("acvae_caption_terms", xb, ld_n, ld_t, tgb, tg_sn, l1, *gd, lp, rk, kl, N, T, V, E, S())
    sums = [guarded(N * 8, 0xFF, what="nll"), guarded(N * 8, 0xFF, what="kl_sum")] + \
           [guarded(N * 4, 0xFF, what=w) for w in ("tokens", "hit1", "hit5")]
    _lib.call("acvae_caption_sums", lp, rk, kl, l1, *[s.view for s in sums], N, T, S())
    got = [s.view.view(torch.float64 if i < 2 else torch.int32).cpu().numpy() for i, s in enumerate(sums)]
    return lp.cpu(), rk.cpu(), kl.cpu(), got


def check_cells(tag, x, tg, lens1, gauss, lp, rk, kl, got):
    N, T, V = x.shape
    ref_lp, ref_rk, ref_kl = LU.terms(x, tg, lens1, gauss)
    m = LU.mask(lens1, N, T)
    print(f"{tag}: logprob err/tol {R.compare(lp, ref_lp, LU.logprob_tol(x, tg, lens1), f'{tag}.logprob'):.3f}", end="")
    assert torch.equal(rk.long(), ref_rk), f"{tag}: rank"
    if gauss is not None:
        print(f", kl err/tol {R.compare(kl, ref_kl, LU.kl_tol(gauss, lens1), f'{tag}.kl'):.3f}", end="")
    print()
    # invalid cells: exact zeros in all three outputs (the prefill was NaN / -1); without a KL request kl is all zeros
    assert bool((lp[~m] == 0).all()) and bool((rk[~m] == 0).all()) and bool((kl[~m] == 0).all())
    assert not bool(torch.isnan(lp).any()) and not bool(torch.isnan(kl).any())
    if gauss is None:
        assert bool((kl == 0).all())
    # the float64 sums of the kernel's own fp32 cells: bit-equal to the sequential host loop; the counts exact
    nll, ks, tokens, h1, h5 = LU.sums(lp.numpy(), rk.numpy(), kl.numpy(), None if lens1 is None else lens1.numpy())
    assert np.array_equal(got[0].view(np.int64), nll.view(np.int64)), f"{tag}: nll sums"
    assert np.array_equal(got[1].view(np.int64), ks.view(np.int64)), f"{tag}: kl sums"
    want_tok = LU.mask(lens1, N, T).sum(1).numpy()
    assert np.array_equal(got[2], want_tok) and np.array_equal(tokens, want_tok)
    assert np.array_equal(got[3], (m & (ref_rk < 1)).sum(1).numpy()) and np.array_equal(got[3], h1)
    assert np.array_equal(got[4], (m & (ref_rk < 5)).sum(1).numpy()) and np.array_equal(got[4], h5)


E_CYCLE = (1, 63, 65, 512, None)


@pytest.mark.parametrize("V", (2, 63, 255, 257, 5001))
@pytest.mark.parametrize("lens_kind", R.CE_LENS)
def test_terms_on_padded_rows_against_fp64(V, lens_kind):
    """text_ref.ce_case: ld_t = V + 3 with NaN in the padding, tg_sn = T + 2 with -1 in the padding, targets 0 and V - 1;
    lens1 NULL / with a zero row / T / T + 3; E in {1, 63, 65, 512} or no KL.  (V + 3 is a multiple of 4 at V = 257 and 5001:
    16-byte loads with a scalar tail; scalar loads at the others.)"""
    buf, tgb, lens1 = R.ce_case(V, lens_kind)
    N, T = buf.shape[:2]
    E = E_CYCLE[((2, 63, 255, 257, 5001).index(V) + R.CE_LENS.index(lens_kind)) % 5]
    gauss = None if E is None else gauss_case(N, T, E, seed=V)
    ldt = V + 3
    runs = [run_terms(buf.cuda(), T * ldt, ldt, tgb.cuda(), T + 2, lens1, gauss, N, T, V) for _ in range(2)]
    check_cells(f"V{V}.{lens_kind}.E{E}", buf[..., :V], tgb[:, :T], lens1, gauss, *runs[0])
    for a, b in zip(runs[0][:3], runs[1][:3]):                           # two calls, identical bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


SHAPES = {                                   # (R, T, V, E, lens): contiguous rows
    "one_cell_16B_path": (1, 1, 5000, 512, None),
    "r3_four_loads_in_flight": (3, 5, 5000, 512, "mixed"),
    "r33_t65_aligned": (33, 65, 64, 4, "mixed"),
    "r161_scalar_path": (161, 5, 257, 65, "mixed"),
    "r3_t65_no_kl": (3, 65, 63, None, "mixed"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_terms_shapes_against_fp64(shape):
    Rr, T, V, E, kind = SHAPES[shape]
    g = torch.Generator().manual_seed(Rr * 1000 + T)
    x = torch.randn(Rr, T, V, generator=g) * 2
    tg = torch.randint(0, V, (Rr, T), generator=g)
    lens1 = None
    if kind == "mixed":                                                  # 0, T, T + 3 and values between
        lens1 = torch.randint(0, T + 1, (Rr,), generator=g)
        lens1[0] = T
        lens1[Rr - 1] = T + 3
        lens1[Rr // 2] = 0
    gauss = None if E is None else gauss_case(Rr, T, E, seed=Rr)
    got = run_terms(x.cuda(), T * V, V, tg.cuda(), T, lens1, gauss, Rr, T, V)
    check_cells(shape, x, tg, lens1, gauss, *got)


@pytest.mark.parametrize("V", (2, 63, 255, 257, 5001))
def test_planted_rows(V):
    """likelihood_util.planted: the target at 0 and at V - 1, ties on both sides of it, all logits equal, a logit 60 above
    the rest on and off the target, a shift of 1e4, -inf off the target - contiguous (scalar loads unless V is a multiple of
    4) and in rows padded to a multiple of 4 with NaN (16-byte loads with a tail)."""
    x, tg = LU.planted(V)
    T = x.shape[1]
    got = run_terms(x.cuda(), T * V, V, tg.cuda(), T, None, None, 1, T, V)
    check_cells(f"planted.V{V}", x, tg, None, None, *got)
    ld = (V + 3) // 4 * 4 + 4
    buf = torch.full((1, T, ld), float("nan"))
    buf[..., :V] = x
    got = run_terms(buf.cuda(), T * ld, ld, tg.cuda(), T, None, None, 1, T, V)
    check_cells(f"planted.V{V}.padded", x, tg, None, None, *got)
    rk = got[1]
    assert int(rk[0, 3]) == int(tg[0, 3]) and int(rk[0, 4]) == 0 and int(rk[0, 5]) >= 1      # all equal; on / off the peak


def test_a_target_outside_the_vocabulary_touches_nothing_out_of_range():
    """include/acvae_hip.h: logprob NaN, rank INT32_MAX, the cell's kl its own; the other cells as ever."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 63, generator=g)
    tg = torch.randint(0, 63, (2, 3), generator=g)
    bad = tg.clone()
    bad[0, 1], bad[1, 2] = 63, -7
    gauss = gauss_case(2, 3, 8)
    lp, rk, kl, _ = run_terms(x.cuda(), 3 * 63, 63, bad.cuda(), 3, None, gauss, 2, 3, 63)
    ref_lp, ref_rk, ref_kl = LU.terms(x, tg, None, gauss)
    ok = bad == tg
    assert bool(torch.isnan(lp[~ok]).all()) and bool((rk[~ok] == INT_MAX).all())
    R.compare(lp[ok], ref_lp[ok], LU.logprob_tol(x, tg, None)[ok], "logprob beside a bad target")
    assert torch.equal(rk[ok].long(), ref_rk[ok])
    R.compare(kl, ref_kl, LU.kl_tol(gauss, None), "kl")


def test_rows_without_a_defined_value():
    """include/acvae_hip.h: a row of nothing but -inf, a row with a +inf logit and a row with a NaN logit, on the target or
    off it, have no log-probability (NaN); the rank stays the count of the comparisons, except that a target whose own logit
    is NaN gets INT32_MAX, so that it is no top-1 / top-5 hit.  The cells beside them are as ever.  Scalar and 16-byte loads."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 6, 63, generator=g)
    tg = torch.full((1, 6), 5, dtype=torch.long)
    inf, nan = float("inf"), float("nan")
    x[0, 0] = -inf                       # no mass anywhere
    x[0, 1, 9] = inf                     # +inf off the target
    x[0, 2, 5] = inf                     # +inf on the target
    x[0, 3, 5] = nan                     # the target's own logit is NaN
    x[0, 4, 9] = nan                     # a NaN off the target
    lp, rk, _, got = run_terms(x.cuda(), 6 * 63, 63, tg.cuda(), 6, None, None, 1, 6, 63)
    assert bool(torch.isnan(lp[0, :5]).all())
    assert int(rk[0, 0]) == 5 and int(rk[0, 1]) == int((x[0, 1] > x[0, 1, 5]).sum()) and int(rk[0, 2]) == 0
    assert int(rk[0, 3]) == INT_MAX and int(rk[0, 4]) == int((x[0, 4] > x[0, 4, 5]).sum())
    ref_lp, ref_rk, _ = LU.terms(x[:, 5:], tg[:, 5:], None)
    R.compare(lp[:, 5:], ref_lp, LU.logprob_tol(x[:, 5:], tg[:, 5:], None), "the cell beside them")
    assert int(rk[0, 5]) == int(ref_rk[0, 0])
    assert int(got[3][0]) == int((rk[0] < 1).sum()) and int(got[4][0]) == int((rk[0] < 5).sum())
    buf = torch.full((1, 6, 64), nan)                    # the same rows at a row stride of 64: 16-byte loads with a tail
    buf[..., :63] = x
    lp4, rk4, _, _ = run_terms(buf.cuda(), 6 * 64, 64, tg.cuda(), 6, None, None, 1, 6, 63)
    assert torch.equal(rk4, rk) and torch.equal(torch.isnan(lp4), torch.isnan(lp))
    R.compare(lp4[:, 5:], ref_lp, LU.logprob_tol(x[:, 5:], tg[:, 5:], None), "the cell beside them, 16-byte loads")


def test_bad_arguments_return_einval_without_a_launch():
    x = torch.randn(2, 3, 8, device="cuda")
    tg = torch.zeros(2, 3, dtype=torch.long, device="cuda")
    lp, rk, kl = out_buffers(2, 3)
    gd = [g.cuda() for g in gauss_case(2, 3, 4)]
    none4 = [None] * 4
    good = [x, 24, 8, tg, 3, None, *none4, lp, rk, kl, 2, 3, 8, 0, S()]

    def with_(**kw):
        names = ["logits", "ld_n", "ld_t", "targets", "tg_sn", "lens1", "qm", "ql", "pm", "pl", "logprob", "rank", "kl", "R", "T",
                 "V", "E", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for kw in (dict(logits=None), dict(targets=None), dict(logprob=None), dict(rank=None), dict(R=0), dict(T=0), dict(R=-1),
               dict(V=1), dict(V=-4), dict(E=-1), dict(ld_t=-8), dict(tg_sn=-1),
               dict(qm=gd[0], ql=gd[1], pm=gd[2], pl=gd[3], E=0), dict(qm=gd[0], ql=gd[1], pm=gd[2], pl=gd[3], E=4, kl=None)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_caption_terms", *with_(**kw))
    d = torch.empty(2, dtype=D, device="cuda")
    i = torch.empty(2, dtype=torch.int32, device="cuda")
    for args in ((None, rk, kl, None, d, d, i, i, i, 2, 3), (lp, None, kl, None, d, d, i, i, i, 2, 3),
                 (lp, rk, kl, None, None, d, i, i, i, 2, 3), (lp, rk, kl, None, d, d, i, i, None, 2, 3),
                 (lp, rk, kl, None, d, d, i, i, i, 0, 3), (lp, rk, kl, None, d, d, i, i, i, 2, 0)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_caption_sums", *args, S())
    torch.cuda.synchronize()
    assert bool(torch.isnan(lp).all()) and bool((rk == -1).all()) and bool(torch.isnan(kl).all())     # nothing ran
    # three of the four Gaussians: no KL is requested, kl comes back as zeros
    _lib.call("acvae_caption_terms", *with_(qm=gd[0], ql=gd[1], pm=gd[2], E=4))
    assert bool((kl == 0).all()) and not bool(torch.isnan(lp).any())


def test_new_kernels_use_no_scratch():
    from acvae_amd.build import resource_usage
    mine = {k: v for k, v in resource_usage().items() if "caption_terms_kernel" in k or "caption_sums_kernel" in k}
    assert len(mine) == 2, sorted(mine)
    assert all(v.get("scratch", -1) == 0 for v in mine.values()), mine


# ------------------------------------------------------------------------------------------------ the front
V, E, TT, L = 44, 64, 64, 7


def make_case(B, C, K, seed, permute=True, A=None):
    """B ragged clips, C captions each (P = B * C pairs in a permuted order with their clip_index; C = 1 unpermuted: no
    clip_index), K draws; the replayed noise in the order of the forward's rows."""
    g = torch.Generator().manual_seed(seed)
    state = O.closed_form_state(O.state_shapes(V, E, E, A, E, 512))
    feats = torch.randn(B, TT, 64, generator=g)
    fl = np.array([TT] + [int(v) for v in torch.randint(17, TT, (B - 1,), generator=g)])
    P = B * C
    cl = np.array([L] + [int(v) for v in torch.randint(2, L + 1, (P - 1,), generator=g)])
    cl = cl[torch.randperm(P, generator=g).numpy()]
    caps = _caps(V, list(cl), L, g)
    ci = None
    if C > 1 or permute:
        ci = np.repeat(np.arange(B), C)[torch.randperm(P, generator=g).numpy()]
    rows = lk.Rows(cl, ci, B, K)
    Tc = int(cl.max()) - 1
    noise = dict(eps_q=torch.randn(P * K, Tc, E, generator=g), eps_p=torch.randn(Tc, P * K, E, generator=g))
    return dict(B=B, P=P, K=K, state=state, feats=feats, fl=fl, cl=cl, caps=caps, ci=ci, rows=rows, Tc=Tc, noise=noise)


def own_forward(model, c, z):
    """The model's own 4-input forward on the rows, under the same noise."""
    rows = c["rows"]
    model.eval()
    model.noise = dict(c["noise"])
    with torch.no_grad():
        return model(c["feats"].cuda(), c["fl"].copy(), c["caps"][torch.from_numpy(rows.pair)], rows.lens, ss_ratio=1.0,
                     dis_ratio=0 if z == "posterior" else 1, clip_index=rows.clip)


def yardstick_on(out, c):
    """likelihood_util on a forward's output (rows in the forward's order) -> per pair and draw, the caller's order:
    (logprob, rank, kl) [P, K, Tc] and their bounds."""
    rows = c["rows"]
    P, K, Tc = c["P"], c["K"], c["Tc"]
    tg = c["caps"][torch.from_numpy(rows.pair)][:, 1:1 + Tc].long()
    lens1 = torch.from_numpy(rows.lens - 1)
    x = out["logits"].detach().cpu()
    gauss = [out[k].detach().cpu() for k in ("q_means", "q_logs", "p_means", "p_logs")]
    back = torch.from_numpy(rows.place)
    vals = list(LU.terms(x, tg, lens1, gauss)) + [LU.logprob_tol(x, tg, lens1), LU.kl_tol(gauss, lens1)]
    return [v.view(P, K, Tc)[back] for v in vals], lens1.view(P, K)[back][:, 0]


FRONT_CASES = {                              # (B, C, K, z)
    "post_k1_no_index": (3, 1, 1, "posterior"),
    "prior_k1_no_index": (3, 1, 1, "prior"),
    "prior_k3_shared": (3, 2, 3, "prior"),
    "post_k3_shared": (2, 2, 3, "posterior"),
    "post_32_rows": (4, 4, 2, "posterior"),                              # the persistent decode launches
    "prior_32_rows": (4, 4, 2, "prior"),
    "post_33_rows": (11, 3, 1, "posterior"),                             # ... and the per-step ones
    "prior_33_rows": (11, 1, 3, "prior"),
}


def check_front(case, c, model, z):
    K = c["K"]
    model.train()
    model.encoder.eval()                                                 # a mixed state, to be found again afterwards
    model.noise = dict(c["noise"])
    fl = c["fl"].copy()
    rec = lk.score_captions(model, c["feats"], fl, c["caps"], c["cl"], clip_index=c["ci"], z=z, samples=K)
    assert model.training and model.decoder.training and not model.encoder.training
    assert np.array_equal(fl, c["fl"]), "the caller's lengths were divided"
    assert rec["z"] == z and rec["samples"] == K and rec["nll"].shape == (c["P"], K)
    assert rec["logprob"].shape == (c["P"], K, c["Tc"]) and rec["nll"].is_cuda
    out = own_forward(model, c, z)
    assert out["logits"].shape[0] == c["P"] * K
    (lp, rk, kl, tlp, tkl), lens1 = yardstick_on(out, c)
    r1 = R.compare(rec["logprob"], lp, tlp, f"{case}.logprob")
    r2 = R.compare(rec["kl_steps"], kl, tkl, f"{case}.kl")
    print(f"{case}: logprob err/tol {r1:.3f}, kl err/tol {r2:.3f}")
    assert torch.equal(rec["rank"].cpu().long(), rk)
    assert torch.equal(rec["tokens"].cpu().long(), lens1)
    assert np.array_equal(rec["tokens"].cpu().numpy(), c["cl"] - 1)
    # the per-row sums are the sequential float64 sums of the record's own cells
    P, Tc = c["P"], c["Tc"]
    flat = lambda t: t.cpu().numpy().reshape(P * K, Tc)
    nll, ks, _, h1, h5 = LU.sums(flat(rec["logprob"]), flat(rec["rank"]), flat(rec["kl_steps"]), np.repeat(c["cl"] - 1, K))
    assert np.array_equal(rec["nll"].cpu().numpy().reshape(-1).view(np.int64), nll.view(np.int64))
    assert np.array_equal(rec["kl"].cpu().numpy().reshape(-1).view(np.int64), ks.view(np.int64))
    assert np.array_equal(rec["hit1"].cpu().numpy().reshape(-1), h1) and np.array_equal(rec["hit5"].cpu().numpy().reshape(-1), h5)
    if K > 1:                                                            # the draws of a pair differ in their noise only
        assert not torch.equal(rec["logprob"][:, 0], rec["logprob"][:, 1])
    # the tie to the existing loss: sum nll / sum tokens against LabelSmoothingLoss(smoothing=0) on the same forward, within
    # that kernel's own summed bound (text_ref.ce_fwd_tol's mean)
    from acvae_amd.train_util import LabelSmoothingLoss
    rows = c["rows"]
    tg = c["caps"][torch.from_numpy(rows.pair)][:, 1:1 + Tc].long()
    l1 = torch.from_numpy(rows.lens - 1)
    ce = float(LabelSmoothingLoss(V, 0.0).masked(out["logits"], tg.cuda(), rows.lens - 1))
    x = out["logits"].detach().cpu()
    tmean = float(R.ce_fwd_tol(x, tg, l1, 0.0, R.lse_tol(x))[1])
    mine = float(rec["nll"].sum()) / float(rec["tokens"].sum() * K)
    print(f"{case}: nll per token {mine:.6f}, unsmoothed CE {ce:.6f}, |d| {abs(mine - ce):.2e} (bound {tmean:.2e})")
    assert abs(mine - ce) <= tmean
    model.check_persistent_launches()


@pytest.mark.parametrize("case", list(FRONT_CASES))
def test_score_captions_equals_the_yardstick_on_the_models_own_forward(case):
    B, C, K, z = FRONT_CASES[case]
    c = make_case(B, C, K, seed=20 + len(case), permute=C > 1)
    check_front(case, c, build_model(V, E, c["state"]), z)


@pytest.mark.parametrize("z", lk.MODES)
def test_score_captions_at_unequal_widths(z):
    """The width the training forward leaves free (tests/widths_util.py: the attention's, A = 160 beside E = H = 64)."""
    import widths_util as W
    c = make_case(3, 2, 2, seed=31, A=160)
    check_front(f"E64_A160.{z}", c, W.build_model(V, E, E, 160, E, c["state"]), z)


MARGIN = 4.0


@pytest.mark.parametrize("z", lk.MODES)
def test_score_captions_against_the_oracle(z):
    """The oracle on the repeated batch (feats[clip of the row]), same weights, captions and noise, evaluation mode, in
    float64 and in fp32: per caption row recon nll and kl (posterior) / the prior route's nll (dis_ratio=1)."""
    c = make_case(3, 2, 2, seed=41)
    rows = c["rows"]
    model = build_model(V, E, c["state"])
    model.noise = dict(c["noise"])
    rec = lk.score_captions(model, c["feats"], c["fl"].copy(), c["caps"], c["cl"], clip_index=c["ci"], z=z, samples=2)
    caps_r, idx = c["caps"][torch.from_numpy(rows.pair)], torch.from_numpy(rows.clip)
    tg = caps_r[:, 1:1 + c["Tc"]].long()
    lens1 = torch.from_numpy(rows.lens - 1)

    def oracle(dtype):
        st = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in c["state"].items()}
        noise = {k: v.to(dtype) for k, v in c["noise"].items()}
        with torch.no_grad():
            o = O.hybrid_forward(st, c["feats"][idx].to(dtype), c["fl"][rows.clip].copy(), caps_r, rows.lens, ss_ratio=1.0,
                                 dis_ratio=0 if z == "posterior" else 1, training=False, noise=noise)
        # the caption's numbers in the oracle's OWN arithmetic (the fp32 run rounds its log-softmax, KL terms and sums to
        # fp32 as any fp32 evaluation of these quantities does; in float64 this is likelihood_util.terms)
        m = LU.mask(lens1, *tg.shape)
        lp = torch.log_softmax(o["logits"], -1).gather(-1, tg.unsqueeze(-1)).squeeze(-1)
        kl = R.kl_terms(*[o[k] for k in ("q_means", "q_logs", "p_means", "p_logs")], dtype=dtype).view(*tg.shape, -1).sum(-1)
        zero = torch.zeros((), dtype=dtype)
        return -torch.where(m, lp, zero).sum(1), torch.where(m, kl, zero).sum(1)

    (nll64, kl64), (nll32, kl32) = oracle(torch.float64), oracle(torch.float32)
    back = torch.from_numpy(rows.place)
    worst = {}
    for name, got, r64, r32 in (("nll", rec["nll"], nll64, nll32), ("kl", rec["kl"], kl64, kl32)):
        r64, r32 = (v.view(c["P"], 2)[back] for v in (r64, r32))
        own = (r32 - r64).abs()
        own = torch.maximum(own, own.mean())
        err = (got.cpu() - r64).abs()
        worst[name] = float((err / own).max())
        print(f"{z}: {name} per caption: HIP |d| max {float(err.max()):.2e}, fp32 oracle |d| max {float((r32 - r64).abs().max()):.2e}, "
              f"worst ratio {worst[name]:.2f} (values ~{float(r64.abs().mean()):.2f})")
    assert max(worst.values()) <= MARGIN, worst


def _eval_case():
    from test_frontend_gpu import tiny_model, tiny_waves, vocab
    from acvae_amd import frontend as F
    fe, model, voc = F.LogMel.panns_16k(), tiny_model(), vocab()
    waves = tiny_waves()
    wav_items = [(f"clip{i}", w) for i, w in enumerate(waves)]
    feat_items = [(k, fe(w[None], [len(w)])[0][0].cpu()) for k, w in wav_items]
    key2caps = {"clip0": ["w1 w2 w3", "w4 not_a_word"], "clip1": ["w5", "w6 w7 w8 w9 w1"], "clip2": [["w2", "w2"], "w3 w1 w1"]}
    return fe, model, voc, wav_items, feat_items, key2caps


def test_evaluate_likelihood_end_to_end(tmp_path):
    fe, model, voc, wav_items, feat_items, key2caps = _eval_case()
    model.train()
    path = tmp_path / "likelihood.json"
    torch.manual_seed(11); random.seed(11)
    got = EV.evaluate_likelihood(model, feat_items, key2caps, voc, output=path, batch_size=2, z=("posterior", "prior"), samples=2)
    assert model.training and model.encoder.training
    assert json.loads(path.read_text()) == got == json.loads(json.dumps(got))
    assert set(got) == {"posterior", "prior"}
    for mode in got:
        res = got[mode]
        assert [p["key"] for p in res["pairs"]] == [[f"clip{i}", j] for i in range(3) for j in range(2)]
        assert [p["tokens"] for p in res["pairs"]] == [4, 3, 2, 6, 3, 4] and res["tokens"] == 22 and res["samples"] == 2
        assert len(res["kl_by_step"]) == 6 and all(np.isfinite(v) for v in res["kl_by_step"])
        assert 0.0 <= res["top1"] <= res["top5"] <= 1.0 and res["perplexity"] > 1.0
        assert (res["pairs"][0]["log_marginal"] is None) == (mode == "posterior")
    # the same records through score_captions and Likelihood: the same draws in the same order
    torch.manual_seed(11); random.seed(11)
    meters = {m: lk.Likelihood(m, 2) for m in ("posterior", "prior")}
    unk, start, end = voc("<unk>"), voc("<start>"), voc("<end>")
    for chunk in (feat_items[:2], feat_items[2:]):
        keys, caps, clip = [], [], []
        for b, (k, _) in enumerate(chunk):
            for j, cap in enumerate(key2caps[k]):
                words = cap.split() if isinstance(cap, str) else cap
                keys.append([k, j]); clip.append(b)
                caps.append([start] + [voc(w) for w in words] + [end])
        lens = np.array([len(cp) for cp in caps])
        pad = torch.zeros(len(caps), int(lens.max()), dtype=torch.long)
        for row, cp in zip(pad, caps):
            row[:len(cp)] = torch.tensor(cp)
        feats = torch.zeros(len(chunk), max(f.shape[0] for _, f in chunk), 64)
        for b, (_, f) in enumerate(chunk):
            feats[b, :f.shape[0]] = f
        fl = np.array([f.shape[0] for _, f in chunk])
        for m in ("posterior", "prior"):
            meters[m].update(keys, lk.score_captions(model, feats, fl, pad, lens, clip_index=np.array(clip), z=m, samples=2))
    assert {m: meters[m].result() for m in meters} == got
    assert voc("not_a_word") == unk
    # waveforms through frontend= give the run on the features that front end produces
    torch.manual_seed(11); random.seed(11)
    from_waves = EV.evaluate_likelihood(model, wav_items, key2caps, voc, batch_size=2, samples=2, frontend=fe)
    assert from_waves == got
    with pytest.raises(ValueError, match="never augments"):
        EV.evaluate_likelihood(model, wav_items, key2caps, voc, frontend=fe.augmented(types.SimpleNamespace(draw_shape=None)))
