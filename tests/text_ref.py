"""fp64 references, derived rounding bounds, fp32 restatements and deliberately wrong variants ("mutants") of the text
side's operations: additive attention forward / backward (csrc/attention.hip), the loss kernels (csrc/losses.hip) and the
recurrent cells (csrc/rnn.hip through acvae_gru_step / acvae_lstm_step / acvae_bigru_seq).  CPU-only code:
tests/test_text_ref_cpu.py checks the references against the oracle and torch, shows that the bounds are reachable by a
correct fp32 implementation and that they flag every mutant; tests/test_text_kernels_gpu.py holds the kernels to them.

Every function takes `dtype`: float64 is the reference (fp32 inputs upcast exactly), float32 the restatement of the same
expression (for attention with the kernels' fast tanh, 1 - 2 / (exp2(2 x log2 e) + 1)).


The bound (`*_tol` functions; `compare` applies it)
---------------------------------------------------
|got - ref| <= tol for EVERY element, no element exempted or masked out.  tol is computed from the fp64 reference and the
inputs only, never from the output under test.  Where the reference is exactly 0 by construction (masked weights, masked
CE rows, `hidden` at t >= len) the derivation gives tol = 0, i.e. equality.

u = 2^-24 is the unit roundoff of fp32.  First-order propagation with two rules:

 (a) an elementary operation's error enters at U6 = 6 u times the magnitude it rounds (the 6-sigma form of
     test_kernels_gpu.chain_tol, which treats u as one sigma); tanh_att's documented 2.5e-7 absolute error per score
     term (csrc/common.h, tests/test_ops_gpu.py) enters the same way, TAU6 = 6 * 2.5e-7;
 (b) an ordered fp32 sum of K terms t_k adds  sum_tol = U6 sqrt(K) max(|sum t_k|, sqrt(sum t_k^2))  - chain_tol's random
     walk with the partial sums' rms magnitude - and the terms' own independent errors e_k add in quadrature,
     sqrt(sum e_k^2) (never the worst case sum |e_k|).  Errors that are common to all terms of a sum (the softmax
     normaliser, the row's `dot` in the backward) are fully correlated and are added linearly.

Attention forward, x = q_a + p_sa, th = tanh x:
   e_th  = TAU6 + U6 |x| (1 - th^2)                      tanh_att's error + the rounding of q + p through tanh'
   d_sc  = sqrt(sum_a (|v_a| (e_th + U6 |th|))^2) + sum_tol_A(v th)          ordered sum over A
   rel_s = d_sc + U6 |sc_s - max| + 8 U6                  exponent's rounding, expf, the scalings of the split form
   com   = sum_s w_s rel_s + (sqrt(S) + 4) U6            the normaliser: weighted mean of rel and the sum over S
   tol_w = w_s (rel_s + com)                              (d w_s = w_s (d_s - sum_j w_j d_j); 0 where masked)
   tol_c = sqrt(sum_s (w_s rel_s (h_se - ctx_e))^2) + sum_tol_S(w h) + (sqrt(S) + 8) U6 |ctx_e|
           (d ctx_e = sum_s w_s d_s (h_se - ctx_e): the common part of the weights' error cancels against the normaliser)

Attention backward (weights are an INPUT, the fp64 weights rounded to fp32):
   dw_s = dctx . h_s         t_dw  = sum_tol_E
   dot  = sum_s w_s dw_s     t_dot = sqrt(sum (w t_dw)^2) + sum_tol_S(w dw) + 2 U6 sqrt(sum (w dw)^2)
   ds_s = w_s (dw_s - dot)   ind_s = w_s t_dw + 4 U6 w_s (|dw_s| + |dot|)   (independent over s),  cor_s = w_s t_dot
   du   = ds v (1 - th^2)    e_sech = 2 |th| e_th + 2 U6
                             du_ind = |v| ((1 - th^2) ind + |ds| (e_sech + 3 U6 (1 - th^2))),  du_cor = |v| (1 - th^2) cor
   dq   = sum_s du           sqrt(sum_s du_ind^2) + sum_s du_cor + sum_tol_S(du)
   dP  += sum_j du           sqrt(sum_j du_ind^2 + du_cor^2) + sum_tol_Tq(du) + U6 (|base| + |base + dP|)
   dH  += sum_j w dctx       sum_tol_Tq(w dctx) + 2 U6 sqrt(sum (w dctx)^2) + U6 (|base| + |base + dH|)
   dv  += sum_js ds th       sqrt(sum_js (|th| ind + |ds| e_th)^2) + sqrt(sum_j (sum_s |th| cor)^2) + sum_tol(ds th) + base

Losses (two-level sums: fp32 within a block of n / nparts elements, the partials finished in double):
   KL element  lv2/2 - lv1/2 + R - 1/2, R = (e^lv1 + d^2) / (2 e^lv2):  e = U6 (8 R + 3 (|lv1|/2 + |lv2|/2 + R + 1/2))
   KL / MSE    (sqrt(sum e^2) + U6 sqrt(n / nparts) max(|sum|, sqrt(sum t^2))) / rows + U6 |out|
   KL backward / reparam: elementwise, 12 U6 times the sum of the magnitudes of the terms of each expression
   lse (row kernel)  d_l = U6 (|lse| + |max| + sqrt(V) + 4);  lse given as the rounded fp64 value: d_l = U6 |lse|
   CE row      (1 - s) t_lpt + s / (V - 1) (V d_l + t_lpt + sqrt(sum (U6 lp_c)^2) + sum_tol_V(lp)) + 4 U6 |row|,
               t_lpt = d_l + U6 (|x_t| + |lp_t|);  mean / sum: the rows' bounds added linearly (d_l may be one-sided)
   d logits    |g| (p_c (d_l + U6 (|x_c| + |l|) + 2 U6) + U6 (p_c + |td_c|)) + 2 U6 |d_c|

Recurrent cells: gi, gh are exact-fp32 GEMM chains (sum_tol over I + 1 and H + 1 terms; an error dh of the incoming h adds
sqrt(dh^2 . W_hh^2)); a sigmoid s passes s (1 - s) t_pre + 4 U6, tanh (1 - n^2) t_pre + 4 U6 |n|; the state update by the
product rule.  The BiGRU carries the bound through the sequence step by step; rows are frozen (and `hidden` is exactly 0)
at t >= len.
"""
import math

import torch
import torch.nn.functional as F

D = torch.float64
U = 2.0 ** -24
U6 = 6 * U
TAU6 = 6 * 2.5e-7
LOG2E2 = 2.8853900817779268        # 2 log2 e, csrc/common.h


# ------------------------------------------------------------------------------------------------ comparator
def ratio(got, ref, tol):
    """max over ALL elements of |got - ref| / tol, with 0 / 0 = 0 and x / 0 = inf (tol = 0 demands equality); NaN -> inf."""
    got = torch.as_tensor(got).detach().cpu().to(D); ref = torch.as_tensor(ref).detach().cpu().to(D)
    tol = torch.as_tensor(tol).detach().cpu().to(D)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = tol.expand_as(ref)
    assert bool((tol >= 0).all()) and bool(torch.isfinite(tol).all()) and bool(torch.isfinite(ref).all())
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def compare(got, ref, tol, what, worst=None):
    """Assert |got - ref| <= tol element-wise (see the module docstring); returns and records the worst err / tol."""
    r = ratio(got, ref, tol)
    if worst is not None:
        worst[what.split(" ")[0]] = max(worst.get(what.split(" ")[0], 0.0), r)
    if r > 1.0:
        got = torch.as_tensor(got).detach().cpu().to(D); ref = torch.as_tensor(ref).detach().cpu().to(D)
        err = (got - ref).abs()
        bad = ~(err <= torch.as_tensor(tol).cpu().to(D).expand_as(ref))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, worst {r:.3g} x tol "
                             f"(max |err| {float(err[torch.isfinite(err)].max()) if bool(torch.isfinite(err).any()) else float('nan'):.3e}, "
                             f"ref rms {float(ref.pow(2).mean().sqrt()):.3e})")
    return r


def flagged(mut, ref, tol):
    return ratio(mut, ref, tol) > 1.0


def rss(e, dim):
    return e.pow(2).sum(dim).sqrt()


def sum_tol(total, sumsq, K):
    return U6 * math.sqrt(K) * torch.maximum(total.abs(), sumsq.clamp_min(0).sqrt())


def fast_tanh(x):
    if x.dtype == D:
        return torch.tanh(x)
    return 1 - 2 / (torch.exp2(x * LOG2E2) + 1)


# ------------------------------------------------------------------------------------------------ attention
def len_mask(lens, S):
    return torch.arange(S).view(1, 1, S) < torch.as_tensor(lens).view(-1, 1, 1)


def attn_fwd(q, p, enc, v, lens, dtype=D, mutant=None):
    """q [N,Tq,A], p = encproj [N,S,A], enc [N,S,E], v [A], lens [N] -> scores, weights [N,Tq,S], ctx [N,Tq,E]
    (models/attn_model.py:29-45: masked_fill(~mask, -1e10) before the softmax, so a len == 0 row is uniform)."""
    q, p, enc, v = (t.to(dtype) for t in (q, p, enc, v))
    S = p.shape[1]
    terms = fast_tanh(q.unsqueeze(2) + p.unsqueeze(1)) * v
    if mutant == "score_drops_channel_A-1":
        terms = terms[..., :-1]
    sc = terms.sum(-1)
    lens = torch.as_tensor(lens)
    mask = len_mask(lens + 1 if mutant == "mask_at_len+1" else lens, S)
    w = torch.softmax(sc.masked_fill(~mask, -1e10), -1)
    return sc, w, w @ enc


def attn_fwd_tol(q, p, enc, v, lens):
    q, p, enc, v = (t.to(D) for t in (q, p, enc, v))
    S, A = p.shape[1], p.shape[2]
    x = q.unsqueeze(2) + p.unsqueeze(1)
    th = torch.tanh(x)
    e_th = TAU6 + U6 * x.abs() * (1 - th * th)
    t = th * v
    d_sc = rss(v.abs() * (e_th + U6 * th.abs()), -1) + sum_tol(t.sum(-1), t.pow(2).sum(-1), A)
    mask = len_mask(lens, S)
    sc = t.sum(-1).masked_fill(~mask, -1e10)
    w = torch.softmax(sc, -1)
    rel = torch.where(mask, d_sc, torch.zeros_like(d_sc)) + U6 * (sc - sc.max(-1, keepdim=True).values).abs() + 8 * U6
    com = (w * rel).sum(-1, keepdim=True) + (math.sqrt(S) + 4) * U6
    tol_w = w * (rel + com)
    ctx = w @ enc
    a = (w * rel).pow(2)
    var = a @ enc.pow(2) - 2 * ctx * (a @ enc) + ctx.pow(2) * a.sum(-1, keepdim=True)
    tol_c = var.clamp_min(0).sqrt() + sum_tol(ctx, w.pow(2) @ enc.pow(2), S) + (math.sqrt(S) + 8) * U6 * ctx.abs()
    return tol_w, tol_c


def attn_bwd(dctx, q, p, enc, v, lens, w=None, dtype=D, mutant=None):
    """The closed form the kernels implement (tests/test_text_ref_cpu.py: equal to autograd through attn_fwd):
    -> dq [N,Tq,A], dencproj [N,S,A], denc through ctx only [N,S,E], dv [N,A] (per clip; the caller sums over clips)."""
    if w is None:
        w = attn_fwd(q, p, enc, v, lens, dtype)[1]
    dctx, q, p, enc, v, w = (t.to(dtype) for t in (dctx, q, p, enc, v, w))
    S = p.shape[1]
    dw = dctx @ enc.transpose(1, 2)
    dot = (w * dw).sum(-1, keepdim=True)
    ds = torch.where(len_mask(lens, S), w * (dw - dot), torch.zeros((), dtype=dtype))
    th = fast_tanh(q.unsqueeze(2) + p.unsqueeze(1))
    du = ds.unsqueeze(-1) * v * (1 - th * th)
    keep = torch.ones(S, dtype=dtype)
    if mutant == "chunk_drops_frame_7":
        keep[7::8] = 0
    last = 8 * ((S + 7) // 8 - 1)
    dq = (du[:, :, :last] if mutant == "dq_without_last_chunk" else du).sum(2)
    dP = du.sum(1) * keep.view(1, S, 1)
    dH = (w.transpose(1, 2) @ dctx) * keep.view(1, S, 1)
    dsth = ds.unsqueeze(-1) * th
    dv = (dsth[:, :1] if mutant == "dv_from_j0_only" else dsth).sum((1, 2))
    return dq, dP, dH, dv


def attn_bwd_autograd(dctx, q, p, enc, v, lens):
    q, p, enc, v = (t.to(D).clone().requires_grad_(True) for t in (q, p, enc, v))
    N = q.shape[0]
    vn = v.unsqueeze(0).repeat(N, 1)                    # one copy of v per clip: dv per clip, as the kernel reports it
    S = p.shape[1]
    sc = (torch.tanh(q.unsqueeze(2) + p.unsqueeze(1)) * vn.view(N, 1, 1, -1)).sum(-1)
    w = torch.softmax(sc.masked_fill(~len_mask(lens, S), -1e10), -1)
    ctx = w @ enc
    vn.retain_grad()
    (ctx * dctx.to(D)).sum().backward()
    return q.grad, p.grad, enc.grad, vn.grad


def attn_bwd_tol(dctx, q, p, enc, v, lens, base_P=None, base_H=None, base_v=None, steps=1):
    """steps > 1: the Tq query rows arrive in `steps` separate calls that accumulate into the same dencproj / denc / dv (the
    decoder's convention): the accumulator is rounded at its own magnitude once per call, sqrt(steps) U6 (|base| + |base + sum|)."""
    rs = math.sqrt(steps)
    dctx, q, p, enc, v = (t.to(D) for t in (dctx, q, p, enc, v))
    N, Tq, A = q.shape
    S, E = enc.shape[1], enc.shape[2]
    w = attn_fwd(q, p, enc, v, lens)[1]
    mask = len_mask(lens, S)
    z = torch.zeros((), dtype=D)
    dw = dctx @ enc.transpose(1, 2)
    t_dw = sum_tol(dw, dctx.pow(2) @ enc.pow(2).transpose(1, 2), E)
    wd = w * dw
    dot = wd.sum(-1, keepdim=True)
    t_dot = rss(w * t_dw, -1).unsqueeze(-1) + sum_tol(dot, wd.pow(2).sum(-1, keepdim=True), S) + 2 * U6 * rss(wd, -1).unsqueeze(-1)
    ds = torch.where(mask, w * (dw - dot), z)
    ind = torch.where(mask, w * t_dw + 4 * U6 * w * (dw.abs() + dot.abs()), z).unsqueeze(-1)
    cor = torch.where(mask, w * t_dot, z).unsqueeze(-1)
    x = q.unsqueeze(2) + p.unsqueeze(1)
    th = torch.tanh(x)
    sech = 1 - th * th
    e_th = TAU6 + U6 * x.abs() * sech
    e_sech = 2 * th.abs() * e_th + 2 * U6
    du = ds.unsqueeze(-1) * v * sech
    du_ind = v.abs() * (sech * ind + ds.abs().unsqueeze(-1) * (e_sech + 3 * U6 * sech))
    du_cor = v.abs() * sech * cor
    dq, dP = du.sum(2), du.sum(1)
    t_dq = rss(du_ind, 2) + du_cor.sum(2) + sum_tol(dq, du.pow(2).sum(2), S)
    bP = torch.zeros_like(dP) if base_P is None else base_P.to(D)
    t_dP = (du_ind.pow(2) + du_cor.pow(2)).sum(1).sqrt() + sum_tol(dP, du.pow(2).sum(1), Tq) + rs * U6 * (bP.abs() + (bP + dP).abs())
    dH = w.transpose(1, 2) @ dctx
    sq = w.pow(2).transpose(1, 2) @ dctx.pow(2)
    bH = torch.zeros_like(dH) if base_H is None else base_H.to(D)
    t_dH = sum_tol(dH, sq, Tq) + 2 * U6 * sq.sqrt() + rs * U6 * (bH.abs() + (bH + dH).abs())
    dsth = ds.unsqueeze(-1) * th
    dv = dsth.sum((1, 2))
    bv = torch.zeros_like(dv) if base_v is None else base_v.to(D)
    t_dv = (th.abs() * ind + ds.abs().unsqueeze(-1) * e_th).pow(2).sum((1, 2)).sqrt() + rss((th.abs() * cor).sum(2), 1) + \
        sum_tol(dv, dsth.pow(2).sum((1, 2)), Tq * S) + rs * U6 * (bv.abs() + (bv + dv).abs())
    return t_dq, t_dP, t_dH, t_dv


def attn_case(N, Tq, S, A, E, seed=0, lens=None):
    """Seeded random operands; lens always contains S and 1 (and whatever `lens` pins: {row: len})."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 131 * Tq + 17 * S + 3 * A + E)
    r = lambda *s: torch.randn(*s, generator=g)
    q, p, enc, v, dctx = r(N, Tq, A), r(N, S, A), r(N, S, E), r(A) * (3.0 / math.sqrt(A)), r(N, Tq, E)
    ln = torch.randint(1, S + 1, (N,), generator=g)
    ln[0] = S
    ln[N - 1] = 1
    for k, val in (lens or {}).items():
        ln[k] = val
    return dict(q=q, p=p, enc=enc, v=v, dctx=dctx, lens=ln)


# (N, Tq, S, A, E, pinned lens, what the case reaches)
ATTN_FWD_CASES = [
    (2, 1, 9, 512, 512, None, "A=512 NA=2, S below one round of 16 waves: clamped four-frame loads"),
    (2, 1, 70, 256, 128, None, "A=256 specialisation NA=1, second round at 1024 threads"),
    (8, 32, 19, 512, 512, None, "256 rows: the 256-thread launch, second round at 4 waves, G=2"),
    (8, 32, 5, 64, 2048, None, "E/4 > blockDim: non-vec fallback at 256 threads"),
    (2, 3, 70, 1028, 36, None, "general vector loop taken twice (A > 1024)"),
    (3, 2, 9, 6, 10, None, "scalar path"),
    (3, 2, 9, 8, 10, None, "scalar path with A % 4 == 0, E % 4 != 0"),
    (3, 2, 9, 64, 64, {1: 0}, "len == 0 clip: uniform weights"),
]
ATTN_STRIDED_FWD = (4, 1, 33, 64, 128)
ATTN_SPLIT_CASES = [
    (2, 1, 17, 64, 64, False, "two splits, the second of one frame"),
    (2, 1, 32, 512, 512, False, "exact multiple of the split"),
    (16, 1, 187, 512, 512, False, "production decode step, 12 splits"),
    (5, 3, 33, 64, 128, True, "strided ctx"),
]
ATTN_BWD_CASES = [
    (2, 2, 8, 64, 64, None, "nchunk 1"),
    (2, 2, 9, 64, 64, None, "nchunk 2, one-frame tail"),
    (2, 2, 65, 64, 64, None, "nchunk 9: a ninth chunk alone in the second batch of eight"),
    (2, 2, 187, 64, 64, None, "nchunk 24: three batches of eight"),
    (2, 2, 9, 2048, 2048, None, "ATB_SLOTS: slot 3 for A and E"),
    (2, 3, 9, 1028, 36, None, "slot 2 for A, slot 0 for E, vector score path"),
    (2, 3, 9, 40, 1100, None, "slot 0 for A, slot 2 for E"),
    (8, 32, 9, 64, 64, None, "256 rows: the 256-thread score kernel"),
    (3, 2, 9, 6, 10, None, "non-vector (scalar) score path"),
    (3, 2, 9, 64, 64, {1: 0}, "len == 0"),
    (3, 2, 12, 64, 64, {1: 1}, "len == 1"),
]
ATTN_BWD_DECODER = (3, 5, 21, 64, 128)      # (N, Tc, S, A, E): Tq = 1 per call, dc_sn = E, dc_sj = 0, slices of [N,Tc,.]
ATTN_BWD_PRIOR = (3, 5, 13, 64, 64)         # Tq = Tc, dctx the middle third of [N,Tc,3E], A = E
FWD_MUTANTS = ("mask_at_len+1", "score_drops_channel_A-1")
BWD_MUTANTS = ("chunk_drops_frame_7", "dq_without_last_chunk", "dv_from_j0_only", "assign_not_accumulate")


# ------------------------------------------------------------------------------------------------ losses
def kl_terms(mu1, lv1, mu2, lv2, dtype=D):
    mu1, lv1, mu2, lv2 = (t.to(dtype).reshape(-1) for t in (mu1, lv1, mu2, lv2))
    return lv2 / 2. - lv1 / 2. + ((torch.exp(lv1) + (mu1 - mu2) ** 2.) / (2. * torch.exp(lv2))) - .5


def kl_fwd(mu1, lv1, mu2, lv2, rows, dtype=D, mutant=None):
    t = kl_terms(mu1, lv1, mu2, lv2, dtype)
    if mutant == "kl_drops_scalar_tail":
        t = t[:t.numel() // 4 * 4]
    return t.sum() / rows


def kl_fwd_tol(mu1, lv1, mu2, lv2, rows, nparts=1):
    t = kl_terms(mu1, lv1, mu2, lv2)
    mu1, lv1, mu2, lv2 = (x.to(D).reshape(-1) for x in (mu1, lv1, mu2, lv2))
    R = (torch.exp(lv1) + (mu1 - mu2) ** 2) / (2 * torch.exp(lv2))
    e = U6 * (8 * R + 3 * (lv1.abs() / 2 + lv2.abs() / 2 + R + .5))
    return (rss(e, 0) + sum_tol(t.sum(), t.pow(2).sum(), t.numel() / nparts)) / rows + U6 * (t.sum() / rows).abs()


def kl_bwd(mu1, lv1, mu2, lv2, g, rows, dtype=D):
    mu1, lv1, mu2, lv2 = (t.to(dtype) for t in (mu1, lv1, mu2, lv2))
    g = g / rows
    d, v1, iv2 = mu1 - mu2, torch.exp(lv1), 1 / torch.exp(lv2)
    return g * d * iv2, g * (-.5 + .5 * v1 * iv2), -g * d * iv2, g * (.5 - .5 * (v1 + d * d) * iv2)


def kl_bwd_tol(mu1, lv1, mu2, lv2, g, rows):
    mu1, lv1, mu2, lv2 = (t.to(D) for t in (mu1, lv1, mu2, lv2))
    g = abs(g) / rows
    d, v1, iv2 = (mu1 - mu2).abs(), torch.exp(lv1), 1 / torch.exp(lv2)
    tm = 12 * U6 * g * d * iv2
    return tm, 12 * U6 * g * (.5 + .5 * v1 * iv2), tm, 12 * U6 * g * (.5 + .5 * (v1 + d * d) * iv2)


def mse_fwd(a, b, dtype=D):
    return ((a.to(dtype) - b.to(dtype)) ** 2).sum() / a.numel()


def mse_fwd_tol(a, b, nparts=1):
    t = (a.to(D) - b.to(D)).reshape(-1) ** 2
    return (rss(3 * U6 * t, 0) + sum_tol(t.sum(), t.pow(2).sum(), t.numel() / nparts)) / t.numel() + U6 * t.mean()


def reparam_fwd(mean, logv, eps, dtype=D):
    return eps.to(dtype) * torch.exp(.5 * logv.to(dtype)) + mean.to(dtype)


def reparam_fwd_tol(mean, logv, eps):
    s = (eps.to(D) * torch.exp(.5 * logv.to(D))).abs()
    return 12 * U6 * (s + mean.to(D).abs())


def reparam_bwd(dz, dmean_ext, dlog_ext, logv, eps, dtype=D):
    """-> d mean, d logvar; any of dz, dmean_ext, dlog_ext may be None (acvae_reparam_bwd's null branches)."""
    logv, eps = logv.to(dtype), eps.to(dtype)
    g = torch.zeros_like(logv) if dz is None else dz.to(dtype)
    dm, dl = g.clone(), g * eps * .5 * torch.exp(.5 * logv)
    if dmean_ext is not None:
        dm = dm + dmean_ext.to(dtype)
    if dlog_ext is not None:
        dl = dl + dlog_ext.to(dtype)
    return dm, dl


def reparam_bwd_tol(dz, dmean_ext, dlog_ext, logv, eps):
    z = torch.zeros_like(logv, dtype=D)
    g = z if dz is None else dz.to(D).abs()
    a = g * (eps.to(D) * .5 * torch.exp(.5 * logv.to(D))).abs()
    return 12 * U6 * (g + (z if dmean_ext is None else dmean_ext.to(D).abs())), \
        12 * U6 * (a + (z if dlog_ext is None else dlog_ext.to(D).abs()))


def ce_mask(lens1, N, T):
    if lens1 is None:
        return torch.ones(N, T, dtype=torch.bool), N * T
    lens1 = torch.as_tensor(lens1)
    return torch.arange(T).view(1, T) < lens1.view(-1, 1), int(torch.clamp(lens1, max=T).sum())


def ce_fwd(logits, targets, lens1, smoothing, dtype=D, mutant=None, lse=None):
    """-> loss rows [N,T] (exactly 0 at t >= lens1[n]), mean over sum_n min(lens1[n], T), sum.  `lse`: use this
    log-sum-exp (the fp32 restatement takes the kernel's input); default: the dtype's own."""
    x = logits.to(dtype)
    N, T, V = x.shape
    lp = x - (torch.logsumexp(x, -1, keepdim=True) if lse is None else lse.to(dtype).unsqueeze(-1))
    lpt = lp.gather(-1, targets.long().unsqueeze(-1)).squeeze(-1)
    rows = -lpt
    if smoothing != 0.0:
        rows = -((1 - smoothing) * lpt + smoothing / (V if mutant == "smoothing_over_V" else V - 1) * (lp.sum(-1) - lpt))
    mask, cnt = ce_mask(lens1, N, T)
    rows = torch.where(mask, rows, torch.zeros((), dtype=dtype))
    if mutant == "mean_over_NT":
        cnt = N * T
    return rows, rows.sum() / cnt, rows.sum()


def ce_bwd(logits, targets, lens1, smoothing, reduction, g, dtype=D, mutant=None, lse=None):
    """d / d logits of sum(rows * g) (reduction 0, g [N,T]), g * mean (1) or g * sum (2)."""
    x = logits.to(dtype)
    N, T, V = x.shape
    pr = torch.exp(x - (torch.logsumexp(x, -1, keepdim=True) if lse is None else lse.to(dtype).unsqueeze(-1)))
    td = torch.full_like(x, smoothing / (V if mutant == "smoothing_over_V" else V - 1))
    td.scatter_(-1, targets.long().unsqueeze(-1), 1.0 - smoothing)
    mask, cnt = ce_mask(lens1, N, T)
    if mutant == "mean_over_NT":
        cnt = N * T
    gr = g.to(dtype) if reduction == 0 else torch.full((N, T), float(g) / (cnt if reduction == 1 else 1), dtype=dtype)
    return torch.where(mask.unsqueeze(-1), gr.unsqueeze(-1) * (pr - td), torch.zeros((), dtype=dtype))


def lse_tol(logits, rounded_only=False):
    x = logits.to(D)
    l = torch.logsumexp(x, -1)
    if rounded_only:
        return U6 * l.abs()
    return U6 * (l.abs() + x.max(-1).values.abs() + math.sqrt(x.shape[-1]) + 4)


def ce_fwd_tol(logits, targets, lens1, smoothing, d_l):
    x = logits.to(D)
    N, T, V = x.shape
    l = torch.logsumexp(x, -1, keepdim=True)
    lp = x - l
    xt = x.gather(-1, targets.long().unsqueeze(-1)).squeeze(-1)
    lpt = xt - l.squeeze(-1)
    t_lpt = d_l + U6 * (xt.abs() + lpt.abs())
    rows = ce_fwd(logits, targets, lens1, smoothing)[0]
    tol = (1 - smoothing) * t_lpt + 4 * U6 * rows.abs()
    if smoothing != 0.0:
        tol = tol + smoothing / (V - 1) * (V * d_l + t_lpt + U6 * rss(lp, -1) + sum_tol(lp.sum(-1), lp.pow(2).sum(-1), V))
    mask, cnt = ce_mask(lens1, N, T)
    tol = torch.where(mask, tol, torch.zeros((), dtype=D))
    return tol, tol.sum() / cnt + U6 * (rows.sum() / cnt).abs(), tol.sum() + U6 * rows.sum().abs()


def ce_bwd_tol(logits, targets, lens1, smoothing, reduction, g, d_l):
    x = logits.to(D)
    l = torch.logsumexp(x, -1, keepdim=True)
    d = ce_bwd(logits, targets, lens1, smoothing, reduction, g)
    N, T, V = x.shape
    mask, cnt = ce_mask(lens1, N, T)
    gr = g.to(D).abs() if reduction == 0 else torch.full((N, T), abs(float(g)) / (cnt if reduction == 1 else 1), dtype=D)
    pr = torch.exp(x - l)
    td = torch.full_like(x, smoothing / (V - 1))
    td.scatter_(-1, targets.long().unsqueeze(-1), 1.0 - smoothing)
    tol = gr.unsqueeze(-1) * (pr * (d_l.unsqueeze(-1) + U6 * (x.abs() + l.abs()) + 2 * U6) + U6 * (pr + td)) + 2 * U6 * d.abs()
    return torch.where(mask.unsqueeze(-1), tol, torch.zeros((), dtype=D))


def ce_case(V, lens_kind, N=3, T=5, seed=0):
    """Logits in rows padded to ld_t = V + 3 (pad NaN), targets in rows padded to tg_sn = T + 2, targets 0 and V - 1 present."""
    g = torch.Generator().manual_seed(31 * V + seed)
    buf = torch.full((N, T, V + 3), float("nan"))
    buf[..., :V] = torch.randn(N, T, V, generator=g) * 2
    tg = torch.full((N, T + 2), -1, dtype=torch.long)
    tg[:, :T] = torch.randint(0, V, (N, T), generator=g)
    tg[0, 0] = 0
    tg[0, 1] = V - 1
    lens1 = {"none": None, "zero": torch.tensor([T, 0, 2]), "T": torch.tensor([T, 1, T]), "T+3": torch.tensor([T + 3, 0, T])}[lens_kind]
    return buf, tg, lens1


CE_V = (2, 255, 257, 5001)
CE_SMOOTH = (0.0, 0.1)
CE_LENS = ("none", "zero", "T", "T+3")
LOSS_SIZES = (3, 15, 1025, 2051 * 512)
REPARAM_SHAPE = (513, 512)


def kl_case(n, seed=0):
    """|logvar| up to 8; the first and the last element carry the extreme pair (lv1 = 8, lv2 = -8), so that no part of the
    sum - the scalar tail least of all - is small against the rest."""
    g = torch.Generator().manual_seed(n + seed)
    mu1, mu2 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    lv1, lv2 = (torch.rand(n, generator=g) * 16 - 8 for _ in range(2))
    for i in (0, n - 1):
        lv1[i] = 8.0
        lv2[i] = -8.0
    return mu1, lv1, mu2, lv2


# ------------------------------------------------------------------------------------------------ recurrent cells
def _lin(x, w, b):
    return F.linear(x, w, b)


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, dtype=D, mutant=None):
    x, h, w_ih, w_hh, b_ih, b_hh = (t.to(dtype) for t in (x, h, w_ih, w_hh, b_ih, b_hh))
    H = h.shape[-1]
    gi, gh = _lin(x, w_ih, b_ih), _lin(h, w_hh, b_hh)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    if mutant == "n_gate_bias_outside_r":
        n = torch.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] - b_hh[2 * H:]) + b_hh[2 * H:])
    else:
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def _lin_tol(x, w, b, K, dx=None):
    y = _lin(x, w, b)
    t = sum_tol(y, _lin(x.pow(2), w.pow(2), b.pow(2)), K)
    if dx is not None:
        t = t + (dx.pow(2) @ w.pow(2).T).sqrt()
    return y, t


def _sig_tol(s, t_pre):
    return s * (1 - s) * t_pre + 4 * U6


def gru_cell_tol(x, h, w_ih, w_hh, b_ih, b_hh, dh=None):
    x, h, w_ih, w_hh, b_ih, b_hh = (t.to(D) for t in (x, h, w_ih, w_hh, b_ih, b_hh))
    H = h.shape[-1]
    gi, t_gi = _lin_tol(x, w_ih, b_ih, x.shape[-1] + 1)
    gh, t_gh = _lin_tol(h, w_hh, b_hh, H + 1, dh)
    sl = lambda a, k: a[:, k * H:(k + 1) * H]
    pre = lambda k: t_gi[:, k * H:(k + 1) * H] + t_gh[:, k * H:(k + 1) * H] + U6 * (sl(gi, k).abs() + sl(gh, k).abs())
    r = torch.sigmoid(sl(gi, 0) + sl(gh, 0)); t_r = _sig_tol(r, pre(0))
    z = torch.sigmoid(sl(gi, 1) + sl(gh, 1)); t_z = _sig_tol(z, pre(1))
    n = torch.tanh(sl(gi, 2) + r * sl(gh, 2))
    t_pn = sl(t_gi, 2) + sl(gh, 2).abs() * t_r + r * sl(t_gh, 2) + U6 * (sl(gi, 2).abs() + 2 * (r * sl(gh, 2)).abs())
    t_n = (1 - n * n) * t_pn + 4 * U6 * n.abs()
    hn = (1 - z) * n + z * h
    t = (h - n).abs() * t_z + (1 - z) * t_n + U6 * (2 * ((1 - z) * n).abs() + 2 * (z * h).abs() + hn.abs())
    return t if dh is None else t + z * dh


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, dtype=D):
    x, h, c, w_ih, w_hh, b_ih, b_hh = (t.to(dtype) for t in (x, h, c, w_ih, w_hh, b_ih, b_hh))
    H = h.shape[-1]
    g = _lin(x, w_ih, b_ih) + _lin(h, w_hh, b_hh)
    i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
    c2 = f * c + i * gg
    return o * torch.tanh(c2), c2


def lstm_cell_tol(x, h, c, w_ih, w_hh, b_ih, b_hh):
    x, h, c, w_ih, w_hh, b_ih, b_hh = (t.to(D) for t in (x, h, c, w_ih, w_hh, b_ih, b_hh))
    H = h.shape[-1]
    gi, t_gi = _lin_tol(x, w_ih, b_ih, x.shape[-1] + 1)
    gh, t_gh = _lin_tol(h, w_hh, b_hh, H + 1)
    g, t_g = gi + gh, t_gi + t_gh + U6 * (gi.abs() + gh.abs())
    sl = lambda a, k: a[:, k * H:(k + 1) * H]
    i, f, o = (torch.sigmoid(sl(g, k)) for k in (0, 1, 3))
    t_i, t_f, t_o = (_sig_tol(s, sl(t_g, k)) for s, k in ((i, 0), (f, 1), (o, 3)))
    gg = torch.tanh(sl(g, 2)); t_gg = (1 - gg * gg) * sl(t_g, 2) + 4 * U6 * gg.abs()
    c2 = f * c + i * gg
    t_c = c.abs() * t_f + gg.abs() * t_i + i * t_gg + U6 * (2 * (f * c).abs() + 2 * (i * gg).abs() + c2.abs())
    tc = torch.tanh(c2)
    t_h = tc.abs() * t_o + o * ((1 - tc * tc) * t_c + 4 * U6 * tc.abs()) + 2 * U6 * (o * tc).abs()
    return t_h, t_c


def bigru(X, lens, w, dtype=D, mutant=None, want_tol=False):
    """Packed bidirectional GRU (pack_padded_sequence(enforce_sorted=False) -> GRU -> pad_packed_sequence): X [n,Tc,E],
    w = the four tensors of the forward direction, then of the reverse -> hidden [n,Tc,2H], exactly 0 at t >= len.
    The reverse direction of row n starts at t = len[n] - 1.  want_tol: (hidden, its bound) from the float64 run."""
    n, Tc, _ = X.shape
    H = w[1].shape[1]
    lens = torch.as_tensor(lens)
    out = torch.zeros(n, Tc, 2 * H, dtype=dtype)
    tol = torch.zeros(n, Tc, 2 * H, dtype=D)
    for d in range(2):
        ws = w[4 * d:4 * d + 4]
        h = torch.zeros(n, H, dtype=dtype)
        dh = torch.zeros(n, H, dtype=D)
        for k in range(Tc):
            t = Tc - 1 - k if d else k
            valid = (t < lens).view(n, 1)
            if mutant == "reverse_starts_at_Tc-1" and d == 1:
                valid_step = torch.ones(n, 1, dtype=torch.bool)
            else:
                valid_step = valid
            hn = gru_cell(X[:, t], h, *ws, dtype=dtype)
            if want_tol:
                dh = torch.where(valid_step, gru_cell_tol(X[:, t], h, *ws, dh=dh), dh)
                tol[:, t, d * H:(d + 1) * H] = torch.where(valid, dh, torch.zeros((), dtype=D))
            h = torch.where(valid_step, hn, h)
            out[:, t, d * H:(d + 1) * H] = torch.where(valid, h, torch.zeros((), dtype=dtype))
    return (out, tol) if want_tol else out


def rnn_weights(kind, I, H, seed=0, bidirectional=False):
    """Seeded torch-default (uniform +-1/sqrt(H)) weights of a GRU / LSTM layer, in state-dict order."""
    torch.manual_seed(1234 + seed + I + H)
    m = (torch.nn.GRU if kind == "gru" else torch.nn.LSTM)(I, H, batch_first=True, bidirectional=bidirectional)
    return m, [p.detach().clone() for p in m.state_dict().values()]


RNN_STEP_CASES = [(1, 3, 5), (7, 50, 33), (32, 1536, 512), (16, 1024, 512)]      # (N, I, H)
BIGRU_CASES = [(1, 1, 20, 33, [1]), (5, 7, 20, 33, [3, 7, 1, 5, 7]), (4, 5, 512, 512, [2, 5, 1, 4])]   # (n, Tc, E, H, unsorted lens)
