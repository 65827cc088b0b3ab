"""tests/text_ref.py checked on the CPU, over the case grid of tests/test_text_kernels_gpu.py:

  * the fp64 references agree with the oracle (seq2seq_attention, normal_kl_loss, masked_ce, gru_cell, lstm_cell), with
    autograd, and with torch's own GRU / LSTM / packed bidirectional GRU in double, to 1e-12 relative;
  * the fp32 restatement of every operation passes the comparator at every case with err / tol <= 0.5 (a correct fp32
    implementation that sums in another order still fits);
  * every mutant is flagged by the comparator at every case it applies to (the bound is not vacuous).
"""
import pytest
import torch

import acvae_oracle as O
import text_ref as R
from text_ref import D

F32 = torch.float32
WORST = {}


def agree(a, b, what, rel=1e-12):
    a, b = torch.as_tensor(a).detach().to(D), torch.as_tensor(b).detach().to(D)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= rel * scale, (what, float((a - b).abs().max()), scale)


def restated(got, ref, tol, what):
    r = R.compare(got, ref, tol, what, WORST)
    assert r <= 0.5, f"{what}: the fp32 restatement is at {r:.2f} of the bound (> 0.5): the derivation is too tight"


ALL_FWD = [c[:6] for c in R.ATTN_FWD_CASES] + [R.ATTN_STRIDED_FWD + (None,)] + [c[:5] + (None,) for c in R.ATTN_SPLIT_CASES]
N_, Tc_, S_, A_, E_ = R.ATTN_BWD_DECODER
ALL_BWD = [c[:6] for c in R.ATTN_BWD_CASES] + [(N_, 1, S_, A_, E_, None), R.ATTN_BWD_PRIOR + (None,)]


@pytest.mark.parametrize("N,Tq,S,A,E,lens", ALL_FWD, ids=lambda x: str(x))
def test_attention_forward_reference_restatement_mutants(N, Tq, S, A, E, lens):
    c = R.attn_case(N, Tq, S, A, E, lens=lens)
    q, p, enc, v, ln = c["q"], c["p"], c["enc"], c["v"], c["lens"]
    sc, w, ctx = R.attn_fwd(q, p, enc, v, ln)
    # the oracle's Seq2SeqAttention on [h_dec; h_enc] with h2attn = [I | I], bias 0: its projections are q and p themselves
    if A <= 64:
        st = {"a.h2attn.weight": torch.cat([torch.eye(A, dtype=D), torch.eye(A, dtype=D)], 1), "a.h2attn.bias": torch.zeros(A, dtype=D),
              "a.v": v.to(D)}
        for j in range(Tq):
            # the oracle adds W_e enc to W_d h_dec: feed p as the encoder memory for the score, enc for the context
            oc, ow = O.seq2seq_attention(st, "a", q[:, j].to(D), p.to(D), ln)
            agree(w[:, j], ow, "weights vs oracle")
            agree(w[:, j].unsqueeze(1) @ enc.to(D), ctx[:, j:j + 1], "ctx")
    for n in range(N):                                   # masked weights are exactly 0; a len == 0 row is uniform
        if 0 < int(ln[n]) < S:
            assert float(w[n, :, int(ln[n]):].abs().max()) == 0.0
        if int(ln[n]) == 0:
            agree(w[n], torch.full_like(w[n], 1.0 / S), "uniform")
    tw, tc = R.attn_fwd_tol(q, p, enc, v, ln)
    _, w32, c32 = R.attn_fwd(q, p, enc, v, ln, dtype=F32)
    restated(w32, w, tw, "attn_fwd.weights restated")
    restated(c32, ctx, tc, "attn_fwd.ctx restated")
    for m in R.FWD_MUTANTS:
        _, wm, cm = R.attn_fwd(q, p, enc, v, ln, mutant=m)
        assert R.flagged(wm, w, tw) and R.flagged(cm, ctx, tc), m


@pytest.mark.parametrize("N,Tq,S,A,E,lens", ALL_BWD, ids=lambda x: str(x))
def test_attention_backward_reference_restatement_mutants(N, Tq, S, A, E, lens):
    c = R.attn_case(N, Tq, S, A, E, lens=lens)
    dctx, q, p, enc, v, ln = c["dctx"], c["q"], c["p"], c["enc"], c["v"], c["lens"]
    ref = R.attn_bwd(dctx, q, p, enc, v, ln)
    for a, b, what in zip(ref, R.attn_bwd_autograd(dctx, q, p, enc, v, ln), ("dq", "dencproj", "denc", "dv")):
        agree(a, b, what + " closed form vs autograd")
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(t.shape, generator=g) for t in ref[1:]]
    tols = R.attn_bwd_tol(dctx, q, p, enc, v, ln, *base)
    w32 = R.attn_fwd(q, p, enc, v, ln)[1].float()          # the kernel's input: the fp64 weights rounded
    got = R.attn_bwd(dctx, q, p, enc, v, ln, w=w32, dtype=F32)
    want = [ref[0]] + [b.to(D) + r for b, r in zip(base, ref[1:])]
    got = [got[0]] + [b + r for b, r in zip(base, got[1:])]
    for gt, wt, tl, what in zip(got, want, tols, ("dq", "dencproj", "denc", "dv")):
        restated(gt, wt, tl, f"attn_bwd.{what} restated")
    applies = {"chunk_drops_frame_7": S >= 8, "dq_without_last_chunk": True, "dv_from_j0_only": Tq > 1, "assign_not_accumulate": True}
    for m in R.BWD_MUTANTS:
        if not applies[m]:
            continue
        mu = R.attn_bwd(dctx, q, p, enc, v, ln, mutant=m)
        mu = [mu[0]] + [(0 if m == "assign_not_accumulate" else b.to(D)) + r for b, r in zip(base, mu[1:])]
        hit = [R.flagged(a, b, t) for a, b, t in zip(mu, want, tols)]
        if m == "chunk_drops_frame_7":
            assert hit[1] and hit[2], m
        elif m == "dq_without_last_chunk":
            assert hit[0], m
        elif m == "dv_from_j0_only":
            assert hit[3], m
        else:
            assert hit[1] and hit[2] and hit[3], m


@pytest.mark.parametrize("n", R.LOSS_SIZES)
def test_kl_mse_reference_restatement_mutants(n):
    mu1, lv1, mu2, lv2 = R.kl_case(n)
    rows = 3 if n % 3 == 0 else 1
    ref = R.kl_fwd(mu1, lv1, mu2, lv2, rows)
    agree(ref, O.normal_kl_loss(*(t.to(D).view(rows, -1) for t in (mu1, lv1, mu2, lv2))), "kl vs oracle")
    nparts = min(1024, (n + 1023) // 1024)
    tol = R.kl_fwd_tol(mu1, lv1, mu2, lv2, rows, nparts)
    got = torch.stack([R.kl_terms(a, b, c, d, F32).sum() for a, b, c, d in
                       zip(*(t.tensor_split(nparts) for t in (mu1, lv1, mu2, lv2)))]).to(D).sum() / rows     # two-level
    restated(got, ref, tol, "kl_fwd restated")
    if n % 4:
        assert R.flagged(R.kl_fwd(mu1, lv1, mu2, lv2, rows, mutant="kl_drops_scalar_tail"), ref, tol)
    ts = [t.to(D).clone().requires_grad_(True) for t in (mu1, lv1, mu2, lv2)]
    (O.normal_kl_loss(*(t.view(rows, -1) for t in ts)) * 0.7).backward()
    gref = R.kl_bwd(mu1, lv1, mu2, lv2, 0.7, rows)
    for a, t, g32, tl in zip(gref, ts, R.kl_bwd(mu1, lv1, mu2, lv2, 0.7, rows, F32), R.kl_bwd_tol(mu1, lv1, mu2, lv2, 0.7, rows)):
        agree(a, t.grad, "kl grads vs autograd of the oracle")
        restated(g32, a, tl, "kl_bwd restated")
    a, b = mu1 * 3, mu2
    mref = R.mse_fwd(a, b)
    agree(mref, torch.nn.functional.mse_loss(a.to(D), b.to(D)), "mse")
    got = torch.stack([((x - y) ** 2).sum() for x, y in zip(a.tensor_split(nparts), b.tensor_split(nparts))]).to(D).sum() / n
    restated(got, mref, R.mse_fwd_tol(a, b, nparts), "mse_fwd restated")


def test_reparam_reference_restatement():
    rows, E = R.REPARAM_SHAPE
    g = torch.Generator().manual_seed(2)
    mean, logv, eps, dz, dm, dl = (torch.randn(rows, E, generator=g) for _ in range(6))
    logv = logv * 2
    z = R.reparam_fwd(mean, logv, eps)
    restated(R.reparam_fwd(mean, logv, eps, F32), z, R.reparam_fwd_tol(mean, logv, eps), "reparam_fwd restated")
    ml = torch.cat([mean, logv], -1).to(D).requires_grad_(True)
    zz = eps.to(D) * torch.exp(.5 * ml[:, E:]) + ml[:, :E]
    ((zz * dz).sum() + (ml[:, :E] * dm).sum() + (ml[:, E:] * dl).sum()).backward()
    rm, rl = R.reparam_bwd(dz, dm, dl, logv, eps)
    agree(torch.cat([rm, rl], -1), ml.grad, "reparam backward vs autograd")
    for args in ((dz, dm, dl), (None, dm, dl), (dz, None, dl), (dz, dm, None)):
        ref, got, tol = R.reparam_bwd(*args, logv, eps), R.reparam_bwd(*args, logv, eps, F32), R.reparam_bwd_tol(*args, logv, eps)
        for a, b, t in zip(got, ref, tol):
            restated(a, b, t, "reparam_bwd restated")


@pytest.mark.parametrize("V", R.CE_V)
@pytest.mark.parametrize("smooth", R.CE_SMOOTH)
@pytest.mark.parametrize("lens_kind", R.CE_LENS)
def test_ce_reference_restatement_mutants(V, smooth, lens_kind):
    buf, tgb, lens1 = R.ce_case(V, lens_kind)
    N, T = buf.shape[:2]
    x, tg = buf[..., :V], tgb[:, :T]
    rows, mean, tot = R.ce_fwd(x, tg, lens1, smooth)
    olens = torch.full((N,), T) if lens1 is None else torch.clamp(lens1, max=T)
    om = O.generate_length_mask(olens).shape[1]
    xo = x.to(D).clone().requires_grad_(True)
    agree(rows[:, :om], O.masked_ce(xo[:, :om], tg[:, :om], olens, smooth, "none"), "rows vs oracle")
    agree(mean, O.masked_ce(xo[:, :om], tg[:, :om], olens, smooth, "mean"), "mean vs oracle")
    agree(tot, O.masked_ce(xo[:, :om], tg[:, :om], olens, smooth, "sum"), "sum vs oracle")
    if lens1 is not None:
        assert float(rows[~R.ce_mask(lens1, N, T)[0]].abs().sum()) == 0.0
    (O.masked_ce(xo[:, :om], tg[:, :om], olens, smooth, "mean") * 1.7).backward()
    agree(R.ce_bwd(x, tg, lens1, smooth, 1, 1.7), xo.grad, "d logits vs autograd of the oracle", 1e-11)
    lse32 = torch.logsumexp(x, -1)                                   # fp32: stands for the row kernel's output
    d_l = R.lse_tol(x)
    restated(lse32, torch.logsumexp(x.to(D), -1), d_l, "lse restated")
    trows, tmean, tsum = R.ce_fwd_tol(x, tg, lens1, smooth, d_l)
    r32, m32, s32 = R.ce_fwd(x, tg, lens1, smooth, F32, lse=lse32)
    restated(r32, rows, trows, "ce_fwd.rows restated")
    restated(m32, mean, tmean, "ce_fwd.mean restated")
    restated(s32, tot, tsum, "ce_fwd.sum restated")
    gr = torch.linspace(0.5, 1.5, N * T).view(N, T)
    tb = {}
    for red, g in ((0, gr), (1, 1.7), (2, 1.7)):
        ref = R.ce_bwd(x, tg, lens1, smooth, red, g)
        tb[red] = (ref, R.ce_bwd_tol(x, tg, lens1, smooth, red, g, d_l))
        restated(R.ce_bwd(x, tg, lens1, smooth, red, g, F32, lse=lse32), ref, tb[red][1], "ce_bwd restated")
    if smooth != 0.0:
        assert R.flagged(R.ce_fwd(x, tg, lens1, smooth, mutant="smoothing_over_V")[0], rows, trows)
    if lens1 is not None and R.ce_mask(lens1, N, T)[1] != N * T:
        assert R.flagged(R.ce_fwd(x, tg, lens1, smooth, mutant="mean_over_NT")[1], mean, tmean)
        assert R.flagged(R.ce_bwd(x, tg, lens1, smooth, 1, 1.7, mutant="mean_over_NT"), *tb[1])


@pytest.mark.parametrize("N,I,H", R.RNN_STEP_CASES)
def test_rnn_cells_reference_restatement_mutants(N, I, H):
    g = torch.Generator().manual_seed(N + I)
    x, h, c = torch.randn(N, I, generator=g), torch.randn(N, H, generator=g) * .5, torch.randn(N, H, generator=g)
    gru, gw = R.rnn_weights("gru", I, H)
    ref = R.gru_cell(x, h, *gw)
    agree(ref, O.gru_cell(x.to(D), h.to(D), *(t.to(D) for t in gw)), "gru vs oracle")
    with torch.no_grad():
        agree(ref, gru.double()(x.to(D).unsqueeze(1), h.to(D).unsqueeze(0))[1][0], "gru vs torch.nn.GRU")
    tol = R.gru_cell_tol(x, h, *gw)
    restated(R.gru_cell(x, h, *gw, dtype=F32), ref, tol, "gru_step restated")
    assert R.flagged(R.gru_cell(x, h, *gw, mutant="n_gate_bias_outside_r"), ref, tol)
    lstm, lw = R.rnn_weights("lstm", I, H)
    rh, rc = R.lstm_cell(x, h, c, *lw)
    oh, oc = O.lstm_cell(x.to(D), h.to(D), c.to(D), *(t.to(D) for t in lw))
    agree(rh, oh, "lstm h vs oracle"); agree(rc, oc, "lstm c vs oracle")
    with torch.no_grad():
        th, tc = lstm.double()(x.to(D).unsqueeze(1), (h.to(D).unsqueeze(0), c.to(D).unsqueeze(0)))[1]
    agree(rh, th[0], "lstm h vs torch.nn.LSTM"); agree(rc, tc[0], "lstm c vs torch.nn.LSTM")
    t_h, t_c = R.lstm_cell_tol(x, h, c, *lw)
    h32, c32 = R.lstm_cell(x, h, c, *lw, dtype=F32)
    restated(h32, rh, t_h, "lstm_step.h restated"); restated(c32, rc, t_c, "lstm_step.c restated")


@pytest.mark.parametrize("n,Tc,E,H,lens", R.BIGRU_CASES, ids=lambda x: str(x))
def test_bigru_reference_restatement_mutants(n, Tc, E, H, lens):
    X = torch.randn(n, Tc, E, generator=torch.Generator().manual_seed(n + Tc))
    gru, w = R.rnn_weights("gru", E, H, bidirectional=True)
    ref, tol = R.bigru(X, lens, w, want_tol=True)
    with torch.no_grad():
        pk = torch.nn.utils.rnn.pack_padded_sequence(X.to(D), torch.tensor(lens), batch_first=True, enforce_sorted=False)
        tref, _ = torch.nn.utils.rnn.pad_packed_sequence(gru.double()(pk)[0], batch_first=True, total_length=Tc)
    agree(ref, tref, "bigru vs torch's packed bidirectional GRU")
    for i, l in enumerate(lens):
        assert float(ref[i, l:].abs().sum()) == 0.0 and float(tol[i, l:].abs().sum()) == 0.0
    restated(R.bigru(X, lens, w, dtype=F32), ref, tol, "bigru_seq restated")
    if min(lens) < Tc:
        assert R.flagged(R.bigru(X, lens, w, mutant="reverse_starts_at_Tc-1"), ref, tol)


def test_zz_worst_restated_ratio_per_tensor():
    """Runs last in this file: the worst err / tol of the fp32 restatement per tensor (printed with -s), all <= 0.5."""
    if not WORST:
        return
    for k in sorted(WORST):
        print(f"{k}: {WORST[k]:.3f}")
    assert max(WORST.values()) <= 0.5
