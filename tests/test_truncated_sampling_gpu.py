"""GPU: top-k / nucleus sampling - acvae_sample_next_word_truncated alone (strided logits, noise and outputs with sentinels
in the gaps, as test_sample_next_word_vs_fp64 has them) against the float64 definition of tests/truncate_util.py, and the
``top_k`` / ``top_p`` keywords of Hybrid_VAEModel end to end on a small model."""
import functools
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import truncate_util as TU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from test_decode_kernels_gpu import lse_bound, sample_scores_fp64, st
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
GUMBEL, MULTINOMIAL = TU.GUMBEL, TU.MULTINOMIAL
METHODS = (GUMBEL, MULTINOMIAL)
TEMPS = (0.5, 1.0, 2.0)
REG_LIMIT = 8192                         # TRUNC_REG_V of csrc/losses.hip: above it the kernel re-reads the row per probe


def make_noise(rng, shape, method):
    if method == GUMBEL:
        u = rng.random(shape, dtype=np.float32)
        return (-np.log(-np.log(u + 1e-20) + 1e-20)).astype(np.float32)
    return np.maximum(rng.exponential(1.0, shape), 1e-30).astype(np.float32)


def winning(method):
    """A noise value that wins any race of these tests, and one that loses it."""
    return (60.0, -60.0) if method == GUMBEL else (1e-30, 1e30)


class Strided:
    """rows / noise [N, T, V] laid out with gaps (ld_t > V, ld_n > T * ld_t, other strides for the noise and the outputs);
    run() launches one entry point and returns w, logprob, kept at the rows' places after checking that nothing between
    them was written."""

    def __init__(self, rows, noise):
        self.N, self.T, self.V = N, T, V = rows.shape
        self.ld_t, self.nz_st, self.o_st = V + 5, V + 3, 2
        self.ld_n, self.nz_sn, self.o_sn = T * self.ld_t + 1, T * self.nz_st + 9, T * self.o_st + 1
        host = np.full(N * self.ld_n, 77.0, np.float32)              # gaps: larger than any logit of a random row
        nz = np.ones(N * self.nz_sn, np.float32)
        for n in range(N):
            for t in range(T):
                host[n * self.ld_n + t * self.ld_t: n * self.ld_n + t * self.ld_t + V] = rows[n, t]
                nz[n * self.nz_sn + t * self.nz_st: n * self.nz_sn + t * self.nz_st + V] = noise[n, t]
        self.x, self.z = torch.from_numpy(host).cuda(), torch.from_numpy(nz).cuda()
        self.sel = np.arange(N)[:, None] * self.o_sn + np.arange(T)[None, :] * self.o_st

    def run(self, method, temp, k=0, p=1.0, old=False):
        n_out = self.N * self.o_sn
        w = torch.full((n_out,), -7, dtype=torch.long, device="cuda")
        lp = torch.full((n_out,), 9.0, device="cuda")
        kept = torch.full((n_out,), -3, dtype=torch.int32, device="cuda")
        head = (self.x, self.ld_n, self.ld_t, self.z, self.nz_sn, self.nz_st, method, temp, w, lp, self.o_sn, self.o_st,
                self.N, self.T, self.V)
        if old:
            _lib.call("acvae_sample_next_word", *head, st())
        else:
            _lib.call("acvae_sample_next_word_truncated", *head, k, p, kept, st())
        w, lp, kept = w.cpu().numpy(), lp.cpu().numpy(), kept.cpu().numpy()
        gaps = np.setdiff1d(np.arange(n_out), self.sel.reshape(-1))
        assert (w[gaps] == -7).all() and (lp[gaps] == 9.0).all() and (kept[gaps] == -3).all()
        return w[self.sel], lp[self.sel], kept[self.sel]


# ------------------------------------------------------------------------------------------------ 1. off = the old kernel
@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1024, 1025, 5000, 5001, 5120, 5121, REG_LIMIT, REG_LIMIT + 1])
def test_truncation_off_is_the_untruncated_kernel_bit_for_bit(V):
    """top_k = 0, top_p = 1.0: the words and log-probabilities of acvae_sample_next_word on the same inputs to the last
    bit, kept = V, the gaps untouched - at every V where the kernel changes its path (registers per lane 4 / 20 / 32, the
    re-reading form above REG_LIMIT) and around the workgroup's width."""
    N, T = 4, 3
    rng = np.random.default_rng(V)
    rows = (rng.standard_normal((N, T, V)) * 2).astype(np.float32)
    for method in METHODS:
        s = Strided(rows, make_noise(rng, (N, T, V), method))
        for temp in TEMPS:
            w0, lp0, _ = s.run(method, temp, old=True)
            w, lp, kept = s.run(method, temp, 0, 1.0)
            assert np.array_equal(w, w0), (method, temp)
            assert np.array_equal(lp.view(np.int32), lp0.view(np.int32)), (method, temp)
            assert (kept == V).all()
            assert ((w >= 0) & (w < V)).all()


# ------------------------------------------------------------------------------------------------ 2. top_k = 1 is greedy
@pytest.mark.parametrize("V", [257, 5000])
def test_top_k_1_is_greedy_whatever_the_noise(V):
    """The noise lets every other word win an untruncated race (the maximum holds the losing value, the rest winning ones);
    duplicate maxima in one thread's stride (c, c + 256) and across wavefronts (c, c + 64): the first maximum is drawn and
    kept = 1, with top_k = 1 and with top_p = 1e-6 alike."""
    N, T = 6, 3
    rng = np.random.default_rng(100 + V)
    rows = (rng.standard_normal((N, T, V)) * 2).astype(np.float32)
    want = np.zeros((N, T), np.int64)
    for n in range(N):
        c = int(rng.integers(0, V - 256))
        for t, off in ((0, 256), (1, 64)):
            rows[n, t, c] = rows[n, t, c + off] = rows[n, t].max() + 1.0
        want[n] = rows[n].argmax(-1)
        assert want[n, 0] == c and want[n, 1] == c
    for method in METHODS:
        win, lose = winning(method)
        noise = np.full((N, T, V), win, np.float32) * (1 + 0.5 * rng.random((N, T, V), dtype=np.float32))
        np.put_along_axis(noise, want[..., None], lose, -1)
        s = Strided(rows, noise)
        for temp in (1.0, 2.0):
            w_full, _, _ = s.run(method, temp, old=True)
            assert (w_full != want).all()                              # untruncated, any other word wins
            for k, p in ((1, 1.0), (0, 1e-6), (1, 1e-6)):
                w, lp, kept = s.run(method, temp, k, p)
                assert np.array_equal(w, want), (method, temp, k, p)
                assert (kept == 1).all()


# ------------------------------------------------------------------------------------------------ 3, 4, 6. random rows
CUTS = ((0, 0.9), (40, 1.0), (7, 0.5), (0, 0.3), (40, 0.95))


@functools.lru_cache(maxsize=None)
def cut_case(V):
    """16 x 6 rows of 2 randn (even n) and 4 randn (odd n), every method, temperature and (k, p): the kernel's outputs and
    the float64 reference (order, mass in front of every rank), computed once and shared by the tests below."""
    N, T = 16, 6
    rng = np.random.default_rng(7 * V)
    rows = rng.standard_normal((N, T, V))
    rows[0::2] *= 2
    rows[1::2] *= 4
    rows = rows.astype(np.float32)
    flat = rows.reshape(N * T, V)
    order = [TU.stable_order(r) for r in flat]
    out = {"rows": rows, "order": order, "runs": {}, "before": {}, "noise": {}}
    for method in METHODS:
        noise = make_noise(rng, (N, T, V), method)
        out["noise"][method] = noise
        s = Strided(rows, noise)
        out[("strided", method)] = s
        for temp in TEMPS:
            out["before"][(method, temp)] = [TU.mass_before(r, method, temp, o)[1] for r, o in zip(flat, order)]
            for k, p in CUTS:
                out["runs"][(method, temp, k, p)] = s.run(method, temp, k, p)
    return out


@pytest.mark.parametrize("V", [257, 5000, 5001])
def test_kept_count_lies_in_the_admissible_interval(V):
    """Every row's kept count against float64: between the counts of the cuts at p - tol and p + tol (tol:
    truncate_util.mass_tol, the fp32 error of the kernel's mass ratio), intersected with k.  No row is skipped."""
    c = cut_case(V)
    tol = TU.mass_tol(V)
    for (method, temp, k, p), (_, _, kept) in c["runs"].items():
        kept = kept.reshape(-1)
        width = 0
        for r, before in enumerate(c["before"][(method, temp)]):
            q = float(np.float32(p))
            lo = TU.kept_count(before, k, q - tol if q < 1.0 else 1.0)
            hi = TU.kept_count(before, k, min(q + tol, np.nextafter(1.0, 0.0)) if q < 1.0 else 1.0)
            width = max(width, hi - lo)
            assert lo <= kept[r] <= hi, (method, temp, k, p, r, int(kept[r]), lo, hi)
            if k > 0:
                assert kept[r] <= k
        print(f"V={V} method={method} temp={temp} k={k} p={p}: kept {kept.min()}..{kept.max()}, widest interval {width + 1}")
        assert width <= 3                                             # the interval is a few words wide at most


@pytest.mark.parametrize("V", [257, 5000, 5001])
def test_winner_is_the_fp64_argmax_over_the_kept_words(V):
    """Given the kernel's own kept count the kept set is the order's prefix; w is the float64 argmax of the score over it
    (first index on ties).  Rows whose float64 top-2 relative gap inside the set is below 1e-5 are within the fp32 rounding of
    the score: skipped and counted, at most 5 % of a case's rows.  logprob is log_softmax(x)[w] of the full row within
    lse_bound."""
    c = cut_case(V)
    rows, order = c["rows"], c["order"]
    R = len(order)
    for (method, temp, k, p), (w, lpo, kept) in c["runs"].items():
        lp, sc = sample_scores_fp64(rows, c["noise"][method], method, temp)
        lp, sc = lp.reshape(R, V), sc.reshape(R, V)
        w, lpo, kept = w.reshape(-1), lpo.reshape(-1).astype(np.float64), kept.reshape(-1)
        skipped = 0
        for r in range(R):
            assert 1 <= kept[r] <= V
            inside = np.full(V, -np.inf)
            idx = order[r][:kept[r]]
            inside[idx] = sc[r, idx]
            top2 = -np.sort(-inside[idx])[:2]
            if top2.size == 2 and (top2[0] - top2[1]) / abs(top2[0]) < 1e-5:
                skipped += 1
                continue
            assert w[r] == int(np.argmax(inside)), (method, temp, k, p, r, int(w[r]), int(np.argmax(inside)))
        print(f"V={V} method={method} temp={temp} k={k} p={p}: {skipped}/{R} rows within rounding of a tie, skipped")
        assert skipped <= R // 20
        lp_w = lp[np.arange(R), w]
        assert (np.abs(lpo - lp_w) <= lse_bound(V, lp_w)).all(), float(np.abs(lpo - lp_w).max())


def test_a_second_run_is_bit_equal():
    c = cut_case(5000)
    for method in METHODS:
        s = c[("strided", method)]
        for temp in TEMPS:
            for k, p in CUTS:
                w0, lp0, kept0 = c["runs"][(method, temp, k, p)]
                w, lp, kept = s.run(method, temp, k, p)
                assert np.array_equal(w, w0) and np.array_equal(kept, kept0)
                assert np.array_equal(lp.view(np.int32), lp0.view(np.int32))


# ------------------------------------------------------------------------------------------------ 5. ties at the cut
@pytest.mark.parametrize("V", [600, 5000])
def test_ties_at_the_cut_keep_the_lower_index(V):
    """(a) top_k = 3 over a row whose ranks 2 and 3 hold bit-equal logits, in one thread's stride (c, c + 256) and across
    wavefronts (c, c + 64): the lower index is kept; the higher one holds the winning noise and is not drawn.  (b) four
    equal logits, the rest at -100, top_p = 0.6: kept = 3, the three lowest indices, the fourth holds the winning noise."""
    N = 8
    rng = np.random.default_rng(300 + V)
    for method in METHODS:
        win, lose = winning(method)
        rows = (rng.standard_normal((N, 3, V)) * 2).astype(np.float32)
        noise = make_noise(rng, (N, 3, V), method)
        kept_sets = {}
        for n in range(N):
            c = int(rng.integers(0, V - 256))
            for t, off in ((0, 256), (1, 64)):
                free = np.setdiff1d(np.arange(V), [c, c + off])
                a, b = rng.choice(free, 2, replace=False)
                top = float(rows[n, t].max())
                rows[n, t, a], rows[n, t, b] = top + 3.0, top + 2.0
                rows[n, t, c] = rows[n, t, c + off] = top + 1.0
                noise[n, t, c + off] = win
                kept_sets[(n, t)] = [a, b, c]
            four = np.sort(rng.choice(V, 4, replace=False))
            rows[n, 2] = -100.0
            rows[n, 2, four] = 1.25
            noise[n, 2, four[3]] = win
            kept_sets[(n, 2)] = list(four[:3])
        s = Strided(rows, noise)
        for temp in TEMPS:
            _, sc = sample_scores_fp64(rows, noise, method, temp)
            for k, p in ((3, 1.0), (0, 0.6)):
                w, _, kept = s.run(method, temp, k, p)
                for (n, t), ks in kept_sets.items():
                    if (t == 2) != (k == 0):
                        continue
                    assert kept[n, t] == 3, (method, temp, n, t, int(kept[n, t]))
                    want = ks[int(np.argmax(sc[n, t, ks]))]
                    assert w[n, t] == want, (method, temp, n, t, int(w[n, t]), ks)


# ------------------------------------------------------------------------------------------------ 7, 8. the model
MV, ME, ML = 257, 64, 8


@pytest.fixture(scope="module")
def small():
    state = O.closed_form_state(O.state_shapes(MV, ME, ME, None, ME, 512))
    feats, caps, feat_lens, cap_lens = O.synthetic_batch(3, 64, MV, 6, seed=5, ragged=False)
    model = build_model(MV, ME, state)
    model.eval()
    return model, feats.cuda(), feat_lens, caps, cap_lens


def host_noise(method, N, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(ML, N, ME, generator=g)
    if method == "gumbel":
        z = -torch.log(-torch.log(torch.rand(ML, N, MV, generator=g) + 1e-20) + 1e-20)
    else:
        z = torch.empty(ML, N, MV).exponential_(1, generator=g)
    return eps, z


def infer(model, feats, lens, noise=None, **kw):
    if noise is not None:
        model.noise = dict(eps_p=noise[0], sample_noise=noise[1])
    with torch.no_grad():
        return model(feats, lens.copy(), max_length=ML, **kw)


def unfinished(seqs, t, end_idx):
    return ~(seqs[:, :t] == end_idx).any(1)


def check_steps_against_the_definition(model, out, method, temp, k, p, noise=None):
    """Per step t and row not yet finished: kept in the admissible interval of logits[:, t], the word inside the kept prefix;
    with the step's noise given, the stand-alone kernel on (logits[:, t], noise[t]) reproduces word and kept exactly."""
    code = GUMBEL if method == "gumbel" else MULTINOMIAL
    logits, seqs, kept = out["logits"].cpu().numpy(), out["seqs"].cpu().numpy(), out["kept"].cpu().numpy()
    assert out["kept"].dtype == torch.int32 and kept.shape == seqs.shape
    N = seqs.shape[0]
    checked = 0
    for t in range(ML):
        live = unfinished(seqs, t, model.end_idx)
        if noise is not None:
            w = torch.empty(N, dtype=torch.long, device="cuda")
            kk = torch.empty(N, dtype=torch.int32, device="cuda")
            x = out["logits"][:, t].contiguous()
            _lib.call("acvae_sample_next_word_truncated", x, MV, 0, noise[1][t].contiguous().cuda(), MV, 0, code, temp, w,
                      None, 1, 0, N, 1, MV, k, p, kk, st())
            assert np.array_equal(w.cpu().numpy()[live], seqs[live, t]), t
            assert np.array_equal(kk.cpu().numpy()[live], kept[live, t]), t
        for n in np.flatnonzero(live):
            lo, hi, order = TU.admissible(logits[n, t], code, temp, k, p)
            assert lo <= kept[n, t] <= hi, (t, n, int(kept[n, t]), lo, hi)
            rank = int(np.flatnonzero(order == seqs[n, t])[0])
            assert rank < kept[n, t], (t, n, rank, int(kept[n, t]))
            checked += 1
    assert checked >= N                                                # (step 0 at least: every row is live there)


def test_model_top_k_1_is_greedy(small):
    model, feats, lens, _, _ = small
    noise = host_noise("sample", 3, 1)
    greedy = infer(model, feats, lens, (noise[0], None), method="greedy")
    for method in ("sample", "gumbel"):
        out = infer(model, feats, lens, host_noise(method, 3, 1), method=method, top_k=1, temp=1.3)
        assert torch.equal(out["seqs"], greedy["seqs"]), method
        assert int(out["kept"].min()) == 1 and int(out["kept"].max()) == 1
    assert "kept" not in greedy


def test_model_truncation_off_is_plain_sampling(small):
    """top_k = 0, top_p = 1.0 under the same torch seed: the random stream, the words, their log-probabilities and the
    logits of plain method="sample" bit for bit, and no "kept" key."""
    model, feats, lens, _, _ = small
    for method, rng in (("sample", "host"), ("gumbel", "host"), ("sample", "device")):
        torch.manual_seed(11)
        a = infer(model, feats, lens, method=method, temp=0.9, rng=rng)
        after_a = torch.rand(1)
        torch.manual_seed(11)
        b = infer(model, feats, lens, method=method, temp=0.9, rng=rng, top_k=0, top_p=1.0)
        after_b = torch.rand(1)
        for key in ("seqs", "sampled_logprobs", "logits"):
            assert torch.equal(a[key], b[key]), (method, rng, key)
        assert "kept" not in a and "kept" not in b
        # and truncation consumes the same draws: the generator stands where it stood
        torch.manual_seed(11)
        infer(model, feats, lens, method=method, temp=0.9, rng=rng, top_k=10, top_p=0.8)
        assert torch.equal(after_a, after_b) and torch.equal(torch.rand(1), after_a)


@pytest.mark.parametrize("method", ["sample", "gumbel"])
def test_model_steps_equal_the_stand_alone_kernel(small, method):
    model, feats, lens, _, _ = small
    noise = host_noise(method, 3, 2)
    out = infer(model, feats, lens, noise, method=method, top_k=10, top_p=0.8, temp=1.5)
    check_steps_against_the_definition(model, out, method, 1.5, 10, 0.8, noise)
    assert int(out["kept"].max()) <= 10
    slp = torch.log_softmax(out["logits"].double(), -1).gather(2, out["seqs"].unsqueeze(-1)).squeeze(-1)
    live = torch.from_numpy(np.stack([unfinished(out["seqs"].cpu().numpy(), t, model.end_idx) for t in range(ML)], 1))
    err = (out["sampled_logprobs"].double() - slp).abs().cpu()[live]
    assert float(err.max()) < 1e-5                                     # the FULL distribution's log-probability


@pytest.mark.parametrize("method", ["sample", "gumbel"])
def test_model_device_rng_words_lie_in_the_admissible_sets(small, method):
    model, feats, lens, _, _ = small
    torch.manual_seed(4)
    out = infer(model, feats, lens, method=method, top_k=10, top_p=0.8, temp=1.5, rng="device")
    check_steps_against_the_definition(model, out, method, 1.5, 10, 0.8)
    model.sample_rng = "device"                                        # the model-wide switch, through the shared-encoder rollout
    try:
        torch.manual_seed(4)
        with torch.no_grad():
            rep = model.rollout_shared_encoder(feats, lens.copy(), 2, method=method, top_p=0.5, max_length=ML)
    finally:
        del model.sample_rng
    assert rep["seqs"].shape == (6, ML) and rep["kept"].shape == (6, ML)
    check_steps_against_the_definition(model, rep, method, 1.0, 0, 0.5)


def test_evaluate_returns_five_sampled_captions_per_clip(small):
    model = small[0]
    voc = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(MV - 4)]:
        voc.add_word(w)
    g = torch.Generator().manual_seed(5)
    items = [(f"clip{i}", torch.randn(64, 64, generator=g)) for i in range(2)]
    torch.manual_seed(9)
    got = EV.evaluate(model, items, voc, method="sample", beam_size=5, top_p=0.9, rng="device", max_length=ML)
    assert [p["filename"] for p in got["predictions"]] == ["clip0", "clip1"]
    assert all(len(p["captions"]) == 5 for p in got["predictions"])
    with pytest.raises(ValueError, match="top_p"):
        EV.evaluate(model, items, voc, method="beam", beam_size=3, top_p=0.9, max_length=ML)


def test_training_forward_feeds_its_truncated_words(small):
    """ss_ratio = 0.5, method="sample", top_k = 5: every word is one of its step's five most probable, kept = 5, and the
    fed words are the forward's seqs - a second, untruncated forward on the same coins and noise whose sampling noise lets
    exactly those words win (so that it feeds them by construction) has the same logits to the last bit."""
    model, feats, lens, caps, cap_lens = small
    N, Tc = caps.shape[0], int(max(cap_lens)) - 1
    g = torch.Generator().manual_seed(3)
    base = dict(eps_q=torch.randn(N, Tc, ME, generator=g), eps_p=torch.randn(Tc, N, ME, generator=g))
    z = torch.empty(Tc, N, MV).exponential_(1, generator=g)

    def train_fwd(sample_noise, **kw):
        model.noise = dict(base, sample_noise=sample_noise)
        random.seed(6)
        with torch.no_grad():
            return model(feats, lens.copy(), caps, cap_lens, ss_ratio=0.5, dis_ratio=0, method="sample", **kw)

    model.train()
    model.encoder.eval()                  # no dropout draws, running statistics: the two forwards see the same memory
    try:
        torch.manual_seed(8)
        out = train_fwd(z, top_k=5)
        random.seed(6)
        coins = [random.random() < 0.5 for _ in range(Tc)]
        assert not all(coins) and Tc >= 3                             # some step feeds a sampled word
        seqs = out["seqs"]
        assert out["kept"].shape == (N, Tc) and bool((out["kept"] == 5).all())
        top5 = out["logits"].topk(5, -1).indices
        assert bool((top5 == seqs.unsqueeze(-1)).any(-1).all())
        forced = torch.full((Tc, N, MV), 1e30)
        forced.scatter_(2, seqs.cpu().t().unsqueeze(-1), 1e-30)
        torch.manual_seed(8)
        again = train_fwd(forced)
        assert torch.equal(again["seqs"], seqs) and "kept" not in again
        assert torch.equal(again["logits"], out["logits"])
    finally:
        model.eval()


def test_training_forward_with_truncation_backpropagates(small):
    """The 4-input forward under autograd with top_k on: "kept" rides beside the other outputs and takes no gradient; the
    backward runs and reaches the decoder and the encoder."""
    model, feats, lens, caps, cap_lens = small
    model.train()
    try:
        torch.manual_seed(12); random.seed(12)
        out = model(feats, lens.copy(), caps, cap_lens, ss_ratio=0.5, dis_ratio=0, method="sample", top_k=5, rng="device")
        assert not out["kept"].requires_grad and bool((out["kept"] == 5).all())
        model.zero_grad(set_to_none=True)
        out["logits"].square().mean().backward()
        torch.cuda.synchronize()
        for p in (model.decoder.classifier.weight, model.encoder.bn0.weight):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()


def test_refusals_on_the_device_model(small):
    """Every refusal of the keywords is raised in front of the first launch: nothing is queued on the stream."""
    model, feats, lens, caps, cap_lens = small
    calls = []
    real = _lib.call
    _lib.call = lambda *a: (calls.append(a[0]), real(*a))[1]
    try:
        for kw in (dict(method="greedy", top_k=3), dict(method="beam", top_p=0.9), dict(method="dbs", top_k=2),
                   dict(method="sample", top_k=-1), dict(method="sample", top_p=0.0), dict(method="sample", top_p=1.5),
                   dict(method="sample", top_p=float("nan")), dict(top_p=0.5)):
            with pytest.raises(ValueError, match="top_k|top_p"):
                model(feats, lens.copy(), max_length=ML, **kw)
        with pytest.raises(ValueError, match="top_k"):
            model(feats, lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, top_k=4)
        model.train()
        with pytest.raises(ValueError, match="differentiable rollout"):
            model(feats, lens.copy(), max_length=ML, method="sample", top_k=4)
        with pytest.raises(ValueError, match="differentiable rollout"):
            model.rollout_shared_encoder(feats, lens.copy(), 2, max_length=ML, method="sample", top_p=0.9)
    finally:
        _lib.call = real
        model.eval()
    assert calls == []
    # the C entry refuses the same before it launches anything
    buf = torch.zeros(4096, device="cuda")
    w = torch.zeros(8, dtype=torch.long, device="cuda")
    for k, p in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_sample_next_word_truncated", buf, 40, 0, buf, 40, 0, 2, 1.0, w, None, 1, 0, 4, 1, 40, k, p, None,
                      st())
    torch.cuda.synchronize()
