"""GPU: the selection kernels of inference (csrc/losses.hip) alone, at the sizes where their thread strides matter, against
exact references.  topk_flat_kernel runs 1024 threads and row_stats_kernel / sample_rows_kernel / dbs_scores_kernel 256:
below those widths no thread holds more than one element, so the in-stride comparisons, the `taken` exclusion and the
lower-index tie-breaks across strides and wavefronts only run at the production sizes (n = beam x V up to 16 x 5000,
V = 5000).  Exact ties are planted where each of those code paths decides."""
import numpy as np
import pytest
import torch

from acvae_amd import _lib
from parity_util import close

pytestmark = pytest.mark.gpu
GUMBEL, MULTINOMIAL = 1, 2
EPS32 = 2.0 ** -24                       # unit roundoff of fp32


def st():
    return _lib.current_stream()


# ------------------------------------------------------------------------------------------------ flat top-k
def topk_ref(x, k):
    """torch.topk(sorted=True) order with ties to the lower index: a stable sort on (-x, index)."""
    order = np.lexsort((np.arange(x.size), -x.astype(np.float64)))
    return order[:k]


def plant_ties(x, rng):
    """Exact ties among the largest values, each where a different comparison decides: two in one thread's stride (i,
    i + 1024), two in one wavefront (j, j + 1), three across wavefronts (a, a + 64, a + 320) - the last set straddles
    k = 5, so one of its members is in and two are out."""
    n = x.size
    if n < 4:
        return
    i = int(rng.integers(0, max(1, n - 1024))) if n > 1024 else 0
    j = int(rng.integers(0, n - 1))
    a = int(rng.integers(0, max(1, n - 320))) if n > 320 else 0
    for pos, v in (((i, i + 1024), 40.0), ((j, j + 1), 30.0), ((a, a + 64, a + 320), 20.0)):
        for p in pos:
            if p < n:
                x[p] = v


def make_group(n, V, rng, kind):
    x = rng.standard_normal(n).astype(np.float32)
    if kind >= 1:
        plant_ties(x, rng)
    if kind == 2 and n >= 2 * V:                   # DBS: finished beams (whole rows) lowered by 1000
        x[V:2 * V] -= 1000.0
    if kind == 3:                                  # -inf entries, most of a small group
        m = rng.random(n) < (0.9 if n <= 16 else 0.2)
        x[m] = -np.inf
    return x


TOPK_N = [1, 2, 16, 1023, 1024, 1025, 5000, 15000, 80000]


@pytest.mark.parametrize("n", TOPK_N)
def test_topk_flat_batched_vs_stable_sort(n):
    """Every (k, groups, stride) at one n: vals bit-equal to the inputs, idx / row / col exact; padding beyond n in a group's
    stride (+inf or 1e30) never selected; row = g * row_base + idx / V with row_base != k."""
    rng = np.random.default_rng(n)
    V = 5000 if n >= 5000 else max(1, n // 3 + 1)
    for groups in (1, 3, 52):
        for pad, fill in ((0, None), (37, np.inf), (1024, 1e30)):
            stride = n + pad
            host = np.full((groups, stride), np.float32(fill if fill is not None else 0.0), np.float32)
            for g in range(groups):
                host[g, :n] = make_group(n, V, rng, g % 4)
            x = torch.from_numpy(host.reshape(-1)).cuda()
            refs = [topk_ref(host[g, :n], 16) for g in range(groups)]
            for k in (1, 3, 5, 16):
                if k > n:
                    continue
                row_base = k + 3
                vals = torch.empty(groups * k, device="cuda")
                idx, row, col = (torch.empty(groups * k, dtype=torch.long, device="cuda") for _ in range(3))
                _lib.call("acvae_topk_flat_batched", x, n, stride, k, V, vals, idx, row, col, groups, row_base, st())
                vals, idx, row, col = (t.cpu().numpy().reshape(groups, k) for t in (vals, idx, row, col))
                for g in range(groups):
                    want = refs[g][:k]
                    what = f"n={n} k={k} groups={groups} stride={stride} group {g}"
                    assert np.array_equal(idx[g], want), (what, idx[g], want)
                    assert np.array_equal(vals[g].view(np.int32), host[g, want].view(np.int32)), what
                    assert np.array_equal(row[g], g * row_base + want // V), what
                    assert np.array_equal(col[g], want % V), what


@pytest.mark.parametrize("n", TOPK_N)
def test_topk_flat_vs_stable_sort(n):
    """The one-group entry point (beam bookkeeping of the step API): row = idx / V, col = idx % V."""
    rng = np.random.default_rng(1000 + n)
    V = 5000 if n >= 5000 else max(1, n // 2 + 1)
    for kind in range(4):
        host = make_group(n, V, rng, kind)
        x = torch.from_numpy(host).cuda()
        ref = topk_ref(host, 16)
        for k in (1, 3, 5, 16):
            if k > n:
                continue
            vals = torch.empty(k, device="cuda")
            idx, row, col = (torch.empty(k, dtype=torch.long, device="cuda") for _ in range(3))
            _lib.call("acvae_topk_flat", x, n, k, V, vals, idx, row, col, st())
            got = idx.cpu().numpy()
            assert np.array_equal(got, ref[:k]), (n, k, kind, got, ref[:k])
            assert np.array_equal(vals.cpu().numpy().view(np.int32), host[ref[:k]].view(np.int32))
            assert np.array_equal(row.cpu().numpy(), ref[:k] // V) and np.array_equal(col.cpu().numpy(), ref[:k] % V)


def test_topk_refusals():
    x = torch.zeros(4096, device="cuda")
    vals = torch.empty(64, device="cuda")
    idx, row, col = (torch.empty(64, dtype=torch.long, device="cuda") for _ in range(3))
    for n, k in ((100, 0), (100, 17), (8, 9)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_topk_flat", x, n, k, 50, vals, idx, row, col, st())
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_topk_flat_batched", x, n, n, k, 50, vals, idx, row, col, 2, k, st())
    with pytest.raises(RuntimeError, match="EINVAL"):          # groups would overlap
        _lib.call("acvae_topk_flat_batched", x, 100, 99, 3, 50, vals, idx, row, col, 2, 3, st())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ row statistics
def lse_bound(V, lse):
    """Error bound of the kernel's lse = m + log(s), s = sum_c expf(x_c - m) in fp32 (m, the row's max, is exact): each
    expf is within 2 ulp (2 * 2^-23 relative); a thread adds ceil(V / 256) of them in sequence and the block tree adds 8
    levels, each addition of positive terms within 2^-24 relative - so |ds| / s <= (4 + ceil(V / 256) + 8) * 2^-24 + ..., and
    logf and the final addition add one ulp each of their results.  Doubled for headroom."""
    rel_s = (4 + -(-V // 256) + 8) * EPS32
    return 2.0 * (rel_s + 2 * EPS32 * np.maximum(np.abs(lse), 1.0))


def fp64_stats(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    ls = np.log(np.exp(x - m).sum(-1))
    return m[..., 0] + ls, -ls, np.argmax(x, -1)


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 4999, 5000, 5001])
def test_row_logsoftmax_argmax_grid_vs_fp64(V):
    """An N x T grid with ld_t > V and padded output strides; duplicate maxima planted in one thread's stride (c, c + 256)
    and in different wavefronts (c, c + 64): the first index wins, as torch.argmax gives."""
    N, T = 3, 5
    ld_t, o_st = V + 7, 3
    ld_n, o_sn = T * ld_t + 11, T * o_st + 2
    rng = np.random.default_rng(V)
    host = np.full(N * ld_n, 123.0, np.float32)                # padding: larger than any logit
    rows = (rng.standard_normal((N, T, V)) * 3).astype(np.float32)
    for n in range(N):
        for t in range(T):
            r = rows[n, t]
            kind = (n * T + t) % 3
            c = int(rng.integers(0, V))
            if kind == 1 and c + 256 < V:
                r[c] = r[c + 256] = r.max() + 1.0
            elif kind == 2 and c + 64 < V:
                r[c] = r[c + 64] = r.max() + 1.0
            host[n * ld_n + t * ld_t: n * ld_n + t * ld_t + V] = r
    x = torch.from_numpy(host).cuda()
    olen = N * o_sn
    am = torch.full((olen,), -5, dtype=torch.long, device="cuda")
    mlp, lse = torch.full((olen,), 7.0, device="cuda"), torch.full((olen,), 7.0, device="cuda")
    _lib.call("acvae_row_logsoftmax_argmax", x, ld_n, ld_t, am, mlp, lse, o_sn, o_st, N, T, V, st())
    am, mlp, lse = am.cpu().numpy(), mlp.cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    want_lse, want_mlp, want_am = fp64_stats(rows)
    sel = (np.arange(N)[:, None] * o_sn + np.arange(T)[None, :] * o_st).reshape(-1)
    assert np.array_equal(am[sel], want_am.reshape(-1)), (am[sel], want_am.reshape(-1))
    assert np.array_equal(am[sel], torch.argmax(torch.from_numpy(rows), -1).reshape(-1).numpy())
    e_lse = np.abs(lse[sel] - want_lse.reshape(-1))
    e_mlp = np.abs(mlp[sel] - want_mlp.reshape(-1))
    b = lse_bound(V, want_lse.reshape(-1))
    print(f"V={V}: |lse err| max {e_lse.max():.2e}, |max logprob err| max {e_mlp.max():.2e} (bound {b.min():.2e})")
    assert (e_lse <= b).all() and (e_mlp <= b).all()
    untouched = np.setdiff1d(np.arange(olen), sel)            # nothing written between the strided outputs
    assert (am[untouched] == -5).all() and (lse[untouched] == 7.0).all() and (mlp[untouched] == 7.0).all()


# ------------------------------------------------------------------------------------------------ sampling
def sample_scores_fp64(rows, noise, method, temp):
    lp = torch.log_softmax(torch.from_numpy(rows).double(), -1).numpy()
    z = noise.astype(np.float64)
    return lp, ((lp + z) / temp if method == GUMBEL else np.exp(lp / temp) / z)


@pytest.mark.parametrize("V", [257, 5000, 5001])
@pytest.mark.parametrize("method", [GUMBEL, MULTINOMIAL])
def test_sample_next_word_vs_fp64(method, V):
    """Strided logits, noise and outputs; the winner is the fp64 argmax of the kernel's own score, (lp + g) / temp or
    exp(lp / temp) / q, with first-index ties.  Rows whose fp64 top-2 relative gap is below 1e-5 are within the fp32
    rounding of the score and are skipped (counted: they must be rare).  Rows with two bit-identical best scores, in one
    thread's stride and in different wavefronts, must give the lower index."""
    N, T = 16, 6
    ld_t, nz_st, o_st = V + 5, V + 3, 2
    ld_n, nz_sn, o_sn = T * ld_t + 1, T * nz_st + 9, T * o_st + 1
    rng = np.random.default_rng(10 * V + method)
    rows = (rng.standard_normal((N, T, V)) * 2).astype(np.float32)
    if method == GUMBEL:
        u = rng.random((N, T, V), dtype=np.float32)
        noise = (-np.log(-np.log(u + 1e-20) + 1e-20)).astype(np.float32)
    else:
        noise = np.maximum(rng.exponential(1.0, (N, T, V)), 1e-30).astype(np.float32)
    planted = {}
    for n in range(N):
        c = int(rng.integers(0, V - 256))
        for t, off in ((0, 256), (1, 64)):                     # identical logit and noise at c and c + off: equal scores,
            rows[n, t, c] = rows[n, t, c + off] = rows[n, t].max() + 6.0       # and larger than any other of the row
            noise[n, t, c + off] = noise[n, t, c] = 1e-20 if method == MULTINOMIAL else 30.0
            planted[(n, t)] = c
    host = np.zeros(N * ld_n, np.float32); nz = np.ones(N * nz_sn, np.float32)
    for n in range(N):
        for t in range(T):
            host[n * ld_n + t * ld_t: n * ld_n + t * ld_t + V] = rows[n, t]
            nz[n * nz_sn + t * nz_st: n * nz_sn + t * nz_st + V] = noise[n, t]
    x, z = torch.from_numpy(host).cuda(), torch.from_numpy(nz).cuda()
    sel = (np.arange(N)[:, None] * o_sn + np.arange(T)[None, :] * o_st)
    for temp in (0.5, 1.0, 2.0):
        w = torch.full((N * o_sn,), -7, dtype=torch.long, device="cuda")
        lpo = torch.full((N * o_sn,), 9.0, device="cuda")
        _lib.call("acvae_sample_next_word", x, ld_n, ld_t, z, nz_sn, nz_st, method, temp, w, lpo, o_sn, o_st, N, T, V, st())
        w, lpo = w.cpu().numpy(), lpo.cpu().numpy().astype(np.float64)
        lp, sc = sample_scores_fp64(rows, noise, method, temp)
        top2 = -np.sort(-sc, -1)[..., :2]
        rel = (top2[..., 0] - top2[..., 1]) / np.abs(top2[..., 0])
        want = np.argmax(sc, -1)
        close_call = rel < 1e-5
        for (n, t), c in planted.items():
            assert w[sel[n, t]] == c, (temp, n, t, w[sel[n, t]], c)
            close_call[n, t] = False
        ok = close_call | (w[sel] == want)
        skipped = int(close_call.sum())
        print(f"method={method} V={V} temp={temp}: {skipped}/{N * T} rows within rounding of a tie, skipped")
        assert ok.all(), (temp, np.argwhere(~ok)[:4], w[sel][~ok][:4], want[~ok][:4])
        assert skipped <= N * T // 20
        lp_w = np.take_along_axis(lp, w[sel][..., None], -1)[..., 0]
        assert (np.abs(lpo[sel] - lp_w) <= lse_bound(V, lp_w)).all(), float(np.abs(lpo[sel] - lp_w).max())
        untouched = np.setdiff1d(np.arange(N * o_sn), sel.reshape(-1))
        assert (w[untouched] == -7).all() and (lpo[untouched] == 9.0).all()


# ------------------------------------------------------------------------------------------------ beam / DBS scores
def test_logprob_add_bit_equal_to_the_fp32_expression():
    """out[n, c] = logits[n, c] - lse[n] + prev[n] over a strided logits buffer (ld > V), prev null and given: bit-equal to
    torch evaluating the same fp32 expression in the same order."""
    V, ld = 5000, 5011
    for N in (1, 7, 48):
        g = torch.Generator().manual_seed(N)
        buf = torch.randn(N * ld, generator=g) * 4
        lse = torch.randn(N, generator=g) + 8
        prev = torch.randn(N, generator=g) * 10 - 20
        logits = buf.view(N, ld)[:, :V]
        for pv in (None, prev):
            out = torch.full((N * V + 5,), 3.0, device="cuda")
            _lib.call("acvae_logprob_add", buf.cuda(), ld, lse.cuda(), None if pv is None else pv.cuda(), out, N, V, st())
            want = logits - lse[:, None]
            if pv is not None:
                want = want + pv[:, None]
            got = out.cpu()
            assert torch.equal(got[:N * V].view(N, V), want), (N, pv is None, float((got[:N * V].view(N, V) - want).abs().max()))
            assert bool((got[N * V:] == 3.0).all())


@pytest.mark.parametrize("V", [5000, 5001])
def test_dbs_scores_one_count_vector_per_clip_vs_fp64(V):
    """rows_per_count > 0 (diverse beam search over a batch: clip i's rows use its own count vector), ld > V, against fp64
    log_softmax(log_softmax(x) / T) - lambda * counts[row / rows_per_count] + prev."""
    ld = V + 13
    for clips, bdash, temp, lam in ((3, 2, 1.0, 0.5), (4, 3, 1.5, 2.0), (2, 5, 0.7, 0.8)):
        N = clips * bdash
        g = torch.Generator().manual_seed(V + N)
        buf = torch.randn(N * ld, generator=g) * 3
        counts = torch.randint(0, 4, (clips, V), generator=g).float()
        prev = torch.randn(N, generator=g) * 5 - 10
        out = torch.empty(N * V, device="cuda")
        _lib.call("acvae_dbs_scores", buf.cuda(), ld, temp, counts.cuda(), lam, prev.cuda(), out, N, V, bdash, st())
        x = buf.view(N, ld)[:, :V].double()
        want = torch.log_softmax(torch.log_softmax(x, 1) / temp, 1) - lam * counts.double().repeat_interleave(bdash, 0) \
            + prev.double()[:, None]
        # |want| <= ~40: fp32 rounding of the two log-sum-exps and the three additions stays within a few 1e-6
        close(out.view(N, V), want, 1e-6, 4e-6, what=f"dbs scores V={V} clips={clips} bdash={bdash}")
