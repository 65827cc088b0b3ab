"""GPU: acvae_ensemble_mix_sample (csrc/ensemble.hip) alone, through the C ABI: V = 1, 2, 255 / 256 / 257 (the 256-thread
stride) and 5000, M = 1, 2, 5, 8 members, R = 1, 3, 160 rows, leading dimensions larger than V, temp 0.5 / 1 / 2, both
methods.  The optional `out` row and `logprobs` against float64 within test_ensemble_kernels_gpu.mix_bound, the word
against float64's wherever float64 decides it by more than twice score_bound (below); and bit for bit: planted ties, a
column at -inf, M copies of one matrix, the held end_idx, a NaN row, every return code.

The seeded inputs are ensemble_rollout_util.kernel_inputs'; test_ensemble_rollout_cpu.py counts, on the CPU and with the
reference alone, the decisions this file leaves out (the same cap applies there)."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_rollout_util as RU
from acvae_amd import _lib
from acvae_amd.encoder import ptr_table
from test_decode_kernels_gpu import EPS32
from test_ensemble_kernels_gpu import PAD, fp64_mix, mix_bound, upload

pytestmark = pytest.mark.gpu
GUMBEL, MULTINOMIAL = 1, 2
CODE = {"gumbel": GUMBEL, "sample": MULTINOMIAL}
EINVAL = -1
MAX_LEFT_OUT = 0.02               # of a parameter set's decisions
MAX_BOUND = 1e-2                  # in log-score: a kernel whose error needs more fails
END = 2


def score_bound(mixb, v, noise, method, temp):
    """Error bound [R, V] of the kernel's score against float64, in the log-score domain ((v + g) / temp for "gumbel";
    v / temp - log q for "sample", the logarithm of expf(v / temp) / q), derived the way mix_bound is (EPS32 = 2^-24, one
    rounding of a result r costs EPS32 * max(|r|, 1)).  The noise is the same fp32 number on both sides.
      - v carries mix_bound (`mixb`, already doubled there), which the division by temp scales: mixb / temp;
      - "gumbel": one rounding of the sum v + g, scaled by 1 / temp, and one of the quotient;
      - "sample": one rounding of the quotient v / temp, which is an absolute error of the exponent and so of the
        log-score; expf within 2 ulp, 4 * EPS32 relative, hence absolute in the logarithm; one rounding of the division
        by q, EPS32 relative.  (Where expf(v / temp) is no normal number its error is below 2^-126 absolute: such a score
        loses to every normal one on both sides.)
    The roundings are doubled for headroom, the file's convention."""
    one = lambda r: EPS32 * np.maximum(np.abs(r), 1.0)
    z = noise.astype(np.float64)
    if method == "gumbel":
        return mixb / temp + 2.0 * (one(v + z) / temp + one((v + z) / temp))
    return mixb / temp + 2.0 * (one(v / temp) + 4 * EPS32 + EPS32)


def mixture_and_bound(rows):
    """-> (the float64 mixture [R, V], its mix_bound [R, V]); formed once per input, whatever the temperature."""
    R, V = rows[0].shape
    want, lse, a, lg, p = fp64_mix(rows, None)
    assert np.allclose(RU.mixture(rows), want, atol=1e-12, rtol=0)         # the yardstick's mixture is that file's
    return want, mix_bound(V, len(rows), lse, a, lg, p[:, None])


def decision_bound(rows, noise, method, temp, v, mixb):
    """-> (pick of the float64 yardstick, the score bound [R] at the row's two best words)."""
    got = RU.pick(rows, noise, method, temp, v=v)
    sb = score_bound(mixb, got["v"], noise, method, temp)
    order = np.argsort(-got["score"], -1, kind="stable")[:, :2]
    return got, np.take_along_axis(sb, order, -1).max(-1)


def st():
    return _lib.current_stream()


def run(rows, noise, method, temp, t=0, T=4, prev_word=None, want_out=True, pad=3):
    """One launch on step t of R rows.  -> (out [R, V] or None, seqs [R, T], logprobs [R, T], word [R]); the padding of
    every buffer is checked to be untouched."""
    M, (R, V) = len(rows), rows[0].shape
    lds = [V + pad + m for m in range(M)]
    bufs = upload(rows, lds)
    ld_nz, ld_out, ld_s, ld_lp = V + 2, V + 5, T + 1, T + 2
    nz = torch.from_numpy(np.pad(noise, ((0, 0), (0, ld_nz - V)), constant_values=np.float32(1e30))).cuda()
    out = torch.full((R * ld_out + 7,), 3.0, device="cuda") if want_out else None
    seqs0 = np.full((R, ld_s), -7, np.int64)
    if prev_word is not None:
        seqs0[:, t - 1] = prev_word
    seqs = torch.from_numpy(seqs0.reshape(-1)).cuda()
    lp = torch.full((R * ld_lp + 3,), 9.0, device="cuda")
    word = torch.full((R + 2,), -5, dtype=torch.long, device="cuda")
    ld = np.asarray(lds, np.int64)
    rc = _lib.lib().acvae_ensemble_mix_sample(ptr_table(bufs), ld.ctypes.data, M, nz.data_ptr(), ld_nz, CODE[method],
                                              float(temp), None if out is None else out.data_ptr(), ld_out, seqs.data_ptr(),
                                              ld_s, lp.data_ptr(), ld_lp, word.data_ptr(), END, t, R, V, st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    seqs_h, lp_h, word_h = seqs.cpu().numpy().reshape(R, ld_s), lp.cpu().numpy(), word.cpu().numpy()
    rest = np.ones((R, ld_s), bool); rest[:, t] = False
    assert np.array_equal(seqs_h[rest], seqs0[rest])
    lp2 = lp_h[:R * ld_lp].reshape(R, ld_lp)
    rest = np.ones((R, ld_lp), bool); rest[:, t] = False
    assert (lp2[rest] == 9.0).all() and (lp_h[R * ld_lp:] == 9.0).all() and (word_h[R:] == -5).all()
    assert np.array_equal(word_h[:R], seqs_h[:, t])                       # the word fed next is the word recorded
    out_h = None
    if out is not None:
        o = out.cpu().numpy()
        out_h = o[:R * ld_out].reshape(R, ld_out)
        assert (out_h[:, V:] == 3.0).all() and (o[R * ld_out:] == 3.0).all()
        out_h = out_h[:, :V]
    return out_h, seqs_h[:, t].copy(), lp2[:, t].copy(), word_h[:R].copy()


@pytest.mark.parametrize("method", RU.METHODS)
@pytest.mark.parametrize("V", RU.VS)
def test_mix_sample_vs_fp64(V, method):
    worst = 0.0
    for M in RU.MS:
        cases = [(R,) + RU.kernel_inputs(V, M, R, method) for R in RU.RS]
        cases = [c + mixture_and_bound(c[1]) for c in cases]
        for temp in RU.TEMPS:
            left_out = total = 0
            for R, rows, noise, v, mixb in cases:
                want, sb = decision_bound(rows, noise, method, temp, v, mixb)
                out, w, lp, _ = run(rows, noise, method, temp, t=1)
                err = np.abs(out.astype(np.float64) - want["v"])
                assert (err <= mixb).all(), (V, M, R, temp, float((err / mixb).max()))
                worst = max(worst, float((err / mixb).max()))
                assert ((w >= 0) & (w < V)).all()
                ar = np.arange(R)
                assert np.array_equal(lp.view(np.int32), out[ar, w].view(np.int32))   # v of the chosen word, the bits of `out`
                assert (np.abs(lp.astype(np.float64) - want["v"][ar, w]) <= mixb[ar, w]).all()
                assert sb.max() <= MAX_BOUND, (V, M, R, temp, float(sb.max()))
                decided = want["gap"] > 2 * sb
                assert np.array_equal(w[decided], want["chosen"][decided]), (V, M, R, temp)
                # out = NULL, the rollout's call: the same words and log-probabilities
                _, w2, lp2, _ = run(rows, noise, method, temp, t=1, want_out=False)
                assert np.array_equal(w2, w) and np.array_equal(lp2.view(np.int32), lp.view(np.int32))
                left_out += int((~decided).sum()); total += R
            print(f"V={V} M={M} {method} temp={temp}: {left_out}/{total} decisions within twice the bound, left out")
            assert left_out <= MAX_LEFT_OUT * total, (V, M, temp, left_out, total)
    print(f"V={V} {method}: worst |out - fp64| / mix_bound {worst:.2f}")


@pytest.mark.parametrize("method", RU.METHODS)
@pytest.mark.parametrize("V", [2, 257, 5000])
def test_planted_ties_first_index_wins(V, method):
    """Two columns equal in every member with equal noise, above everything else: equal scores, the lower index wins
    whether the two lie one thread's stride, two wavefronts or one lane apart."""
    for M in (1, 5, 8):
        R = 6
        rows, noise = RU.kernel_inputs(V, M, R, method)
        planted = {}
        for r in range(R):
            off = (256, 64, 1)[r % 3]
            if V > off:
                c = (37 * r + 11) % (V - off)
                for row in rows:
                    row[r, c] = row[r, c + off] = max(x[r].max() for x in rows) + 30.0
                noise[r, c] = noise[r, c + off] = noise[r].mean()
                planted[r] = c
        assert planted
        out, w, lp, _ = run(rows, noise, method, 1.0)
        for r, c in planted.items():
            off = (256, 64, 1)[r % 3]
            assert out[r, c].view(np.int32) == out[r, c + off].view(np.int32)
            assert w[r] == c, (V, M, r, w[r], c)
            assert lp[r].view(np.int32) == out[r, c].view(np.int32)


@pytest.mark.parametrize("method", RU.METHODS)
def test_column_at_minus_inf_in_every_member_is_never_chosen(method):
    for V in (2, 257, 5000):
        for M in (1, 2, 8):
            R = 5
            rows, noise = RU.kernel_inputs(V, M, R, method)
            cols = [(r * 97) % V for r in range(R)]
            for r, c in enumerate(cols):
                for row in rows:
                    row[r, c] = -np.inf
                noise[r, c] = 80.0 if method == "gumbel" else 1e-30     # the noise most in the column's favour
            out, w, lp, _ = run(rows, noise, method, 2.0)
            for r, c in enumerate(cols):
                assert out[r, c] == -np.inf and w[r] != c and np.isfinite(lp[r])


@pytest.mark.parametrize("method", RU.METHODS)
@pytest.mark.parametrize("V", [1, 257, 5000])
def test_copies_of_one_matrix_are_one_member_bit_for_bit(V, method):
    """M copies: every term of s is expf(0) = 1, s = M exactly, s / M = 1, logf(1) = 0: the M = 1 row, word and logprob."""
    rows, noise = RU.kernel_inputs(V, 1, 5, method)
    one = run(rows, noise, method, 0.5)
    for M in (2, 5, 8):
        got = run([rows[0].copy() for _ in range(M)], noise, method, 0.5)
        assert np.array_equal(got[0].view(np.int32), one[0].view(np.int32)), (V, M)
        assert np.array_equal(got[1], one[1]) and np.array_equal(got[2].view(np.int32), one[2].view(np.int32))


@pytest.mark.parametrize("method", RU.METHODS)
def test_row_fed_end_keeps_end_and_nan_row_stays_in_range(method):
    V, M, R = 257, 2, 6
    rows, noise = RU.kernel_inputs(V, M, R, method)
    free = run(rows, noise, method, 1.0, t=2, prev_word=np.full(R, 5))
    assert (free[1] != END).all()                                       # (seeded: no row draws END by itself)
    prev = np.array([END, 5, END, 7, 9, END])
    out, w, lp, word = run(rows, noise, method, 1.0, t=2, prev_word=prev)
    held = prev == END
    assert (w[held] == END).all() and np.array_equal(w[~held], free[1][~held]) and np.array_equal(word, w)
    assert np.array_equal(lp.view(np.int32), free[2].view(np.int32))    # the chosen word's, held or not
    # t = 0 has no previous word: whatever lies in front of the row is not read as one
    assert np.array_equal(run(rows, noise, method, 1.0, t=0)[1], free[1])
    for r in (1, 4):
        for row in rows:
            row[r, :] = np.nan
    _, w, _, _ = run(rows, noise, method, 1.0, t=0)
    assert ((w >= 0) & (w < V)).all() and np.array_equal(w[[0, 2, 3, 5]], free[1][[0, 2, 3, 5]])


def test_mix_sample_return_codes():
    V, R, T = 50, 4, 6
    lib = _lib.lib()
    ptrs = (ctypes.c_void_p * 9)(*([0x1000] * 9))
    ld = np.full(9, V, np.int64)
    good = dict(logits=ptrs, ld=ld.ctypes.data, M=2, noise=0x1000, ld_noise=V, method=MULTINOMIAL, temp=1.0, out=None,
                ld_out=0, seqs=0x1000, ld_seqs=T, logprobs=0x1000, ld_logprobs=T, word=0x1000, end_idx=END, t=T - 1, R=R,
                V=V, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.acvae_ensemble_mix_sample(*a.values())

    for kw in (dict(M=0), dict(M=9), dict(logits=None), dict(ld=None), dict(noise=None), dict(ld_noise=V - 1),
               dict(method=0), dict(method=3), dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")),
               dict(temp=float("inf")), dict(out=0x1000, ld_out=V - 1), dict(seqs=None), dict(logprobs=None),
               dict(word=None), dict(t=-1), dict(t=T), dict(ld_logprobs=T - 1), dict(R=0), dict(V=0)):
        assert call(**kw) == EINVAL, kw
    ld[1] = V - 1
    assert call() == EINVAL
    ld[1] = V; ptrs[1] = None
    assert call() == EINVAL
    ptrs[1] = 0x1000
    rows, noise = RU.kernel_inputs(V, 2, R, "sample")                  # and the well-formed set is taken
    assert run(rows, noise, "sample", 1.0)[1].shape == (R,)
    assert PAD > 0
