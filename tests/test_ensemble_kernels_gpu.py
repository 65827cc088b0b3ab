"""GPU: acvae_ensemble_mix (csrc/ensemble.hip) alone, at the row kernel's thread-stride boundaries (256 threads: V = 255 /
256 / 257), at V = 1 and 2, and at the production width (4999 / 5000 / 5001), for M = 1, 2, 3, 8 members with leading
dimensions larger than V, `prev` given and null: against float64 within a bound derived below, the argmax wherever float64
decides it by more than twice that bound, planted exact ties, the two exact identities the search relies on (M = 1 is the
acvae_row_logsoftmax_argmax + acvae_logprob_add route bit for bit; M copies of one matrix are M = 1 bit for bit), and
nothing written between the strided outputs or behind the last row."""
import numpy as np
import pytest
import torch

from acvae_amd import _lib
from acvae_amd.encoder import ptr_table
from test_decode_kernels_gpu import EPS32, lse_bound

pytestmark = pytest.mark.gpu
VS = [1, 2, 255, 256, 257, 4999, 5000, 5001]
PAD = 123.0                      # fills the padding of the logits buffers: larger than any logit, so a read of it shows
SCALE = 3.0                      # N(0, 1) * 3 logits: see test_random_logits_leave_the_argmax_decided


def st():
    return _lib.current_stream()


def mix_bound(V, M, lse, a, lg, prev):
    """Error bound of out = (a + logf(s / M)) + prev against float64, the way lse_bound is derived in
    test_decode_kernels_gpu.py (EPS32 = 2^-24, one rounding of a result r costs EPS32 * max(|r|, 1)):
      - lp_m = x - lse_m carries the error of lse_m, the largest member's lse_bound(V, lse_m) (taken without that function's
        own doubling), and the log of a convex combination of probabilities each within a factor e^d is within d;
      - s = sum_m expf(lp_m - a): M expf of 2 ulp (4 * EPS32 relative), M - 1 additions and one division,
        (4 + M + 2) * EPS32 relative in s, hence absolute in log(s / M);
      - one rounding each of |a| (the subtraction that forms lp), of the log and of the two final sums.
    Doubled for headroom, the file's convention."""
    member = np.max(np.stack([lse_bound(V, l) for l in lse]), 0)[:, None] / 2.0          # per row
    rel_s = (4 + M + 2) * EPS32
    one = lambda r: EPS32 * np.maximum(np.abs(r), 1.0)
    return 2.0 * (member + rel_s + one(a) + one(lg) + one(a + lg) + one(a + lg + prev))


def fp64_mix(rows, prev):
    """rows: list of M float32 arrays [R, V] -> (out, per-member lse, a, log(s / M)) in float64."""
    x = [r.astype(np.float64) for r in rows]
    lse = [np.log(np.exp(v - v.max(-1, keepdims=True)).sum(-1)) + v.max(-1) for v in x]
    lp = np.stack([v - l[:, None] for v, l in zip(x, lse)])
    a = lp.max(0)
    lg = np.log(np.exp(lp - a).sum(0) / len(rows))
    p = np.zeros(rows[0].shape[0]) if prev is None else prev.astype(np.float64)
    return a + lg + p[:, None], lse, a, lg, p


def make_rows(rng, M, R, V, ties=False):
    rows = [(rng.standard_normal((R, V)) * SCALE + 2.0 * m - 3.0).astype(np.float32) for m in range(M)]
    planted = {}
    if ties:
        for r in range(R):
            off = (256, 64, 1)[r % 3]                 # one thread's stride, two wavefronts, neighbouring lanes
            if V > off:
                c = int(rng.integers(0, V - off))
                for row in rows:                      # the two columns equal in every member, above everything else
                    row[r, c] = row[r, c + off] = row[r].max() + 1.0
                planted[r] = c
    return rows, planted


def upload(rows, lds):
    bufs = []
    for row, ld in zip(rows, lds):
        host = np.full((row.shape[0], ld), PAD, np.float32)
        host[:, :row.shape[1]] = row
        bufs.append(torch.from_numpy(host).cuda())
    return bufs


def run_mix(bufs, lds, prev, R, V, ld_out, o_stride, want_out=True, want_sel=True):
    M = len(bufs)
    out = torch.full((R * ld_out + 7,), 3.0, device="cuda") if want_out else None
    am = torch.full((R * o_stride + 2,), -5, dtype=torch.long, device="cuda") if want_sel else None
    best = torch.full((R * o_stride + 2,), 7.0, device="cuda") if want_sel else None
    ld = np.asarray(lds, np.int64)
    _lib.call("acvae_ensemble_mix", ptr_table(bufs), ld.ctypes.data, M, None if prev is None else prev, out, ld_out, am, best,
              o_stride, R, V, st())
    return tuple(None if t is None else t.cpu().numpy() for t in (out, am, best))


def test_random_logits_leave_the_argmax_decided():
    """The float64 reference alone, on the CPU: at SCALE the mixture's top-1 minus top-2 exceeds twice the bound on all but
    a few per cent of the rows test_mix_vs_fp64 draws at each V (at most 5 % may be left out there)."""
    for V in VS[1:]:
        total = out_of = 0
        rng = np.random.default_rng(V)
        for R in (1, 5):
            for M in (1, 2, 3, 8):
                rows, _ = make_rows(rng, M, R, V)
                want, lse, a, lg, p = fp64_mix(rows, None)
                top = -np.sort(-want, -1)[:, :2]
                c = np.argmax(want, -1)
                b = mix_bound(V, M, lse, a, lg, p[:, None])[np.arange(R), c]
                total += R
                out_of += int(((top[:, 0] - top[:, 1]) <= 2 * b).sum())
        assert out_of <= total // 20, (V, out_of, total)


@pytest.mark.parametrize("V", VS)
def test_mix_vs_fp64(V):
    rng, prng = np.random.default_rng(V), np.random.default_rng(1000 + V)     # rows as the CPU check above draws them
    worst, skipped, total = (0.0, 0.0, 0.0), 0, 0                    # (err / bound, err, bound) at the worst element
    for R in (1, 5):
        for M in (1, 2, 3, 8):
            rows, _ = make_rows(rng, M, R, V)
            lds = [V + 3 + m for m in range(M)]
            bufs = upload(rows, lds)
            for with_prev in (False, True):
                prev = (prng.standard_normal(R) * 10 - 20).astype(np.float32) if with_prev else None
                ld_out, o_stride = V + 5, 3
                out, am, best = run_mix(bufs, lds, None if prev is None else torch.from_numpy(prev).cuda(), R, V, ld_out,
                                        o_stride)
                want, lse, a, lg, p = fp64_mix(rows, prev)
                bound = mix_bound(V, M, lse, a, lg, p[:, None])
                got = out[:R * ld_out].reshape(R, ld_out)
                err = np.abs(got[:, :V].astype(np.float64) - want)
                k = np.unravel_index(np.argmax(err / bound), err.shape)
                worst = max(worst, (float(err[k] / bound[k]), float(err[k]), float(bound[k])))
                assert (err <= bound).all(), (V, R, M, with_prev, float(err[k]), float(bound[k]))
                # nothing between the strided outputs or behind the last row
                assert (got[:, V:] == 3.0).all() and (out[R * ld_out:] == 3.0).all()
                sel = np.arange(R) * o_stride
                rest = np.setdiff1d(np.arange(am.size), sel)
                assert (am[rest] == -5).all() and (best[rest] == 7.0).all()
                # the selection: the row's first maximum of the kernel's own scores, bit for bit ...
                assert np.array_equal(am[sel], np.argmax(got[:, :V], -1))
                assert np.array_equal(best[sel].view(np.int32), got[np.arange(R), am[sel]].view(np.int32))
                # ... and float64's wherever float64 decides it by more than twice the bound
                c = np.argmax(want, -1)
                if V > 1:
                    top = -np.sort(-want, -1)[:, :2]
                    decided = (top[:, 0] - top[:, 1]) > 2 * bound[np.arange(R), c]
                else:
                    decided = np.ones(R, bool)
                assert np.array_equal(am[sel][decided], c[decided]), (V, R, M, with_prev)
                skipped += int((~decided).sum()); total += R
    print(f"V={V}: worst |out - fp64| {worst[1]:.2e} (bound there {worst[2]:.2e}); {skipped}/{total} rows within twice the bound "
          "of an argmax tie, skipped")
    assert skipped <= total // 20


@pytest.mark.parametrize("V", [2, 257, 5000])
def test_mix_planted_ties_first_index_wins(V):
    rng = np.random.default_rng(100 + V)
    for M in (1, 3, 8):
        R = 6
        rows, planted = make_rows(rng, M, R, V, ties=True)
        lds = [V + 1 + 2 * m for m in range(M)]
        out, am, best = run_mix(upload(rows, lds), lds, None, R, V, V, 1)
        got = out[:R * V].reshape(R, V)
        assert planted
        for r, c in planted.items():
            off = (256, 64, 1)[r % 3]
            assert got[r, c].view(np.int32) == got[r, c + off].view(np.int32)          # equal inputs, equal scores
            assert am[r] == c, (V, M, r, am[r], c)
        # selection only (out == NULL, the greedy search's call): the same argmax and value
        _, am2, best2 = run_mix(upload(rows, lds), lds, None, R, V, V, 1, want_out=False)
        assert np.array_equal(am2, am) and np.array_equal(best2.view(np.int32), best.view(np.int32))


@pytest.mark.parametrize("V", VS)
def test_mix_one_member_is_the_two_kernel_route_bit_for_bit(V):
    """M = 1: s = expf(0) = 1, logf(1 / 1) = 0, so out = (x - lse) + prev exactly as acvae_row_logsoftmax_argmax +
    acvae_logprob_add form it on the same buffer; the argmax is that kernel's argmax."""
    rng = np.random.default_rng(200 + V)
    R, ld = 5, V + 9
    rows, _ = make_rows(rng, 1, R, V, ties=True)
    buf = upload(rows, [ld])[0]
    lse = torch.empty(R, device="cuda")
    am0 = torch.empty(R, dtype=torch.long, device="cuda")
    _lib.call("acvae_row_logsoftmax_argmax", buf, ld, ld, am0, None, lse, 1, 1, R, 1, V, st())
    for with_prev in (False, True):
        prev = torch.from_numpy((rng.standard_normal(R) * 10 - 20).astype(np.float32)).cuda() if with_prev else None
        want = torch.empty(R * V, device="cuda")
        _lib.call("acvae_logprob_add", buf, ld, lse, prev, want, R, V, st())
        out, am, _ = run_mix([buf], [ld], prev, R, V, V, 1)
        assert np.array_equal(out[:R * V].view(np.int32), want.cpu().numpy().view(np.int32)), (V, with_prev)
        assert np.array_equal(am[:R], am0.cpu().numpy())


@pytest.mark.parametrize("V", [1, 257, 5000])
def test_mix_copies_of_one_matrix_are_one_member_bit_for_bit(V):
    """M copies: every term of s is expf(0) = 1, s = M exactly, s / M = 1, logf(1) = 0."""
    rng = np.random.default_rng(300 + V)
    R, ld = 5, V + 2
    rows, _ = make_rows(rng, 1, R, V)
    buf = upload(rows, [ld])[0]
    prev = torch.from_numpy((rng.standard_normal(R) * 10 - 20).astype(np.float32)).cuda()
    one, am1, best1 = run_mix([buf], [ld], prev, R, V, V, 1)
    for M in (2, 3, 5, 8):
        copies = [buf] + [buf.clone() for _ in range(M - 1)]
        out, am, best = run_mix(copies, [ld] * M, prev, R, V, V, 1)
        assert np.array_equal(out.view(np.int32), one.view(np.int32)), (V, M)
        assert np.array_equal(am, am1) and np.array_equal(best.view(np.int32), best1.view(np.int32))
