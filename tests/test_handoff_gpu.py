"""GPU: the cross-workgroup reductions of the composite drivers, called directly at the shapes where they go wrong.

Each of them hands partial results from workgroup to workgroup without a fence: the partials are stored with agent-scope
stores, one lane takes a ticket, and the workgroup that draws the last ticket sums the partials in a fixed order and resets
the ticket.  Covered here:
  * the skinny NT product split over K (gemm_skinny_kernel, gridDim.z = S > 1) and its dual form;
  * the pair form (two products in one launch, no split): bit for bit the single product;
  * the TN product with its slab sum in the same launch: bit for bit the two-launch acvae_gemm_tn;
  * the column sums, single (acvae_colsum) and batched (colsum_batch_kernel): bit for bit the single launch.
Every case asserts the plan the dispatcher makes for its shape (the *_plan queries call the dispatchers' own helpers), so a
shape that silently takes another path fails instead of testing nothing.  The ticket sequences run one reset call and then
calls that rely on every reducer having reset its ticket, on one workspace whose slabs still hold the previous call's
partials: a stale read or a ticket left behind shows as a wrong value, and the tickets must read back as zero.  None of these
kernels waits on a ticket, so a wrong ticket gives a wrong value, never a hang.  References are fp64 on the host."""
import ctypes
import math

import numpy as np
import pytest
import torch

from acvae_amd import _lib
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -3


def lib():
    return _lib.lib()


def stream():
    return _lib.current_stream()


def chain_tol(K):
    """|err| bound for an fp32 K-term chain with O(1) result (tests/test_kernels_gpu.py): 6 sigma of the rounding random
    walk 2^-24 sqrt(K) rms, floor 1e-5."""
    return max(1e-5, 6 * 2.0 ** -24 * math.sqrt(K))


def assert_every_element(got, ref, K, what):
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rms = float(ref.pow(2).mean().sqrt())
    tol = chain_tol(K) * torch.maximum(ref.abs(), torch.full_like(ref, rms))
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, worst " \
                                f"{float((err / tol).max()):.2f} x tol (|err| {float(err.max()):.3e}, rms {rms:.3e})"


def assert_bits(got, want, what):
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        f"{what}: {int((got != want).sum())}/{got.numel()} elements differ, max |d| {float((got - want).abs().max()):.3e}"


class Mat:
    """A [rows, cols] fp32 operand with row stride ld, `off` floats into a device buffer (off % 4 != 0: not 16-B aligned)."""

    def __init__(self, g, rows, cols, ld=None, off=0):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld or cols, off
        self.buf = torch.randn(off + rows * self.ld, generator=g)
        self.host = self.buf[off:].view(rows, self.ld)[:, :cols].double()
        self.dev = self.buf.cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * self.off


def garbage_ws(nbytes):
    """A workspace of exactly `nbytes` between guards (tests/ws_guard.py) whose slabs hold NaN (0xFF bytes), tickets full
    counters until a reset zeroes them.  The handle answers data_ptr() and numel() as the tensor it stands for."""
    return guarded(nbytes, 0xFF)


def tickets(ws, words):
    return ws.view[:4 * words].view(torch.int32).cpu()


# ------------------------------------------------------------------------------------------------ skinny split-K
SK_WS = None


def sk_ws_bytes():
    global SK_WS
    if SK_WS is None:
        SK_WS = lib().acvae_gemm_nt_splitk_workspace_bytes()
    return SK_WS


class SkCase:
    """C[M,N] (+)= A1 . B1^T (+ A2 . B2^T) (+ bias) with fresh inputs from `seed`."""

    def __init__(self, seed, M, N, K1, K2=0, lda_pad=0, off=0, bias=False, acc=False):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K1, self.K2, self.acc = M, N, K1, K2, int(acc)
        s = 1.0 / math.sqrt(K1 + K2)
        self.A1 = Mat(g, M, K1, K1 + lda_pad, off); self.B1 = Mat(g, N, K1)
        self.A2 = Mat(g, M, K2, K2 + lda_pad) if K2 else None
        self.B2 = Mat(g, N, K2, K2 + lda_pad, off) if K2 else None
        self.bias = torch.randn(N, generator=g) if bias else None
        self.bias_d = self.bias.cuda() if bias else None
        self.C0 = torch.randn(M, N, generator=g) * s
        ref = self.A1.host @ self.B1.host.T
        if K2:
            ref = ref + self.A2.host @ self.B2.host.T
        if bias:
            ref = ref + self.bias.double()
        if acc:
            ref = ref + self.C0.double()
        self.ref = ref

    def plan(self, with_ws=True):
        return lib().acvae_gemm_nt_split_plan(self.M, self.N, self.K1, self.K2, int(with_ws))

    def run(self, ws, reset, C=None):
        if C is None:
            C = self.C0.cuda()
        A2, B2 = self.A2, self.B2
        rc = lib().acvae_gemm_nt_dual_ws(self.A1.ptr, self.A1.ld, self.B1.ptr, self.B1.ld, self.K1,
                                         A2.ptr if A2 else None, A2.ld if A2 else 0, B2.ptr if B2 else None,
                                         B2.ld if B2 else 0, self.K2, self.bias_d.data_ptr() if self.bias is not None else None,
                                         C.data_ptr(), self.N, self.M, self.N, self.acc,
                                         ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                         int(reset), stream())
        assert rc == 0, rc
        return C

    def terms(self):
        return self.K1 + self.K2 + 2


# (M, N, K1, K2, lda_pad, off, bias, acc, S): 1 to 16 tiles, M in {1, 7, 32, 33, 64}, Ktot 1024 .. 4096 -> every S of 4..8;
# K % 8 != 0, K % 4 != 0, an odd lda and a misaligned pointer take the VEC4 = false kernel
SK_CASES = [
    (1, 32, 1024, 0, 0, 0, False, False, 4),
    (1, 1, 1027, 0, 0, 0, True, True, 4),
    (7, 500, 1280, 0, 0, 0, True, True, 5),
    (32, 512, 1536, 0, 0, 0, False, False, 6),
    (33, 256, 1790, 0, 0, 0, True, False, 6),
    (64, 100, 2048, 0, 1, 0, False, True, 8),
    (64, 64, 4096, 0, 0, 0, True, True, 8),
    (64, 256, 1024, 0, 0, 1, False, False, 4),
    (32, 512, 1536, 512, 0, 0, True, True, 8),
    (7, 300, 1001, 1023, 0, 0, False, False, 7),
    (33, 96, 600, 700, 3, 0, True, True, 5),
    (1, 480, 1800, 92, 0, 0, False, True, 7),
]


@pytest.mark.parametrize("M,N,K1,K2,pad,off,bias,acc,S", SK_CASES)
def test_skinny_split_k_against_fp64(M, N, K1, K2, pad, off, bias, acc, S):
    c = SkCase(100 + M + N + K1, M, N, K1, K2, pad, off, bias, acc)
    assert c.plan() == S and c.plan(with_ws=False) == 1
    ws = garbage_ws(sk_ws_bytes())
    got = c.run(ws, reset=True)
    again = c.run(ws, reset=False)
    unsplit = c.run(None, reset=False)
    torch.cuda.synchronize()
    assert_every_element(got, c.ref, c.terms(), f"split-K S={S}")
    assert_bits(again, got, f"split-K S={S}, second call")
    assert_every_element(unsplit, c.ref, c.terms(), "no split")
    assert not bool(tickets(ws, 1024).any())


# A ticket sequence: geometries whose tile 0 sees S = 8, 4, 6, ... and whose tile counts change from call to call
SK_SEQ = [(32, 512, 2048, 0, 8), (7, 64, 1024, 0, 4), (64, 256, 1536, 0, 6), (1, 32, 4096, 0, 8), (33, 64, 1300, 0, 5),
          (32, 480, 1024, 512, 6), (64, 256, 1024, 0, 4), (7, 100, 1800, 7, 7), (32, 512, 2000, 0, 7), (1, 1, 2048, 0, 8)]


def sk_sequence(base):
    cases = []
    for i, (M, N, K1, K2, S) in enumerate(SK_SEQ):
        c = SkCase(base + i, M, N, K1, K2, bias=i % 2 == 0, acc=i % 3 == 0)
        assert c.plan() == S, (M, N, K1, K2, c.plan(), S)
        cases.append(c)
    return cases


def test_skinny_ticket_reuse_sequence():
    """One reset call, then nine that rely on the reducers' resets, all on one workspace: each result equals the same call on a
    freshly reset workspace bit for bit, and the tickets are zero at the end."""
    cases = sk_sequence(500)
    want = [c.run(garbage_ws(sk_ws_bytes()), reset=True) for c in cases]
    ws = garbage_ws(sk_ws_bytes())
    got = [c.run(ws, reset=(i == 0)) for i, c in enumerate(cases)]
    torch.cuda.synchronize()
    for i, (c, g_, w_) in enumerate(zip(cases, got, want)):
        assert_bits(g_, w_, f"sequence call {i} (S={c.plan()})")
        assert_every_element(g_, c.ref, c.terms(), f"sequence call {i}")
    assert not bool(tickets(ws, 1024).any())


def test_skinny_ticket_sequences_on_two_streams():
    """The same sequence on two streams at once, a workspace each (the decoder's two chains): bit-identical to the serial run."""
    cases = sk_sequence(700)
    ws0 = garbage_ws(sk_ws_bytes())
    serial = [c.run(ws0, reset=(i == 0)) for i, c in enumerate(cases)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [garbage_ws(sk_ws_bytes()) for _ in streams]
    outs = [[c.C0.cuda() for c in cases] for _ in streams]
    main = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(main)
    for i, c in enumerate(cases):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                c.run(wss[k], reset=(i == 0), C=outs[k][i])
    for s in streams:
        main.wait_stream(s)
    torch.cuda.synchronize()
    for k in range(2):
        for i in range(len(cases)):
            assert_bits(outs[k][i], serial[i], f"stream {k}, call {i}")
        assert not bool(tickets(wss[k], 1024).any())


# ------------------------------------------------------------------------------------------------ pair
def pair_side(g, M, N, K, off, bias, acc):
    A, B = Mat(g, M, K, off=off), Mat(g, N, K)
    b = torch.randn(N, generator=g) if bias else None
    C0 = torch.randn(M, N, generator=g)
    ref = A.host @ B.host.T + (b.double() if bias else 0) + (C0.double() if acc else 0)
    return dict(A=A, B=B, K=K, N=N, bias=b.cuda() if bias else None, C0=C0, acc=int(acc), ref=ref)


def run_pair(p0, p1, M):
    C0, C1 = p0["C0"].cuda(), p1["C0"].cuda()
    bp = lambda p: p["bias"].data_ptr() if p["bias"] is not None else None
    rc = lib().acvae_gemm_nt_pair_c(p0["A"].ptr, p0["A"].ld, p0["B"].ptr, p0["B"].ld, p0["K"], bp(p0), C0.data_ptr(), p0["N"],
                                    p0["N"], p0["acc"], p1["A"].ptr, p1["A"].ld, p1["B"].ptr, p1["B"].ld, p1["K"], bp(p1),
                                    C1.data_ptr(), p1["N"], p1["N"], p1["acc"], M, stream())
    assert rc == 0, rc
    return C0, C1


def run_single(p, M):
    C = p["C0"].cuda()
    rc = lib().acvae_gemm_nt(p["A"].ptr, p["A"].ld, p["B"].ptr, p["B"].ld,
                             p["bias"].data_ptr() if p["bias"] is not None else None, C.data_ptr(), p["N"], M, p["N"], p["K"],
                             p["acc"], stream())
    assert rc == 0, rc
    return C


# (M, N0, K0, off0, N1, K1, off1): both products aligned (VEC4) or both not, so the single call picks the pair's VEC4
PAIR_SAME = [(1, 512, 512, 0, 1536, 512, 0), (32, 100, 64, 0, 37, 200, 0), (64, 512, 512, 0, 1536, 256, 0),
             (32, 33, 63, 0, 70, 131, 0), (64, 96, 64, 1, 40, 100, 3)]


@pytest.mark.parametrize("M,N0,K0,off0,N1,K1,off1", PAIR_SAME)
def test_pair_equals_the_single_product_bit_for_bit(M, N0, K0, off0, N1, K1, off1):
    g = torch.Generator().manual_seed(M * 7 + N0 + K1)
    p0 = pair_side(g, M, N0, K0, off0, bias=True, acc=False)
    p1 = pair_side(g, M, N1, K1, off1, bias=False, acc=True)
    # no workspace: the single call takes the 32x32-tile kernel unsplit, the arithmetic of a pair tile
    assert lib().acvae_gemm_nt_split_plan(M, N0, K0, 0, 0) == 1 and lib().acvae_gemm_nt_split_plan(M, N1, K1, 0, 0) == 1
    c0, c1 = run_pair(p0, p1, M)
    s0, s1 = run_single(p0, M), run_single(p1, M)
    torch.cuda.synchronize()
    assert_bits(c0, s0, "pair, first product")
    assert_bits(c1, s1, "pair, second product")
    assert_every_element(c0, p0["ref"], K0 + 1, "pair, first product")
    assert_every_element(c1, p1["ref"], K1 + 1, "pair, second product")


def test_pair_with_mixed_alignment_against_fp64():
    """One aligned product beside one that is not: the pair takes the unaligned kernel for both."""
    g = torch.Generator().manual_seed(77)
    p0 = pair_side(g, 33, 300, 512, 0, bias=False, acc=True)
    p1 = pair_side(g, 33, 64, 61, 0, bias=True, acc=False)
    c0, c1 = run_pair(p0, p1, 33)
    torch.cuda.synchronize()
    assert_every_element(c0, p0["ref"], 513, "mixed pair, first product")
    assert_every_element(c1, p1["ref"], 62, "mixed pair, second product")


# ------------------------------------------------------------------------------------------------ fused TN
TN_TICKETS = 256


class TnCase:
    """C[M,N] (+)= A[K,M]^T . B[K,N]."""

    def __init__(self, seed, M, N, K, acc):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.acc = M, N, K, int(acc)
        self.A = Mat(g, K, M); self.B = Mat(g, K, N)
        self.C0 = torch.randn(M, N, generator=g)
        self.ref = self.A.host.T @ self.B.host + (self.C0.double() if acc else 0)

    def ws_bytes(self):
        return lib().acvae_gemm_tn_fused_workspace_bytes(self.M, self.N, self.K)

    def plan(self, ws_bytes=None):
        return lib().acvae_gemm_tn_fused_plan(self.M, self.N, self.K, self.ws_bytes() if ws_bytes is None else ws_bytes)

    def fused(self, ws, reset, ws_bytes=None, C=None):
        if C is None:
            C = self.C0.cuda()
        rc = lib().acvae_gemm_tn_fused_c(self.A.ptr, self.M, self.B.ptr, self.N, C.data_ptr(), self.N, self.M, self.N, self.K,
                                         self.acc, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, int(reset),
                                         stream())
        assert rc == 0, rc
        return C

    def two_launch(self):
        C = self.C0.cuda()
        nb = lib().acvae_gemm_tn_workspace_bytes(self.M, self.N, self.K)
        slab = garbage_ws(nb)
        rc = lib().acvae_gemm_tn(self.A.ptr, self.M, self.B.ptr, self.N, C.data_ptr(), self.N, self.M, self.N, self.K,
                                 self.acc, slab.data_ptr(), nb, stream())
        assert rc == 0, rc
        return C


# (M, N, K, acc, slices): narrow (M <= 64) and wide tiles, 2 slices up to the most the dispatcher plans, M / N not multiples of 4
TN_CASES = [
    (256, 256, 100, False, 2),
    (512, 512, 672, True, 11),
    (512, 512, 1984, False, 16),
    (100, 203, 3000, True, 47),
    (30, 50, 777, False, 13),
    (64, 576, 4096, True, 43),
    (128, 128, 100000, False, 250),
    (1024, 1024, 672, True, 4),
]


@pytest.mark.parametrize("M,N,K,acc,slices", TN_CASES)
def test_fused_tn_equals_the_two_launch_form_bit_for_bit(M, N, K, acc, slices):
    c = TnCase(M + N + K, M, N, K, acc)
    assert c.plan() == slices
    ws = garbage_ws(c.ws_bytes())
    got = c.fused(ws, reset=True)
    want = c.two_launch()
    torch.cuda.synchronize()
    assert_bits(got, want, f"fused TN, {slices} slices")
    assert_every_element(got, c.ref, K + 1, f"fused TN, {slices} slices")
    assert not bool(tickets(ws, TN_TICKETS).any())


def test_fused_tn_single_slice_and_short_workspace_against_fp64():
    one = TnCase(5, 5000, 512, 672, True)
    assert one.plan() == 1 and one.ws_bytes() == 0
    ws = garbage_ws(0)
    got_one = one.fused(ws, reset=True)
    short = TnCase(6, 512, 512, 672, False)
    assert short.plan() == 11 and short.plan(short.ws_bytes() - 4) == 1
    ws2 = garbage_ws(short.ws_bytes())
    got_short = short.fused(ws2, reset=True, ws_bytes=short.ws_bytes() - 4)
    torch.cuda.synchronize()
    assert_every_element(got_one, one.ref, 673, "fused TN, one slice")
    assert_every_element(got_short, short.ref, 673, "fused TN, workspace too small")


# slice counts and tile counts change from call to call
TN_SEQ = [(64, 576, 4096, 43), (256, 256, 100, 2), (512, 512, 672, 11), (30, 50, 777, 13), (100, 203, 3000, 47),
          (512, 512, 1984, 16), (1024, 1024, 672, 4), (64, 576, 1000, 16), (256, 256, 300, 5)]


def test_fused_tn_ticket_reuse_sequence():
    cases = []
    for i, (M, N, K, s) in enumerate(TN_SEQ):
        c = TnCase(900 + i, M, N, K, i % 2 == 1)
        assert c.plan() == s, (M, N, K, c.plan(), s)
        cases.append(c)
    ws = garbage_ws(max(c.ws_bytes() for c in cases))       # one workspace for the sequence; each call is told its own size
    got = [c.fused(ws, reset=(i == 0), ws_bytes=c.ws_bytes()) for i, c in enumerate(cases)]
    want = [c.two_launch() for c in cases]
    torch.cuda.synchronize()
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert_bits(g_, w_, f"TN sequence call {i}")
    assert not bool(tickets(ws, TN_TICKETS).any())


# ------------------------------------------------------------------------------------------------ column sums
CS_WIDTHS = [1, 63, 64, 65, 576, 1536, 8192]
CS_ROWS = [1, 15, 16, 17, 1024, 1025, 4096, 4097, 8000]      # every row-group count of cs_groups: P, 16, 32, 64
_CS_X = None


def cs_matrix():
    global _CS_X
    if _CS_X is None:
        _CS_X = torch.randn(max(CS_ROWS), max(CS_WIDTHS), generator=torch.Generator().manual_seed(31))
    return _CS_X


def colsum_ref(x):
    return x.double().sum(0)


def assert_colsum(got, x, what):
    ref = colsum_ref(x)
    want = ref.float().double()
    ulp = torch.from_numpy(np.spacing(np.abs(ref.float().numpy()))).double()
    tol = ulp + 1e-12 * x.double().abs().sum(0)
    err = (got.cpu().double() - want).abs()
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} columns off, worst {float((err / tol).max()):.2f} x tol"


def colsum(xd, out=None):
    P, w = xd.shape
    nb = lib().acvae_colsum_workspace_bytes(w)
    ws = garbage_ws(nb)
    out = torch.full((w,), float("nan"), device="cuda") if out is None else out
    rc = lib().acvae_colsum(xd.data_ptr(), P, w, out.data_ptr(), ws.data_ptr(), nb, stream())
    return rc, out


@pytest.mark.parametrize("width", CS_WIDTHS)
def test_colsum_against_fp64(width):
    X = cs_matrix()
    for P in CS_ROWS:
        x = X[:P, :width].contiguous()
        rc, got = colsum(x.cuda())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert_colsum(got, x, f"colsum P={P} width={width}")


def test_colsum_width_beyond_the_tickets_is_unsupported():
    x = torch.zeros(4, 8193, device="cuda")
    rc, _ = colsum(x)
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def ptrs(v):
    return (ctypes.c_void_p * len(v))(*v)


class CsBatch:
    def __init__(self, seed, jobs):      # jobs: [(P, width, with_out_b)]
        g = torch.Generator().manual_seed(seed)
        self.jobs = jobs
        self.x = [torch.randn(P, w, generator=g).cuda() for P, w, _ in jobs]
        self.P, self.W = ints([P for P, _, _ in jobs]), ints([w for _, w, _ in jobs])

    def ws_bytes(self):
        return lib().acvae_colsum_batch_workspace_bytes(len(self.jobs), self.P, self.W)

    def plan(self, nb):
        return lib().acvae_colsum_batch_plan(len(self.jobs), self.P, self.W, nb)

    def run(self, ws, nb, reset):
        n = len(self.jobs)
        out = [torch.full((w,), float("nan"), device="cuda") for _, w, _ in self.jobs]
        out_b = [torch.full((w,), float("nan"), device="cuda") if b else None for _, w, b in self.jobs]
        table_b = ptrs([o.data_ptr() if o is not None else None for o in out_b]) if any(b for *_, b in self.jobs) else None
        rc = lib().acvae_colsum_batch(n, ptrs([x.data_ptr() for x in self.x]), self.P, self.W, ptrs([o.data_ptr() for o in out]),
                                      table_b, ws.data_ptr(), nb, int(reset), stream())
        assert rc == 0, rc
        return out, out_b

    def check(self, out, out_b, what):
        for j, (x, o, ob) in enumerate(zip(self.x, out, out_b)):
            _, want = colsum(x)
            torch.cuda.synchronize()
            assert_bits(o, want, f"{what}, job {j}")
            if ob is not None:
                assert_bits(ob, want, f"{what}, job {j} (second output)")


# (P, width, out_b): R = cs_groups(P) differs between the jobs, so the launch's grid y (the largest R) exceeds most jobs' R
CS_BATCHES = [
    [(4097, 64, False), (2000, 130, True), (10, 1, False), (672, 512, True)],
    [(32, 1536, True), (5, 100, False)],
    [(8000, 576, False), (17, 65, True), (1, 63, False), (1025, 64, True), (4096, 1000, False), (3, 7, True)],
]


@pytest.mark.parametrize("k", range(len(CS_BATCHES)))
def test_colsum_batch_equals_the_single_launches_bit_for_bit(k):
    b = CsBatch(40 + k, CS_BATCHES[k])
    nb = b.ws_bytes()
    assert b.plan(nb) == 1
    ws = garbage_ws(nb)
    out, out_b = b.run(ws, nb, reset=True)
    torch.cuda.synchronize()
    b.check(out, out_b, f"batch {k}")
    assert not bool(tickets(ws, 128).any())


def test_colsum_batch_fallbacks():
    """More than 128 column blocks, a single job, and a workspace too small for all group sums: one launch per job."""
    wide = CsBatch(50, [(100, 8192, False), (50, 100, True)])
    single = CsBatch(51, [(1025, 300, True)])
    short = CsBatch(52, CS_BATCHES[0])
    small = max(lib().acvae_colsum_batch_workspace_bytes(1, ints([P]), ints([w])) for P, w, _ in CS_BATCHES[0])
    cases = [(wide, wide.ws_bytes(), "more than 128 column blocks"), (single, single.ws_bytes(), "one job"),
             (short, small, "workspace too small")]
    for b, nb, what in cases:
        assert b.plan(nb) == 0, what
        ws = garbage_ws(nb)
        out, out_b = b.run(ws, nb, reset=True)
        torch.cuda.synchronize()
        b.check(out, out_b, what)
        for x, o in zip(b.x, out):
            assert_colsum(o, x.cpu(), what)


def test_colsum_batch_ticket_reuse_sequence():
    """One reset call, then batches of other shapes on the same workspace that rely on the reducers' resets."""
    seq = [CsBatch(60 + i, jobs) for i, jobs in enumerate(CS_BATCHES + CS_BATCHES[::-1] + CS_BATCHES)]
    nb = max(b.ws_bytes() for b in seq)
    assert all(b.plan(nb) == 1 for b in seq)
    ws = garbage_ws(nb)
    res = [b.run(ws, nb, reset=(i == 0)) for i, b in enumerate(seq)]
    torch.cuda.synchronize()
    for i, (b, (out, out_b)) in enumerate(zip(seq, res)):
        b.check(out, out_b, f"batch sequence call {i}")
    assert not bool(tickets(ws, 128).any())
