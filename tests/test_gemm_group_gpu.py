"""GPU: several TN products in ONE launch (acvae_gemm_tn_group_c, gemm_tn_group_kernel) against each product's own
acvae_gemm_tn_fused_c call, bit for bit.

The decode backward sends a chain's trailing weight gradients out this way.  All jobs of a launch are live at once, so every
sliced job must have slabs and tickets of its own: a slab or ticket range shared by two jobs shows here as a result that
depends on the order of the jobs, and a ticket a reducer did not reset as a second launch that differs from the first.  No
workgroup waits on a ticket, so a wrong ticket gives a wrong value, never a hang.

The table (M, N, K -> slices of the job's own plan, asserted below):
  (132,  68,  200) ->  4   ragged tiles
  (128, 128,   70) ->  2   the shortest K that is still sliced (a job of ONE slice is in test_one_slice_job_writes_c_itself:
                           tn_splits cuts every K > 64 of a one-tile product)
  (260, 192,  672) -> 11   several tiles and slices
  (512, 512,   96) ->  2   written with ldc > N into the right-hand column block of a wider matrix
  (256, 128, 1984) -> 31   long K
"""
import ctypes

import pytest
import torch

from acvae_amd import _lib
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu

TN_TICKETS = 256
JOBS = [(132, 68, 200, 4), (128, 128, 70, 2), (260, 192, 672, 11), (512, 512, 96, 2), (256, 128, 1984, 31)]
LEFT = 160            # job 4's matrix is [512, LEFT + 512]: the job owns the columns from LEFT on
SENTINEL = -7.25


def lib():
    return _lib.lib()


def stream():
    return _lib.current_stream()


def garbage_ws(nbytes):
    """Exactly `nbytes` between guards (tests/ws_guard.py); slabs (and, until a reset, tickets) of 0xFF bytes - NaN and full
    counters: a slab element read before it is written shows.  The handle answers data_ptr() and numel() as a tensor."""
    return guarded(nbytes, 0xFF)


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def longs(v):
    return (ctypes.c_int64 * len(v))(*v)


def ptrs(v):
    return (ctypes.c_void_p * len(v))(*v)


class Job:
    def __init__(self, seed, M, N, K, left=0):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.left, self.ldc = M, N, K, left, left + N
        self.A_host = torch.randn(K, M, generator=g)
        self.B_host = torch.randn(K, N, generator=g)
        self.A, self.B = self.A_host.cuda(), self.B_host.cuda()

    def out(self):
        return torch.full((self.M, self.ldc), SENTINEL, device="cuda")

    def c_ptr(self, C):
        return C.data_ptr() + 4 * self.left

    def own_call(self):
        """The product's own fused launch, on a workspace of its own."""
        nb = lib().acvae_gemm_tn_fused_workspace_bytes(self.M, self.N, self.K)
        ws = garbage_ws(nb)
        C = self.out()
        rc = lib().acvae_gemm_tn_fused_c(self.A.data_ptr(), self.M, self.B.data_ptr(), self.N, self.c_ptr(C), self.ldc, self.M,
                                         self.N, self.K, 0, ws.data_ptr(), nb, 1, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return C


def group_ws_bytes(jobs):
    nb = lib().acvae_gemm_tn_group_workspace_bytes(len(jobs), ints([j.M for j in jobs]), ints([j.N for j in jobs]),
                                                   ints([j.K for j in jobs]))
    assert nb >= 0, nb
    return nb


def group_call(jobs, ws, reset):
    outs = [j.out() for j in jobs]
    rc = lib().acvae_gemm_tn_group_c(len(jobs), ptrs([j.A.data_ptr() for j in jobs]), longs([j.M for j in jobs]),
                                     ptrs([j.B.data_ptr() for j in jobs]), longs([j.N for j in jobs]),
                                     ptrs([j.c_ptr(C) for j, C in zip(jobs, outs)]), longs([j.ldc for j in jobs]),
                                     ints([j.M for j in jobs]), ints([j.N for j in jobs]), ints([j.K for j in jobs]),
                                     ws.data_ptr(), ws.numel(), int(reset), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return outs


def assert_bits(got, want, what):
    assert torch.equal(got, want), \
        f"{what}: {int((got != want).sum())}/{got.numel()} elements differ, max |d| {float((got - want).abs().max()):.3e}"


_TABLE = None


def table():
    """The five jobs and each one's own fused result: computed once, never modified."""
    global _TABLE
    if _TABLE is None:
        jobs = [Job(40 + i, M, N, K, LEFT if i == 3 else 0) for i, (M, N, K, _) in enumerate(JOBS)]
        for j, (M, N, K, s) in zip(jobs, JOBS):
            assert lib().acvae_gemm_tn_fused_plan(M, N, K, lib().acvae_gemm_tn_fused_workspace_bytes(M, N, K)) == s, (M, N, K)
        _TABLE = (jobs, [j.own_call() for j in jobs])
    return _TABLE


def test_workspace_is_the_sum_of_the_jobs_slabs():
    jobs, _ = table()
    assert group_ws_bytes(jobs) == 4 * (TN_TICKETS + sum(s * M * N for M, N, K, s in JOBS))


def test_each_job_equals_its_own_fused_call_and_the_tickets_reset_themselves():
    jobs, want = table()
    ws = garbage_ws(group_ws_bytes(jobs))
    first = group_call(jobs, ws, reset=True)
    for i, (g, w) in enumerate(zip(first, want)):
        assert_bits(g, w, f"job {i + 1} {JOBS[i][:3]}")       # job 4: the whole wide matrix, so the left columns as well
    assert bool((first[3][:, :LEFT] == SENTINEL).all()), "job 4 wrote outside its column block"
    assert not bool(ws.view[:4 * TN_TICKETS].view(torch.int32).any().cpu()), "a ticket was left behind"
    second = group_call(jobs, ws, reset=False)                # no zeroing in between: the slabs hold the first launch's partials
    for i, (g, w) in enumerate(zip(second, first)):
        assert_bits(g, w, f"second launch, job {i + 1}")
    assert not bool(ws.view[:4 * TN_TICKETS].view(torch.int32).any().cpu())


def test_reversed_table_gives_the_same_results():
    jobs, want = table()
    ws = garbage_ws(group_ws_bytes(jobs))
    got = group_call(jobs[::-1], ws, reset=True)[::-1]
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bits(g, w, f"reversed table, job {i + 1}")


def test_job_three_against_fp64():
    """Guards the equalities above against comparing a wrong result with itself.  Bound: tests/test_kernels_gpu.py's
    assert_every_element for an fp32 chain of K terms: 6 sigma of the rounding random walk 2^-24 sqrt(K), floor 1e-5,
    relative to max(|ref|, rms(ref))."""
    jobs, _ = table()
    ws = garbage_ws(group_ws_bytes(jobs))
    got = group_call(jobs, ws, reset=True)[2].cpu().double()
    j = jobs[2]
    ref = j.A_host.double().T @ j.B_host.double()
    tol = max(1e-5, 6 * 2.0 ** -24 * j.K ** 0.5) * torch.maximum(ref.abs(), torch.full_like(ref, float(ref.pow(2).mean().sqrt())))
    err = (got - ref).abs()
    assert bool((err <= tol).all()), f"worst {float((err / tol).max()):.2f} x tol (|err| {float(err.max()):.3e})"


def test_one_slice_job_writes_c_itself():
    """K <= 64: the job's own call is the unsliced gemm_tn_kernel, and so is its share of the group; beside a sliced job, and
    alone (a group without a sliced job needs no workspace)."""
    one, sliced = Job(7, 196, 132, 64), Job(8, 132, 68, 200)
    assert lib().acvae_gemm_tn_fused_plan(196, 132, 64, 1 << 30) == 1
    want = [one.own_call(), sliced.own_call()]
    ws = garbage_ws(group_ws_bytes([one, sliced]))
    got = group_call([one, sliced], ws, reset=True)
    assert_bits(got[0], want[0], "one slice, beside a sliced job")
    assert_bits(got[1], want[1], "sliced job beside it")
    assert group_ws_bytes([one]) == 0
    assert_bits(group_call([one], garbage_ws(0), reset=False)[0], want[0], "one slice, alone")
