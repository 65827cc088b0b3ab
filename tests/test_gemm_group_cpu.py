"""CPU: acvae_gemm_tn_group_c (several TN products in one launch, include/acvae_hip.h) refuses a bad table before any HIP
call, and its workspace query is the sum over the sliced jobs - all jobs of a launch are live at once."""
import ctypes

import __graft_entry__ as ge
from acvae_amd import _lib

EINVAL, EWORKSPACE = -1, -4
TN_TICKETS, CAPACITY = 256, 8


def lib():
    ge.build()
    return _lib.lib()


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def longs(v):
    return (ctypes.c_int64 * len(v))(*v)


def ptrs(v):
    return (ctypes.c_void_p * len(v))(*v)


def call(M, N, K, ws_bytes, A=None, lda=None, ws=16, n=None):
    """Every pointer is 16: never dereferenced, because each call here fails its checks first."""
    k = len(M)
    return lib().acvae_gemm_tn_group_c(k if n is None else n, ptrs([16] * k) if A is None else A,
                                       longs(M) if lda is None else lda, ptrs([16] * k), longs(N), ptrs([16] * k), longs(N),
                                       ints(M), ints(N), ints(K), ctypes.c_void_p(ws) if ws else None, ws_bytes, 1, None)


def test_the_entry_and_its_query_are_exported():
    l = lib()
    assert hasattr(l, "acvae_gemm_tn_group_c") and hasattr(l, "acvae_gemm_tn_group_workspace_bytes")
    assert "acvae_gemm_tn_group_c" in _lib.PROTOS and "acvae_gemm_tn_group_workspace_bytes" in _lib.PROTOS


def test_workspace_query():
    q = lib().acvae_gemm_tn_group_workspace_bytes
    # (512, 512, 672): 11 slices; (1536, 1536, 672): 144 tiles, one slice, no slab
    assert q(2, ints([512, 1536]), ints([512, 1536]), ints([672, 672])) == 4 * (TN_TICKETS + 11 * 512 * 512)
    assert q(2, ints([512, 512]), ints([512, 512]), ints([672, 1984])) == 4 * (TN_TICKETS + (11 + 16) * 512 * 512)
    assert q(1, ints([1536]), ints([1536]), ints([672])) == 0
    assert q(0, ints([512]), ints([512]), ints([672])) == -1
    assert q(1, None, ints([512]), ints([672])) == -1
    assert q(1, ints([48]), ints([512]), ints([672])) == -1                    # the 64 x 256 tile: not a group's
    assert q(CAPACITY + 1, ints([512] * 9), ints([512] * 9), ints([672] * 9)) == -1
    # 4 x (1024, 1024, 672): 64 tiles of 4 slices each, all 256 tickets; a fifth does not fit
    assert q(4, ints([1024] * 4), ints([1024] * 4), ints([672] * 4)) == 4 * (TN_TICKETS + 4 * 4 * 1024 * 1024)
    assert q(5, ints([1024] * 5), ints([1024] * 5), ints([672] * 5)) == -1


def test_bad_tables_are_refused_without_a_launch():
    M, N, K = [512, 256], [512, 128], [672, 1984]
    need = lib().acvae_gemm_tn_group_workspace_bytes(2, ints(M), ints(N), ints(K))
    assert need > 0
    assert call(M, N, K, need, A=ptrs([16, None])) == EINVAL                  # a null operand
    assert lib().acvae_gemm_tn_group_c(2, None, longs(M), ptrs([16, 16]), longs(N), ptrs([16, 16]), longs(N), ints(M), ints(N),
                                       ints(K), ctypes.c_void_p(16), need, 1, None) == EINVAL
    assert call(M, N, K, need, n=0) == EINVAL and call(M, N, K, need, n=-1) == EINVAL
    assert call([512, 0], N, K, need) == EINVAL and call(M, N, [672, 0], need) == EINVAL and call(M, [512, -4], K, need) == EINVAL
    assert call([512] * 9, [512] * 9, [672] * 9, 1 << 40) == EINVAL           # the table holds 8
    assert call([512, 48], N, K, need) == EINVAL                              # M <= 64: not the 128 x 128 tile
    assert call([512, 130], [512, 128], K, need) == EINVAL                    # M not a multiple of 4: the scalar loader
    assert call(M, N, K, need, A=ptrs([16, 20])) == EINVAL                    # an operand that is not 16-byte aligned
    assert call(M, N, K, need, lda=longs([512, 258])) == EINVAL               # lda not a multiple of 4
    assert call(M, N, K, need - 4) == EWORKSPACE                              # one float short
    assert call(M, N, K, need, ws=None) == EWORKSPACE
    assert call([1024] * 5, [1024] * 5, [672] * 5, 1 << 40) == EWORKSPACE     # more sliced tiles than tickets
