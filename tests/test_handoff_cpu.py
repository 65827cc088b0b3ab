"""CPU: the test entry points of the cross-workgroup reductions (include/acvae_hip.h) refuse bad arguments before any launch,
and their plan queries - the dispatchers' own helpers - pin the decisions the composite drivers get at BASELINE configs[1]
(B = 32, E = H = A = 512, V = 5000, Tc = 21, S = 62 frames of encoder memory) and at the tests/test_model_gpu.py sizes."""
import ctypes

import __graft_entry__ as ge
from acvae_amd import _lib

SK_MAX_TILES, TN_TICKETS, CS_TICKETS = 1024, 256, 128


def lib():
    ge.build()
    return _lib.lib()


def cdiv(a, b):
    return (a + b - 1) // b


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_bad_arguments_are_refused_without_a_launch():
    l = lib()
    p = ctypes.c_void_p(16)                    # never dereferenced: every call below fails its checks first
    assert l.acvae_gemm_nt_dual_ws(None, 4, p, 4, 4, None, 0, None, 0, 0, None, p, 4, 4, 4, 0, None, 0, 1, None) == -1
    assert l.acvae_gemm_nt_dual_ws(p, 4, p, 4, 0, None, 0, None, 0, 0, None, p, 4, 4, 4, 0, None, 0, 1, None) == -1
    assert l.acvae_gemm_nt_dual_ws(p, 4, p, 4, 4, p, 4, None, 4, 4, None, p, 4, 4, 4, 0, None, 0, 1, None) == -1
    assert l.acvae_gemm_nt_dual_ws(p, 4, p, 4, 4, p, 4, p, 4, 0, None, p, 4, 4, 4, 0, None, 0, 1, None) == -1
    assert l.acvae_gemm_nt_dual_ws(p, 4, p, 4, 4, None, 0, None, 0, 0, None, p, 4, 0, 4, 0, None, 0, 1, None) == -1
    # a workspace smaller than the split-K layout is refused before the ticket reset
    assert l.acvae_gemm_nt_dual_ws(p, 4, p, 4, 4, None, 0, None, 0, 0, None, p, 4, 4, 4, 0, p, 4096, 1, None) == -4
    assert l.acvae_gemm_nt_pair_c(None, 4, p, 4, 4, None, p, 4, 4, 0, p, 4, p, 4, 4, None, p, 4, 4, 0, 4, None) == -1
    assert l.acvae_gemm_nt_pair_c(p, 4, p, 4, 4, None, p, 4, 4, 0, p, 4, p, 4, 4, None, p, 4, 4, 0, 65, None) == -1
    assert l.acvae_gemm_nt_pair_c(p, 4, p, 4, 4, None, p, 4, 0, 0, p, 4, p, 4, 4, None, p, 4, 4, 0, 4, None) == -1
    assert l.acvae_gemm_tn_fused_c(None, 4, p, 4, p, 4, 4, 4, 4, 0, p, 1 << 20, 1, None) == -1
    assert l.acvae_gemm_tn_fused_c(p, 4, p, 4, p, 4, 4, 4, 0, 0, p, 1 << 20, 1, None) == -1
    x = (ctypes.c_void_p * 2)(16, 16)
    assert l.acvae_colsum_batch(2, None, ints([4, 4]), ints([8, 8]), x, None, p, 1 << 20, 1, None) == -1
    assert l.acvae_colsum_batch(2, x, ints([4, 0]), ints([8, 8]), x, None, p, 1 << 20, 1, None) == -1
    assert l.acvae_colsum_batch(2, x, ints([4, 4]), ints([8, 8]), x, None, None, 1 << 20, 1, None) == -1
    assert l.acvae_colsum_batch(7, x, ints([4] * 7), ints([8] * 7), x, None, p, 1 << 20, 1, None) == -1     # table holds 6
    assert l.acvae_colsum_batch(0, x, None, None, x, None, p, 1 << 20, 1, None) == -1
    x_null = (ctypes.c_void_p * 2)(16, None)
    assert l.acvae_colsum_batch(2, x_null, ints([4, 4]), ints([8, 8]), x, None, p, 1 << 20, 1, None) == -1
    # scratch below what the largest single job needs (one-launch-per-job fallback): refused
    assert l.acvae_colsum_batch(2, x, ints([4, 4]), ints([8, 8]), x, None, p, 64 * 8, 1, None) == -4
    assert l.acvae_gemm_nt_split_plan(0, 4, 4, 0, 1) == -1 and l.acvae_gemm_nt_split_plan(4, 4, 4, -1, 1) == -1
    assert l.acvae_gemm_tn_fused_plan(4, 0, 4, 0) == -1
    assert l.acvae_gemm_tn_fused_workspace_bytes(4, 4, 0) == -1
    assert l.acvae_colsum_batch_plan(2, None, ints([8, 8]), 1 << 20) == -1
    assert l.acvae_colsum_batch_workspace_bytes(0, None, None) == -1


def test_plan_queries_at_documented_shapes():
    l = lib()
    assert l.acvae_gemm_nt_splitk_workspace_bytes() == (SK_MAX_TILES + SK_MAX_TILES * 1024) * 4
    # skinny: 0 = the 128-row tile kernel; S = min(128 / tiles, Ktot / 256, 8) for <= 16 tiles and Ktot >= 1024
    for K, S in ((1023, 1), (1024, 4), (1280, 5), (1536, 6), (1792, 7), (2048, 8), (4096, 8)):
        assert l.acvae_gemm_nt_split_plan(32, 512, K, 0, 1) == S, K
    assert l.acvae_gemm_nt_split_plan(32, 512, 4096, 0, 0) == 1               # no workspace: no split
    assert l.acvae_gemm_nt_split_plan(32, 544, 4096, 0, 1) == 1               # 17 tiles
    assert l.acvae_gemm_nt_split_plan(1, 32, 4096, 0, 1) == 8
    assert l.acvae_gemm_nt_split_plan(32, 512, 1024, 1024, 1) == 8            # dual: Ktot = K1 + K2
    assert l.acvae_gemm_nt_split_plan(672, 5000, 512, 0, 1) == 0              # 240 blocks of 128 x 128
    assert l.acvae_gemm_nt_split_plan(8192, 512, 512, 0, 1) == 0
    assert l.acvae_gemm_nt_split_plan(8192, 512, 512, 512, 1) == 1            # the dual form is always the 32x32 kernel
    # fused TN: the slices launched, 1 = acvae_gemm_tn without a workspace
    full = l.acvae_gemm_tn_fused_workspace_bytes
    assert l.acvae_gemm_tn_fused_plan(128, 128, 100000, full(128, 128, 100000)) == 250
    assert full(128, 128, 100000) == TN_TICKETS * 4 + 256 * 128 * 128 * 4
    assert l.acvae_gemm_tn_fused_plan(64, 576, 4096, full(64, 576, 4096)) == 43
    assert l.acvae_gemm_tn_fused_plan(5000, 512, 672, 1 << 40) == 1 and full(5000, 512, 672) == 0
    assert l.acvae_gemm_tn_fused_plan(512, 512, 672, full(512, 512, 672)) == 11
    assert l.acvae_gemm_tn_fused_plan(512, 512, 672, full(512, 512, 672) - 4) == 1
    assert l.acvae_gemm_tn_fused_plan(512, 512, 672, 0) == 1
    # column sums: one launch unless one job, more than 128 column blocks, or too little scratch
    P, W = ints([4097, 2000, 10, 672]), ints([64, 130, 1, 512])
    nb = l.acvae_colsum_batch_workspace_bytes(4, P, W)
    assert nb == (CS_TICKETS // 2 + 64 * 64 + 32 * 130 + 10 * 1 + 16 * 512) * 8     # R = cs_groups(P): 64, 32, P, 16
    assert l.acvae_colsum_batch_plan(4, P, W, nb) == 1 and l.acvae_colsum_batch_plan(4, P, W, nb - 8) == 0
    assert l.acvae_colsum_batch_plan(1, ints([1025]), ints([300]), 1 << 30) == 0
    assert l.acvae_colsum_batch_plan(2, ints([100, 50]), ints([8192, 100]), 1 << 30) == 0      # 130 column blocks
    assert l.acvae_colsum_batch_plan(2, ints([100, 50]), ints([8128, 64]), 1 << 30) == 1       # 128


def driver_shapes(B, E, V, Tc, S, Eenc=None):
    """(call site in acvae_amd/csrc/decoder.hip, M, N, K1, K2) of the NT products the decode / posterior drivers issue with a split-K
    workspace, and (line, M, N, K) of their fused TN weight gradients, for one-layer posterior, H = A = Hp = Hq = E."""
    H = A = Hp = Hq = E
    R, NS = B * Tc, B * S
    Eenc = Eenc or E
    nt = [("334/350 posterior gi", R, 3 * Hq, E, 0), ("354 posterior gh", B, 3 * Hq, Hq, 0),
          ("366 posterior ml", R, 2 * E, 2 * Hq, 0), ("429 posterior dhid", R, 2 * Hq, 2 * E, 0),
          ("449 posterior BPTT dh", B, Hq, 3 * Hq, 0), ("525 posterior dx", R, E, 3 * Hq, 0),
          ("644 ln", NS, E, Eenc, 0), ("648 encproj prior", NS, E, E, 0), ("651 encproj dec", NS, A, E, 0),
          ("663 prior query", R, E, E, 0), ("669 prior gates", R, 4 * Hp, 2 * E, 0),
          ("683 prior step (dual)", B, 4 * Hp, E, Hp), ("688 prior ml", B, 2 * E, Hp, 0),
          ("710 dec_pre, two calls", R, 3 * H, E, 0), ("729 dec query", B, A, H, 0), ("730 dec gh", B, 3 * H, H, 0),
          ("735 dec gi", B, 3 * H, E, 0), ("761 classifier", R, V, H, 0), ("838 p_means_utt", B, 2 * E, H, 0),
          ("928 dhid", B, H, 2 * E, 0), ("931 d_out", R, H, V, 0), ("992 dctx", B, E, 3 * H, 0),
          ("998 BPTT dh (dual)", B, H, 3 * H, A), ("1005 dmem", NS, E, A, 0), ("1012/1036 dz, demb", R, E, 3 * H, 0),
          ("1083 prior dhp", B, Hp, 2 * E, 0), ("1087 prior dhp2", B, Hp, 4 * Hp, 0), ("1088 prior dlz", B, E, 4 * Hp, 0),
          ("1099 prior drnn", R, 2 * E, 4 * Hp, 0), ("1106 prior dmem", NS, E, E, 0), ("1120 prior dqp", R, E, E, 0),
          ("1180 ln bwd", NS, Eenc, E, 0)]
    tn = [("433 posterior ml", 2 * E, 2 * Hq, R), ("493 stacked ih", 3 * Hq, 2 * Hq, R), ("495/523 whh", 3 * Hq, Hq, R),
          ("521 wih", 3 * Hq, E, R), ("936 mlo", 2 * E, H, B), ("943 classifier", V, H, R), ("1024 dec wih", 3 * H, 3 * E, R),
          ("1025 dec whh", 3 * H, H, R), ("1033 dec att q", A, H, R), ("1034 dec att mem", A, E, NS),
          ("1110 prior ml", 2 * E, Hp, R), ("1111 prior wih", 4 * Hp, 3 * E, R), ("1112 prior whh", 4 * Hp, Hp, R),
          ("1121 prior att q", E, E, R), ("1122 prior att mem", E, E, NS), ("1181 ln", E, Eenc, NS)]
    return nt, tn


def check_bounds(nt, tn):
    l = lib()
    sk, tns = {}, {}
    for what, M, N, K1, K2 in nt:
        S = l.acvae_gemm_nt_split_plan(M, N, K1, K2, 1)
        assert S >= 0, what
        if S > 1:                                  # S = 1 leaves the workspace alone
            assert cdiv(M, 32) * cdiv(N, 32) * S <= SK_MAX_TILES, what
        sk[what] = S
    for what, M, N, K in tn:
        s = l.acvae_gemm_tn_fused_plan(M, N, K, l.acvae_gemm_tn_fused_workspace_bytes(M, N, K))
        narrow = M <= 64
        if s > 1:
            assert cdiv(M, 64 if narrow else 128) * cdiv(N, 256 if narrow else 128) <= TN_TICKETS, what
        tns[what] = s
    return sk, tns


def test_configs1_plans_are_pinned_and_within_the_ticket_tables():
    """The decisions of the dispatchers at BASELINE configs[1]: a change of S, of the slice counts or of the kernel choice
    shows here (and so does a refactor of the plan helpers that drifts from the code it came from)."""
    sk, tn = check_bounds(*driver_shapes(32, 512, 5000, 21, 62))
    split = {k: v for k, v in sk.items() if v != 1}
    assert split == {"449 posterior BPTT dh": 6, "761 classifier": 0, "928 dhid": 4, "992 dctx": 6, "998 BPTT dh (dual)": 8,
                     "1083 prior dhp": 4, "1087 prior dhp2": 8, "1088 prior dlz": 8}, split
    assert tn == {"433 posterior ml": 4, "493 stacked ih": 2, "495/523 whh": 5, "521 wih": 5, "936 mlo": 1,
                  "943 classifier": 1, "1024 dec wih": 1, "1025 dec whh": 5, "1033 dec att q": 11, "1034 dec att mem": 16,
                  "1110 prior ml": 7, "1111 prior wih": 1, "1112 prior whh": 4, "1121 prior att q": 11,
                  "1122 prior att mem": 16, "1181 ln": 16}, tn


def test_model_test_sizes_stay_within_the_ticket_tables():
    # tests/test_model_gpu.py: V, E, B, Tt, L = 40, 64, 3, 96, 6 and 60, 64, 4, 96, 8 (S = Tt / 16 frames); smoke: 52, 64, 3
    for V, B, L, S in ((40, 3, 6, 6), (60, 4, 8, 6), (52, 3, 7, 4)):
        check_bounds(*driver_shapes(B, 64, V, L - 1, S))
