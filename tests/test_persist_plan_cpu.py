"""CPU: the plans of the persistent launches (acvae_amd/csrc/persist_plan.h: role counts, grid, LDS, counters and hand-off
scratch of the decode forward, the decode BPTT and the posterior BiGRU as pure functions of the dims).  A small C++ driver is
built against the header with ROCm's host compiler (no HIP) and checks, over a sweep of shapes, what the kernels and the
workspace layouts rely on, then literal values recorded from the functions the plans replaced (printed by a scratch build of the
commit before the plans: never taken from the header under test) and cross-checks worked by hand from those formulas.
The second test pins the workspace sizes of the C ABI, which the layouts now read from the plans, to the numbers the library
returned before."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acvae_amd", "csrc")
CXX = "/opt/rocm/llvm/bin/clang++"

DRIVER = r"""
#include <cstdio>
#include "persist_plan.h"
using namespace acvae;

static int failures = 0;
static int cur[6];
#define CHECK(c) do { if (!(c)) { if (++failures < 40) std::printf("line %d (N %d Tc %d S %d E %d H %d A %d): %s\n", __LINE__, \
    cur[0], cur[1], cur[2], cur[3], cur[4], cur[5], #c); } } while (0)

static void counters(long words, long abort_index, int roles, int Tc) {
  CHECK(words % 4 == 0 && words >= (long)roles * Tc + 1);
  CHECK(abort_index == (long)roles * Tc && abort_index < words && words - abort_index <= 4);   // the last counted word
}

static void properties(int N, int Tc, int S, int E, int H, int A) {
  const int dims[6] = {N, Tc, S, E, H, A};
  for (int k = 0; k < 6; ++k) cur[k] = dims[k];
  for (int res = 0; res < 2; ++res) {
    const PdPlan f = decode_fwd_plan(N, Tc, S, E, H, A, res != 0);
    CHECK(f.N == N && f.Tc == Tc && f.S == S && f.E == E && f.H == H && f.A == A);
    // decode_persist_kernel dispatches blockIdx.x on n_d1 | N | n_d3 | n_p1 | n_p2; the readers of D1 wait for A/32 and 3H/32 tiles
    CHECK(f.grid == f.n_d1 + N + f.n_d3 + f.n_p1 + f.n_p2);
    CHECK(f.n_d1 == A / 32 + 3 * H / 32 && f.n_d3 == H / 16 && f.n_p1 == E / 8 && f.n_p2 == E / 16);
    counters(f.counter_words, f.abort_index, PD_C_COUNT, Tc);
    if (!res) CHECK(f.att_resident == 0);
    if (f.shape_ok) {
      CHECK(f.shm >= PD_SMEM_BYTES && f.shm >= att_lds_bytes(pd_att_floats(S, A, f.att_resident != 0)));
      CHECK((long)f.shm <= PERSIST_LDS_MAX);
      CHECK(pd_att_part_off(S) >= S + 16 && pd_att_part_off(S) % 4 == 0);      // scores, 16 reduction words, aligned partials
      CHECK(PD_ATT_PART_FLOATS >= (1024 / (E / 4)) * E);
      if (f.att_resident) CHECK(S <= 8 * (1024 / (E / 4)));                      // 8 register slots per context group
    }
  }
  const PbPlan b = decode_bwd_plan(N, Tc, S, E, H, A);
  CHECK(b.N == N && b.Tc == Tc && b.S == S && b.E == E && b.H == H && b.A == A);
  // decode_persist_bwd_kernel dispatches on n_ra | n_rb | N * rc_splits | n_pa | n_pb
  CHECK(b.grid == b.n_ra + b.n_rb + N * b.rc_splits + b.n_pa + b.n_pb);
  CHECK(b.n_ra == H / 32 && b.n_rb == (E / 32) * b.ks_rb && b.n_pa == (E / 16) * b.ks_pa && b.n_pb == E / 32);
  CHECK(b.ks_rb >= 1 && b.ks_rb <= PB_KS_MAX && b.ks_pa >= 1 && b.ks_pa <= 2);   // RC sums four partials, PB two
  CHECK((3 * H) % b.ks_rb == 0 && (4 * E) % b.ks_pa == 0);
  counters(b.counter_words, b.abort_index, PB_C_COUNT, Tc);
  // the three hand-off regions: inside the scratch, in this order, each with room for its ks x N x width floats
  CHECK(b.dctx_part_off >= 0 && b.dctx_part_off + (long)b.ks_rb * N * E <= b.dhp_part_off);
  CHECK(b.dhp_part_off + (long)b.ks_pa * N * E <= b.dml_part_off);
  CHECK(b.dml_part_off + (long)b.ks_pa * N * 2 * E <= b.part_floats);
  CHECK(b.rc_splits * 64 >= S && (b.rc_splits - 1) * 64 < S);
  if (S <= 192) {
    CHECK((b.dqd_part_floats == 0) == (b.rc_splits == 1));
    if (b.rc_splits > 1) CHECK(b.dqd_part_floats == (long)b.rc_splits * N * Tc * A);
    CHECK(b.dv_rows <= b.dv_rows_max);
  } else {
    CHECK(!b.shape_ok && b.dqd_part_floats == 0);      // no such launch: nothing reserved
  }
  CHECK(b.dv_rows == N * b.rc_splits);
  CHECK(b.shm >= PB_SMEM_BYTES && b.shm >= att_lds_bytes(pb_att_floats(S < 64 ? S : 64, A)));
  if (b.shape_ok) {
    CHECK(decode_fwd_plan(N, Tc, S, E, H, A, false).shape_ok && H == E && E <= 512 && A <= 512);
    CHECK((long)b.shm <= PERSIST_LDS_MAX && b.dv_rows <= b.dv_rows_max);
  }
  const PqPlan q = posterior_plan(N, Tc, E);
  CHECK(q.N == N && q.Tc == Tc && q.Hq == E && q.grid == 2 * (E / 32) && q.shm >= PQ_SMEM_BYTES);
  CHECK(q.hbuf_floats == 4L * N * E);
  counters(q.counter_words, q.abort_index, 2, Tc);
}

// ---- values of the replaced functions, printed by a scratch build of the commit before the plans
struct FwdRow { int ok, grid; long shm; int att_resident; long words; };
struct BwdRow { int ok, ks_rb, ks_pa, rc_splits, grid; long shm, words, part_floats, dqd_floats; };
struct Row { int d[6]; FwdRow res, str; BwdRow b; };
static const Row recorded[] = {
  {{32, 21, 62, 512, 512, 512}, {1, 224, 143696, 1, 128}, {1, 224, 38020, 0, 128}, {1, 3, 2, 1, 176, 131600, 108, 262144, 0}},
  {{16, 21, 187, 512, 512, 512}, {1, 208, 38020, 0, 128}, {1, 208, 38020, 0, 128}, {1, 3, 2, 3, 192, 135696, 108, 131072, 516096}},
  {{5, 8, 12, 512, 512, 512}, {1, 197, 41088, 1, 52}, {1, 197, 38020, 0, 52}, {1, 3, 2, 1, 149, 33796, 44, 40960, 0}},
  {{3, 6, 4, 64, 64, 64}, {1, 27, 38020, 1, 40}, {1, 27, 38020, 0, 40}, {1, 1, 1, 1, 13, 33796, 32, 3072, 0}},
  {{17, 11, 20, 128, 128, 128}, {1, 65, 38020, 1, 68}, {1, 65, 38020, 0, 68}, {1, 1, 1, 1, 37, 33796, 56, 34816, 0}},
  {{4, 5, 4, 2048, 2048, 2048}, {1, 772, 49248, 1, 32}, {1, 772, 38020, 0, 32}, {0, 1, 1, 1, 324, 37392, 28, 131072, 0}},
  {{2, 4, 64, 512, 512, 512}, {1, 194, 147792, 1, 28}, {1, 194, 38020, 0, 28}, {1, 3, 2, 1, 146, 135696, 24, 16384, 0}},
  {{2, 4, 66, 512, 512, 512}, {1, 194, 38020, 0, 28}, {1, 194, 38020, 0, 28}, {1, 3, 2, 2, 148, 135696, 24, 16384, 8192}},
  {{32, 21, 65, 512, 512, 512}, {1, 224, 38020, 0, 128}, {1, 224, 38020, 0, 128}, {1, 3, 2, 2, 208, 135696, 108, 262144, 688128}},
  {{1, 1, 1, 32, 32, 32}, {1, 13, 38020, 1, 8}, {1, 13, 38020, 0, 8}, {1, 1, 1, 1, 6, 33796, 8, 512, 0}},
  {{33, 21, 62, 512, 512, 512}, {0, 225, 143696, 1, 128}, {0, 225, 38020, 0, 128}, {0, 3, 2, 1, 177, 131600, 108, 270336, 0}},
  {{16, 21, 193, 512, 512, 512}, {1, 208, 38020, 0, 128}, {1, 208, 38020, 0, 128}, {0, 3, 2, 4, 208, 135696, 108, 131072, 0}},
  {{8, 6, 513, 512, 512, 512}, {0, 200, 38020, 0, 40}, {0, 200, 38020, 0, 40}, {0, 3, 2, 9, 216, 135696, 32, 65536, 0}},
  {{8, 21, 128, 1024, 1024, 1024}, {1, 392, 38020, 0, 128}, {1, 392, 38020, 0, 128}, {0, 1, 1, 2, 176, 266768, 108, 131072, 344064}},
  {{8, 21, 100, 256, 256, 128}, {1, 100, 68064, 1, 128}, {1, 100, 38020, 0, 128}, {1, 1, 1, 2, 56, 37392, 108, 32768, 43008}},
  {{8, 21, 100, 256, 512, 256}, {1, 144, 119264, 1, 128}, {1, 144, 38020, 0, 128}, {0, 3, 1, 2, 80, 70160, 108, 32768, 86016}},
  {{7, 3, 192, 512, 512, 512}, {1, 199, 38020, 0, 20}, {1, 199, 38020, 0, 20}, {1, 3, 2, 3, 165, 135696, 16, 57344, 32256}},
  {{32, 21, 512, 64, 64, 64}, {1, 56, 149584, 1, 128}, {1, 56, 38020, 0, 128}, {0, 1, 1, 8, 266, 33796, 108, 32768, 0}},
  {{32, 21, 16, 2048, 2048, 2048}, {1, 800, 147600, 1, 128}, {1, 800, 38020, 0, 128}, {0, 1, 1, 1, 352, 135696, 108, 1048576, 0}},
  {{8, 21, 40, 512, 512, 96}, {1, 187, 38020, 1, 128}, {1, 187, 38020, 0, 128}, {1, 3, 2, 1, 152, 33796, 108, 65536, 0}},
  {{8, 21, 62, 48, 64, 64}, {0, 29, 38020, 1, 128}, {0, 29, 38020, 0, 128}, {0, 1, 1, 1, 15, 33796, 108, 6144, 0}},
};
struct PostRow { int d[3]; int ok, grid; long shm, words; };
static const PostRow recorded_post[] = {
  {{32, 21, 512}, 1, 32, 33796, 44}, {{32, 21, 544}, 0, 34, 33796, 44}, {{32, 21, 48}, 0, 2, 33796, 44},
  {{33, 21, 512}, 0, 32, 33796, 44}, {{1, 1, 32}, 1, 2, 33796, 4},      {{3, 6, 64}, 1, 4, 33796, 16},
  {{17, 11, 128}, 1, 8, 33796, 24},  {{4, 5, 256}, 1, 16, 33796, 12},   {{8, 0, 512}, 0, 32, 33796, 4},
};

static void check_fwd(const PdPlan& f, const FwdRow& r) {
  CHECK((int)f.shape_ok == r.ok && f.grid == r.grid && f.counter_words == r.words);
  if (r.ok) CHECK((long)f.shm == r.shm && f.att_resident == r.att_resident);   // (the geometry of a refused shape means nothing)
}

int main() {
  // PdSmem / PbSmem / PqSmem of decode_persist.hip (static_asserts there tie the structs to these)
  CHECK(PD_SMEM_BYTES == 38020 && PB_SMEM_BYTES == 33796 && PQ_SMEM_BYTES == 33796);
  CHECK(PB_ATT_LDS.w == 0 && PB_ATT_LDS.ds == 64 && PB_ATT_LDS.dwred == 128 && PB_ATT_LDS.dc == 640 && PB_ATT_LDS.pl == 1152);

  const int Ns[] = {1, 3, 17, 32, 33}, Tcs[] = {1, 6, 21}, Ss[] = {1, 4, 62, 64, 65, 128, 187, 192, 193, 512, 513};
  const int Es[] = {32, 64, 128, 512, 1024, 2048};
  const int mixed[][3] = {{256, 256, 128}, {256, 512, 256}, {512, 512, 96}, {512, 256, 512}, {512, 512, 1024}, {128, 128, 512}};   // E, H, A
  for (int N : Ns) for (int Tc : Tcs) for (int S : Ss) {
    for (int E : Es) properties(N, Tc, S, E, E, E);
    for (auto& m : mixed) properties(N, Tc, S, m[0], m[1], m[2]);
  }

  for (const Row& r : recorded) {
    for (int k = 0; k < 6; ++k) cur[k] = r.d[k];
    const int N = r.d[0], Tc = r.d[1], S = r.d[2], E = r.d[3], H = r.d[4], A = r.d[5];
    check_fwd(decode_fwd_plan(N, Tc, S, E, H, A, true), r.res);
    check_fwd(decode_fwd_plan(N, Tc, S, E, H, A, false), r.str);
    const PbPlan b = decode_bwd_plan(N, Tc, S, E, H, A);
    CHECK((int)b.shape_ok == r.b.ok && b.ks_rb == r.b.ks_rb && b.ks_pa == r.b.ks_pa && b.rc_splits == r.b.rc_splits);
    CHECK(b.grid == r.b.grid && (long)b.shm == r.b.shm && b.counter_words == r.b.words);
    CHECK(b.part_floats == r.b.part_floats && b.dqd_part_floats == r.b.dqd_floats);
    // acvae_decode_bwd used to carve the scratch up as 4 N E | 4 N E | 8 N E, and the layout reserved 3 N rows of dvpart
    CHECK(b.dctx_part_off == 0 && b.dhp_part_off == 4L * N * E && b.dml_part_off == 8L * N * E && b.dv_rows_max == 3 * N);
  }
  for (const PostRow& r : recorded_post) {
    cur[0] = r.d[0]; cur[1] = r.d[1]; cur[2] = 0; cur[3] = r.d[2]; cur[4] = cur[5] = 0;
    const PqPlan q = posterior_plan(r.d[0], r.d[1], r.d[2]);
    CHECK((int)q.shape_ok == r.ok && q.grid == r.grid && (long)q.shm == r.shm && q.counter_words == r.words);
  }

  // ---- worked by hand from the replaced formulas, E = H = A, Tc = 21
  for (int k = 0; k < 6; ++k) cur[k] = 0;
  auto fwd = [](int E, int N, int S, bool res) { return decode_fwd_plan(N, 21, S, E, E, E, res); };
  auto bwd = [](int E, int N, int S) { return decode_bwd_plan(N, 21, S, E, E, E); };
  CHECK(fwd(512, 32, 62, true).grid == 224 && fwd(64, 3, 4, true).grid == 27 && fwd(128, 17, 20, true).grid == 65);
  CHECK(fwd(2048, 4, 4, true).grid == 772);
  CHECK(fwd(512, 32, 62, true).att_resident == 1 && fwd(512, 32, 64, true).att_resident == 1);
  CHECK(fwd(512, 32, 65, true).att_resident == 0 && fwd(512, 32, 187, true).att_resident == 0);
  CHECK(fwd(512, 32, 65, true).shape_ok && fwd(512, 32, 187, true).shape_ok);
  {
    const PbPlan b = bwd(512, 32, 62);
    CHECK(b.shape_ok && b.ks_rb == 3 && b.ks_pa == 2 && b.rc_splits == 1 && b.grid == 176 && b.part_floats == 262144);
  }
  CHECK(bwd(512, 16, 187).shape_ok && bwd(512, 16, 187).rc_splits == 3 && bwd(512, 16, 187).grid == 192);
  CHECK(bwd(64, 3, 4).shape_ok && bwd(64, 3, 4).grid == 13);
  CHECK(bwd(128, 17, 20).shape_ok && bwd(128, 17, 20).grid == 37);
  CHECK(!bwd(2048, 4, 4).shape_ok && !bwd(512, 16, 193).shape_ok && !decode_bwd_plan(8, 21, 62, 512, 256, 512).shape_ok);
  CHECK(fwd(512, 32, 62, true).counter_words == 128 && bwd(512, 32, 62).counter_words == 108);
  CHECK(posterior_plan(32, 21, 512).counter_words == 44);
  CHECK(posterior_plan(32, 21, 512).shape_ok && posterior_plan(32, 21, 512).grid == 32);
  CHECK(!posterior_plan(32, 21, 544).shape_ok && !posterior_plan(32, 21, 48).shape_ok && !posterior_plan(33, 21, 512).shape_ok);

  if (failures == 0) std::printf("ok\n");
  else std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.fail(f"{CXX} not found: the ROCm host compiler is needed to build the plan driver")
    d = tmp_path_factory.mktemp("persist_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def test_plans_hold_what_the_kernels_and_layouts_rely_on(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# (N, Tc, S, E = H = A, V, Eenc, Hq): the shapes of tests/test_decode_persist_gpu.py (S = frames / 16, Tc = L - 1), S = 64 / 66 of its
# changing-shape test, a clip too long for the persistent BPTT and a width it does not take.  Per row: acvae_decode_saved_bytes,
# _scratch_bytes, _saved_lse_offset, then acvae_posterior_stack_saved_bytes / _scratch_bytes for num_layers = 1 and 3 - all as
# returned by the library built from the commit before the layouts read the plans.
SIZES = [
    ((32, 21, 62, 512, 5000, 512, 512), [89386240, 241794816, 41263104], [[18027776, 139927040], [51057920, 162078720]]),
    ((16, 21, 187, 512, 5000, 512, 512), [81144064, 228756224, 33087744], [[9014016, 122396160], [25529088, 142909440]]),
    ((5, 8, 12, 512, 300, 512, 512), [40475904, 14542080, 2091520], [[1085952, 27323904], [3052032, 46444032]]),
    ((3, 6, 4, 64, 50, 512, 64), [711680, 8945152, 106752], [[61696, 4996608], [172288, 5306880]]),
    ((17, 11, 20, 128, 200, 512, 128), [5029888, 25903872, 2549504], [[1263616, 11728896], [3561472, 13563136]]),
    ((32, 21, 25, 512, 500, 512, 512), [72796416, 211048192, 33889280], [[18027776, 139927040], [51057920, 162078720]]),
    ((4, 5, 4, 2048, 60, 2048, 256), [608372224, 39139328, 3834624], [[418048, 44006912], [909568, 48799232]]),
    ((2, 4, 64, 512, 50, 512, 512), [38992896, 17613824, 1132800], [[221440, 25624064], [614656, 44563968]]),
    ((2, 4, 66, 512, 50, 512, 512), [39017728, 19817984, 1157632], [[221440, 25624064], [614656, 44563968]]),
    ((16, 21, 193, 512, 5000, 512, 512), [81742080, 228936448, 33685760], [[9014016, 122396160], [25529088, 142909440]]),
    ((8, 21, 128, 2048, 5000, 2048, 512), [699226880, 148560384, 54154752], [[5539328, 107257344], [13796864, 152117248]]),
]


def test_workspace_sizes_are_what_they_were():
    import __graft_entry__ as ge
    from acvae_amd import _lib
    ge.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    names = ("acvae_decode_saved_bytes", "acvae_decode_scratch_bytes", "acvae_decode_saved_lse_offset",
             "acvae_posterior_stack_saved_bytes", "acvae_posterior_stack_scratch_bytes")
    for n in names:
        getattr(so, n).restype = ctypes.c_int64
    for (N, Tc, S, E, V, Eenc, Hq), dec, post in SIZES:
        got = [getattr(so, n)(N, Tc, S, E, E, E, V, Eenc) for n in names[:3]]
        assert got == dec, ((N, Tc, S, E), got, dec)
        for NL, want in zip((1, 3), post):
            got = [getattr(so, n)(N, Tc, E, Hq, V, NL) for n in names[3:]]
            assert got == want, ((N, Tc, E, Hq, NL), got, want)


def test_width_sets_meant_for_a_persistent_launch_are_taken_by_the_plans():
    """The training width sets of tests/widths_util.py (A != E) that tests/test_text_widths_gpu.py means for the persistent
    decode launches: the forward and BPTT plans take them, with the role counts, K-splits and d qd shares the sets are
    there for; the two whose A is no multiple of 32 are refused (per-step paths).  Likewise the posterior widths."""
    import widths_util as W
    want = {  # name: (n_d1 = A/32 + 3H/32, ks_rb, ks_pa, rc_splits)
        "E64_A32": (1 + 6, 1, 1, 1), "E64_A160": (5 + 6, 1, 1, 1), "E128_A96": (3 + 12, 1, 1, 1),
        "E64_A160_T1056": (5 + 6, 1, 1, 2), "E512_A256": (8 + 48, 3, 2, 1)}
    assert set(want) == set(W.TRAIN_PERSISTENT)
    for name in W.TRAIN_SETS:
        B, T, V, E, A, S, Tc = W.train_dims(name)
        p = W.plans(B, Tc, S, E, E, A, E)
        if name in W.TRAIN_PERSISTENT:
            assert p["fwd_ok"] and p["bwd_ok"] and p["post_ok"], (name, p)
            assert (p["fwd_n_d1"], p["ks_rb"], p["ks_pa"], p["rc_splits"]) == want[name], (name, p)
            assert p["dqd_part_floats"] == (p["rc_splits"] * B * Tc * A if p["rc_splits"] > 1 else 0), (name, p)
        else:
            assert A % 32 != 0 and not p["fwd_ok"] and not p["bwd_ok"] and p["post_ok"], (name, p)
    for E, H, A in W.INFER_SETS:                       # H != E: no persistent BPTT (a rollout's backward goes per step)
        assert not W.plans(3, 6, 4, E, H, A, E)["bwd_ok"], (E, H, A)
    for (E, Hq), ok in zip(W.POSTERIOR_SETS, (1, 1, 1, 1, 0)):
        for N in (5, 32, 33):
            assert W.plans(N, 6, 4, 64, 64, 64, Hq)["post_ok"] == (ok and N <= 32), (E, Hq, N)
