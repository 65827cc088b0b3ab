// The pure part of the four persistent launches of decode_persist.hip (decode forward, decode BPTT, posterior forward and
// backward): ONE value per launch - a plan - that says, from the dims alone, whether the kernel takes the shape, how many
// workgroups play each role, the K-splits, the grid, the dynamic LDS, the arrival counters and the hand-off scratch.  The
// kernels dispatch on the plan's counts, the launchers launch its grid, the workspace layouts of decoder.hip reserve its sizes
// and the attention roles carve their LDS by the maps below: nothing is restated anywhere else.  No HIP in this header (it
// compiles with the plain host compiler: tests/test_persist_plan_cpu.py); whether a plan's grid is RESIDENT on a device is the
// launchers' question (decode_persist.h).
//
// Sizes (counter words, scratch floats) are filled for every shape, refused ones included, so that the workspace layouts stay
// a function of the dims; the geometry of a refused plan (shape_ok == false) means nothing.
#pragma once
#include <cstddef>

enum { PD_C_D1Q, PD_C_D1H, PD_C_D2, PD_C_D3, PD_C_P1, PD_C_P2, PD_C_COUNT };   // arrival counters: [role][step]
enum { PB_C_RA, PB_C_RB, PB_C_RC, PB_C_PA, PB_C_PB, PB_C_COUNT };

namespace acvae {

constexpr int PD_THREADS = 512;                 // threads of a workgroup of every persistent kernel: 8 wavefronts, as gemm_skinny_kernel
constexpr int PD_WAVES = PD_THREADS / 64;
constexpr int PD_U = 8;                         // K-groups of a wavefront's resident batch: K <= 64 PD_U stays in registers
constexpr long PERSIST_LDS_MAX = 150 * 1024;    // dynamic LDS a workgroup may ask for
// the roles' LDS structs (decode_persist.hip asserts the sizes): reduction tiles [PD_WAVES][32][33] (+ D3's [32][33]) and a flag
constexpr size_t PD_SMEM_BYTES = (size_t)(PD_WAVES * 32 * 33 + 32 * 33) * sizeof(float) + sizeof(int);
constexpr size_t PB_SMEM_BYTES = (size_t)(PD_WAVES * 32 * 33) * sizeof(float) + sizeof(int);
constexpr size_t PQ_SMEM_BYTES = PB_SMEM_BYTES;

constexpr long persist_counter_words(int counters, int Tc) { return ((long)counters * Tc + 1 + 3) & ~3L; }   // + the abort word

// The attention roles carve the dynamic LDS themselves: ATT_LDS_HEAD floats (the wait flag, in the first) and then the role's
// area, in floats from its start:
constexpr int ATT_LDS_HEAD = 4;
constexpr size_t att_lds_bytes(long area_floats) { return (size_t)(ATT_LDS_HEAD + area_floats) * sizeof(float); }
// forward (role_d2): S scores, from S on 16 words of the block reductions, then the context partials (1024 / (E/4) groups x E)
// and, memory-resident form only, encproj [S][A]
constexpr int PD_ATT_PART_FLOATS = 4096;
constexpr int pd_att_part_off(int S) { return (S + 16 + 3) & ~3; }
constexpr long pd_att_floats(int S, int A, bool resident) { return pd_att_part_off(S) + PD_ATT_PART_FLOATS + (resident ? (long)S * A : 0); }
// BPTT (role_rc): weights and d scores of the workgroup's (up to) 64 frames, the eight wave shares of dw [8][64], the step's
// dctx [512] and encproj of the frames [frames][A]
constexpr int PB_RC_FRAMES = 64;                // frames per attention workgroup (2 x 32 register slots)
constexpr int PB_RC_SPLITS_MAX = 3;             // ... and workgroups per clip: S <= 192 (BASELINE configs[3] has 187)
constexpr int PB_KS_MAX = 4;                    // cap of the K-splits (the reader sums four partials)
constexpr struct PbAttLds { int w, ds, dwred, dc, pl; } PB_ATT_LDS = {0, PB_RC_FRAMES, 2 * PB_RC_FRAMES, 2 * PB_RC_FRAMES + PD_WAVES * 64,
                                                                     2 * PB_RC_FRAMES + PD_WAVES * 64 + 512};
constexpr long pb_att_floats(int frames, int A) { return PB_ATT_LDS.pl + (long)frames * A; }

// ---------------------------------------------------------------------------------------------------- decode forward
struct PdPlan {
  bool shape_ok;
  int N, Tc, S, E, H, A;
  int n_d1, n_d3, n_p1, n_p2;      // workgroups per role (the attention role: N)
  int grid;
  size_t shm;
  int att_resident;                // the attention keeps its clip's memory on the CU (asked for AND possible at this shape)
  long counter_words, abort_index; // words at PdParams::cnt; the abort word is the last counted one
};
// resident: ask for the memory-resident attention form; plan.att_resident tells whether the shape has one
constexpr PdPlan decode_fwd_plan(int N, int Tc, int S, int E, int H, int A, bool resident) {
  PdPlan p{};
  p.N = N; p.Tc = Tc; p.S = S; p.E = E; p.H = H; p.A = A;
  p.abort_index = (long)PD_C_COUNT * Tc;
  p.counter_words = persist_counter_words(PD_C_COUNT, Tc);
  p.n_d1 = A / 32 + 3 * H / 32;
  p.n_d3 = H / 16;
  p.n_p1 = E / 8;
  p.n_p2 = E / 16;
  p.grid = p.n_d1 + N + p.n_d3 + p.n_p1 + p.n_p2;
  // one 32-row tile of clips; whole 32 / 16 / 8-wide slices and K-groups of 8; one score per thread in the softmax; E a
  // power of two so that the context groups of the per-step attention kernel (1024 / (E / 4)) can be replayed exactly
  p.shape_ok = N >= 1 && N <= 32 && Tc >= 1 && S >= 1 && S <= PD_THREADS && E >= 32 && E <= 2048 && (E & (E - 1)) == 0 &&
               H % 32 == 0 && A % 32 == 0;
  if (!p.shape_ok) return p;
  // resident form: the clip's projected memory in LDS and its memory rows in registers (8 frames for each of a thread's 2
  // context groups)
  const int GV = 1024 / (E / 4);
  p.att_resident = (resident && S <= 8 * GV && (long)att_lds_bytes(pd_att_floats(S, A, true)) <= PERSIST_LDS_MAX) ? 1 : 0;
  const size_t att = att_lds_bytes(pd_att_floats(S, A, p.att_resident != 0));
  p.shm = att > PD_SMEM_BYTES ? att : PD_SMEM_BYTES;
  return p;
}

// ---------------------------------------------------------------------------------------------------- decode backward (BPTT)
struct PbPlan {
  bool shape_ok;
  int N, Tc, S, E, H, A;
  int ks_rb, ks_pa;                // K-splits of the RB / PA products
  int rc_splits;                   // attention workgroups per clip (PB_RC_FRAMES frames each)
  int n_ra, n_rb, n_pa, n_pb;      // workgroups per role (the attention role: N * rc_splits)
  int grid;
  size_t shm;
  long counter_words, abort_index;
  // K-split partials handed over inside the launch, one scratch region: dctx [ks_rb][N][E], dhp [ks_pa][N][Hp], dml [ks_pa][N][2E]
  long part_floats, dctx_part_off, dhp_part_off, dml_part_off;
  long dqd_part_floats;            // the attention shares of d qd [rc_splits][N][Tc][A]; 0 when a clip is one share (or the launch takes no such S)
  int dv_rows, dv_rows_max;        // rows of dvpart the launch writes (one per clip and share), and what a layout reserves
};
constexpr PbPlan decode_bwd_plan(int N, int Tc, int S, int E, int H, int A) {
  PbPlan p{};
  p.N = N; p.Tc = Tc; p.S = S; p.E = E; p.H = H; p.A = A;
  p.abort_index = (long)PB_C_COUNT * Tc;
  p.counter_words = persist_counter_words(PB_C_COUNT, Tc);
  // K-splits: one resident batch (K <= 512) per workgroup where the K of the product divides that way, at most PB_KS_MAX
  p.ks_rb = (3 * H) % 512 == 0 && 3 * H / 512 <= PB_KS_MAX ? 3 * H / 512 : 1;
  p.ks_pa = E == 512 ? 2 : 1;      // K = 4Hp = 2048 = 2 x 1024 and 2E = 1024: the shapes the split products are written for
  p.rc_splits = (S + PB_RC_FRAMES - 1) / PB_RC_FRAMES;
  p.n_ra = H / 32;
  p.n_rb = (E / 32) * p.ks_rb;
  p.n_pa = (E / 16) * p.ks_pa;
  p.n_pb = E / 32;
  p.grid = p.n_ra + p.n_rb + N * p.rc_splits + p.n_pa + p.n_pb;
  const size_t att = att_lds_bytes(pb_att_floats(S < PB_RC_FRAMES ? S : PB_RC_FRAMES, A));
  p.shm = att > PB_SMEM_BYTES ? att : PB_SMEM_BYTES;
  // every region holds PB_KS_MAX shares, whatever the splits of this shape
  p.dctx_part_off = 0;
  p.dhp_part_off = p.dctx_part_off + (long)PB_KS_MAX * N * E;
  p.dml_part_off = p.dhp_part_off + (long)PB_KS_MAX * N * E;
  p.part_floats = p.dml_part_off + (long)PB_KS_MAX * N * 2 * E;
  const bool frames_ok = p.rc_splits <= PB_RC_SPLITS_MAX;
  p.dqd_part_floats = p.rc_splits > 1 && frames_ok ? (long)p.rc_splits * N * Tc * A : 0;
  p.dv_rows = N * p.rc_splits;
  p.dv_rows_max = N * PB_RC_SPLITS_MAX;
  // the forward's shapes; an attention workgroup keeps its frames in registers and its channels in 512 thread columns
  p.shape_ok = decode_fwd_plan(N, Tc, S, E, H, A, false).shape_ok && frames_ok && E <= 512 && A <= 512 && H % 32 == 0 && H == E &&
               (long)p.shm <= PERSIST_LDS_MAX;
  return p;
}

// ---------------------------------------------------------------------------------------------------- posterior BiGRU (both passes)
struct PqPlan {
  bool shape_ok;
  int N, Tc, Hq;
  int grid;
  size_t shm;
  long counter_words, abort_index;
  long hbuf_floats;                // forward: the state in flight [2 directions][2 step parities][N][Hq]
};
constexpr PqPlan posterior_plan(int N, int Tc, int Hq) {
  PqPlan p{};
  p.N = N; p.Tc = Tc; p.Hq = Hq;
  p.abort_index = 2L * Tc;
  p.counter_words = persist_counter_words(2, Tc);       // one counter per direction and step
  p.grid = 2 * (Hq / 32);
  p.shm = PQ_SMEM_BYTES;
  p.hbuf_floats = 4L * N * Hq;
  // one 32-row tile of clips; 32 hidden units per workgroup; a wavefront's share of K = Hq is one resident batch
  p.shape_ok = N >= 1 && N <= 32 && Tc >= 1 && Hq >= 32 && Hq <= 64 * PD_U && Hq % 32 == 0;
  return p;
}

}  // namespace acvae
