// decode_persist.hip: the teacher-forced decode loop, its backward through time and the posterior's BiGRU as persistent
// launches (internal C++ interface of the C ABI entries of decoder.hip; `flags`: ACVAE_FLAG_* of include/acvae_hip.h).
// Per launch a caller
//   1. makes the PLAN from the dims (persist_plan.h: pure - role counts, grid, LDS, counters, scratch; the workspace layouts
//      read the same plans),
//   2. asks *_resident() whether the kernel takes the shape AND the plan's whole grid is resident on the current device at
//      once - the only place that talks to the occupancy calculator, its answers cached per device - and takes the per-step
//      path if not,
//   3. fills the parameter struct's pointers and launches with the plan: the launcher copies the plan's dims and counts into
//      the struct, derives nothing and queries nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "persist_plan.h"

struct PdParams {
  // decoder (models/decoder.py:175-203): attention h2attn [A, H + E] (query half = columns 0..H), GRU weight_hh [3H, H] /
  // bias_hh, weight_ih [3H, 3E] (context part = columns E..2E), attention vector v [A]
  const float *w_att, *w_hh, *b_hh, *w_ih, *att_v;
  // prior (models/text_encoder.py:247-268): LSTM weight_ih [4Hp, 3E] (last_z part = columns 2E..3E), weight_hh [4Hp, Hp] /
  // bias_hh, mean_log_out [2E, Hp] / bias
  const float *pw_ih, *pw_hh, *pb_hh, *w_ml, *b_ml;
  // produced in front of the launch
  const float *encproj, *mem;      // [N, S, A], [N, S, E]
  const int64_t* mem_lens;         // [N]
  const float *gi, *gates_p;       // hoisted input projections [N, Tc, 3H], [N, Tc, 4Hp]
  const float *eps_p, *zeros;      // [Tc, N, E]; N x max(H, Hp) zeros
  // written by the launch ([N, Tc, .] batch-major like the reference's outputs)
  float *qd, *gh, *rnn_d, *attn_w, *outputs, *gru_save, *hprev_d;
  float *rnn_p, *hp_all, *c_all, *lstm_save, *p_means, *p_logs, *p_z;
  unsigned* cnt;                   // PdPlan::counter_words words, zeroed by the launcher
  // everything below is set by the launcher, from the plan
  unsigned* abort_word;            // cnt + PdPlan::abort_index
  unsigned spin_limit;             // polls after which a wait gives up and raises abort_word
  int N, Tc, S, E, H, A;
  int n_d1, n_d3, n_p1, n_p2;
  int att_resident;                // the attention keeps its clip's memory on the CU
};

// backward through time of the same loop (acvae_decode_bwd)
struct PbParams {
  // transposed weights (acvae_decode_bwd's scratch): [H][3H], [H+E][A], [3E][3H], [Hp][4Hp], [3E][4Hp], [Hp][2E]
  const float *wt_dhh, *wt_datt, *wt_dih, *wt_phh, *wt_pih, *wt_pml;
  const float* att_v;
  // saved by the forward
  const float *encproj, *mem, *qd, *attn_w, *gru_save, *hprev_d, *lstm_save, *c_all, *p_logs, *eps_p;
  const int64_t* mem_lens;
  // upstream gradients ([N, Tc, .]; the three of the prior may be NULL)
  const float *d_out, *d_p_z, *d_p_means, *d_p_logs;
  // written by the launch (dctx: [N, Tc, E], one slot per step)
  float *dgi, *dgh, *dqd, *dctx, *dencproj, *dmem, *dvpart, *dgates, *dml_all, *dhp;
  // clips of more than 64 frames: the attention role runs as rc_splits workgroups per clip (set by the launcher); their shares
  // of d qd [rc_splits][N][Tc][A] (PbPlan::dqd_part_floats; RA adds them and writes the sum to dqd for the steps it reads,
  // 1 .. Tc - 1.  Step 0's rows of dqd are the CALLER's: they meet h_{-1} = 0 only, so acvae_decode_bwd zeroes dqd at its
  // entry instead of the launch summing shares nobody needs) and the forward's rnn_d ([N][Tc][3E]: ctx = columns E..2E)
  float* dqd_part;
  const float* ctx;
  int rc_splits;
  // K-split partials handed over inside the launch: dctx [ks_rb][N][E], dhp [ks_pa][N][Hp], dml [ks_pa][N][2E], at
  // PbPlan::*_part_off of one scratch region of PbPlan::part_floats
  float *dctx_part, *dhp_part, *dml_part;
  unsigned* cnt;                   // PbPlan::counter_words words
  // set by the launcher, from the plan
  unsigned* abort_word;
  unsigned spin_limit;
  int N, Tc, S, E, H, A;
  int n_ra, n_rb, n_pa, n_pb;
  int ks_rb, ks_pa;                // K-splits of the RB / PA products
};

namespace acvae {
// internal flag beside the public ACVAE_FLAG_* of a launch: the caller has zeroed p.cnt in this stream (with its other tickets,
// one launch: rnn.h ZeroBatch) - the launcher skips its own memset
#define ACVAE_FLAG_INT_CNT_ZEROED (1 << 16)
// The plan whose grid is resident on the current device: with the attention's memory on the CU where the shape has that form
// and it fits, else streamed.  false: the kernel does not take the shape, or neither form fits.
bool decode_fwd_resident(int N, int Tc, int S, int E, int H, int A, PdPlan& plan);
int decode_persist_fwd(PdParams p, const PdPlan& plan, hipStream_t st, int flags);
bool decode_bwd_resident(const PbPlan& plan);
int decode_persist_bwd(PbParams p, const PbPlan& plan, hipStream_t st, int flags);   // p.dqd_part / p.ctx: needed when plan.rc_splits > 1
}  // namespace acvae


// ---------------------------------------------------------------------------------------------------------------------
// The posterior's packed bidirectional GRU (PosteriorRNN_hybrid, models/text_encoder.py:189-191) as one persistent launch per
// pass: both directions, all Tc steps.  A workgroup owns 32 hidden units of one direction: forward it forms the three gate
// tiles gh = h . Whh^T + b of its units (weight fragments resident in registers), runs the GRU cell and hands its slice of h to
// the direction's other workgroups; backward it forms dh = dh . z + dgh . Whh for its units, runs the cell backward and
// hands over its slice of dgh.  One hand-off per step and direction (protocol of decode_persist.hip).
struct PqParams {
  const float* w_hh[2];        // [3Hq][Hq] per direction
  const float* b_hh[2];        // [3Hq]
  const float* gi[2];          // hoisted input projections [N][Tc][3Hq]
  const int64_t* lens1;        // [N]
  float* hid;                  // [N][Tc][2Hq]
  float* save[2];              // [N][Tc][4Hq] = r | z | n | gh_n
  float* hprev[2];             // [N][Tc][Hq]
  float* hbuf;                 // [2 directions][2 step parities][N][Hq]: the state in flight, ZEROED by the caller (step 0 reads parity 1)
  unsigned* cnt;               // PqPlan::counter_words words, zeroed by the launcher
  unsigned* abort_word;        // set by the launcher, as are the fields below
  unsigned spin_limit;
  int N, Tc, Hq;
};
struct PqbParams {
  const float* wt[2];          // transposed weight_hh: [Hq][3Hq]
  const float* dhid;           // [N][Tc][2Hq]
  const float* save[2];
  const float* hprev[2];
  const int64_t* lens1;
  float* dgi[2];               // [N][Tc][3Hq]
  float* dgh[2];               // [N][Tc][3Hq] (handed over inside the launch)
  unsigned* cnt;
  unsigned* abort_word;
  unsigned spin_limit;
  int N, Tc, Hq;
};
namespace acvae {
bool posterior_resident(const PqPlan& plan);     // both passes: a forward on the persistent path is followed by such a backward
int posterior_persist_fwd(PqParams p, const PqPlan& plan, hipStream_t st, int flags);
int posterior_persist_bwd(PqbParams p, const PqPlan& plan, hipStream_t st, int flags);
}  // namespace acvae
