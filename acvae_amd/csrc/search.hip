// The inference search of the text side, each entry point ONE library call with no synchronisation inside:
//   - single decode steps, the per-step API of the reference's pnet / decoder modules (acvae_prior_step_fwd,
//     acvae_decoder_step_fwd, acvae_attn_precompute);
//   - the search over M members' averaged word probabilities, greedy or beam (acvae_ensemble_search), and the validation
//     beam search of one model (acvae_beam_search), which is its M = 1 case plus beam 0's attention-weight history;
//   - rollouts from the mixture, sample_n sampled or greedy rows per clip (acvae_ensemble_rollout): the same driver, a
//     rollout's pick in the place of the flat top-k;
//   - diverse beam search over M >= 1 members (acvae_ensemble_dbs_search; acvae_dbs_search is its M = 1 case), at the end.
// The two drivers keep their own loops, search() over t and dbs_search() over (t, group), and share what belongs to a
// member: its layout (MemberLayout), its prologue, its step and its gather by parent.
// The training-time composites are decoder.hip.
#include <utility>
#include "common.h"
#include "constrain.h"
#include "conv.h"
#include "dbs_rules.h"
#include "rnn.h"
#include "text_common.h"

// ==========================================================================================
// single decode steps (inference only): the per-step API of the reference's pnet / decoder modules, used by the
// beam search (models/vae_model.py:896-995) and by anyone calling the sub-modules directly
// ==========================================================================================
namespace {
struct StepLayout { long skws, encproj, rnn, q, gates, gh, ml, words, attws, attws_bytes, total; };
int step_layout(int N, int S, int E, int H, int A, int V, StepLayout& L) {
  if (N <= 0 || S <= 0 || E <= 0 || H <= 0 || A <= 0 || V <= 1) return ACVAE_EINVAL;
  Bump b;
  L.skws = b.take(acvae_skinny_ws_floats());
  L.encproj = b.take((long)N * S * (A > E ? A : E));
  L.rnn = b.take((long)N * 3 * E);
  L.q = b.take((long)N * (A > E ? A : E));
  L.gates = b.take((long)N * (4 * E > 3 * H ? 4 * E : 3 * H));      // the prior's LSTM gates [N, 4E] and the decoder's gi [N, 3H]
  L.gh = b.take((long)N * 3 * H);
  L.ml = b.take((long)N * 2 * E);
  L.words = b.take((long)N * 2);
  // workspace of the split-over-frames attention (acvae_attn_fwd: few query rows); its counters are zeroed by every entry point
  L.attws_bytes = acvae_attn_fwd_workspace_bytes(N, 1, S, A, E);
  const long w2 = acvae_attn_fwd_workspace_bytes(N, 1, S, E, E);
  if (w2 > L.attws_bytes) L.attws_bytes = w2;
  L.attws = b.take(L.attws_bytes / 4 + 64);
  L.total = b.off;
  return ACVAE_OK;
}
inline int step_attws_reset(float* sc, const StepLayout& L, hipStream_t st) {
  return L.attws_bytes > 0 ? zero(sc + L.attws, 256, st) : ACVAE_OK;
}
}  // namespace

// One buffer serves both step entries: acvae_decoder_step_fwd lays it out by (E, H, A), acvae_prior_step_fwd - which is not
// told H and A - by (E, E, E), and with H < E and A <= E the latter is the larger.
extern "C" int64_t acvae_step_scratch_bytes(int N, int S, int E, int H, int A, int V) {
  StepLayout L, Lp;
  if (step_layout(N, S, E, H, A, V, L) != ACVAE_OK || step_layout(N, S, E, E, E, V, Lp) != ACVAE_OK) return -1;
  return (L.total > Lp.total ? L.total : Lp.total) * 4;
}

// encproj = mem . W[:, hs_dec:]^T + b for the decoder attention (which = 0) or the prior attention (which = 1)
extern "C" int acvae_attn_precompute(const void* const* params, int which, const float* mem, float* encproj, int N,
                                     int S, int E, int H, int A, void* stream) {
  if (!params || !mem || !encproj || N <= 0 || S <= 0) return ACVAE_EINVAL;
  Ctx st{(hipStream_t)stream, nullptr};
  auto P = [&](int i) { return (const float*)params[i]; };
  if (which == 0) return gemm(mem, E, P(TP_DEC_ATT_W) + H, E + H, P(TP_DEC_ATT_B), encproj, A, N * S, A, E, 0, st);
  return gemm(mem, E, P(TP_P_ATT_W) + E, 2 * E, P(TP_P_ATT_B), encproj, E, N * S, E, E, 0, st);
}

namespace {
// One prior / decoder step over R = Nm * Tq rows: row r = n * Tq + j attends over memory n (Tq = 1: one memory per row,
// the sub-module API; Tq = beam: the beams of a clip share its memory, no replicated copy).
int prior_step(const void* const* params, const int64_t* word, const float* mem, const int64_t* mem_lens, const float* ep,
               const float* h_prev, const float* c_prev, const float* last_z, const float* eps, float* mean, float* logv,
               float* z, float* h_out, float* c_out, float* attw, float* sc, const StepLayout& L, int Nm, int Tq, int S,
               int E, int V, const Ctx& st) {
  auto P = [&](int i) { return (const float*)params[i]; };
  const int N = Nm * Tq, Hp = E;
  float* rnn = sc + L.rnn;
  float* q = sc + L.q;
  float* gates = sc + L.gates;
  float* ml = sc + L.ml;
  ACVAE_TRY(acvae::embed_gather(word, 1, P(TP_P_EMB), V, rnn, 3 * E, N, E, st));
  ACVAE_TRY(gemm(rnn, 3 * E, P(TP_P_ATT_W), 2 * E, nullptr, q, E, N, E, E, 0, st));
  ACVAE_TRY(acvae_attn_fwd(q, (long)Tq * E, E, ep, mem, mem_lens, P(TP_P_ATT_V), rnn + E, (long)Tq * 3 * E, 3 * E, attw,
                           (long)Tq * S, S, Nm, Tq, S, E, E, L.attws_bytes > 0 ? sc + L.attws : nullptr, L.attws_bytes, st, 0));
  ACVAE_TRY(acvae::copy_rows(rnn + 2 * E, 3 * E, last_z, E, N, E, st));
  ACVAE_TRY(gemm(rnn, 3 * E, P(TP_P_WIH), 3 * E, P(TP_P_BIH), gates, 4 * Hp, N, 4 * Hp, 3 * E, 0, st));
  ACVAE_TRY(gemm(h_prev, Hp, P(TP_P_WHH), Hp, P(TP_P_BHH), gates, 4 * Hp, N, 4 * Hp, Hp, 1, st));
  ACVAE_TRY(acvae::lstm_fwd(gates, 4 * Hp, c_prev, Hp, h_out, Hp, c_out, Hp, nullptr, 0, N, Hp, st));
  ACVAE_TRY(gemm(h_out, Hp, P(TP_P_ML_W), Hp, P(TP_P_ML_B), ml, 2 * E, N, 2 * E, Hp, 0, st));
  return acvae_reparam_fwd(ml, 2 * E, eps, E, mean, logv, z, E, nullptr, 0, N, E, st);
}

int decoder_step(const void* const* params, const int64_t* word, const float* h_prev, const float* mem,
                 const int64_t* mem_lens, const float* ed, const float* z, float* logits, float* h_out, float* attw,
                 float* rnn_input, float* sc, const StepLayout& L, int Nm, int Tq, int S, int E, int H, int A, int V,
                 const Ctx& st) {
  auto P = [&](int i) { return (const float*)params[i]; };
  const int N = Nm * Tq;
  float* q = sc + L.q;
  float* gi = sc + L.gates;
  float* gh = sc + L.gh;
  ACVAE_TRY(acvae::embed_gather(word, 1, P(TP_DEC_EMB), V, rnn_input, 3 * E, N, E, st));
  ACVAE_TRY(gemm(h_prev, H, P(TP_DEC_ATT_W), E + H, nullptr, q, A, N, A, H, 0, st));
  ACVAE_TRY(acvae_attn_fwd(q, (long)Tq * A, A, ed, mem, mem_lens, P(TP_DEC_ATT_V), rnn_input + E, (long)Tq * 3 * E, 3 * E,
                           attw, (long)Tq * S, S, Nm, Tq, S, A, E, L.attws_bytes > 0 ? sc + L.attws : nullptr, L.attws_bytes, st, 0));
  ACVAE_TRY(acvae::copy_rows(rnn_input + 2 * E, 3 * E, z, E, N, E, st));
  ACVAE_TRY(gemm(rnn_input, 3 * E, P(TP_DEC_WIH), 3 * E, P(TP_DEC_BIH), gi, 3 * H, N, 3 * H, 3 * E, 0, st));
  ACVAE_TRY(gemm(h_prev, H, P(TP_DEC_WHH), H, P(TP_DEC_BHH), gh, 3 * H, N, 3 * H, H, 0, st));
  ACVAE_TRY(acvae::gru_fwd(gi, 3 * H, gh, 3 * H, h_prev, H, h_out, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, N,
                           H, st));
  return gemm(h_out, H, P(TP_DEC_CLS_W), H, P(TP_DEC_CLS_B), logits, V, N, V, H, 0, st);
}
}  // namespace

extern "C" int acvae_prior_step_fwd(const void* const* params, const int64_t* word, const float* mem,
                                    const int64_t* mem_lens, const float* encproj_p, const float* h_prev,
                                    const float* c_prev, const float* last_z, const float* eps, float* mean, float* logv,
                                    float* z, float* h_out, float* c_out, float* attw, void* scratch_v,
                                    int64_t scratch_bytes, int N, int S, int E, int V, void* stream) {
  StepLayout L;
  ACVAE_TRY(step_layout(N, S, E, E, E, V, L));
  if (!params || !word || !mem || !mem_lens || !h_prev || !c_prev || !last_z || !eps || !mean || !logv || !z ||
      !h_out || !c_out || !attw || !scratch_v)
    return ACVAE_EINVAL;
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  float* sc = (float*)scratch_v;
  Ctx st{(hipStream_t)stream, sc + L.skws};
  ACVAE_TRY(acvae_skinny_ws_reset(st.skws, st.s));
  ACVAE_TRY(step_attws_reset(sc, L, st.s));
  const float* ep = encproj_p;
  if (!ep) {
    ACVAE_TRY(acvae_attn_precompute(params, 1, mem, sc + L.encproj, N, S, E, E, E, stream));
    ep = sc + L.encproj;
  }
  return prior_step(params, word, mem, mem_lens, ep, h_prev, c_prev, last_z, eps, mean, logv, z, h_out, c_out, attw, sc,
                    L, N, 1, S, E, V, st);
}

extern "C" int acvae_decoder_step_fwd(const void* const* params, const int64_t* word, const float* h_prev,
                                      const float* mem, const int64_t* mem_lens, const float* encproj_d, const float* z,
                                      float* logits, float* h_out, float* attw, float* rnn_input, void* scratch_v,
                                      int64_t scratch_bytes, int N, int S, int E, int H, int A, int V, void* stream) {
  StepLayout L;
  ACVAE_TRY(step_layout(N, S, E, H, A, V, L));
  if (!params || !word || !h_prev || !mem || !mem_lens || !z || !logits || !h_out || !attw || !rnn_input || !scratch_v)
    return ACVAE_EINVAL;
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  float* sc = (float*)scratch_v;
  Ctx st{(hipStream_t)stream, sc + L.skws};
  ACVAE_TRY(acvae_skinny_ws_reset(st.skws, st.s));
  ACVAE_TRY(step_attws_reset(sc, L, st.s));
  const float* ed = encproj_d;
  if (!ed) {
    ACVAE_TRY(acvae_attn_precompute(params, 0, mem, sc + L.encproj, N, S, E, H, A, stream));
    ed = sc + L.encproj;
  }
  return decoder_step(params, word, h_prev, mem, mem_lens, ed, z, logits, h_out, attw, rnn_input, sc, L, N, 1, S, E, H,
                      A, V, st);
}

// ==========================================================================================
// The search as ONE call, over M >= 1 members: BaseRunner._ensemble_batch / _ensemble_batch_beam_search
// (runners/base_runner.py:562-694) carried onto Hybrid_VAEModel's step (prior step -> z -> decoder step,
// models/vae_model.py:896-995; the reference's own ensemble code calls model.decoder without z).  All clips advance
// together, the beams of a clip share its memory, and nothing but kernels is enqueued per step.  Every
// member keeps its own memory, attention projections and recurrent states; all are fed the same word;
// acvae_ensemble_mix averages their word probabilities (base_runner.py:616-618, 675-680; at M = 1 the member's own
// log-softmax plus the running beam score, bit for bit) and the word is picked from the average:
//   beam   - flat top-k over beam * V per clip at every step (the rows of a clip differ in z from t = 0 on, so the
//            reference's "row 0 only at t = 0", :681-682, does not carry over), states gathered by parent once per member.
//            Instead of re-gathering the word and attention-weight histories by prev_word_inds every step
//            (vae_model.py:917-921, :979), each step's parent row and word (and, for the single-model entry, member 0's
//            weights) are kept and beam 0 is traced back once at the end, which yields the same seqs[0] / attn_weights[0]
//            (:990-995);
//   greedy - the mix kernel's own argmax; a row that has produced end_idx keeps emitting and feeding it, and all
//            max_length steps run without a host read-back: seqs prefilled with end_idx, as :584, 622-630 leave it.
// Members run one after the other on the one stream.
// ==========================================================================================
namespace {
struct SearchMember { const void* const* params; const float* mem; const int64_t* mem_lens; const float* eps; int S, E, H, A; };
// One member's buffers, for either driver; a step runs R rows (the beams of the N clips, or those of one DBS group).
//   cur: the states a step reads, [G][R][H + 3E]: one block h | hp | cp | last_z per group (beam and greedy: G = 1);
//   nxt: the states a step writes, one such block shared by the groups: a beam search gathers it into cur by parent,
//        greedy swaps the two.  (The parts of a block lie on 16 bytes when H and E are multiples of 4: DESIGN.md 4e.)
struct MemberLayout { StepLayout sl; long step, encd, encp, cur, nxt, mean, logv, attp, attw, logits, rnn; };
int member_layout(Bump& b, const SearchMember& mb, int N, long R, int G, int attw_steps, int V, MemberLayout& o) {
  const long S = mb.S, e = mb.E, h = mb.H;
  ACVAE_TRY(step_layout((int)R, mb.S, mb.E, mb.H, mb.A, V, o.sl));
  o.step = b.take(o.sl.total);
  o.encd = b.take((long)N * S * mb.A); o.encp = b.take((long)N * S * e);
  o.cur = b.take((long)G * R * (h + 3 * e)); o.nxt = b.take(R * (h + 3 * e));
  o.mean = b.take(R * e); o.logv = b.take(R * e);
  o.attp = b.take(R * S); o.attw = b.take((long)attw_steps * R * S);
  o.logits = b.take(R * V); o.rnn = b.take(R * 3 * e);
  return ACVAE_OK;
}
struct States { float *h, *hp, *cp, *lz; };
inline States states_at(float* block, long R, const SearchMember& b) {
  return {block, block + R * b.H, block + R * (b.H + b.E), block + R * (b.H + 2 * b.E)};
}

struct SearchLayout { MemberLayout m[ACVAE_ENSEMBLE_MAX]; long scores, topk, best, words, whist, frec, norm, total; int keep_attw, keep_hist, keep_fin; };
// keep_attw: member 0's decoder attention weights of every step, [T][R][S], for the trace-back; else [R][S], overwritten.
// keep_hist: the rows' word histories of a constrained beam search, int64 [2][R][T] (the one read, the one gathered into).
// keep_fin: the records of a finishing beam search, f [T][R], and its norm table [T].
int search_layout(const SearchMember* mb, int M, int N, int beam, int T, int V, int keep_attw, int keep_hist, int keep_fin,
                  SearchLayout& L) {
  if (M < 1 || M > ACVAE_ENSEMBLE_MAX || N <= 0 || beam <= 0 || T <= 0) return ACVAE_EINVAL;
  const long R = (long)N * beam;
  if (R > (1L << 20)) return ACVAE_EUNSUPPORTED;
  L.keep_attw = keep_attw; L.keep_hist = keep_hist; L.keep_fin = keep_fin;
  Bump b;
  for (int m = 0; m < M; ++m) ACVAE_TRY(member_layout(b, mb[m], N, R, 1, keep_attw && m == 0 ? T : 1, V, L.m[m]));
  L.scores = b.take(R * V);
  L.topk = b.take(R);
  L.best = b.take(R);
  L.words = b.take(2 * ((long)(3 * T + 2) * R));        // int64: word [R], argmax [R], per step idx / parent / word [T][R]
  L.whist = keep_hist ? b.take(2 * (2 * R * T)) : 0;     // int64; behind everything else: the rest lies where it lay
  L.frec = keep_fin ? b.take((long)T * R) : 0;
  L.norm = keep_fin ? b.take(T) : 0;
  L.total = b.off;
  return ACVAE_OK;
}

struct GatherJob { const float* src; float* dst; int width; };
using GatherTable = acvae::JobTable<GatherJob, 4>;
// A constrained beam search's word histories follow their parents too: one more job (blockIdx.y == g.n, launched only
// then), row r's history becomes its parent's t words and the word the row was given at step t.
struct HistJob { const int64_t* src; int64_t* dst; const int64_t* word; int t, T; };
__global__ __launch_bounds__(256) void beam_gather_kernel(GatherTable g, const int64_t* __restrict__ parent, HistJob hj) {
  const long r = blockIdx.x, p = parent[r];
  if ((int)blockIdx.y == g.n) {
    for (int i = threadIdx.x; i < hj.t; i += blockDim.x) hj.dst[r * hj.T + i] = hj.src[p * hj.T + i];
    if (threadIdx.x == 0) hj.dst[r * hj.T + hj.t] = hj.word[r];
    return;
  }
  const GatherJob j = g.job[blockIdx.y];
  for (int i = threadIdx.x; i < j.width; i += blockDim.x) j.dst[r * j.width + i] = j.src[p * j.width + i];
}

// ---- what both drivers do with a member (sc: the call's scratch, o: the member's part of it).  In front of the first step:
// tickets and counters zeroed, both attention projections, every group's states zero, the logits entered.
int member_prologue(const SearchMember& b, const MemberLayout& o, float* sc, int N, long R, int G, int V,
                    const float*& logit_ptr, int64_t& logit_ld, hipStream_t s) {
  float* ssc = sc + o.step;
  ACVAE_TRY(acvae_skinny_ws_reset(ssc + o.sl.skws, s));
  ACVAE_TRY(step_attws_reset(ssc, o.sl, s));
  ACVAE_TRY(acvae_attn_precompute(b.params, 0, b.mem, sc + o.encd, N, b.S, b.E, b.H, b.A, s));
  ACVAE_TRY(acvae_attn_precompute(b.params, 1, b.mem, sc + o.encp, N, b.S, b.E, b.E, b.E, s));
  ACVAE_TRY(zero(sc + o.cur, (long)G * R * (b.H + 3 * b.E), s));
  logit_ptr = sc + o.logits; logit_ld = V;
  return ACVAE_OK;
}
// One step of N * Tq rows fed `word`, from the state block `cur` into `nxt`: the prior step, then the decoder step on its z.
int member_step(const SearchMember& b, const MemberLayout& o, float* sc, const int64_t* word, float* cur, float* nxt,
                const float* eps, float* attw, int N, int Tq, int V, hipStream_t s) {
  const States c = states_at(cur, (long)N * Tq, b), n = states_at(nxt, (long)N * Tq, b);
  float* ssc = sc + o.step;
  Ctx st{s, ssc + o.sl.skws};
  ACVAE_TRY(prior_step(b.params, word, b.mem, b.mem_lens, sc + o.encp, c.hp, c.cp, c.lz, eps, sc + o.mean, sc + o.logv, n.lz,
                       n.hp, n.cp, sc + o.attp, ssc, o.sl, N, Tq, b.S, b.E, V, st));
  return decoder_step(b.params, word, c.h, b.mem, b.mem_lens, sc + o.encd, n.lz, sc + o.logits, n.h, attw, sc + o.rnn, ssc,
                      o.sl, N, Tq, b.S, b.E, b.H, b.A, V, st);
}
// The next step's states follow their parents (vae_model.py:961-968): row r of `cur` becomes row parent[r] of `nxt`; hj, if
// not null, is the word-history job of a constrained beam search riding along.
void member_gather(const SearchMember& b, float* cur, float* nxt, int R, const int64_t* parent, const HistJob* hj,
                   hipStream_t s) {
  const States c = states_at(cur, R, b), n = states_at(nxt, R, b);
  GatherTable g;
  g.add({n.h, c.h, b.H}); g.add({n.hp, c.hp, b.E}); g.add({n.cp, c.cp, b.E}); g.add({n.lz, c.lz, b.E});
  hipLaunchKernelGGL(beam_gather_kernel, dim3(R, g.n + (hj ? 1 : 0)), dim3(256), 0, s, g, parent, hj ? *hj : HistJob{});
}

__global__ void fill_words_kernel(int64_t* w, int64_t v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = v;
}
// greedy bookkeeping of one step (base_runner.py:618-628): a finished row keeps end_idx
__global__ void greedy_pick_kernel(const int64_t* __restrict__ arg, const float* __restrict__ best,
                                   int64_t* __restrict__ seqs, float* __restrict__ logprobs, int64_t* __restrict__ word,
                                   int64_t end_idx, int t, int T, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  int64_t w = arg[r];
  if (t > 0 && seqs[(long)r * T + t - 1] == end_idx) w = end_idx;
  seqs[(long)r * T + t] = w;
  logprobs[(long)r * T + t] = best[r];
  word[r] = w;
}
// one workgroup per clip: follow beam 0's parents from the last step to the first.  logprobs (beam 0's final score) and
// attw_out ([N,S,T], from the [T][R][S] history attw) may each be null.
__global__ __launch_bounds__(256) void beam_trace_kernel(const int64_t* __restrict__ parent, const int64_t* __restrict__ word,
                                                         const float* __restrict__ topk, const float* __restrict__ attw,
                                                         int64_t* __restrict__ seqs, float* __restrict__ logprobs,
                                                         float* __restrict__ attw_out, long hist_stride, int R, int beam, int T,
                                                         int S) {
  const int n = blockIdx.x;
  long r = (long)n * beam;
  if (logprobs && threadIdx.x == 0) logprobs[n] = topk[r];
  for (int t = T - 1; t >= 0; --t) {
    const long p = parent[t * hist_stride + r];
    if (threadIdx.x == 0) seqs[(long)n * T + t] = word[t * hist_stride + r];
    if (attw_out) {
      const float* w = attw + ((long)t * R + p) * S;
      for (int s = threadIdx.x; s < S; s += blockDim.x) attw_out[((long)n * S + s) * T + t] = w[s];
    }
    r = p;
  }
}

// ---- finishing mode (include/acvae_hip.h has the definition): hypotheses end at end_idx, n-best by score / norm[t]
// Finishing as the entries receive it; `norm` is a HOST array [T].  Off: no launch is added and no buffer is kept.
struct Finishing {
  int on = 0, nbest = 1;
  const float* norm = nullptr;
  int64_t* nb_seqs = nullptr; float* nb_scores = nullptr; float* nb_logprobs = nullptr; int* nb_lengths = nullptr;
};
// Values alone (what acvae_beam_finish refuses too).
int finishing_check(const Finishing& f, int beam, int T) {
  if (!f.on) return ACVAE_OK;
  if (f.nbest < 1 || f.nbest > beam || beam > 16 || T <= 0) return ACVAE_EINVAL;
  if (!f.norm || !f.nb_seqs || !f.nb_scores || !f.nb_logprobs || !f.nb_lengths) return ACVAE_EINVAL;
  for (int t = 0; t < T; ++t)
    if (!isfinite(f.norm[t]) || !(f.norm[t] > 0.f)) return ACVAE_EINVAL;
  return ACVAE_OK;
}
// The norm table goes to the device as the suppress list does, by value in kernel arguments, 64 entries a launch.
struct NormChunk { float v[64]; };
__global__ __launch_bounds__(64) void norm_fill_kernel(NormChunk c, float* __restrict__ dst, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}
int norm_upload(const float* norm_host, float* dst, int T, hipStream_t s) {
  for (int b = 0; b < T; b += 64) {
    NormChunk c;
    const int n = T - b < 64 ? T - b : 64;
    for (int i = 0; i < 64; ++i) c.v[i] = i < n ? norm_host[b + i] : 1.f;
    hipLaunchKernelGGL(norm_fill_kernel, dim3(1), dim3(64), 0, s, c, dst + b, n);
  }
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
// Steps 1-3 on the R rows of a step, after its top-k: record, then retire.  One thread per row.
__global__ __launch_bounds__(256) void beam_retire_kernel(float* __restrict__ c, const int64_t* __restrict__ word,
                                                          float* __restrict__ f, int64_t end_idx, int last, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float v = c[r];
  const bool ends = word[r] == end_idx;
  f[r] = (v > -INFINITY && (ends || last)) ? v : -INFINITY;
  if (ends) c[r] = -INFINITY;
}
// One workgroup per clip.  nbest selection passes over the clip's T * beam records in topk_flat_kernel's idiom (value, then
// index, through wavefront shuffles): candidate i = t * beam + j, so the lower index is the earlier step, then the lower
// row.  Then lane q walks hypothesis q's parents back from its step and writes its words, and the workgroup copies
// hypothesis 0's attention weights.  A parent outside [0, R) is clamped into it (the driver's come from the top-k and are
// in range; a caller-built history is the caller's).
constexpr int FIN_THREADS = 256;
__global__ __launch_bounds__(FIN_THREADS) void beam_finish_kernel(
    const int64_t* __restrict__ parent, const int64_t* __restrict__ word, long hist_stride, const float* __restrict__ f,
    const float* __restrict__ norm, const float* __restrict__ attw, int64_t* __restrict__ seqs, float* __restrict__ logprobs,
    float* __restrict__ attw_out, int64_t* __restrict__ nb_seqs, float* __restrict__ nb_scores,
    float* __restrict__ nb_logprobs, int* __restrict__ nb_lengths, int R, int beam, int T, int S, int nbest,
    int64_t end_idx) {
  __shared__ float rv[FIN_THREADS / 64];
  __shared__ int ri[FIN_THREADS / 64];
  __shared__ int sel[16];                                // the selected records, -1: none left
  const int n = blockIdx.x, tid = threadIdx.x;
  const long r0 = (long)n * beam;
  const int cand = T * beam;
  for (int q = 0; q < nbest; ++q) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < cand; i += FIN_THREADS) {
      const int t = i / beam;
      const float fv = f[(long)t * R + r0 + (i - t * beam)];
      if (!(fv > -INFINITY)) continue;                   // not a record
      bool taken = false;
      for (int p = 0; p < q; ++p) taken = taken || (sel[p] == i);
      const float v = __fdiv_rn(fv, norm[t]);
      if (!taken && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < FIN_THREADS / 64; ++w)
        if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
      sel[q] = bi == 0x7fffffff ? -1 : bi;
    }
    __syncthreads();
  }
  if (tid < nbest) {                                     // one lane per hypothesis
    const int i = sel[tid];
    const int t0 = i < 0 ? -1 : i / beam;
    long r = i < 0 ? 0 : r0 + (i - t0 * beam);
    const long o = (long)n * nbest + tid;
    const float fv = i < 0 ? -INFINITY : f[(long)t0 * R + r];
    nb_logprobs[o] = fv;
    nb_scores[o] = i < 0 ? -INFINITY : __fdiv_rn(fv, norm[t0]);
    nb_lengths[o] = t0 + 1;
    if (tid == 0 && logprobs) logprobs[n] = fv;
    int64_t* row = nb_seqs + o * T;
    int64_t* row0 = tid == 0 ? seqs : nullptr;
    if (row0) row0 += (long)n * T;
    for (int t = T - 1; t > t0; --t) {
      row[t] = end_idx;
      if (row0) row0[t] = end_idx;
    }
    for (int t = t0; t >= 0; --t) {
      const int64_t w = word[t * hist_stride + r];
      row[t] = w;
      if (row0) row0[t] = w;
      const long p = parent[t * hist_stride + r];
      r = p < 0 ? 0 : (p >= R ? R - 1 : p);
    }
  }
  if (!attw_out) return;                                 // uniform over the block
  const int i0 = sel[0];
  const int t0 = i0 < 0 ? -1 : i0 / beam;
  long r = i0 < 0 ? 0 : r0 + (i0 - t0 * beam);
  for (int t = T - 1; t > t0; --t)
    for (int s = tid; s < S; s += FIN_THREADS) attw_out[((long)n * S + s) * T + t] = 0.f;
  for (int t = t0; t >= 0; --t) {                        // the weights of step t are those of the row's parent, as beam_trace_kernel
    long p = parent[t * hist_stride + r];
    p = p < 0 ? 0 : (p >= R ? R - 1 : p);
    const float* w = attw + ((long)t * R + p) * S;
    for (int s = tid; s < S; s += FIN_THREADS) attw_out[((long)n * S + s) * T + t] = w[s];
    r = p;
  }
}

// How a step of search() chooses its words.  Beam: the flat top-k.  The others are rollouts, `beam` independent rows per
// clip that never change places (the states swap, no gather): greedy takes the mix kernel's argmax; gumbel / multinomial
// draw on noise [T][R][V], by acvae_ensemble_mix_sample (one launch: mix, draw and bookkeeping) or, with top_k / top_p on,
// by acvae_sample_next_word_truncated on the mixed row, which the `scores` block holds.
struct Pick {
  int mode;                                              // PICK_BEAM, or the ACVAE_SAMPLE_* code of a rollout
  const float* noise = nullptr;
  float temp = 1.f;
  int top_k = 0;
  float top_p = 1.f;
  bool truncated() const { return top_k > 0 || top_p < 1.f; }
};
constexpr int PICK_BEAM = -1;

// The driver behind both entry points; they have refused every bad argument, so nothing here fails before a launch.
// greedy: seqs [R,T], logprobs [R,T].  Beam: seqs [N,T], logprobs [N] or null, attw_out [N,S,T] or null (not null only
// with a layout made with keep_attw).
// con: the controls of constrained decoding (constrain.hip), applied to every member's logits in front of the mixing; the
// history of a row is its seqs row (greedy) or the word history kept beside the states (beam, L.keep_hist).  With
// nothing on, no launch is added and no buffer is kept.
// fin: finishing mode (beam only, L.keep_fin): one beam_retire_kernel launch behind every top-k, and beam_finish_kernel in
// the place of beam_trace_kernel.  Off: neither, as with con.
// pick: see Pick.  "greedy" below stands for every rollout: seqs [R,T] and logprobs [R,T], whatever picks the word.
int search(const SearchMember* mb, int M, const SearchLayout& L, int64_t start_idx, int64_t end_idx, const Pick& pick,
           int64_t* seqs, float* logprobs, float* attw_out, float* sc, int N, int beam, int T, int V,
           const acvae::Constraints& con, const Finishing& fin, hipStream_t s) {
  const int R = N * beam;
  const bool greedy = pick.mode != PICK_BEAM;            // a rollout: rows keep their place, seqs is their history
  float* frec = fin.on ? sc + L.frec : nullptr;
  if (fin.on) ACVAE_TRY(norm_upload(fin.norm, sc + L.norm, T, s));
  int64_t* wh = L.keep_hist && con.on() ? (int64_t*)(sc + L.whist) : nullptr;   // the rows' histories at this step
  int64_t* wh2 = wh ? wh + (long)R * T : nullptr;
  // per member: the state blocks that change hands from step to step (greedy swaps them, the beam search gathers by parent)
  float *cur[ACVAE_ENSEMBLE_MAX], *nxt[ACVAE_ENSEMBLE_MAX];
  const float* logit_ptr[ACVAE_ENSEMBLE_MAX];
  int64_t logit_ld[ACVAE_ENSEMBLE_MAX];
  for (int m = 0; m < M; ++m) {
    ACVAE_TRY(member_prologue(mb[m], L.m[m], sc, N, R, 1, V, logit_ptr[m], logit_ld[m], s));
    cur[m] = sc + L.m[m].cur; nxt[m] = sc + L.m[m].nxt;
  }
  float* topk = sc + L.topk;
  float* best = sc + L.best;
  int64_t* word = (int64_t*)(sc + L.words);
  int64_t* arg = word + R;
  int64_t* hist = arg + R;                               // [T][3][R]: flat index, parent row, word (beam search)
  ACVAE_TRY(zero(topk, R, s));
  hipLaunchKernelGGL(fill_words_kernel, dim3((R + 255) / 256), dim3(256), 0, s, word, start_idx, R);
  const int64_t* w_t = word;
  for (int t = 0; t < T; ++t) {
    int64_t* idx_t = hist + (long)t * 3 * R;
    int64_t* par_t = idx_t + R;
    int64_t* nxt_t = par_t + R;
    for (int m = 0; m < M; ++m) {
      const MemberLayout& o = L.m[m];
      const SearchMember& b = mb[m];
      float* attw_t = sc + o.attw + (L.keep_attw && m == 0 ? (long)t * R * b.S : 0);
      ACVAE_TRY(member_step(b, o, sc, w_t, cur[m], nxt[m], b.eps + (long)t * R * b.E, attw_t, N, beam, V, s));
      ACVAE_TRY(acvae::constrain_rows(sc + o.logits, V, greedy ? seqs : wh, T, t, R, V, (int)end_idx, con, s));
    }
    if (greedy) {
      const float* noise_t = pick.noise ? pick.noise + (long)t * R * V : nullptr;
      if (pick.mode != ACVAE_SAMPLE_GREEDY && !pick.truncated()) {
        ACVAE_TRY(acvae_ensemble_mix_sample(logit_ptr, logit_ld, M, noise_t, V, pick.mode, pick.temp, nullptr, 0, seqs, T,
                                            logprobs, T, word, end_idx, t, R, V, s));
      } else {
        if (pick.mode == ACVAE_SAMPLE_GREEDY) {
          ACVAE_TRY(acvae_ensemble_mix(logit_ptr, logit_ld, M, nullptr, nullptr, 0, arg, best, 1, R, V, s));
        } else {
          ACVAE_TRY(acvae_ensemble_mix(logit_ptr, logit_ld, M, nullptr, sc + L.scores, V, nullptr, nullptr, 0, R, V, s));
          ACVAE_TRY(acvae_sample_next_word_truncated(sc + L.scores, V, 0, noise_t, V, 0, pick.mode, pick.temp, arg, best, 1,
                                                     0, R, 1, V, pick.top_k, pick.top_p, nullptr, s));
        }
        hipLaunchKernelGGL(greedy_pick_kernel, dim3((R + 255) / 256), dim3(256), 0, s, arg, best, seqs, logprobs, word,
                           end_idx, t, T, R);
      }
      for (int m = 0; m < M; ++m) std::swap(cur[m], nxt[m]);   // the new states become the next step's previous ones
      continue;
    }
    ACVAE_TRY(acvae_ensemble_mix(logit_ptr, logit_ld, M, topk, sc + L.scores, V, nullptr, nullptr, 0, R, V, s));
    ACVAE_TRY(acvae_topk_flat_batched(sc + L.scores, (int64_t)beam * V, (int64_t)beam * V, beam, V, topk, idx_t, par_t,
                                      nxt_t, N, beam, s));
    if (fin.on)
      hipLaunchKernelGGL(beam_retire_kernel, dim3((R + 255) / 256), dim3(256), 0, s, topk, nxt_t, frec + (long)t * R,
                         end_idx, t == T - 1, R);
    if (t + 1 < T) {
      const HistJob hj{wh, wh2, nxt_t, t, T};            // the histories ride with member 0's states
      for (int m = 0; m < M; ++m) member_gather(mb[m], cur[m], nxt[m], R, par_t, wh && m == 0 ? &hj : nullptr, s);
      std::swap(wh, wh2);
      w_t = nxt_t;
    }
  }
  if (!greedy && fin.on)
    hipLaunchKernelGGL(beam_finish_kernel, dim3(N), dim3(FIN_THREADS), 0, s, hist + R, hist + 2 * R, 3L * R, frec,
                       sc + L.norm, sc + L.m[0].attw, seqs, logprobs, attw_out, fin.nb_seqs, fin.nb_scores, fin.nb_logprobs,
                       fin.nb_lengths, R, beam, T, mb[0].S, fin.nbest, end_idx);
  else if (!greedy)                                      // hist rows are [idx | parent | word] per step: strided views
    hipLaunchKernelGGL(beam_trace_kernel, dim3(N), dim3(256), 0, s, hist + R, hist + 2 * R, topk, sc + L.m[0].attw, seqs,
                       logprobs, attw_out, 3L * R, R, beam, T, mb[0].S);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
}  // namespace

namespace {
// SearchMember[M] from the per-member arrays (the widths alone for a size function; a null array leaves null pointers).
int members_of(SearchMember* mb, int M, const int* S, const int* E, const int* H, const int* A,
               const void* const* const* params = nullptr, const float* const* mem = nullptr,
               const int64_t* const* mem_lens = nullptr, const float* const* eps = nullptr) {
  if (M < 1 || M > ACVAE_ENSEMBLE_MAX || !S || !E || !H || !A) return ACVAE_EINVAL;
  for (int m = 0; m < M; ++m)
    mb[m] = {params ? params[m] : nullptr, mem ? mem[m] : nullptr, mem_lens ? mem_lens[m] : nullptr,
             eps ? eps[m] : nullptr, S[m], E[m], H[m], A[m]};
  return ACVAE_OK;
}
bool members_complete(const SearchMember* mb, int M) {
  for (int m = 0; m < M; ++m)
    if (!mb[m].params || !mb[m].mem || !mb[m].mem_lens || !mb[m].eps) return false;
  return true;
}
template <class Layout>                                  // what a size function answers: -1 where the layout was refused
int64_t layout_bytes(int rc, const Layout& L) { return rc == ACVAE_OK ? L.total * 4 : -1; }

int beam_search_entry(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                      int64_t start_idx, int64_t* seqs, float* attw_out, void* scratch_v, int64_t scratch_bytes, int N,
                      int beam, int max_length, int S, int E, int H, int A, int V, int64_t end_idx,
                      const acvae::Constraints& con, const Finishing& fin, void* stream) {
  const SearchMember mb{params, mem, mem_lens, eps, S, E, H, A};
  SearchLayout L;
  ACVAE_TRY(acvae::constraints_check_loop(con, V, (int)end_idx, max_length, beam));
  ACVAE_TRY(search_layout(&mb, 1, N, beam, max_length, V, 1, con.on() || fin.on, fin.on, L));   // (one size per mode)
  ACVAE_TRY(finishing_check(fin, beam, max_length));
  if (fin.on && (end_idx < 0 || end_idx >= V)) return ACVAE_EINVAL;
  if (!members_complete(&mb, 1) || !seqs || !attw_out || !scratch_v) return ACVAE_EINVAL;
  // acvae_topk_flat_batched selects k <= 16 and would answer a wider beam with the same code.  (The decoder GRU's width H is
  // free: the prior LSTM is E wide whatever H is, and every state row is kept, zeroed and gathered by its own width.)
  if (start_idx < 0 || start_idx >= V || beam > 16) return ACVAE_EINVAL;
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  return search(&mb, 1, L, start_idx, end_idx, Pick{PICK_BEAM}, seqs, nullptr, attw_out, (float*)scratch_v, N, beam,
                max_length, V, con, fin, (hipStream_t)stream);
}

int ensemble_search_entry(const void* const* const* params, const float* const* mem, const int64_t* const* mem_lens,
                          const float* const* eps, const int* S, const int* E, const int* H, const int* A, int M,
                          int64_t start_idx, int64_t end_idx, int greedy, int64_t* seqs, float* logprobs, void* scratch_v,
                          int64_t scratch_bytes, int N, int beam, int max_length, int V, const acvae::Constraints& con,
                          const Finishing& fin, void* stream) {
  SearchMember mb[ACVAE_ENSEMBLE_MAX];
  ACVAE_TRY(members_of(mb, M, S, E, H, A, params, mem, mem_lens, eps));
  if (!members_complete(mb, M) || !seqs || !logprobs || !scratch_v) return ACVAE_EINVAL;
  if (beam > 64 || (greedy && beam != 1)) return ACVAE_EINVAL;
  if (start_idx < 0 || start_idx >= V || end_idx < 0 || end_idx >= V) return ACVAE_EINVAL;
  ACVAE_TRY(acvae::constraints_check_loop(con, V, (int)end_idx, max_length, beam));
  SearchLayout L;
  if (fin.on && greedy) return ACVAE_EINVAL;             // a greedy row has nothing to choose among
  ACVAE_TRY(finishing_check(fin, beam, max_length));
  ACVAE_TRY(search_layout(mb, M, N, beam, max_length, V, 0, (con.on() || fin.on) && !greedy, fin.on, L));
  if (!greedy && beam > 16) return ACVAE_EUNSUPPORTED;   // acvae_topk_flat_batched selects k <= 16: refused here, not mid-call
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  return search(mb, M, L, start_idx, end_idx, Pick{greedy ? ACVAE_SAMPLE_GREEDY : PICK_BEAM}, seqs, logprobs, nullptr,
                (float*)scratch_v, N, beam, max_length, V, con, fin, (hipStream_t)stream);
}

// A rollout of sample_n rows per clip: the driver with a rollout's pick, and a rollout's refusals in front of it.
int ensemble_rollout_entry(const void* const* const* params, const float* const* mem, const int64_t* const* mem_lens,
                           const float* const* eps, const int* S, const int* E, const int* H, const int* A, int M,
                           int64_t start_idx, int64_t end_idx, const Pick& pick, int64_t* seqs, float* logprobs,
                           void* scratch_v, int64_t scratch_bytes, int N, int sample_n, int max_length, int V,
                           const acvae::Constraints& con, void* stream) {
  SearchMember mb[ACVAE_ENSEMBLE_MAX];
  ACVAE_TRY(members_of(mb, M, S, E, H, A, params, mem, mem_lens, eps));
  if (!members_complete(mb, M) || !seqs || !logprobs || !scratch_v) return ACVAE_EINVAL;
  if (sample_n < 1) return ACVAE_EINVAL;
  if (pick.mode != ACVAE_SAMPLE_GREEDY && pick.mode != ACVAE_SAMPLE_GUMBEL && pick.mode != ACVAE_SAMPLE_MULTINOMIAL)
    return ACVAE_EINVAL;
  if (!isfinite(pick.temp) || !(pick.temp > 0.f)) return ACVAE_EINVAL;
  if (pick.top_k < 0 || !(pick.top_p > 0.f && pick.top_p <= 1.f)) return ACVAE_EINVAL;     // (a NaN top_p fails both)
  if (pick.mode == ACVAE_SAMPLE_GREEDY ? pick.truncated() : !pick.noise) return ACVAE_EINVAL;
  if (start_idx < 0 || start_idx >= V || end_idx < 0 || end_idx >= V) return ACVAE_EINVAL;
  ACVAE_TRY(acvae::constraints_check_loop(con, V, (int)end_idx, max_length, 1));
  SearchLayout L;
  ACVAE_TRY(search_layout(mb, M, N, sample_n, max_length, V, 0, 0, 0, L));
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  return search(mb, M, L, start_idx, end_idx, pick, seqs, logprobs, nullptr, (float*)scratch_v, N, sample_n, max_length, V,
                con, Finishing{}, (hipStream_t)stream);
}

acvae::Constraints constraints_of(float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                  const int* suppress_host, int n_suppress) {
  acvae::Constraints c;
  c.repetition_penalty = repetition_penalty; c.no_repeat_ngram_size = no_repeat_ngram_size; c.min_length = min_length;
  c.suppress = suppress_host; c.n_suppress = n_suppress;
  return c;
}

Finishing finishing_of(const float* length_norm_host, int nbest, int64_t* nb_seqs, float* nb_scores, float* nb_logprobs,
                       int* nb_lengths) {
  Finishing f;
  f.on = 1; f.nbest = nbest; f.norm = length_norm_host;
  f.nb_seqs = nb_seqs; f.nb_scores = nb_scores; f.nb_logprobs = nb_logprobs; f.nb_lengths = nb_lengths;
  return f;
}

int64_t ensemble_scratch(int M, int N, int beam, int max_length, const int* S, const int* E, const int* H, const int* A, int V,
                         int keep_hist, int keep_fin = 0, int keep_attw = 0) {
  SearchMember mb[ACVAE_ENSEMBLE_MAX];
  if (members_of(mb, M, S, E, H, A) != ACVAE_OK) return -1;
  SearchLayout L;
  return layout_bytes(search_layout(mb, M, N, beam, max_length, V, keep_attw, keep_hist, keep_fin, L), L);
}
int64_t beam_scratch(int N, int beam, int max_length, int S, int E, int H, int A, int V, int keep_hist, int keep_fin = 0) {
  return ensemble_scratch(1, N, beam, max_length, &S, &E, &H, &A, V, keep_hist, keep_fin, 1);
}
}  // namespace

extern "C" int64_t acvae_beam_search_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A, int V) {
  return beam_scratch(N, beam, max_length, S, E, H, A, V, 0);
}
extern "C" int64_t acvae_beam_search_constrained_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A,
                                                               int V) {
  return beam_scratch(N, beam, max_length, S, E, H, A, V, 1);
}

extern "C" int acvae_beam_search(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                                 int64_t start_idx, int64_t* seqs, float* attw_out, void* scratch_v, int64_t scratch_bytes,
                                 int N, int beam, int max_length, int S, int E, int H, int A, int V, void* stream) {
  return beam_search_entry(params, mem, mem_lens, eps, start_idx, seqs, attw_out, scratch_v, scratch_bytes, N, beam,
                           max_length, S, E, H, A, V, 0, acvae::Constraints{}, Finishing{}, stream);
}
extern "C" int acvae_beam_search_constrained(const void* const* params, const float* mem, const int64_t* mem_lens,
                                             const float* eps, int64_t start_idx, int64_t* seqs, float* attw_out,
                                             void* scratch_v, int64_t scratch_bytes, int N, int beam, int max_length, int S,
                                             int E, int H, int A, int V, void* stream, int64_t end_idx,
                                             float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                             const int* suppress_host, int n_suppress) {
  return beam_search_entry(params, mem, mem_lens, eps, start_idx, seqs, attw_out, scratch_v, scratch_bytes, N, beam,
                           max_length, S, E, H, A, V, end_idx,
                           constraints_of(repetition_penalty, no_repeat_ngram_size, min_length, suppress_host, n_suppress),
                           Finishing{}, stream);
}
extern "C" int64_t acvae_beam_search_finishing_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A,
                                                             int V) {
  return beam_scratch(N, beam, max_length, S, E, H, A, V, 1, 1);
}
extern "C" int acvae_beam_search_finishing(const void* const* params, const float* mem, const int64_t* mem_lens,
                                           const float* eps, int64_t start_idx, int64_t* seqs, float* attw_out,
                                           void* scratch_v, int64_t scratch_bytes, int N, int beam, int max_length, int S,
                                           int E, int H, int A, int V, void* stream, int64_t end_idx,
                                           float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                           const int* suppress_host, int n_suppress, const float* length_norm_host,
                                           int nbest, int64_t* nbest_seqs, float* nbest_scores, float* nbest_logprobs,
                                           int* nbest_lengths) {
  return beam_search_entry(params, mem, mem_lens, eps, start_idx, seqs, attw_out, scratch_v, scratch_bytes, N, beam,
                           max_length, S, E, H, A, V, end_idx,
                           constraints_of(repetition_penalty, no_repeat_ngram_size, min_length, suppress_host, n_suppress),
                           finishing_of(length_norm_host, nbest, nbest_seqs, nbest_scores, nbest_logprobs, nbest_lengths),
                           stream);
}

extern "C" int64_t acvae_ensemble_search_scratch_bytes(int M, int N, int beam, int max_length, const int* S, const int* E,
                                                       const int* H, const int* A, int V) {
  return ensemble_scratch(M, N, beam, max_length, S, E, H, A, V, 0);
}
extern "C" int64_t acvae_ensemble_search_constrained_scratch_bytes(int M, int N, int beam, int max_length, const int* S,
                                                                   const int* E, const int* H, const int* A, int V) {
  return ensemble_scratch(M, N, beam, max_length, S, E, H, A, V, 1);
}

extern "C" int acvae_ensemble_search(const void* const* const* params, const float* const* mem,
                                     const int64_t* const* mem_lens, const float* const* eps, const int* S, const int* E,
                                     const int* H, const int* A, int M, int64_t start_idx, int64_t end_idx, int greedy,
                                     int64_t* seqs, float* logprobs, void* scratch_v, int64_t scratch_bytes, int N, int beam,
                                     int max_length, int V, void* stream) {
  return ensemble_search_entry(params, mem, mem_lens, eps, S, E, H, A, M, start_idx, end_idx, greedy, seqs, logprobs,
                               scratch_v, scratch_bytes, N, beam, max_length, V, acvae::Constraints{}, Finishing{}, stream);
}
extern "C" int acvae_ensemble_search_constrained(const void* const* const* params, const float* const* mem,
                                                 const int64_t* const* mem_lens, const float* const* eps, const int* S,
                                                 const int* E, const int* H, const int* A, int M, int64_t start_idx,
                                                 int64_t end_idx, int greedy, int64_t* seqs, float* logprobs,
                                                 void* scratch_v, int64_t scratch_bytes, int N, int beam, int max_length,
                                                 int V, void* stream, float repetition_penalty, int no_repeat_ngram_size,
                                                 int min_length, const int* suppress_host, int n_suppress) {
  return ensemble_search_entry(params, mem, mem_lens, eps, S, E, H, A, M, start_idx, end_idx, greedy, seqs, logprobs,
                               scratch_v, scratch_bytes, N, beam, max_length, V,
                               constraints_of(repetition_penalty, no_repeat_ngram_size, min_length, suppress_host, n_suppress),
                               Finishing{}, stream);
}
extern "C" int64_t acvae_ensemble_search_finishing_scratch_bytes(int M, int N, int beam, int max_length, const int* S,
                                                                 const int* E, const int* H, const int* A, int V) {
  return ensemble_scratch(M, N, beam, max_length, S, E, H, A, V, 1, 1);
}
extern "C" int acvae_ensemble_search_finishing(const void* const* const* params, const float* const* mem,
                                               const int64_t* const* mem_lens, const float* const* eps, const int* S,
                                               const int* E, const int* H, const int* A, int M, int64_t start_idx,
                                               int64_t end_idx, int greedy, int64_t* seqs, float* logprobs, void* scratch_v,
                                               int64_t scratch_bytes, int N, int beam, int max_length, int V, void* stream,
                                               float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                               const int* suppress_host, int n_suppress, const float* length_norm_host,
                                               int nbest, int64_t* nbest_seqs, float* nbest_scores, float* nbest_logprobs,
                                               int* nbest_lengths) {
  return ensemble_search_entry(params, mem, mem_lens, eps, S, E, H, A, M, start_idx, end_idx, greedy, seqs, logprobs,
                               scratch_v, scratch_bytes, N, beam, max_length, V,
                               constraints_of(repetition_penalty, no_repeat_ngram_size, min_length, suppress_host, n_suppress),
                               finishing_of(length_norm_host, nbest, nbest_seqs, nbest_scores, nbest_logprobs, nbest_lengths),
                               stream);
}

extern "C" int64_t acvae_ensemble_rollout_scratch_bytes(int M, int N, int sample_n, int max_length, const int* S,
                                                        const int* E, const int* H, const int* A, int V) {
  return sample_n < 1 ? -1 : ensemble_scratch(M, N, sample_n, max_length, S, E, H, A, V, 0);
}
extern "C" int acvae_ensemble_rollout(const void* const* const* params, const float* const* mem,
                                      const int64_t* const* mem_lens, const float* const* eps, const int* S, const int* E,
                                      const int* H, const int* A, int M, int64_t start_idx, int64_t end_idx, int method,
                                      float temp, int top_k, float top_p, const float* noise, int64_t* seqs, float* logprobs,
                                      void* scratch_v, int64_t scratch_bytes, int N, int sample_n, int max_length, int V,
                                      void* stream, float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                      const int* suppress_host, int n_suppress) {
  Pick pick{method, noise, temp, top_k, top_p};
  return ensemble_rollout_entry(params, mem, mem_lens, eps, S, E, H, A, M, start_idx, end_idx, pick, seqs, logprobs,
                                scratch_v, scratch_bytes, N, sample_n, max_length, V,
                                constraints_of(repetition_penalty, no_repeat_ngram_size, min_length, suppress_host, n_suppress),
                                stream);
}

// ---- the two finishing kernels alone, on caller-built histories
extern "C" int acvae_beam_retire(float* c, const int64_t* word, float* f, int64_t end_idx, int last, int R, void* stream) {
  if (!c || !word || !f || R <= 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(beam_retire_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, word, f, end_idx,
                     last != 0, R);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
extern "C" int acvae_beam_finish(const int64_t* parent, const int64_t* word, int64_t hist_stride, const float* f,
                                 const float* length_norm_host, float* norm_dev, const float* attw, int64_t* seqs,
                                 float* logprobs, float* attw_out, int64_t* nbest_seqs, float* nbest_scores,
                                 float* nbest_logprobs, int* nbest_lengths, int N, int beam, int T, int S, int nbest,
                                 int64_t end_idx, void* stream) {
  if (N <= 0 || beam <= 0 || T <= 0 || (long)N * beam > (1L << 20)) return ACVAE_EINVAL;
  ACVAE_TRY(finishing_check(finishing_of(length_norm_host, nbest, nbest_seqs, nbest_scores, nbest_logprobs, nbest_lengths),
                            beam, T));
  if (!parent || !word || !f || !norm_dev || hist_stride < (long)N * beam) return ACVAE_EINVAL;
  if ((attw == nullptr) != (attw_out == nullptr) || (attw && S <= 0)) return ACVAE_EINVAL;
  ACVAE_TRY(norm_upload(length_norm_host, norm_dev, T, (hipStream_t)stream));
  hipLaunchKernelGGL(beam_finish_kernel, dim3(N), dim3(FIN_THREADS), 0, (hipStream_t)stream, parent, word, (long)hist_stride,
                     f, norm_dev, attw, seqs, logprobs, attw_out, nbest_seqs, nbest_scores, nbest_logprobs, nbest_lengths,
                     N * beam, beam, T, S, nbest, end_idx);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// ==========================================================================================
// Diverse beam search as ONE call, over M >= 1 members (include/acvae_hip.h has the definition): CaptionModel.
// diverse_beam_search, models/word_model.py:297-394, with Hybrid_VAEModel's step.  G groups of bdash beams per clip, all
// N clips together: a group's step runs R = N * bdash rows through prior_step / decoder_step exactly as search() does, so
// the logits are the step API's bits.  Every (time step, group) pair is: the members' steps, the mix (M > 1 only), the
// scores with the sparse penalty (losses.hip), the flat top-k, dbs_advance_kernel, and the state gather by parent.  The
// groups' parent / word / record tables [G][T][R] stay in the scratch; dbs_finish_kernel ranks and traces at the end.
// No atomics, no hand-off between workgroups, no host synchronisation.
// ==========================================================================================
namespace {
// Behind the top-k of step (g, lt): the step's parent and word go into the group's tables, the row's record is its
// score c if it emitted end_idx or this is the last step (else "none", a NaN), and a recorded row is retired:
// c <- c - 1000.0f.  One thread per row.
__global__ __launch_bounds__(256) void dbs_advance_kernel(float* __restrict__ c, const int64_t* __restrict__ parent,
                                                          const int64_t* __restrict__ word, int* __restrict__ par_out,
                                                          int* __restrict__ word_out, float* __restrict__ rec_out,
                                                          int64_t end_idx, int last, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float v = c[r];
  const int64_t w = word[r];
  const bool ends = acvae::dbs::recorded(w, end_idx, last);
  par_out[r] = (int)parent[r];
  word_out[r] = (int)w;
  rec_out[r] = ends ? v : acvae::dbs::no_record();
  if (ends) c[r] = acvae::dbs::retired(v);
}
// One wavefront per (clip, group).  `keep` selection passes over the group's T * bdash records in beam_finish_kernel's
// idiom: key (double)c / (double)(lt + 1), descending, ties to the lower candidate index i = lt * bdash + b, which is the
// order of recording.  Then lane q walks record q's parents back from its step.  A parent outside [0, R) is clamped.
__global__ __launch_bounds__(64) void dbs_finish_kernel(const int* __restrict__ par_tab, const int* __restrict__ word_tab,
                                                        const float* __restrict__ rec, int64_t* __restrict__ seqs,
                                                        double* __restrict__ scores, int* __restrict__ lengths, int R,
                                                        int bdash, int T, int keep, int64_t end_idx) {
  __shared__ int sel[16];
  namespace D = acvae::dbs;
  const int n = blockIdx.x, g = blockIdx.y, G = gridDim.y, lane = threadIdx.x;
  const int cand = T * bdash;
  for (int q = 0; q < keep; ++q) {
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < cand; i += 64) {
      const int lt = D::cand_step(i, bdash);
      const float fv = rec[D::at(g, lt, D::cand_row(i, bdash, n), T, R)];
      if (!D::is_record(fv)) continue;
      bool taken = false;
      for (int p = 0; p < q; ++p) taken = taken || (sel[p] == i);
      const double v = D::key(fv, lt);
      if (!taken && D::better(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (D::better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) sel[q] = bi == 0x7fffffff ? -1 : bi;
    __syncthreads();
  }
  if (lane >= keep) return;
  const int i = sel[lane];
  const int t0 = i < 0 ? -1 : D::cand_step(i, bdash);
  const long r = i < 0 ? 0 : D::cand_row(i, bdash, n);
  const long o = D::out_row(n, g, lane, G, keep);
  scores[o] = i < 0 ? -INFINITY : D::key(rec[D::at(g, t0, r, T, R)], t0);
  lengths[o] = t0 + 1;
  D::trace(par_tab, word_tab, g, t0, r, T, R, end_idx, seqs + o * T);
}

struct DbsLayout { MemberLayout m[ACVAE_ENSEMBLE_MAX]; long mix, scores, gscore, gword, gpar, idx, par_tab, word_tab, rec, total; };
int dbs_layout(const SearchMember* mb, int M, int N, int G, int bdash, int T, int V, DbsLayout& L) {
  if (M < 1 || M > ACVAE_ENSEMBLE_MAX || N <= 0 || G <= 0 || bdash <= 0 || T <= 0) return ACVAE_EINVAL;
  if (G > 16 || bdash > 16) return ACVAE_EUNSUPPORTED;
  const long R = (long)N * bdash;
  if (R > (1L << 20)) return ACVAE_EUNSUPPORTED;
  Bump b;
  for (int m = 0; m < M; ++m) ACVAE_TRY(member_layout(b, mb[m], N, R, G, 1, V, L.m[m]));
  L.mix = M > 1 ? b.take(R * V) : 0;
  L.scores = b.take(R * V);
  L.gscore = b.take((long)G * R);
  L.gword = b.take(2 * (long)G * R);                     // int64 [G][R]: the word each group's next step is fed
  L.gpar = b.take(2 * (long)G * R);                      // int64 [G][R]: its parent rows
  L.idx = b.take(2 * R);                                 // int64 [R]: the top-k's flat indices (unused)
  L.par_tab = b.take((long)G * T * R);                   // int32 [G][T][R]
  L.word_tab = b.take((long)G * T * R);
  L.rec = b.take((long)G * T * R);
  L.total = b.off;
  return ACVAE_OK;
}

int dbs_search(const SearchMember* mb, int M, const DbsLayout& L, int64_t start_idx, int64_t end_idx, int N, int G,
               int bdash, int T, int V, float temperature, float lambda, int group_nbest, int64_t* seqs, double* scores,
               int* lengths, float* sc, hipStream_t s) {
  const int R = N * bdash;
  const float* logit_ptr[ACVAE_ENSEMBLE_MAX];
  int64_t logit_ld[ACVAE_ENSEMBLE_MAX];
  for (int m = 0; m < M; ++m)                            // lt = 0: every group's states are zero
    ACVAE_TRY(member_prologue(mb[m], L.m[m], sc, N, R, G, V, logit_ptr[m], logit_ld[m], s));
  float* gscore = sc + L.gscore;
  int64_t* gword = (int64_t*)(sc + L.gword);
  int64_t* gpar = (int64_t*)(sc + L.gpar);
  int64_t* idx = (int64_t*)(sc + L.idx);
  int* par_tab = (int*)(sc + L.par_tab);
  int* word_tab = (int*)(sc + L.word_tab);
  float* rec = sc + L.rec;
  auto group_states = [&](int m, int g) { return sc + L.m[m].cur + (long)g * R * (mb[m].H + 3 * mb[m].E); };
  ACVAE_TRY(zero(gscore, (long)G * R, s));
  hipLaunchKernelGGL(fill_words_kernel, dim3((G * R + 255) / 256), dim3(256), 0, s, gword, start_idx, G * R);
  long k = 0;
  for (int t = 0; t < T + G - 1; ++t) {
    for (int g = 0; g < G; ++g) {
      const int lt = t - g;
      if (lt < 0 || lt > T - 1) continue;
      int64_t* w_g = gword + (long)g * R;
      int64_t* par_g = gpar + (long)g * R;
      float* c_g = gscore + (long)g * R;
      for (int m = 0; m < M; ++m)
        ACVAE_TRY(member_step(mb[m], L.m[m], sc, w_g, group_states(m, g), sc + L.m[m].nxt, mb[m].eps + k * R * mb[m].E,
                              sc + L.m[m].attw, N, bdash, V, s));
      const float* x = sc + L.m[0].logits;
      if (M > 1) {                                       // log(mean_m softmax(logits_m)) takes the logits' place
        ACVAE_TRY(acvae_ensemble_mix(logit_ptr, logit_ld, M, nullptr, sc + L.mix, V, nullptr, nullptr, 0, R, V, s));
        x = sc + L.mix;
      }
      ACVAE_TRY(acvae_dbs_scores_sparse(x, V, temperature, lambda, c_g, sc + L.scores, par_tab, word_tab, N, bdash, T, V, G,
                                        g, lt, s));
      ACVAE_TRY(acvae_topk_flat_batched(sc + L.scores, lt == 0 ? (int64_t)V : (int64_t)bdash * V, (int64_t)bdash * V, bdash,
                                        V, c_g, idx, par_g, w_g, N, bdash, s));
      const long at = ((long)g * T + lt) * R;
      hipLaunchKernelGGL(dbs_advance_kernel, dim3((R + 255) / 256), dim3(256), 0, s, c_g, par_g, w_g, par_tab + at,
                         word_tab + at, rec + at, end_idx, lt == T - 1, R);
      if (lt + 1 < T)                                    // the group's next step reads its states through the parents
        for (int m = 0; m < M; ++m) member_gather(mb[m], group_states(m, g), sc + L.m[m].nxt, R, par_g, nullptr, s);
      ++k;
    }
  }
  hipLaunchKernelGGL(dbs_finish_kernel, dim3(N, G), dim3(64), 0, s, par_tab, word_tab, rec, seqs, scores, lengths, R, bdash,
                     T, group_nbest ? bdash : 1, end_idx);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

int dbs_entry(const SearchMember* mb, int M, int64_t start_idx, int64_t end_idx, int N, int G, int bdash, int T, int V,
              float temperature, float lambda, int group_nbest, int64_t* seqs, double* scores, int* lengths, void* scratch_v,
              int64_t scratch_bytes, void* stream) {
  DbsLayout L;
  ACVAE_TRY(dbs_layout(mb, M, N, G, bdash, T, V, L));
  if (!members_complete(mb, M) || !seqs || !scores || !lengths || !scratch_v) return ACVAE_EINVAL;
  if (start_idx < 0 || start_idx >= V || end_idx < 0 || end_idx >= V) return ACVAE_EINVAL;
  if (!(temperature > 0.f) || !isfinite(temperature) || !isfinite(lambda)) return ACVAE_EINVAL;
  if (scratch_bytes < L.total * 4) return ACVAE_EWORKSPACE;
  return dbs_search(mb, M, L, start_idx, end_idx, N, G, bdash, T, V, temperature, lambda, group_nbest, seqs, scores, lengths,
                    (float*)scratch_v, (hipStream_t)stream);
}
}  // namespace

extern "C" int64_t acvae_dbs_search_scratch_bytes(int N, int G, int bdash, int T, int S, int E, int H, int A, int V) {
  return acvae_ensemble_dbs_search_scratch_bytes(1, N, G, bdash, T, &S, &E, &H, &A, V);
}
extern "C" int acvae_dbs_search(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                                int64_t start_idx, int64_t end_idx, int N, int G, int bdash, int T, int S, int E, int H, int A,
                                int V, float temperature, float diversity_lambda, int group_nbest, int64_t* seqs,
                                double* scores, int* lengths, void* scratch, int64_t scratch_bytes, void* stream) {
  const SearchMember mb{params, mem, mem_lens, eps, S, E, H, A};
  return dbs_entry(&mb, 1, start_idx, end_idx, N, G, bdash, T, V, temperature, diversity_lambda, group_nbest, seqs, scores,
                   lengths, scratch, scratch_bytes, stream);
}
extern "C" int64_t acvae_ensemble_dbs_search_scratch_bytes(int M, int N, int G, int bdash, int T, const int* S, const int* E,
                                                           const int* H, const int* A, int V) {
  SearchMember mb[ACVAE_ENSEMBLE_MAX];
  if (members_of(mb, M, S, E, H, A) != ACVAE_OK) return -1;
  DbsLayout L;
  return layout_bytes(dbs_layout(mb, M, N, G, bdash, T, V, L), L);
}
extern "C" int acvae_ensemble_dbs_search(const void* const* const* params, const float* const* mem,
                                         const int64_t* const* mem_lens, const float* const* eps, const int* S, const int* E,
                                         const int* H, const int* A, int M, int64_t start_idx, int64_t end_idx, int N, int G,
                                         int bdash, int T, int V, float temperature, float diversity_lambda, int group_nbest,
                                         int64_t* seqs, double* scores, int* lengths, void* scratch, int64_t scratch_bytes,
                                         void* stream) {
  SearchMember mb[ACVAE_ENSEMBLE_MAX];
  if (!params || !mem || !mem_lens || !eps) return ACVAE_EINVAL;   // (in front of the layout's refusals, as M and the widths)
  ACVAE_TRY(members_of(mb, M, S, E, H, A, params, mem, mem_lens, eps));
  return dbs_entry(mb, M, start_idx, end_idx, N, G, bdash, T, V, temperature, diversity_lambda, group_nbest, seqs, scores,
                   lengths, scratch, scratch_bytes, stream);
}

// ---- the advance and finish kernels alone, on caller-built tables
extern "C" int acvae_dbs_advance(float* c, const int64_t* parent, const int64_t* word, int* parent_out, int* word_out,
                                 float* rec_out, int64_t end_idx, int last, int R, void* stream) {
  if (!c || !parent || !word || !parent_out || !word_out || !rec_out || R <= 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(dbs_advance_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, parent, word,
                     parent_out, word_out, rec_out, end_idx, last != 0, R);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
extern "C" int acvae_dbs_finish(const int* parent_tab, const int* word_tab, const float* rec, int64_t* seqs, double* scores,
                                int* lengths, int N, int G, int bdash, int T, int group_nbest, int64_t end_idx,
                                void* stream) {
  if (!parent_tab || !word_tab || !rec || !seqs || !scores || !lengths || N <= 0 || G <= 0 || bdash <= 0 || T <= 0)
    return ACVAE_EINVAL;
  if (G > 16 || bdash > 16 || (long)N * bdash > (1L << 20)) return ACVAE_EUNSUPPORTED;
  hipLaunchKernelGGL(dbs_finish_kernel, dim3(N, G), dim3(64), 0, (hipStream_t)stream, parent_tab, word_tab, rec, seqs,
                     scores, lengths, N * bdash, bdash, T, group_nbest ? bdash : 1, end_idx);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
