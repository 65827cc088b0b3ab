// What the text side's two drivers share (decoder.hip: training composites; search.hip: inference search): the scratch
// bump allocator, the call context with its skinny-GEMM shorthand, and the text-parameter table.
#pragma once
#include "common.h"
#include "conv.h"
#include "../../include/acvae_hip.h"

namespace {

struct Bump {
  long off = 0;
  long take(long n) { const long o = off; off = (off + n + 63) & ~63L; return o; }
};

// call context: the stream plus the split-K workspace of the skinny GEMM (converts to hipStream_t for everything else)
struct Ctx {
  hipStream_t s;
  float* skws;
  operator hipStream_t() const { return s; }
};
inline int gemm(const float* A, long lda, const float* B, long ldb, const float* bias, float* C, long ldc, int M, int N,
                int K, int acc, const Ctx& st) {
  return acvae_gemm_nt_dual(A, lda, B, ldb, K, nullptr, 0, nullptr, 0, 0, bias, C, ldc, M, N, acc, st.s, st.skws);
}
inline int zero(float* p, long n, hipStream_t st) {
  return hipMemsetAsync(p, 0, (size_t)n * sizeof(float), st) == hipSuccess ? ACVAE_OK : (int)hipGetLastError();
}

// text-parameter table (state-dict order after the encoder; see include/acvae_hip.h)
enum {
  TP_DEC_EMB, TP_DEC_WIH, TP_DEC_WHH, TP_DEC_BIH, TP_DEC_BHH, TP_DEC_CLS_W, TP_DEC_CLS_B, TP_DEC_ATT_V, TP_DEC_ATT_W,
  TP_DEC_ATT_B, TP_Q_EMB, TP_Q_WIH, TP_Q_WHH, TP_Q_BIH, TP_Q_BHH, TP_Q_WIH_R, TP_Q_WHH_R, TP_Q_BIH_R, TP_Q_BHH_R,
  TP_Q_TML_W, TP_Q_TML_B, TP_P_EMB, TP_P_ATT_V, TP_P_ATT_W, TP_P_ATT_B, TP_P_WIH, TP_P_WHH, TP_P_BIH, TP_P_BHH,
  TP_P_ML_W, TP_P_ML_B, TP_MLO_W, TP_MLO_B, TP_LN_W, TP_LN_B, TP_COUNT
};
static_assert(TP_COUNT == ACVAE_TEXT_NPARAMS, "text parameter table out of sync with the header");

}  // namespace
