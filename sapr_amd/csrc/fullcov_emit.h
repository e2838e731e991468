// The pack geometry and the log density of ONE state of the full-covariance models, shared by full_emit_kernel
// (fullcov_ops.h: one thread per frame under the model of its tile) and full_vocab_kernel (full_vocab.hip: one lane per
// utterance under every word model).  Like gmm_ops.h this header is included INSIDE the unit's
// `namespace sapr { namespace {`, after it (kMaxS, kMaxD).
//
//   y_i = sum_{j<=i} Winv[i][j] (x_j - mu_j)        logb = c - 1/2 sum_i y_i^2
//
// One running dot product per row of Winv, every FMA an explicit fma(): the build runs with -ffp-contract=off, so the
// same calls in the same order give the same bits in both kernels.  The difference is taken directly (c0 sits near
// -300) and again for every row, so that no second DP-wide vector lives beside the frame.  The frame comes through an
// accessor, as in mix_log_terms: a float32 frame promoted inside the chain is exact.  mu, wr (row stride DP) and c are
// wavefront-uniform.
#pragma once

// per model: log_start[SP], log_trans[SP][SP], log_transT[SP][SP], c[SP], mu[SP][DP], Winv[SP][DP][DP]
constexpr size_t full_model_doubles(int SP, int DP) {
  return static_cast<size_t>(SP) + 2 * static_cast<size_t>(SP) * SP + static_cast<size_t>(SP) +
         static_cast<size_t>(SP) * DP + static_cast<size_t>(SP) * DP * DP;
}

inline int check_full_shape(int32_t S, int32_t D) {
  if (S > kMaxS || D > kMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "the full-covariance kernels serve S in 1..%d, D in 1..%d; got S=%d D=%d", kMaxS,
                kMaxD, S, D);
  return 0;
}

template <int DP, class FX>
__device__ __forceinline__ double full_log_density(FX x, const double *__restrict__ mu, const double *__restrict__ wr,
                                                   double c) {
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double y = 0.0;
#pragma unroll
    for (int j = 0; j <= i; ++j) y = fma(wr[i * DP + j], x(j) - mu[j], y);
    q = fma(y, y, q);
  }
  return c - 0.5 * q;
}
