// The full-covariance log density of ONE state, shared by full_emit_kernel (fullcov_ops.h: one thread per frame under
// the model of its tile) and full_vocab_kernel (full_vocab.hip: one lane per utterance under every word model).  Like
// gmm_ops.h this header is included INSIDE the unit's `namespace sapr { namespace {`.
//
//   y_i = sum_{j<=i} Winv[i][j] (x_j - mu_j)        logb = c - 1/2 sum_i y_i^2
//
// One running dot product per row of Winv, every FMA an explicit fma(): the build runs with -ffp-contract=off, so the
// same calls in the same order give the same bits in both kernels.  The difference is taken directly (c0 sits near
// -300) and again for every row, so that no second DP-wide vector lives beside the frame.  The frame comes through an
// accessor, as in mix_log_terms: a float32 frame promoted inside the chain is exact.  mu, wr (row stride DP) and c are
// wavefront-uniform.
#pragma once

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
