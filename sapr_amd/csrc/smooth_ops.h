// The two helpers of the bidiagonal smoothing recursion (estep.hip: fb_smooth_kernel, fb_smooth_obs_kernel), shared with
// the posterior lattice of state_posteriors.hip.  Like lse_ops.h this header is included INSIDE the unit's
// `namespace sapr { namespace {`, after lse_ops.h (exp_unit).
#pragma once

template <int S>
__device__ __forceinline__ void softmax_last_row(const double *__restrict__ lat_b, int64_t n_slots, int64_t slot, int T,
                                                 double (&g)[S]) {
  double lg[S];
#pragma unroll
  for (int s = 0; s < S; ++s) lg[s] = lat_b[(static_cast<int64_t>(T - 1) * S + s) * n_slots + slot];
  double mx = lg[0];
#pragma unroll
  for (int s = 1; s < S; ++s) mx = lg[s] > mx ? lg[s] : mx;
  double den = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    lg[s] = exp_unit(lg[s] - mx);  // all -inf: NaN, as exp(lg - (-inf)) is in the reference
    den += lg[s];
  }
  const double inv = 1.0 / den;
#pragma unroll
  for (int s = 0; s < S; ++s) g[s] = lg[s] * inv;
}

// one step t -> t-1 of the smoothing recursion: g = gamma_t on entry, gamma_(t-1) on exit; xs += the xi terms of the step
// ([i] = (i,i), [S+i-1] = (i-1,i)); st[1..S-1] = the stay shares of frame t
template <int S>
__device__ __forceinline__ void smooth_step(double (&g)[S], const double (&st)[S], double (&xs)[2 * S]) {
  double x_stay[S], x_move[S];
  x_stay[0] = g[0];
  x_move[0] = 0.0;
  xs[0] += x_stay[0];
#pragma unroll
  for (int i = 1; i < S; ++i) {
    x_stay[i] = g[i] * st[i];
    x_move[i] = g[i] - x_stay[i];
    xs[i] += x_stay[i];
    xs[S + i - 1] += x_move[i];
  }
#pragma unroll
  for (int i = 0; i < S; ++i) g[i] = x_stay[i] + (i + 1 < S ? x_move[i + 1] : 0.0);
}
