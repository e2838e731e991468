// The rows of the backward half — the posterior soft-max, the dense backward_log row and the bidiagonal smoothing step —
// shared by estep.hip (fb_smooth_kernel, fb_smooth_obs_kernel, fb_backward_dense_kernel) and the posterior lattice of
// state_posteriors.hip.  Like lse_ops.h this header is included INSIDE the unit's `namespace sapr { namespace {`, after
// lse_ops.h (exp_unit, lse_all).
#pragma once

// base.py _compute_posteriors_log, one row: g = exp(lg - logsumexp(lg)), evaluated as exp(lg - max) / sum — the S
// exponentials of the logsumexp are the numerators
template <int S>
__device__ __forceinline__ void softmax_row(const double (&lg)[S], double (&g)[S]) {
  double mx = lg[0];
#pragma unroll
  for (int s = 1; s < S; ++s) mx = lg[s] > mx ? lg[s] : mx;
  double e[S], den = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    e[s] = exp_unit(lg[s] - mx);  // all -inf: NaN, as exp(lg - (-inf)) is in the reference
    den += e[s];
  }
  const double inv = 1.0 / den;
#pragma unroll
  for (int s = 0; s < S; ++s) g[s] = e[s] * inv;
}

// the posteriors of an utterance's last frame: the soft-max of row T - 1 of a [t][s][slot] lattice of forward values
template <int S>
__device__ __forceinline__ void softmax_last_row(const double *__restrict__ lat_b, int64_t n_slots, int64_t slot, int T,
                                                 double (&g)[S]) {
  double lg[S];
#pragma unroll
  for (int s = 0; s < S; ++s) lg[s] = lat_b[(static_cast<int64_t>(T - 1) * S + s) * n_slots + slot];
  softmax_row<S>(lg, g);
}

// _hmmc.cpp backward_log, one row of a dense model: nb[i] = logsumexp_j(log a_ij + b_t[j] + bwd_t[j]) = bwd_(t-1)[i]
template <int S>
__device__ __forceinline__ void dense_backward_row(const double *__restrict__ lt, const double *b_t,
                                                   const double (&bwd)[S], double (&nb)[S]) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    double work[S];
#pragma unroll
    for (int j = 0; j < S; ++j) work[j] = lt[i * S + j] + b_t[j] + bwd[j];
    nb[i] = lse_all<S>(work);
  }
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
