// The log-sum-exp forms of hmmlearn's _hmmc.cpp recursions on top of lse_unit.h, shared by the forward kernels of
// estep.hip and forward_vocab.hip.  Like lse_unit.h (whose tables are per translation unit) this header is included
// INSIDE the unit's `namespace sapr { namespace {`, after sapr_common.h.
#pragma once

#include "lse_unit.h"

// _hmmc.cpp logsumexp over the two candidates of a bidiagonal column/row: log(exp(a - m) + exp(b - m)) + m with
// m = max(a, b).  One of the two exponentials is exp(0) = 1, so this is m + log1p(exp(-|a - b|)): one exponential
// instead of two, same value to the last bit or two (the E-step is compared at 1e-9, §4.3).  Round 4: the exponential,
// the reciprocal and the logarithm come from ONE short chain (lse_unit.h: 58 float64 instructions where the library's
// exp, two IEEE divisions and the log1p series took ~105) and the call is branch-free — an infinite maximum (an
// unreachable state, or an overflow) runs the arithmetic on d = 0 and is selected away — so that the nine independent
// calls of a frame interleave instead of forming one dependent chain each behind its own divergent branch.
__device__ __forceinline__ double lse2(double a, double b) {
  // both -inf: a - b is NaN and v_max_f64 returns its other operand, 0 — the arithmetic then runs on d = 0 and the
  // infinite maximum absorbs the finite log 2 (no select on the way: a v_cndmask_b32 that takes its mask from vcc is
  // the slowest vector instruction of this chip, scripts/ubench/mix_rate)
  const double m = __builtin_fmax(a, b), d = __builtin_fmax(__builtin_fabs(a - b), 0.0);
  double e, inv, l1p;
  lse2_terms(d, &e, &inv, &l1p);
  return m + l1p;
}

// the same, together with the share of the SECOND argument in the sum, exp(b - result) = 1 / (1 + e) or e / (1 + e):
// the backward pass of the bidiagonal E-step is a smoothing recursion over these shares (fb_smooth_obs_kernel).  An
// unreachable state (both arguments -inf) gets the share 1/2 of d = 0: its posterior is 0 whatever the share.
__device__ __forceinline__ double lse2_share(double a, double b, double &share_b) {
  const double m = __builtin_fmax(a, b), d = __builtin_fmax(__builtin_fabs(a - b), 0.0);
  double e, inv, l1p;
  lse2_terms(d, &e, &inv, &l1p);
  share_b = b >= a ? inv : e * inv;
  return m + l1p;
}

// _hmmc.cpp logaddexp
__device__ __forceinline__ double logaddexp(double a, double b) {
  const double m = a > b ? a : b;
  double e, inv, l1p;
  lse2_terms(isinf(m) ? 0.0 : fabs(b - a), &e, &inv, &l1p);
  const double r = m + l1p;
  return a == neg_inf() ? b : (b == neg_inf() ? a : r);
}

template <int S>
__device__ __forceinline__ double lse_all(const double (&v)[S]) {
  double m = v[0];
#pragma unroll
  for (int i = 1; i < S; ++i) m = v[i] > m ? v[i] : m;
  if (isinf(m)) return m;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) acc += exp_unit(v[i] - m);
  return log(acc) + m;
}
