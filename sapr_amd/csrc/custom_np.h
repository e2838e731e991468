// What the four custom-HMM units (custom_emission.hip, custom_estep.hip, custom_decode.hip, custom_update.hip) share:
// the shape limits, numpy's logaddexp and pair-wise sum in numpy's own operation order, the model pack and the lattice
// view.  Like lse_ops.h and smooth_ops.h this header is included INSIDE the unit's `namespace sapr { namespace {`, after
// sapr_common.h and <type_traits>; the tables of lse_unit.h are per translation unit.
//
// float64 throughout; exp / reciprocal / log(1 + e) of the two-term logaddexp come from lse_unit.h (agreement with
// numpy ~1e-13, the tests use 1e-9).
#pragma once

constexpr int kMaxS = 20, kMaxD = 40;  // run-time shapes: 3 <= S <= kMaxS states, D <= kMaxD dimensions
constexpr int kBlock = 64;             // one lane per (utterance, model) problem, one wavefront per workgroup

#include "lse_unit.h"

// numpy's logaddexp (npy_logaddexp)
// np.logaddexp(a, b) together with the shares of its two arguments in the sum, exp(a - r) and exp(b - r), from the
// exponential it evaluates anyway (one division instead of two more exponentials)
__device__ __forceinline__ double np_logaddexp_shares(double a, double b, double &share_a, double &share_b) {
  // npy_logaddexp's three cases (a == b; a > b: a + log1p(exp(b - a)); a <= b: b + log1p(exp(a - b)); NaN otherwise) as
  // ONE evaluation with selects: the lanes of a wavefront are different utterances and disagree about which argument
  // is the larger, so as branches both sides ran for every call (16 exponentials and 32 divisions per frame of the
  // forward loop at 10 states instead of 8 and 16).  exp(-|a - b|) is the argument either branch would pass; NaN
  // runs through the arithmetic to the result and to both shares.
  const double tmp = a - b;
  double e, inv, l1p;  // exp(-|a - b|), 1 / (1 + e), log(1 + e) from one short chain (lse_unit.h, round 4)
  lse2_terms(fabs(tmp), &e, &inv, &l1p);
  const double small = e * inv;
  const bool a_larger = tmp > 0;
  const bool same = a == b;  // handles inf == inf
  const double r = (a_larger ? a : b) + l1p;
  share_a = same ? 0.5 : (a_larger ? inv : small);
  share_b = same ? 0.5 : (a_larger ? small : inv);
  return same ? a + 0.693147180559945309417232121458176568 : r;
}
__device__ __forceinline__ double np_logaddexp(double a, double b) {
  const double tmp = a - b;
  double e, inv, l1p;
  lse2_terms(fabs(tmp), &e, &inv, &l1p);
  const double r = (tmp > 0 ? a : b) + l1p;
  return a == b ? a + 0.693147180559945309417232121458176568 : r;  // handles inf == inf
}

// numpy pair-wise sum of n strided values: blocks of <= 128 with 8 accumulators, recursive halving
// above.  The recursion is unrolled at compile time (depth 8: n <= 32768) — device code with a real
// recursive call needs a dynamic stack, which this library avoids.
template <typename T>
__device__ __forceinline__ T np_pairwise_block(const T *p, int n, int stride) {
  if (n < 8) {
    T r = 0;
    for (int i = 0; i < n; ++i) r += p[static_cast<int64_t>(i) * stride];
    return r;
  }
  T r[8];
  for (int j = 0; j < 8; ++j) r[j] = p[static_cast<int64_t>(j) * stride];
  int i;
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += p[static_cast<int64_t>(i + j) * stride];
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += p[static_cast<int64_t>(i) * stride];
  return res;
}
template <typename T, int DEPTH>
__device__ T np_pairwise(const T *p, int n, int stride) {
  if constexpr (DEPTH == 0) {
    return np_pairwise_block<T>(p, n, stride);
  } else {
    if (n <= 128) return np_pairwise_block<T>(p, n, stride);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise<T, DEPTH - 1>(p, n2, stride) +
           np_pairwise<T, DEPTH - 1>(p + static_cast<int64_t>(n2) * stride, n - n2, stride);
  }
}

template <int B, int E, class F>
__device__ __forceinline__ void static_for_c(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for_c<B + 1, E>(f);
  }
}

struct CustomPack {
  const double *means;   // [W][S][D]
  const double *inv;     // [W][S][D][D]  inverse of (cov + 1e-6 I), numpy/LAPACK on the host
  const double *cterm;   // [W][S]        D*log(2*pi) + logdet
  const double *A;       // [W][S][S]
  const double *logA;    // [W][S][S]     np.log(A) (−inf for zeros)
};

// A (T, S) lattice of one utterance: element (t, j) lives at p[(t * S + j) * es].  es = 1 is the
// reference's per-utterance row layout (what the per-method API hands out); es = n_slots with p offset
// by the utterance's slot is the lane-contiguous layout the batched E-step uses internally, where the
// 64 lanes of a wavefront touch 64 consecutive doubles (one 512-byte row) instead of 64 cache lines.
struct Lat {
  double *p;
  int64_t es;
  int S;
  __device__ __forceinline__ double &at(int t, int j) const { return p[(static_cast<int64_t>(t) * S + j) * es]; }
};

// host: the shapes every entry point of the four units accepts
inline int check_dims(int S, int D) {
  if (S < 3 || S > kMaxS || D < 1 || D > kMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "custom-HMM kernels support 3 <= S <= %d, D <= %d (got S=%d D=%d)", kMaxS,
                kMaxD, S, D);
  return 0;
}
