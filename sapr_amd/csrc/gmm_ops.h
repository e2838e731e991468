// Device functions and pack geometry shared by the Gaussian-mixture translation units (gmm_hmm.hip: the E-step and
// the Viterbi decoder of one model per tile; gmm_vocab.hip: every utterance under every word model).  Like lse_ops.h
// this header is included INSIDE the unit's `namespace sapr { namespace {`, after sapr_common.h and lse_ops.h.
//
// The whole build runs with -ffp-contract=off and the emission's one FMA is an explicit fma(): the same functions
// called in the same order give the same bits in every kernel that includes them.
#pragma once

constexpr int kMaxS = 18, kMaxM = 8, kMaxD = 39;

constexpr int sp_of(int S) { return S <= 4 ? 4 : (S <= 10 ? 10 : 18); }
constexpr int mp_of(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8)); }
constexpr int dp_of(int D) { return D <= 13 ? 13 : (D <= 26 ? 26 : 39); }

// per model: log_start[SP], log_trans[SP][SP], its transpose [SP][SP] (the forward recursion walks columns), cc[SP][MP],
// prm[SP][DP][MP][2] = {mean, -1 / (2 var)}
constexpr size_t model_doubles(int SP, int MP, int DP) {
  return static_cast<size_t>(SP) + 2 * static_cast<size_t>(SP) * SP + static_cast<size_t>(SP) * MP +
         static_cast<size_t>(SP) * DP * MP * 2;
}
constexpr int off_log_start() { return 0; }
constexpr int off_log_trans(int SP) { return SP; }
constexpr int off_log_transT(int SP) { return SP + SP * SP; }
constexpr int off_cc(int SP) { return SP + 2 * SP * SP; }
constexpr int off_prm(int SP, int MP) { return SP + 2 * SP * SP + SP * MP; }

inline int check_shape(int32_t S, int32_t M, int32_t D) {
  if (S > kMaxS || M > kMaxM || D > kMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "the mixture kernels serve S in 1..%d, M in 1..%d, D in 1..%d; got S=%d M=%d D=%d",
                kMaxS, kMaxM, kMaxD, S, M, D);
  return 0;
}

// the frames of an utterance: T = 0 for anything that points outside the batch or is longer than max_T (never followed)
struct Span {
  int64_t u, beg;
  int T;
};

__device__ __forceinline__ Span utt_span(const int64_t *offsets, int64_t u, bool ok, int64_t n_utts,
                                         int64_t total_frames, int32_t max_T) {
  Span s{-1, 0, 0};
  if (ok && u >= 0 && u < n_utts) {
    const int64_t beg = offsets[u], end = offsets[u + 1];
    s.u = u;
    if (beg >= 0 && end >= beg && end <= total_frames && end - beg <= max_T) {
      s.beg = beg;
      s.T = static_cast<int>(end - beg);
    }
  }
  return s;
}

template <int DP>
__device__ __forceinline__ void load_frame_pad(const float *__restrict__ xp, int D, bool live, double (&x)[DP]) {
#pragma unroll
  for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? static_cast<double>(xp[d]) : 0.0;
}

// lc[m] = cc[m] + sum_d (x_d - mu_dm)^2 * (-1 / (2 var_dm)) for one state; p, cc wavefront-uniform
template <int MP, int DP, int UNROLL = DP, class FX>
__device__ __forceinline__ void mix_log_terms(FX x, const double *__restrict__ p, const double *__restrict__ cc,
                                              double (&lc)[MP]) {
  double acc[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) acc[m] = 0.0;
#pragma unroll UNROLL
  for (int d = 0; d < DP; ++d) {
    const double xd = x(d);
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      const double diff = xd - p[(d * MP + m) * 2];
      acc[m] = fma(diff * diff, p[(d * MP + m) * 2 + 1], acc[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < MP; ++m) lc[m] = cc[m] + acc[m];
}

__device__ __forceinline__ double quiet_nan() { return __builtin_nan(""); }

// first maximum of the first n values; a NaN, once met, is kept (np.argmax)
template <int S>
__device__ __forceinline__ int argmax_first(const double (&g)[S], int n) {
  int best = 0;
  double bv = g[0];
#pragma unroll
  for (int s = 1; s < S; ++s) {
    const bool take = s < n && !(bv != bv) && (g[s] > bv || g[s] != g[s]);
    bv = take ? g[s] : bv;
    best = take ? s : best;
  }
  return best;
}

// _hmmc.cpp logsumexp (VIT: the maximum) over the terms a(k) + c(k) whose c(k) — a wavefront-uniform log transition —
// is above -inf; the skipped terms would add exp(-inf) = +0.0.  A NaN term gives NaN.
template <int S, bool VIT, class FA, class FC>
__device__ __forceinline__ double reduce_finite(FA a, FC c) {
  double work[S];
  double m = neg_inf();
  bool nan = false;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const double ck = c(k);
    if (ck > neg_inf()) {
      const double v = a(k) + ck;
      work[k] = v;
      nan = nan || v != v;
      m = v > m ? v : m;
    }
  }
  if (nan) return quiet_nan();
  if (VIT || isinf(m)) return m;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    if (c(k) > neg_inf()) acc += exp_unit(work[k] - m);
  }
  return log(acc) + m;
}
