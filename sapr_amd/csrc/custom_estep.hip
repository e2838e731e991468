// The E-step of the reference's from-scratch HMM (assignment2/custom_hmm.py:146-322 and the per-utterance sums
// baum_welch accumulates, :434-439): emission as the Gram-matrix ROW-SUM "Mahalanobis" term of :168-172, evaluated
// as d_t . (C^-1 sum_s d_s); forward with non-emitting entry / exit states and the global max-shift (:176-211);
// backward (:213-246); gamma (:248-257); per-frame renormalised xi (:259-322).
// CPU restatement: oracle/custom_hmm_oracle.py.
//
//   custom_estep_kernel        every (S, D) and both lattice layouts: one lane per utterance, run-time shapes, the
//                              recurrences as device functions over lattices in HBM
//   custom_piece_kernel        the same device functions one at a time (the reference's per-method API)
//   custom_emit_kernel<S, D, STAGED> + custom_estep_fast_kernel<S, PASS, MIN_BLOCKS>
//                              slot layout without dense xi at S in {10, 18}, D in {13, 39}: register-resident rows
//   custom_stage_kernel, custom_frame_sums_kernel   the slot-major feature copy and frame sums the fast path reads
// custom_estep_impl picks between the two E-steps by (layout, xi_dense, S, D).
#include <type_traits>

#include "sapr_common.h"

namespace sapr {
namespace {

#include "custom_np.h"
#include "lse_ops.h"
#include "smooth_ops.h"  // softmax_row

// E[t][j] for all frames of one utterance under model w
__device__ void emission_rows(const float *__restrict__ x, int T, int D, int S, const CustomPack &P, int w,
                              const Lat E) {
  double xs[kMaxD], v[kMaxD];
  for (int d = 0; d < D; ++d) xs[d] = 0.0;
  for (int t = 0; t < T; ++t)
    for (int d = 0; d < D; ++d) xs[d] += static_cast<double>(x[static_cast<int64_t>(t) * D + d]);
  for (int t = 0; t < T; ++t) {
    E.at(t, 0) = neg_inf();
    E.at(t, S - 1) = neg_inf();
  }
  for (int j = 1; j < S - 1; ++j) {
    const double *mu = P.means + (static_cast<int64_t>(w) * S + j) * D;
    const double *iv = P.inv + (static_cast<int64_t>(w) * S + j) * D * D;
    for (int a = 0; a < D; ++a) {
      double acc = 0.0;
      for (int b = 0; b < D; ++b) acc += iv[a * D + b] * (xs[b] - T * mu[b]);
      v[a] = acc;
    }
    const double c = P.cterm[static_cast<int64_t>(w) * S + j];
    for (int t = 0; t < T; ++t) {
      double qd = 0.0;
      for (int d = 0; d < D; ++d) qd += (static_cast<double>(x[static_cast<int64_t>(t) * D + d]) - mu[d]) * v[d];
      E.at(t, j) = -0.5 * (c + qd);
    }
  }
}

// ---- the four recurrences as device functions ----------------------------------------------------
// forward (custom_hmm.py:176-211): returns the global scale = max(alpha), alpha is stored shifted
__device__ double forward_rows(const Lat E, const double *__restrict__ lA, int T, int S, const Lat al) {
  for (int s = 0; s < S; ++s) al.at(0, s) = neg_inf();
  al.at(0, 0) = 0.0;
  al.at(0, 1) = lA[0 * S + 1] + E.at(0, 1);
  for (int t = 1; t < T; ++t) {
    al.at(t, 0) = neg_inf();
    for (int j = 1; j < S - 1; ++j)
      al.at(t, j) = np_logaddexp(al.at(t - 1, j - 1) + lA[(j - 1) * S + j], al.at(t - 1, j) + lA[j * S + j]) + E.at(t, j);
    al.at(t, S - 1) = al.at(t - 1, S - 2) + lA[(S - 2) * S + S - 1];
  }
  double scale = neg_inf();
  for (int t = 0; t < T; ++t)
    for (int s = 0; s < S; ++s) {
      const double v = al.at(t, s);
      if (v > scale || v != v) scale = v;  // np.max propagates NaN
    }
  for (int t = 0; t < T; ++t)
    for (int s = 0; s < S; ++s) al.at(t, s) -= scale;
  return scale;
}

// backward (custom_hmm.py:213-246)
__device__ void backward_rows(const Lat E, const double *__restrict__ lA, int T, int S, double scale, const Lat be) {
  for (int t = 0; t < T; ++t)
    for (int s = 0; s < S; ++s) be.at(t, s) = neg_inf();
  be.at(T - 1, S - 1) = 0.0;
  for (int t = T - 2; t >= 0; --t) {
    be.at(t, 0) = lA[0 * S + 1] + E.at(t + 1, 1) + be.at(t + 1, 1);
    for (int i = 1; i < S - 2; ++i)
      be.at(t, i) = np_logaddexp(lA[i * S + i] + E.at(t + 1, i) + be.at(t + 1, i),
                                 lA[i * S + i + 1] + E.at(t + 1, i + 1) + be.at(t + 1, i + 1));
    {
      const int i = S - 2;
      be.at(t, i) = np_logaddexp(lA[i * S + i] + E.at(t + 1, i) + be.at(t + 1, i), lA[i * S + i + 1] + be.at(t + 1, i + 1));
    }
  }
  for (int t = 0; t < T - 1; ++t)
    for (int s = 0; s < S; ++s) be.at(t, s) -= scale;
}

// gamma (custom_hmm.py:248-257): row soft-max of alpha + beta via logaddexp.reduce
__device__ void gamma_rows(const Lat al, const Lat be, int T, int S, const Lat ga) {
  for (int t = 0; t < T; ++t) {
    double norm = al.at(t, 0) + be.at(t, 0);
    for (int s = 1; s < S; ++s) norm = np_logaddexp(norm, al.at(t, s) + be.at(t, s));
    for (int s = 0; s < S; ++s) ga.at(t, s) = exp((al.at(t, s) + be.at(t, s)) - norm);
  }
}

__device__ double seq_loglik(const Lat al, int T, int S) {
  double ll = al.at(T - 1, 0);
  for (int s = 1; s < S; ++s) ll = np_logaddexp(ll, al.at(T - 1, s));
  return ll;
}

// xi (custom_hmm.py:259-322), renormalised per frame; exit column uses emission = -inf.
// xi_dense (optional) receives rows t < T-1 of [S][S]; agg (optional) accumulates sum_t xi[t].
//
// Only 2S-1 entries of the (S,S) matrix can be non-zero: (0,1), (i,i) and (i,i+1) for the emitting
// states, (S-1,S-1).  np.sum over the flattened matrix is numpy's pair-wise sum; for S*S <= 128 that is
// eight strided accumulators (element k goes to accumulator k % 8, in increasing k), a fixed tree over
// them, then the S*S % 8 trailing elements one by one.  Adding an exact +0.0 never changes an
// accumulator of non-negative terms, so walking the non-zero entries in flattened order through the
// same accumulators gives the same bits as the dense sum without the S*S-element scratch array.
struct XiEntry {
  int pos;
  double val;
};

__device__ void xi_rows_dense(const Lat al, const Lat be, const Lat E, const double *__restrict__ A,
                              const double *__restrict__ lA, int T, int S, double *__restrict__ xi_dense,
                              double *__restrict__ agg) {
  const double ll = seq_loglik(al, T, S);
  double xr[kMaxS * kMaxS];
  double a[kMaxS], e[kMaxS], b[kMaxS];
  for (int t = 0; t < T - 1; ++t) {
    for (int i = 0; i < S; ++i) {
      a[i] = al.at(t, i);
      e[i] = E.at(t + 1, i);
      b[i] = be.at(t + 1, i);
    }
    for (int k = 0; k < S * S; ++k) xr[k] = 0.0;
    xr[0 * S + 1] = exp(a[0] + lA[0 * S + 1] + e[1] + b[1] - ll);
    for (int i = 1; i < S - 1; ++i) {
      if (A[i * S + i] > 0) xr[i * S + i] = exp(a[i] + lA[i * S + i] + e[i] + b[i] - ll);
      if (i < S - 2) xr[i * S + i + 1] = exp(a[i] + lA[i * S + i + 1] + e[i + 1] + b[i + 1] - ll);
    }
    xr[(S - 2) * S + S - 1] = exp(a[S - 2] + lA[(S - 2) * S + S - 1] + e[S - 1] + b[S - 1] - ll);
    xr[(S - 1) * S + S - 1] = exp(a[S - 1] + lA[(S - 1) * S + S - 1] + e[S - 1] + b[S - 1] - ll);
    // np.sum over the (S,S) matrix: pair-wise over the flattened contiguous array
    const double tot = np_pairwise<double, 3>(xr, S * S, 1);
    if (tot > 0)
      for (int k = 0; k < S * S; ++k) xr[k] /= tot;
    if (agg)
      for (int k = 0; k < S * S; ++k) agg[k] += xr[k];
    if (xi_dense) {
      double *xd = xi_dense + static_cast<int64_t>(t) * S * S;
      for (int k = 0; k < S * S; ++k) xd[k] = xr[k];
    }
  }
}

__device__ void xi_rows(const Lat al, const Lat be, const Lat E, const double *__restrict__ A,
                        const double *__restrict__ lA, int T, int S, double *__restrict__ xi_dense,
                        double *__restrict__ agg) {
  const int n = S * S;
  if (n > 128) return xi_rows_dense(al, be, E, A, lA, T, S, xi_dense, agg);
  const double ll = seq_loglik(al, T, S);
  const int n8 = n - n % 8;
  XiEntry nz[2 * kMaxS];
  double acc[2 * kMaxS];  // running sums of the non-zero entries (same order of additions as agg[k] += ...)
  for (int i = 0; i < 2 * S; ++i) acc[i] = 0.0;
  int cnt = 0;
  double a[kMaxS], e[kMaxS], b[kMaxS];
  for (int t = 0; t < T - 1; ++t) {
    for (int i = 0; i < S; ++i) {
      a[i] = al.at(t, i);
      e[i] = E.at(t + 1, i);
      b[i] = be.at(t + 1, i);
    }
    cnt = 0;
    nz[cnt++] = {0 * S + 1, exp(a[0] + lA[0 * S + 1] + e[1] + b[1] - ll)};
    for (int i = 1; i < S - 1; ++i) {
      // slots keep a fixed meaning across frames (2i-1: self loop, 2i: step to i+1) so that acc[] lines up
      nz[cnt++] = {i * S + i, A[i * S + i] > 0 ? exp(a[i] + lA[i * S + i] + e[i] + b[i] - ll) : 0.0};
      nz[cnt++] = {i * S + i + 1, exp(a[i] + lA[i * S + i + 1] + e[i + 1] + b[i + 1] - ll)};
    }
    nz[cnt++] = {(S - 1) * S + S - 1, exp(a[S - 1] + lA[(S - 1) * S + S - 1] + e[S - 1] + b[S - 1] - ll)};
    double tot;
    if (n < 8) {
      tot = 0.0;
      for (int i = 0; i < cnt; ++i) tot += nz[i].val;
    } else {
      double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < cnt; ++i) {
        const int pos = nz[i].pos;
        if (pos < n8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = (pos % 8 == j) ? r[j] + nz[i].val : r[j];
        }
      }
      tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (int i = 0; i < cnt; ++i)
        if (nz[i].pos >= n8) tot += nz[i].val;
    }
    if (tot > 0)
      for (int i = 0; i < cnt; ++i) nz[i].val /= tot;
    for (int i = 0; i < cnt; ++i) acc[i] += nz[i].val;
    if (xi_dense) {
      double *xd = xi_dense + static_cast<int64_t>(t) * n;
      for (int k = 0; k < n; ++k) xd[k] = 0.0;
      for (int i = 0; i < cnt; ++i) xd[nz[i].pos] = nz[i].val;
    }
  }
  if (agg && T > 1)
    for (int i = 0; i < cnt; ++i) agg[nz[i].pos] += acc[i];
}

// one lane = one utterance against model utt_model[u].  lane_slots == 0: lattices E/alpha/beta/gamma are
// [total_frames][S] rows at the utterance's frame offset (the reference's layout); lane_slots > 0: they
// are [max_T][S][lane_slots] with the utterance index as the fastest axis (coalesced; what baum_welch
// uses).  xi_dense (optional) is [total_frames][S][S] (rows t < T-1 used).
// utt_out[u] = {LL (scaled alpha, logaddexp.reduce(alpha[-1])), scale, agg_gamma[S], agg_xi[S][S]}
__global__ __launch_bounds__(kBlock) void custom_estep_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets,
    const int32_t *__restrict__ utt_model, int64_t n_utts, int D, int S, CustomPack P, int64_t lane_slots,
    double *__restrict__ Eo, double *__restrict__ alpha, double *__restrict__ beta,
    double *__restrict__ gamma, double *__restrict__ xi_dense, double *__restrict__ utt_out) {
  const int64_t u = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x;
  if (u >= n_utts) return;
  const int w = utt_model ? utt_model[u] : 0;
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  const int K = 2 + S + S * S;
  double *out = utt_out + u * K;
  for (int k = 0; k < K; ++k) out[k] = 0.0;
  if (T <= 0) return;
  const int64_t base = lane_slots ? u : beg * S, es = lane_slots ? lane_slots : 1;
  const Lat E{Eo + base, es, S}, al{alpha + base, es, S}, be{beta + base, es, S}, ga{gamma + base, es, S};
  const double *lA = P.logA + static_cast<int64_t>(w) * S * S;
  const double *A = P.A + static_cast<int64_t>(w) * S * S;

  emission_rows(feats + beg * D, T, D, S, P, w, E);
  const double scale = forward_rows(E, lA, T, S, al);
  backward_rows(E, lA, T, S, scale, be);
  gamma_rows(al, be, T, S, ga);
  {  // aggregated_gamma += sum(gamma[:-1])   (custom_hmm.py:434)
    double gs[kMaxS];
    for (int s = 0; s < S; ++s) gs[s] = 0.0;
    for (int t = 0; t < T - 1; ++t)
      for (int s = 0; s < S; ++s) gs[s] += ga.at(t, s);
    for (int s = 0; s < S; ++s) out[2 + s] = gs[s];
  }
  out[0] = seq_loglik(al, T, S);  // of the SCALED alpha (custom_hmm.py:438)
  out[1] = scale;
  xi_rows(al, be, E, A, lA, T, S, xi_dense ? xi_dense + beg * S * S : nullptr, out + 2 + S);
}

// ---- batched E-step, compile-time shapes --------------------------------------------------------------
// Same arithmetic as custom_estep_kernel (operation for operation: the golden-vector tests cover both), laid
// out for registers: S and D are template parameters, so the per-row state (alpha / beta rows, the 2S-2
// structurally non-zero xi entries and their running sums, the row-sum vector v) lives in VGPRs instead of
// the 4.9 KB of scratch memory per lane the run-time-shaped kernel needs.  Lattices are the lane-contiguous
// [max_T][S][lane_slots] layout only.  alpha and beta are stored UNSHIFTED; the reference's `alpha -= scale`
// / `beta[:-1] -= scale` (custom_hmm.py:208-209,244) happen on the fly where the values are read, which is
// the same single rounding and saves a read-modify-write pass over each lattice; gamma is produced inside
// the backward loop (it needs only row t of both lattices).
template <int S>
constexpr int xi_pos(int i) {  // flattened (S,S) position of the i-th structurally non-zero xi entry
  return i == 0 ? 1 : (i == 2 * S - 3 ? (S - 1) * S + S - 1 : ((i + 1) / 2) * S + (i + 1) / 2 + (i % 2 == 0 ? 1 : 0));
}
// np.sum over the flattened (S,S) matrix = numpy's pair-wise sum of S*S values of which only the entries at
// xi_pos are non-zero: walk numpy's recursion at compile time and feed each entry to the accumulator its
// position selects (adding the exact zeros in between changes nothing)
template <int S, int START, int N>
__device__ __forceinline__ double xi_pairwise(const double (&val)[2 * S - 2]) {
  if constexpr (N > 128) {
    constexpr int n2 = N / 2 - (N / 2) % 8;
    const double left = xi_pairwise<S, START, n2>(val);
    return left + xi_pairwise<S, START + n2, N - n2>(val);
  } else if constexpr (N < 8) {
    double r = 0.0;
    static_for_c<0, 2 * S - 2>([&](auto ic) {
      constexpr int i = decltype(ic)::value, p = xi_pos<S>(i) - START;
      if constexpr (p >= 0 && p < N) r += val[i];
    });
    return r;
  } else {
    constexpr int n8 = N - N % 8;
    double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    static_for_c<0, 2 * S - 2>([&](auto ic) {
      constexpr int i = decltype(ic)::value, p = xi_pos<S>(i) - START;
      if constexpr (p >= 0 && p < n8) r[p % 8] += val[i];
    });
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    static_for_c<0, 2 * S - 2>([&](auto ic) {
      constexpr int i = decltype(ic)::value, p = xi_pos<S>(i) - START;
      if constexpr (p >= n8 && p < N) res += val[i];
    });
    return res;
  }
}

// ---- emission of the batched E-step: E[t][j] = -0.5 (c_j + d_t . v_j),  v_j = C_j^-1 (sum_s x_s - T mu_j)
// (custom_hmm.py:146-174).  Inside the lane-per-utterance E-step kernel this was one pass over the utterance's frames per
// emitting state: 9 x 0.5 GB of features streamed from HBM per 100 000 utterances (a wavefront's 336 KB do not stay in
// cache between passes) — half of that kernel's time.  Here a WORKGROUP holds 64 utterances and a wavefront one of eight
// states: the eight wavefronts walk the same frames at the same time on one CU, so a feature row crosses HBM once and
// reaches the other seven from L1 / L2.  Every lane performs the operations it performed inside the E-step kernel, in
// the same order (the frame sum is evaluated by each wavefront, as before by each lane).
// STAGED: features from the slot-major copy feat_t[t][d][slot] (sapr_custom_stage_features) — a wavefront's load of one
// value is one 256-byte row instead of 64 private 4-byte reads.
constexpr int kEmitStates = 8;  // wavefronts (states) per workgroup; S - 2 is a multiple at the batched shapes
template <int S, int D, bool STAGED>
__global__ __launch_bounds__(kBlock * kEmitStates) __attribute__((amdgpu_waves_per_eu(D <= 13 ? 4 : 2))) void custom_emit_kernel(const float *__restrict__ feats,
                                                             const int64_t *__restrict__ offsets,
                                                             const int32_t *__restrict__ utt_model, int64_t n_utts,
                                                             CustomPack P, int64_t es, double *__restrict__ Eo,
                                                             const float *__restrict__ feat_t,
                                                             const double *__restrict__ frame_sums) {
  static_assert((S - 2) % kEmitStates == 0, "whole workgroups of states");
  const int64_t u = blockIdx.x * static_cast<int64_t>(kBlock) + (threadIdx.x & (kBlock - 1));
  if (u >= n_utts) return;
  const int j = static_cast<int>(blockIdx.y) * kEmitStates + static_cast<int>(threadIdx.x / kBlock) + 1;
  const int w = utt_model ? utt_model[u] : 0;
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  if (T <= 0) return;
  const float *__restrict__ x = feats + beg * D;
  const float *__restrict__ xt = STAGED ? feat_t + u : nullptr;
  auto feat = [&](int t, int d) -> double {
    if constexpr (STAGED)
      return static_cast<double>(xt[(static_cast<int64_t>(t) * D + d) * es]);
    else
      return static_cast<double>(x[static_cast<int64_t>(t) * D + d]);
  };
  double *__restrict__ E = Eo + u;
  auto at = [es](int t, int jj) { return (static_cast<int64_t>(t) * S + jj) * es; };
  // frame sums: the dimensions are dealt to the workgroup's wavefronts (each sum still runs over the frames in order, in
  // one lane) and exchanged through LDS — two feature rows per frame and wavefront instead of all D; four frames of
  // loads in flight per step
  constexpr int kNd = (D + kEmitStates - 1) / kEmitStates;
  __shared__ double s_xs[D][kBlock];
  const int wv = static_cast<int>(threadIdx.x / kBlock), ln = static_cast<int>(threadIdx.x & (kBlock - 1));
  // (round 4) the frame sums do not change between EM iterations: sapr_custom_stage_features evaluates them once per
  // batch — the same additions in the same order, custom_frame_sums_kernel — and every iteration's pass over the
  // features for them (0.5 GB per 100 000 utterances, a third of this kernel's HBM traffic) falls away
  if (frame_sums == nullptr) {
    double part[kNd];
#pragma unroll
    for (int k = 0; k < kNd; ++k) part[k] = 0.0;
    int t = 0;
    for (; t + 4 <= T; t += 4) {
      double f[4][kNd];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < kNd; ++k) f[q][k] = (wv + k * kEmitStates < D) ? feat(t + q, wv + k * kEmitStates) : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < kNd; ++k) part[k] += f[q][k];
    }
    for (; t < T; ++t)
#pragma unroll
      for (int k = 0; k < kNd; ++k)
        if (wv + k * kEmitStates < D) part[k] += feat(t, wv + k * kEmitStates);
#pragma unroll
    for (int k = 0; k < kNd; ++k)
      if (wv + k * kEmitStates < D) s_xs[wv + k * kEmitStates][ln] = part[k];
  }
  __syncthreads();  // (frame_sums is a kernel argument: the branch above is uniform)
  double xs[D];
#pragma unroll
  for (int d = 0; d < D; ++d) xs[d] = frame_sums ? frame_sums[static_cast<int64_t>(d) * es + u] : s_xs[d][ln];
  if (j == 1) {  // entry and exit state never emit
    for (int t = 0; t < T; ++t) {
      E[at(t, 0)] = neg_inf();
      E[at(t, S - 1)] = neg_inf();
    }
  }
  const double *mu = P.means + (static_cast<int64_t>(w) * S + j) * D;
  const double *iv = P.inv + (static_cast<int64_t>(w) * S + j) * D * D;
  double v[D], m[D];
#pragma unroll
  for (int a = 0; a < D; ++a) m[a] = mu[a];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < D; ++b) acc += iv[a * D + b] * (xs[b] - T * m[b]);
    v[a] = acc;
    // one row of the inverse covariance in flight at a time: left free, the compiler issues all D x D loads at once and
    // spills ~600 bytes per lane around them (0.5 GB of scratch traffic per 100 000 utterances x 8 states)
    asm volatile("" ::: "memory");
  }
  const double c = P.cterm[static_cast<int64_t>(w) * S + j];
  constexpr int kNf = D <= 13 ? 4 : 2;  // frames of loads in flight
  int t = 0;
  for (; t + kNf <= T; t += kNf) {
    float xf[kNf][D];
#pragma unroll
    for (int q = 0; q < kNf; ++q)
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if constexpr (STAGED)
          xf[q][d] = xt[(static_cast<int64_t>(t + q) * D + d) * es];
        else
          xf[q][d] = x[static_cast<int64_t>(t + q) * D + d];
      }
#pragma unroll
    for (int q = 0; q < kNf; ++q) {
      double qd = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) qd += (static_cast<double>(xf[q][d]) - m[d]) * v[d];
      E[at(t + q, j)] = -0.5 * (c + qd);
    }
  }
  for (; t < T; ++t) {
    double qd = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) qd += (feat(t, d) - m[d]) * v[d];
    E[at(t, j)] = -0.5 * (c + qd);
  }
}

// the end of both passes: utt_out[u][2 ..] = the aggregated gamma, then += the aggregated xi at its non-zero positions
template <int S>
__device__ __forceinline__ void store_counts(double *out, const double (&gs)[S], const double (&acc)[2 * S - 2], int T) {
#pragma unroll
  for (int s = 0; s < S; ++s) out[2 + s] = gs[s];
  if (T > 1) {
    double *agg = out + 2 + S;
    static_for_c<0, 2 * S - 2>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      agg[xi_pos<S>(i)] += acc[i];
    });
  }
}

// PASS 0: every utterance — forward pass over the stored log-densities, then the backward half as a smoothing recursion wherever that
// returns what the reference returns (see the classification below); the utterances where it would not are appended
// to `redo`.  PASS 1: the utterances of `redo` again, start to end in the reference's own operation order.
// (10 states x 13 dimensions: capped at 256 registers so that two workgroups share a CU — 100 000 utterances are 1.5
// rounds of one wavefront per SIMD otherwise, and the second wavefront covers the first's exp / log1p latencies;
// the larger shapes keep every register they can get in pass 1)
// The features enter through E only, so D shows in MIN_BLOCKS alone (launch_estep_fast).
template <int S, int PASS, int MIN_BLOCKS>
__global__ __launch_bounds__(kBlock, MIN_BLOCKS) void custom_estep_fast_kernel(
    const int64_t *__restrict__ offsets, const int32_t *__restrict__ utt_model, int64_t n_utts, CustomPack P,
    int64_t es, double *__restrict__ Eo, double *__restrict__ alpha, double *__restrict__ beta,
    double *__restrict__ gamma, double *__restrict__ utt_out, int32_t *__restrict__ redo,
    int32_t *__restrict__ redo_count) {
  constexpr bool kFirst = PASS != 1;
  int64_t u = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x;
  if constexpr (kFirst) {
    if (u >= n_utts) return;
  } else {
    if (u >= *redo_count) return;  // (the grid covers n_utts: almost every workgroup leaves here)
    u = redo[u];
  }
  const int w = utt_model ? utt_model[u] : 0;
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  constexpr int K = 2 + S + S * S;
  double *out = utt_out + u * K;
  if constexpr (kFirst)
    for (int k = 0; k < K; ++k) out[k] = 0.0;
  if (T <= 0) return;
  double *__restrict__ E = Eo + u, *__restrict__ al = alpha + u, *__restrict__ be = beta + u,
                      *__restrict__ ga = gamma + u;
  auto at = [es](int t, int j) { return (static_cast<int64_t>(t) * S + j) * es; };
  const double *__restrict__ lA = P.logA + static_cast<int64_t>(w) * S * S;
  const double *__restrict__ A = P.A + static_cast<int64_t>(w) * S * S;

  // (the log-densities E are in their lattice: custom_emit_kernel ran before pass 0)

  // ---- forward (custom_hmm.py:176-211); scale = np.max(alpha) (NaN propagates).  Pass 0 keeps the rows in registers
  // only (its smoothing recursion needs the last one): the alpha lattice is written by pass 1, which runs the forward
  // pass again for the utterances it redoes (the same operations: the same values) and reads the rows back, unshifted,
  // in its backward half — 0.8 GB of lattice writes per 100 000 utterances less in pass 0
  double scale = neg_inf();
  double prev[S];
  {
    double cur[S];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) prev[s2] = neg_inf();
    prev[0] = 0.0;
    prev[1] = lA[0 * S + 1] + E[at(0, 1)];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) {
      if constexpr (!kFirst) al[at(0, s2)] = prev[s2];
      if (prev[s2] > scale || prev[s2] != prev[s2]) scale = prev[s2];
    }
    // (round 4) the log-densities of frame t + 1 are requested at the top of frame t: left to the compiler the loads
    // sat behind the frame's exp / log chains, a few instructions in front of their use — 46 % of the kernel's
    // wave-cycles were s_waitcnt vmcnt at the 1.5 wavefronts per SIMD a 100 000-utterance grid gives
    double e_cur[S], e_nxt[S];
    if (T > 1) {
#pragma unroll
      for (int j = 1; j < S - 1; ++j) e_nxt[j] = E[at(1, j)];
    }
    for (int t = 1; t < T; ++t) {
#pragma unroll
      for (int j = 1; j < S - 1; ++j) e_cur[j] = e_nxt[j];
      if (t + 1 < T) {
#pragma unroll
        for (int j = 1; j < S - 1; ++j) e_nxt[j] = E[at(t + 1, j)];
      }
      cur[0] = neg_inf();
#pragma unroll
      for (int j = 1; j < S - 1; ++j) {
        // the share of state j's forward mass that STAYED in j (the rest came from j - 1): the smoothing form of the
        // backward pass (below) runs on it; it waits in the beta lattice, which holds nothing else for an utterance
        // that takes that form
        if constexpr (kFirst) {
          double move, stay;
          cur[j] = np_logaddexp_shares(prev[j - 1] + lA[(j - 1) * S + j], prev[j] + lA[j * S + j], move, stay) + e_cur[j];
          be[at(t, j)] = stay;
        } else {
          cur[j] = np_logaddexp(prev[j - 1] + lA[(j - 1) * S + j], prev[j] + lA[j * S + j]) + e_cur[j];
        }
      }
      cur[S - 1] = prev[S - 2] + lA[(S - 2) * S + S - 1];
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        if constexpr (!kFirst) al[at(t, s2)] = cur[s2];
        if (cur[s2] > scale || cur[s2] != cur[s2]) scale = cur[s2];
        prev[s2] = cur[s2];
      }
    }
    // LL of the SCALED alpha: logaddexp.reduce(alpha[-1] - scale)   (custom_hmm.py:268,438)
    double l = prev[0] - scale;
#pragma unroll
    for (int s2 = 1; s2 < S; ++s2) l = np_logaddexp(l, prev[s2] - scale);
    out[0] = l;
    out[1] = scale;
  }
  const double ll = out[0];

  // ---- which form of the backward pass this utterance takes (round 3b).  custom_hmm.py:213-322 computes beta in the
  // log domain, gamma = softmax(alpha + beta) and the xi terms exp(alpha - s + log a + e + beta - s - LL), renormalised
  // per frame: 46 of the 62 float64 transcendentals of a frame.  In exact arithmetic all of it follows from the
  // forward pass: the shares move / stay of state j's forward mass at frame t + 1 are P(q_t | q_(t+1) = j, O), so
  //     xi_t(j-1 -> j) = gamma_(t+1)(j) move,   xi_t(j -> j) = gamma_(t+1)(j) stay,   gamma_t(i) = xi_t(i -> i) + xi_t(i -> i+1)
  // — multiplications and additions.  What the reference returns differs where its exponentials underflow: every xi
  // term carries the factor rho exp(-s) (s = max alpha of the utterance, rho = the exit state's share of the last
  // forward row) until the per-frame renormalisation divides it out, so with c0 = log rho - s
  //     c0 >= -678   no term above 1e-13 leaves the normal range (exp(-708)): the smoothing recursion gives the
  //                  reference's values to rounding
  //     c0 <  -750   EVERY term underflows to exactly 0 (exp(x) = 0 below -745.2), the frame totals are 0, nothing is
  //                  renormalised: the utterance contributes posteriors but no transition counts (trained models
  //                  with densities >> 1, e.g. digital silence)
  //     otherwise    (or NaN, or -inf) some terms are denormal or gone: the reference's own operation order (pass 1)
  // The exit state's xi term is exp(-inf) = 0 in every mode, so the last step (all mass in the exit state) adds nothing.
  if constexpr (kFirst) {
    const double c0 = (prev[S - 1] - (ll + scale)) - scale;
    // c0 = -inf: the utterance is too short to reach the exit state.  The reference's posteriors are then NaN in
    // every state of every row (softmax over a row of -inf), the exit state included, while the smoothing form keeps
    // exact zeros there: such an utterance takes the reference's order too.
    const int mode = c0 >= -678.0 ? 0 : ((c0 < -750.0 && c0 > neg_inf()) ? 1 : 2);
    if (mode == 2) {  // pass 1 takes this utterance again
      redo[atomicAdd(redo_count, 1)] = static_cast<int32_t>(u);
      return;
    }
    double gs[S];
    constexpr int CNT = 2 * S - 2;
    double acc[CNT];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) gs[s2] = 0.0;
#pragma unroll
    for (int i = 0; i < CNT; ++i) acc[i] = 0.0;
    double g1[S];  // gamma of row t + 1
    {
      double lg[S];
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) lg[s2] = (prev[s2] - scale) + (s2 == S - 1 ? 0.0 : neg_inf());
      softmax_row<S>(lg, g1);
    }
    // shares of the step into row t + 1, read one row ahead
    double sy[S];
    if (T > 1) {
#pragma unroll
      for (int j = 1; j < S - 1; ++j) sy[j] = be[at(T - 1, j)];
    }
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) ga[at(T - 1, s2)] = g1[s2];
    for (int t = T - 2; t >= 0; --t) {
      double nsy[S];
      if (t >= 1) {
#pragma unroll
        for (int j = 1; j < S - 1; ++j) nsy[j] = be[at(t, j)];
      }
      double g0[S], x_move[S], x_stay[S];  // xi_t(j-1 -> j), xi_t(j -> j) for the emitting j
#pragma unroll
      for (int j = 1; j < S - 1; ++j) {
        x_stay[j] = g1[j] * sy[j];
        x_move[j] = g1[j] - x_stay[j];  // the two shares add up to 1 (to rounding): one lattice instead of two
      }
      g0[0] = x_move[1];
#pragma unroll
      for (int i = 1; i < S - 2; ++i) g0[i] = x_stay[i] + x_move[i + 1];
      g0[S - 2] = x_stay[S - 2] + g1[S - 1];  // the exit state is entered from S - 2 only
      g0[S - 1] = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        ga[at(t, s2)] = g0[s2];
        gs[s2] += g0[s2];
      }
      if (mode == 0 && t + 1 < T - 1) {
        acc[0] += x_move[1];
#pragma unroll
        for (int i = 1; i < S - 1; ++i) {
          acc[2 * i - 1] += x_stay[i];
          if (i + 1 < S - 1) acc[2 * i] += x_move[i + 1];
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) g1[s2] = g0[s2];
#pragma unroll
      for (int j = 1; j < S - 1; ++j) sy[j] = nsy[j];
    }
    store_counts<S>(out, gs, acc, T);
    return;
  } else {
  // ---- backward (custom_hmm.py:213-246) with gamma (:248-257) of each finished row, and — while row t+1 of beta,
  // the emissions of frame t+1 and row t of alpha are in registers — the xi terms of step t (:259-322) and the
  // aggregated gamma over t < T-1 (:434).  The reference adds those over ascending t; here they are added in the
  // order the backward recursion meets them (descending t): the same sums to rounding, compared at 1e-9, and
  // three lattice re-reads per frame less than a separate pass.
  {
    double nxt[S], cur[S];  // unshifted beta rows t+1 and t
    double gs[S];
    constexpr int CNT = 2 * S - 2;
    double acc[CNT];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) {
      nxt[s2] = neg_inf();
      gs[s2] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < CNT; ++i) acc[i] = 0.0;
    nxt[S - 1] = 0.0;
    // gamma of row t; a[] receives alpha[t] - scale, g[] the posteriors
    auto gamma_row = [&](int t, const double (&b)[S], bool shifted_row, double (&a)[S], double (&g)[S]) {
      double lg[S];
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        a[s2] = al[at(t, s2)] - scale;
        lg[s2] = a[s2] + (shifted_row ? b[s2] - scale : b[s2]);
      }
      // exp(lg - logaddexp.reduce(lg)) as exp(lg - max) / sum: S exponentials and one division instead of S - 1
      // logaddexp (exp + log1p each) and S more exponentials; same value to rounding (gamma is compared at 1e-9).
      // (softmax_row<S> operation for operation, as pass 0 calls it; called here it costs <18, 1, 1> two more AGPRs)
      double mx = lg[0];
#pragma unroll
      for (int s2 = 1; s2 < S; ++s2) mx = lg[s2] > mx ? lg[s2] : mx;
      double den = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        lg[s2] = exp_unit(lg[s2] - mx);
        den += lg[s2];
      }
      const double inv = 1.0 / den;
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        g[s2] = lg[s2] * inv;
        ga[at(t, s2)] = g[s2];
      }
    };
    double arow[S], grow[S];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) be[at(T - 1, s2)] = nxt[s2];
    gamma_row(T - 1, nxt, false, arow, grow);  // the last beta row is not shifted (be[:-1] -= scale)
    for (int t = T - 2; t >= 0; --t) {
      double e1[S];
      e1[0] = e1[S - 1] = neg_inf();
#pragma unroll
      for (int s2 = 1; s2 < S - 1; ++s2) e1[s2] = E[at(t + 1, s2)];
      cur[0] = lA[0 * S + 1] + e1[1] + nxt[1];
#pragma unroll
      for (int i = 1; i < S - 2; ++i)
        cur[i] = np_logaddexp(lA[i * S + i] + e1[i] + nxt[i], lA[i * S + i + 1] + e1[i + 1] + nxt[i + 1]);
      cur[S - 2] = np_logaddexp(lA[(S - 2) * S + S - 2] + e1[S - 2] + nxt[S - 2],
                                lA[(S - 2) * S + S - 1] + nxt[S - 1]);
      cur[S - 1] = neg_inf();
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) be[at(t, s2)] = cur[s2];
      gamma_row(t, cur, true, arow, grow);
      // xi of step t: alpha[t] - scale, emissions and (shifted) beta of frame t+1
      {
        const bool shifted = (t + 1) < (T - 1);
        double b[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
          gs[i] += grow[i];
          b[i] = shifted ? nxt[i] - scale : nxt[i];
        }
        double val[CNT];
        val[0] = exp_unit(arow[0] + lA[0 * S + 1] + e1[1] + b[1] - ll);
#pragma unroll
        for (int i = 1; i < S - 1; ++i) {
          val[2 * i - 1] = A[i * S + i] > 0 ? exp_unit(arow[i] + lA[i * S + i] + e1[i] + b[i] - ll) : 0.0;
          val[2 * i] = exp_unit(arow[i] + lA[i * S + i + 1] + e1[i + 1] + b[i + 1] - ll);
        }
        val[CNT - 1] = exp_unit(arow[S - 1] + lA[(S - 1) * S + S - 1] + e1[S - 1] + b[S - 1] - ll);
        const double tot = xi_pairwise<S, 0, S * S>(val);
        if (tot > 0) {
#pragma unroll
          for (int i = 0; i < CNT; ++i) val[i] /= tot;
        }
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] += val[i];
      }
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) nxt[s2] = cur[s2];
    }
    store_counts<S>(out, gs, acc, T);
  }
  }  // PASS == 1
}

// single-utterance pieces with caller-supplied inputs (the reference's per-method API, used by its
// tests): op 0 emission(features) 1 forward(E) 2 backward(E, scale) 3 gamma(alpha, beta) 4 xi(alpha, beta, E)
__global__ void custom_piece_kernel(int op, const float *__restrict__ x, int T, int D, int S, CustomPack P,
                                    double *__restrict__ E, double *__restrict__ al, double *__restrict__ be,
                                    double *__restrict__ ga, double *__restrict__ xi, double *__restrict__ scalar) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Lat LE{E, 1, S}, La{al, 1, S}, Lb{be, 1, S}, Lg{ga, 1, S};
  if (op == 0) emission_rows(x, T, D, S, P, 0, LE);
  if (op == 1) scalar[0] = forward_rows(LE, P.logA, T, S, La);
  if (op == 2) backward_rows(LE, P.logA, T, S, scalar[0], Lb);
  if (op == 3) gamma_rows(La, Lb, T, S, Lg);
  if (op == 4) xi_rows(La, Lb, LE, P.A, P.logA, T, S, xi, nullptr);
}

// feat_t[t][d][slot] = feats[offsets[slot] + t][d] (0 past the utterance's end): the slot-major copy the batched E-step
// reads (one coalesced row per wavefront and value).  A 64 x 64 transpose through LDS: an utterance's frames are
// contiguous floats, so the reads are 256-byte runs per utterance and the writes 256-byte runs per (frame, dimension).
__global__ __launch_bounds__(256) void custom_stage_kernel(const float *__restrict__ feats,
                                                           const int64_t *__restrict__ offsets, int64_t n_utts, int D,
                                                           int max_T, int64_t es, float *__restrict__ out) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * 64;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * 64;  // index into an utterance's T * D floats
  for (int uu = ty; uu < 64; uu += 4) {
    const int64_t u = u0 + uu;
    float v = 0.0f;
    if (u < n_utts) {
      const int64_t beg = offsets[u];
      const int64_t len = (offsets[u + 1] - beg) * D;
      if (r0 + tx < len) v = feats[beg * D + r0 + tx];
    }
    tile[uu][tx] = v;
  }
  __syncthreads();
  const int64_t rows = static_cast<int64_t>(max_T) * D;
  for (int rr = ty; rr < 64; rr += 4)
    if (r0 + rr < rows && u0 + tx < es) out[(r0 + rr) * es + u0 + tx] = tile[tx][rr];
}

// frame_sums[d][slot] = sum_t x_t[d] of the slot's utterance, the frames added one after another in float64 — what
// custom_emit_kernel evaluates per call when it is not given them (custom_hmm.py:168-172's row sum needs sum_s d_s).
// One lane per slot, coalesced rows of the slot-major copy, four frames of loads in flight.
__global__ __launch_bounds__(256) void custom_frame_sums_kernel(const float *__restrict__ feat_t,
                                                               const int64_t *__restrict__ offsets, int64_t n_utts,
                                                               int D, int64_t es, double *__restrict__ frame_sums) {
  const int64_t u = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  const int d = static_cast<int>(blockIdx.y);
  if (u >= es) return;
  double acc = 0.0;
  if (u < n_utts) {
    const int T = static_cast<int>(offsets[u + 1] - offsets[u]);
    const float *__restrict__ p = feat_t + static_cast<int64_t>(d) * es + u;
    const int64_t step = static_cast<int64_t>(D) * es;
    int t = 0;
    for (; t + 4 <= T; t += 4) {
      const float f0 = p[t * step], f1 = p[(t + 1) * step], f2 = p[(t + 2) * step], f3 = p[(t + 3) * step];
      acc += static_cast<double>(f0);
      acc += static_cast<double>(f1);
      acc += static_cast<double>(f2);
      acc += static_cast<double>(f3);
    }
    for (; t < T; ++t) acc += static_cast<double>(p[t * step]);
  }
  frame_sums[static_cast<int64_t>(d) * es + u] = acc;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

// the register-resident E-step at one batched shape: emission (from the staged features when there are any), then
// the two passes.  Two workgroups per CU at (10, 13), see custom_estep_fast_kernel.
struct FastEstepArgs {
  const float *feats;
  const int64_t *offsets;
  const int32_t *utt_model;
  int64_t n_utts;
  CustomPack P;
  int64_t lane_slots;
  double *E, *alpha, *beta, *gamma, *utt_out;
  int32_t *redo, *redo_count;
  const float *feat_t;
  const double *frame_sums;
};
template <int S, int D>
static void launch_estep_fast(hipStream_t st, const FastEstepArgs &a) {
  constexpr int kMinBlocks = (S <= 10 && D <= 13) ? 2 : 1;
  const dim3 grid(static_cast<unsigned>((a.n_utts + kBlock - 1) / kBlock)), block(kBlock);
  const dim3 egrid(grid.x, static_cast<unsigned>((S - 2) / kEmitStates)), eblock(kBlock * kEmitStates);
  if (a.feat_t)
    SAPR_LAUNCH((custom_emit_kernel<S, D, true>), egrid, eblock, 0, st, a.feats, a.offsets, a.utt_model, a.n_utts, a.P,
                a.lane_slots, a.E, a.feat_t, a.frame_sums);
  else
    SAPR_LAUNCH((custom_emit_kernel<S, D, false>), egrid, eblock, 0, st, a.feats, a.offsets, a.utt_model, a.n_utts, a.P,
                a.lane_slots, a.E, a.feat_t, static_cast<const double *>(nullptr));
  SAPR_LAUNCH((custom_estep_fast_kernel<S, 0, kMinBlocks>), grid, block, 0, st, a.offsets, a.utt_model, a.n_utts, a.P,
              a.lane_slots, a.E, a.alpha, a.beta, a.gamma, a.utt_out, a.redo, a.redo_count);
  SAPR_LAUNCH((custom_estep_fast_kernel<S, 1, kMinBlocks>), grid, block, 0, st, a.offsets, a.utt_model, a.n_utts, a.P,
              a.lane_slots, a.E, a.alpha, a.beta, a.gamma, a.utt_out, a.redo, a.redo_count);
}

static int custom_estep_impl(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                             int64_t n_utts, int32_t D, int32_t S, int32_t W, const double *means,
                             const double *inv, const double *cterm, const double *A, const double *logA,
                             int64_t lane_slots, double *E, double *alpha, double *beta, double *gamma,
                             double *xi_dense, double *utt_out, void *stream, const float *feat_t,
                             const double *frame_sums = nullptr) {
  (void)W;
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0, "bad n_utts");
  SAPR_REQUIRE(lane_slots == 0 || lane_slots >= n_utts, "lane_slots must be 0 (row layout) or >= n_utts");
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(feats && offsets && means && inv && cterm && A && logA && E && alpha && beta && gamma && utt_out,
               "NULL pointer argument");
  CustomPack P{means, inv, cterm, A, logA};
  const dim3 grid(static_cast<unsigned>((n_utts + kBlock - 1) / kBlock));
  if (lane_slots > 0 && xi_dense == nullptr && (S == 10 || S == 18) && (D == 13 || D == 39)) {
    // batched training shapes: the register-resident kernels (alpha is left UNSHIFTED in its lattice; the beta lattice
    // holds scratch except for the utterances pass 1 redoes).  Two passes: forward + smoothing for every utterance, then
    // the reference-order kernel for the few whose xi terms the reference computes in the denormal range
    hipStream_t st = as_stream(stream);
    int32_t *redo = nullptr;
    SAPR_HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&redo), (static_cast<size_t>(n_utts) + 1) * sizeof(int32_t), st));
    int32_t *redo_count = redo + n_utts;
    SAPR_HIP_TRY(hipMemsetAsync(redo_count, 0, sizeof(int32_t), st));
    const FastEstepArgs a{feats, offsets, utt_model, n_utts, P,          lane_slots, E,         alpha,
                          beta,  gamma,   utt_out,   redo,   redo_count, feat_t,     frame_sums};
    if (S == 10 && D == 13)
      launch_estep_fast<10, 13>(st, a);
    else if (S == 18 && D == 39)
      launch_estep_fast<18, 39>(st, a);
    else if (S == 10 && D == 39)
      launch_estep_fast<10, 39>(st, a);
    else
      launch_estep_fast<18, 13>(st, a);
    (void)hipFreeAsync(redo, st);
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  SAPR_LAUNCH(custom_estep_kernel, grid, dim3(kBlock), 0,
                     as_stream(stream), feats, offsets, utt_model, n_utts, D, S, P, lane_slots, E, alpha, beta, gamma,
                     xi_dense, utt_out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sapr_custom_estep(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                 int64_t n_utts, int32_t D, int32_t S, int32_t W, const double *means,
                                 const double *inv, const double *cterm, const double *A, const double *logA,
                                 int64_t lane_slots, double *E, double *alpha, double *beta, double *gamma,
                                 double *xi_dense, double *utt_out, void *stream) {
  return custom_estep_impl(feats, offsets, utt_model, n_utts, D, S, W, means, inv, cterm, A, logA, lane_slots, E, alpha,
                           beta, gamma, xi_dense, utt_out, stream, nullptr);
}

// the same with the features also given in slot-major order (sapr_custom_stage_features, same lane_slots): the
// batched training shapes read them from there
extern "C" int sapr_custom_estep_staged(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                        int64_t n_utts, int32_t D, int32_t S, int32_t W, const double *means,
                                        const double *inv, const double *cterm, const double *A, const double *logA,
                                        int64_t lane_slots, double *E, double *alpha, double *beta, double *gamma,
                                        double *xi_dense, double *utt_out, const float *feat_t,
                                        const double *frame_sums, void *stream) {
  SAPR_REQUIRE(feat_t == nullptr || lane_slots > 0, "staged features need the slot layout (lane_slots > 0)");
  SAPR_REQUIRE(frame_sums == nullptr || feat_t != nullptr, "frame sums come with the staged features");
  return custom_estep_impl(feats, offsets, utt_model, n_utts, D, S, W, means, inv, cterm, A, logA, lane_slots, E, alpha,
                           beta, gamma, xi_dense, utt_out, stream, feat_t, frame_sums);
}

// feat_t[max_T][D][lane_slots] (float32) = the frame-major features in slot-major order, zero past each utterance;
// frame_sums[D][lane_slots] (float64, may be NULL) = every utterance's sum over its frames, in frame order
extern "C" int sapr_custom_stage_features(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D,
                                          int32_t max_T, int64_t lane_slots, float *feat_t, double *frame_sums,
                                          void *stream) {
  SAPR_REQUIRE(feats && offsets && feat_t && n_utts >= 0 && D > 0 && D <= kMaxD && max_T >= 0, "bad arguments");
  SAPR_REQUIRE(lane_slots >= n_utts && lane_slots > 0, "lane_slots must be >= n_utts");
  const int64_t rows = static_cast<int64_t>(max_T) * D;
  SAPR_REQUIRE((rows + 63) / 64 <= 65535, "max_T * D exceeds one launch's grid");
  if (rows > 0)
    SAPR_LAUNCH(custom_stage_kernel, dim3(static_cast<unsigned>((lane_slots + 63) / 64), static_cast<unsigned>((rows + 63) / 64)),
                dim3(256), 0, as_stream(stream), feats, offsets, n_utts, D, max_T, lane_slots, feat_t);
  SAPR_HIP_TRY(hipGetLastError());
  if (frame_sums) {
    SAPR_LAUNCH(custom_frame_sums_kernel, dim3(static_cast<unsigned>((lane_slots + 255) / 256), static_cast<unsigned>(D)),
                dim3(256), 0, as_stream(stream), feat_t, offsets, n_utts, D, lane_slots, frame_sums);
    SAPR_HIP_TRY(hipGetLastError());
  }
  return 0;
}

extern "C" int sapr_custom_piece(int32_t op, const float *x, int32_t T, int32_t D, int32_t S, const double *means,
                                 const double *inv, const double *cterm, const double *A, const double *logA,
                                 double *E, double *alpha, double *beta, double *gamma, double *xi, double *scalar,
                                 void *stream) {
  if (int rc = check_dims(S, D > 0 ? D : 1)) return rc;
  SAPR_REQUIRE(op >= 0 && op <= 4 && T > 0, "bad op / T");
  CustomPack P{means, inv, cterm, A, logA};
  SAPR_LAUNCH(custom_piece_kernel, dim3(1), dim3(64), 0, as_stream(stream), op, x, T, D, S, P, E, alpha, beta,
                     gamma, xi, scalar);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
