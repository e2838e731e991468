// The forward recursion of the diagonal-Gaussian family, once: the lane and its model, one frame of _hmmc.cpp
// forward_log, the NF-frame walk over the quick-form log-densities and the (D, S) ladder.  estep.hip (GaussianHMM.score,
// the E-step), state_posteriors.hip (pass 1) and forward_vocab.hip are this body plus what each of them keeps:
//     fb_score_kernel            forward_step on numpy-order log-densities           keeps nothing
//     fb_forward_kernel          its own NF-frame loop over the slot-major copy      keeps the stay shares
//     fb_forward_dense_kernel    forward_step on fb_emit_kernel's stored rows        stores the forward rows
//     sp_forward_kernel          quick_forward_walk over the frame-major batch       shares, or forward rows + densities
//     forward_vocab_kernel       quick_forward_walk over the frame-major batch       keeps nothing
// Like lse_ops.h this header is included INSIDE the unit's `namespace sapr { namespace {`, after emission_quick.h and
// lse_ops.h (lse2, lse2_share, lse_all).
#pragma once

// One lane = one utterance: u < 0 is an empty slot (T = 0, nothing stored).  How a slot finds its utterance
// (slot_utt[slot]; order[slot] or the slot itself) is the caller's.  Tw: the longest utterance of the wavefront.
struct Lane {
  int64_t u, beg;
  bool live;
  int T, Tw;
};
__device__ __forceinline__ Lane lane_of(const int64_t *__restrict__ offsets, int64_t u) {
  Lane ln;
  ln.u = u;
  ln.live = u >= 0;
  ln.beg = ln.live ? offsets[u] : 0;
  ln.T = ln.live ? static_cast<int>(offsets[u + 1] - ln.beg) : 0;
  ln.Tw = wave_max_i32(ln.T);
  return ln;
}

// model w of the pack: wavefront-uniform pointers -> scalar loads
struct DiagModel {
  const double4 *__restrict__ prm;
  const double *__restrict__ gc, *__restrict__ ls, *__restrict__ lt;
};
template <int D, int S>
__device__ __forceinline__ DiagModel diag_model(const double4 *__restrict__ prm_all, const double *__restrict__ gconst,
                                                const double *__restrict__ log_start,
                                                const double *__restrict__ log_trans, int w) {
  return {prm_all + static_cast<int64_t>(w) * S * D, gconst + static_cast<int64_t>(w) * S,
          log_start + static_cast<int64_t>(w) * S, log_trans + static_cast<int64_t>(w) * S * S};
}
// the chain alone, for a kernel that reads stored log-densities and has no emission parameters
template <int S>
__device__ __forceinline__ DiagModel diag_model(const double *__restrict__ log_start,
                                                const double *__restrict__ log_trans, int w) {
  return {nullptr, nullptr, log_start + static_cast<int64_t>(w) * S, log_trans + static_cast<int64_t>(w) * S * S};
}

// policy of the bidiagonal update: keep nothing (lse2).  Any other type is a callable (t, j, stay) that is handed the
// share of state j's mass at frame t that STAYED in j (lse2_share; the rest came from j - 1).  State 0 has no
// predecessor: its share is the constant 1 and is not handed over.
struct NoShares {};

// One frame of _hmmc.cpp forward_log from the frame's log-densities b: fwd = alpha_(t-1) on entry (log_start for
// t == 0), alpha_t on exit.  What a caller keeps of a frame (the dense lattice rows) it stores after the step.
template <int S, bool BIDIAG, class Shares = NoShares>
__device__ __forceinline__ void forward_step(int t, const double (&b)[S], const double *__restrict__ lt,
                                             double (&fwd)[S], Shares &&shares = Shares{}) {
  if (t == 0) {
#pragma unroll
    for (int j = 0; j < S; ++j) fwd[j] += b[j];
  } else if constexpr (BIDIAG) {
    // descending j: fwd[j - 1] is still the previous frame's value when state j reads it
#pragma unroll
    for (int j = S - 1; j >= 1; --j) {
      if constexpr (std::is_same_v<std::decay_t<Shares>, NoShares>) {
        fwd[j] = lse2(fwd[j - 1] + lt[(j - 1) * S + j], fwd[j] + lt[j * S + j]) + b[j];
      } else {
        double stay;
        fwd[j] = lse2_share(fwd[j - 1] + lt[(j - 1) * S + j], fwd[j] + lt[j * S + j], stay) + b[j];
        shares(t, j, stay);
      }
    }
    fwd[0] = (fwd[0] + lt[0]) + b[0];
  } else {
    double prev[S], work[S];
#pragma unroll
    for (int s = 0; s < S; ++s) prev[s] = fwd[s];
#pragma unroll
    for (int j = 0; j < S; ++j) {
#pragma unroll
      for (int i = 0; i < S; ++i) work[i] = prev[i] + lt[i * S + j];
      fwd[j] = lse_all<S>(work) + b[j];
    }
  }
}

// frames per walk over the SGPR-resident parameters (256 registers: two wavefronts per SIMD)
template <int D, int S>
constexpr int quick_frames() {
  return (D >= 39 || S > 10) ? 2 : 4;
}
// 39-dimensional frames stay float32 in registers and are promoted inside the chain (emission_quick.h)
template <int D>
using quick_x_t = std::conditional_t<(D >= 39), float, double>;

// a frame of the frame-major batch, for the `load` of quick_forward_walk
template <int D>
__device__ __forceinline__ void load_quick_frame(const float *__restrict__ p, double (&x)[D]) {
  emission::load_frame<D>(p, x);
}
template <int D>
__device__ __forceinline__ void load_quick_frame(const float *__restrict__ p, float (&x)[D]) {
  emission::load_frame_f32<D>(p, x);
}

struct NoRows {
  template <int S>
  __device__ __forceinline__ void operator()(int, const double (&)[S], const double (&)[S]) const {}
};

// The whole forward pass of one lane in the quick emission form: fwd = log_start, then NF frames per walk —
// load(t, x_row) fills a frame's float32 features, frame_log_densities_quick evaluates the NF x S log-densities in one pass
// over the parameters, forward_step consumes them frame by frame and rows(t, b, fwd) sees each finished frame.
template <int D, int S, bool BIDIAG, class Load, class Shares = NoShares, class Rows = NoRows>
__device__ __forceinline__ void quick_forward_walk(const Lane &ln, const DiagModel &m, double (&fwd)[S], Load &&load,
                                                   Shares &&shares = Shares{}, Rows &&rows = Rows{}) {
  constexpr int NF = quick_frames<D, S>();
  const int T = ln.T;
#pragma unroll
  for (int s = 0; s < S; ++s) fwd[s] = m.ls[s];
  for (int t0 = 0; t0 < ln.Tw; t0 += NF) {
    if (t0 < T) {
      // frames past the end: the walk's first frame again (it is always there), evaluated and not used — with T - 1
      // for them the walk held two more VGPRs, a wavefront per SIMD in sp_forward_kernel<39, 10, dense>
      float xf[NF][D];
#pragma unroll
      for (int f = 0; f < NF; ++f) load(t0 + f < T ? t0 + f : t0, xf[f]);
      // float64 walks (D = 13): every load of the NF frames is issued before the first value is widened — left to
      // itself the scheduler waits for each frame's loads before it issues the next frame's (3 - 8 % of the 13 x 10
      // walks).  float32 walks widen nothing here.
      if constexpr (!std::is_same_v<quick_x_t<D>, float>) __builtin_amdgcn_sched_barrier(0);
      quick_x_t<D> xq[NF][D];
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int d = 0; d < D; ++d) xq[f][d] = static_cast<quick_x_t<D>>(xf[f][d]);  // float32 -> float64 is exact
      double bq[NF][S];
      emission::frame_log_densities_quick<D, S, NF>(
          xq, m.prm, m.gc, [&](auto jc, int f, double bv) { bq[f][decltype(jc)::value] = bv; });
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (t0 + f < T) {
          forward_step<S, BIDIAG>(t0 + f, bq[f], m.lt, fwd, shares);
          rows(t0 + f, bq[f], fwd);
        }
    }
  }
}

// The (D, S) shapes the trellis kernels are instantiated for: f(integral_constant<D>, integral_constant<S>).
template <class F>
int dispatch_ds(int D, int S, F &&f) {
  using std::integral_constant;
  if (D == 13 && S == 10) return f(integral_constant<int, 13>{}, integral_constant<int, 10>{});
#ifndef SAPR_ONLY_13_10
  if (D == 13 && S == 18) return f(integral_constant<int, 13>{}, integral_constant<int, 18>{});
  if (D == 39 && S == 10) return f(integral_constant<int, 39>{}, integral_constant<int, 10>{});
  if (D == 39 && S == 18) return f(integral_constant<int, 39>{}, integral_constant<int, 18>{});
#endif
  return fail(SAPR_ERR_UNSUPPORTED, "trellis kernels are instantiated for (D,S) in {13,39}x{10,18}; got D=%d S=%d", D,
              S);
}
