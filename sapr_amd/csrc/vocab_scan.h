// The lane-per-utterance scan behind the vocabulary scorers of the mixture and the full-covariance models
// (gmm_vocab.hip, full_vocab.hip), and the host path the two entry points share.  Like gmm_ops.h this header is
// included INSIDE the unit's `namespace sapr { namespace {`, after viterbi_shared.h, lse_ops.h and gmm_ops.h.
//
// The two families differ in the emission of state j (a callable), in the DP from which the frame stays float32 (XT)
// and in whether the next frame is prefetched (PREFETCH): the kernels choose these and hand over their model's
// log_start and transposed log_trans.  Everything else — the span of the utterance, the rolled loop over the states,
// the NaN and -inf rules of reduce_finite, the first-maximum ending — is here once.
#pragma once

#include "vocab_epilogue.h"

template <int DP, class XT>
__device__ __forceinline__ void load_frame_as(const float *__restrict__ xp, int D, bool live, XT (&x)[DP]) {
#pragma unroll
  for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? static_cast<XT>(xp[d]) : static_cast<XT>(0);
}

// score[u][w] for the utterance of this lane's slot in `tile` under word w: the forward log-likelihood (_hmmc.cpp
// forward_log) or, VIT, the Viterbi log-probability.  emit(x, j) is the log density of state j at the frame x(d)
// (float64 from an accessor); ls and ltT are wavefront-uniform.
template <int SP, int DP, bool VIT, class XT, bool PREFETCH, class EMIT>
__device__ __forceinline__ void vocab_scan(const float *__restrict__ feats, const int64_t *__restrict__ offsets,
                                           const int32_t *__restrict__ order, int64_t n_utts, int64_t total_frames,
                                           int64_t tile, int w, int32_t D, int32_t max_T, int32_t W, int32_t S,
                                           const double *__restrict__ ls, const double *__restrict__ ltT,
                                           double *__restrict__ score, EMIT emit) {
  const int64_t slot = tile * kBlock + threadIdx.x;
  const bool live = slot < n_utts;
  const int64_t u = live ? (order ? static_cast<int64_t>(order[slot]) : slot) : -1;
  const Span sp = utt_span(offsets, u, live, n_utts, total_frames, max_T);  // served as empty: T = 0
  const int T = sp.T;
  const int Tw = __builtin_amdgcn_readfirstlane(wave_max_i32(T));
  const float *__restrict__ xp = feats + sp.beg * D;

  XT xn[PREFETCH ? DP : 1];
  if constexpr (PREFETCH) load_frame_as<DP>(xp, D, T > 0, xn);

  double fwd[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) fwd[s] = neg_inf();  // (a padded state keeps it: -inf + -inf in the per-model kernels)

  for (int t = 0; t < Tw; ++t) {
    if (t < T) {
      XT x[DP];
      double prev[SP];
      if constexpr (PREFETCH) {
#pragma unroll
        for (int d = 0; d < DP; ++d) x[d] = xn[d];
        const int tn = t + 1 < T ? t + 1 : t;  // the next frame in flight under this frame's arithmetic
        load_frame_as<DP>(xp + static_cast<int64_t>(tn) * D, D, true, xn);
      } else {
        load_frame_as<DP>(xp + static_cast<int64_t>(t) * D, D, true, x);
      }
#pragma unroll
      for (int s = 0; s < SP; ++s) prev[s] = fwd[s];
      // state after state in a rolled loop over the model's own S states: the parameters of state j and column j of
      // the transition matrix are runs of scalar loads, and the value lands in register j by a uniform select
#pragma unroll 1
      for (int j = 0; j < S; ++j) {
        const double lb = emit([&](int d) { return static_cast<double>(x[d]); }, j);
        double v;
        if (t == 0) {  // (uniform)
          v = ls[j];
        } else {
          const double *__restrict__ col = ltT + j * SP;
          v = reduce_finite<SP, VIT>([&](int i) { return prev[i]; }, [&](int i) { return col[i]; });
        }
#pragma unroll
        for (int k = 0; k < SP; ++k) fwd[k] = k == j ? v + lb : fwd[k];
      }
    }
  }
  if (sp.u < 0) return;  // no utterance in this slot (or an `order` entry outside the batch: never followed)
  double out = neg_inf();
  if (T > 0) {
    if constexpr (!VIT) {
      out = lse_all<SP>(fwd);
    } else {  // _hmmc.cpp viterbi: the first maximum of the last row
      const int st = argmax_first<SP>(fwd, S);
      out = fwd[0];
#pragma unroll
      for (int s = 1; s < SP; ++s) out = s == st ? fwd[s] : out;
    }
  }
  score[sp.u * W + w] = out;
}

// ---- host -----------------------------------------------------------------------------------
struct VocabArgs {
  const float *feats;
  const int64_t *offsets;
  const int32_t *order;
  int64_t n_utts, total_frames;
  int32_t D, max_T, W, S;
  const double *pack;
  double *score;
  hipStream_t stream;
  int64_t n_tiles;  // (filled by vocab_run)
  unsigned blocks;
};

// One instantiation of a vocabulary kernel: they all take these arguments.
using VocabKernel = void (*)(const float *, const int64_t *, const int32_t *, int64_t, int64_t, int64_t, int32_t,
                             int32_t, int32_t, int32_t, const double *, double *);

inline int launch_vocab_kernel(VocabKernel kernel, const VocabArgs &a) {
  SAPR_LAUNCH(kernel, dim3(a.blocks), dim3(kBlock), 0, a.stream, a.feats, a.offsets, a.order, a.n_utts, a.total_frames,
              a.n_tiles, a.D, a.max_T, a.W, a.S, a.pack, a.score);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// What follows an entry point's own size, mode and shape checks: the rule for word_post, the grid, the family's
// dispatch over its instantiations (launch(a, vit) -> error code) and the epilogue.
template <class LAUNCH>
int vocab_run(VocabArgs a, bool vit, int32_t *best_word, double *word_post, LAUNCH launch) {
  SAPR_REQUIRE(!vit || !word_post, "word_post is served in forward mode only: a soft-max of path scores is no posterior");
  a.n_tiles = (a.n_utts + kBlock - 1) / kBlock;
  const int64_t blocks = round_up(a.n_tiles, kXcd) * a.W;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (a.n_utts == 0) return 0;
  SAPR_REQUIRE(a.feats && a.offsets && a.pack && a.score, "NULL pointer argument");
  a.blocks = static_cast<unsigned>(blocks);
  if (int rc = launch(a, vit)) return rc;
  if (best_word || word_post) return launch_vocab_epilogue(a.n_utts, a.W, a.score, best_word, word_post, a.stream);
  return 0;
}
