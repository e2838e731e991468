// Scoring over the vocabulary for full-covariance Gaussian HMMs on gfx950 (hmmlearn's GaussianHMM with
// covariance_type "full" or "tied"): score[n_utts][W] — the forward log-likelihood or the Viterbi log-probability of
// every utterance under EVERY word model — the arg-max word and, for forward scores, the posterior over the words.
//
// Extends the full-covariance path of gmm_hmm.hip (fullcov_ops.h), which evaluates an utterance under the ONE model
// of its tile, over the model loop of decoder.py:42, as gmm_vocab.hip does for the mixtures.  CPU restatement:
// tests/_fullcov_ref.py looped over the words.
//
// Mapping: gmm_vocab_kernel's.  The (utterance tile, word) grid of forward_vocab.hip (viterbi_shared.h decode_block:
// the W workgroups that read the same 256 utterances sit on one XCD, so the features cross HBM once), one lane per
// utterance, the model wavefront-uniform (scalar loads from the pack of sapr_full_pack_layout, nothing else is
// packed).  Per frame the lane walks the model's own S states in a rolled loop: the emission of state j
// (fullcov_emit.h full_log_density: the triangle Winv_j (x - mu_j), one running dot product per row) is evaluated
// where it is consumed, next to the transition term of column j (reduce_finite: a -inf log transition is skipped by a
// uniform branch).  The recursion's state is SP float64 registers per lane: no lattice and no logb ever reach memory,
// and there is no workspace (sapr_full_vocab_workspace_bytes returns 0; the argument pair stays in the ABI for a
// staged path).  Lanes whose utterance has ended idle until the wavefront's longest one ends.
//
// Registers: from DP = 26 on the frame stays float32 in registers and is promoted inside the chain (exact), and the
// next frame is prefetched only where its registers do not cost a wavefront per SIMD (kPrefetch below).  No
// instantiation uses scratch memory or spills a vector register (DESIGN 4.3h has the table).
//
// These are the device functions of full_emit_kernel and gmm_forward_kernel, called in the same order on the same
// values (the build runs with -ffp-contract=off, every FMA of the emission is an explicit fma()): score[u][w] carries
// the bits sapr_full_estep / sapr_full_viterbi return for that pair.  Every score is a function of its (utterance,
// model) pair alone; the launch is deterministic.
#include "viterbi_shared.h"

#include <type_traits>

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "fullcov_emit.h"
#include "vocab_epilogue.h"

// per model (fullcov_ops.h full_model_doubles): log_start[SP], log_trans[SP][SP], log_transT[SP][SP], c[SP],
// mu[SP][DP], Winv[SP][DP][DP]
constexpr size_t fv_model_doubles(int SP, int DP) {
  return static_cast<size_t>(SP) + 2 * static_cast<size_t>(SP) * SP + static_cast<size_t>(SP) +
         static_cast<size_t>(SP) * DP + static_cast<size_t>(SP) * DP * DP;
}

inline int check_fv_shape(int32_t S, int32_t D) {
  if (S > kMaxS || D > kMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "the full-covariance kernels serve S in 1..%d, D in 1..%d; got S=%d D=%d", kMaxS,
                kMaxD, S, D);
  return 0;
}

template <int DP, class XT>
__device__ __forceinline__ void load_frame_as(const float *__restrict__ xp, int D, bool live, XT (&x)[DP]) {
#pragma unroll
  for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? static_cast<XT>(xp[d]) : static_cast<XT>(0);
}

template <int SP, int DP, bool VIT>
__global__ __launch_bounds__(kBlock) void full_vocab_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
    int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, int32_t W, int32_t S,
    const double *__restrict__ pack, double *__restrict__ score) {
  int64_t tile;
  int w;
  decode_block(W, n_tiles, tile, w);
  if (tile >= n_tiles) return;  // grid padding (whole block leaves together)

  const int64_t slot = tile * kBlock + threadIdx.x;
  const bool live = slot < n_utts;
  const int64_t u = live ? (order ? static_cast<int64_t>(order[slot]) : slot) : -1;
  const Span sp = utt_span(offsets, u, live, n_utts, total_frames, max_T);  // served as empty: T = 0
  const int T = sp.T;
  const int Tw = __builtin_amdgcn_readfirstlane(wave_max_i32(T));

  // wavefront-uniform model pointers -> scalar loads
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * static_cast<int64_t>(fv_model_doubles(SP, DP));
  const double *__restrict__ ls = mdl;
  const double *__restrict__ ltT = mdl + SP + SP * SP;
  const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
  const double *__restrict__ mu = cc + SP;
  const double *__restrict__ wi = mu + SP * DP;
  const float *__restrict__ xp = feats + sp.beg * D;

  using XT = std::conditional_t<(DP >= 26), float, double>;
  // the next frame in flight under this frame's arithmetic where its DP registers do not cost a wavefront per SIMD (the
  // register table of DESIGN 4.3h was taken for both settings of every instantiation)
  constexpr bool kPrefetch = DP < 26 || (DP >= 39 && SP <= 4);
  XT xn[kPrefetch ? DP : 1];
  if constexpr (kPrefetch) load_frame_as<DP>(xp, D, T > 0, xn);

  double fwd[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) fwd[s] = neg_inf();  // (a padded state keeps it: -inf + -inf in the per-model kernels)

  for (int t = 0; t < Tw; ++t) {
    if (t < T) {
      XT x[DP];
      double prev[SP];
      if constexpr (kPrefetch) {
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
        const double lb = full_log_density<DP>([&](int d) { return static_cast<double>(x[d]); }, mu + j * DP,
                                               wi + static_cast<int64_t>(j) * DP * DP, cc[j]);
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

struct VocabArgs {
  const float *feats;
  const int64_t *offsets;
  const int32_t *order;
  int64_t n_utts, total_frames, n_tiles;
  int32_t D, max_T, W, S;
  const double *pack;
  double *score;
  unsigned blocks;
  hipStream_t stream;
};

template <int SP, int DP>
int launch_vocab(const VocabArgs &a, bool vit) {
  const dim3 grid(a.blocks), block(kBlock);
  if (vit)
    SAPR_LAUNCH((full_vocab_kernel<SP, DP, true>), grid, block, 0, a.stream, a.feats, a.offsets, a.order, a.n_utts,
                a.total_frames, a.n_tiles, a.D, a.max_T, a.W, a.S, a.pack, a.score);
  else
    SAPR_LAUNCH((full_vocab_kernel<SP, DP, false>), grid, block, 0, a.stream, a.feats, a.offsets, a.order, a.n_utts,
                a.total_frames, a.n_tiles, a.D, a.max_T, a.W, a.S, a.pack, a.score);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int SP>
int launch_vocab_dp(const VocabArgs &a, bool vit) {
  switch (dp_of(a.D)) {
    case 13: return launch_vocab<SP, 13>(a, vit);
    case 26: return launch_vocab<SP, 26>(a, vit);
    default: return launch_vocab<SP, 39>(a, vit);
  }
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_full_vocab_workspace_bytes(int64_t n_utts, int64_t total_frames, int32_t W, int32_t S, int32_t D,
                                               size_t *bytes) {
  SAPR_REQUIRE(bytes && n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0 && D > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d D=%d)", (long long)n_utts, (long long)total_frames,
               W, S, D);
  if (int rc = check_fv_shape(S, D)) return rc;
  *bytes = 0;  // every instantiation takes the fused path: nothing is staged
  return 0;
}

extern "C" int sapr_full_vocab(const float *feats, const int64_t *offsets, const int32_t *order, int64_t n_utts,
                               int64_t total_frames, int32_t D, int32_t max_T, const double *pack, int32_t W,
                               int32_t S, int32_t mode, void *workspace, size_t workspace_bytes, double *score,
                               int32_t *best_word, double *word_post, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0 && D > 0 && max_T >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d D=%d max_T=%d)", (long long)n_utts,
               (long long)total_frames, W, S, D, max_T);
  SAPR_REQUIRE(mode == SAPR_FULL_VOCAB_FORWARD || mode == SAPR_FULL_VOCAB_VITERBI, "bad mode %d", mode);
  if (int rc = check_fv_shape(S, D)) return rc;
  const bool vit = mode == SAPR_FULL_VOCAB_VITERBI;
  SAPR_REQUIRE(!vit || !word_post, "word_post is served in forward mode only: a soft-max of path scores is no posterior");
  const int64_t n_tiles = (n_utts + kBlock - 1) / kBlock;
  const int64_t blocks = round_up(n_tiles, kXcd) * W;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  size_t need = 0;
  if (int rc = sapr_full_vocab_workspace_bytes(n_utts, total_frames, W, S, D, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(feats && offsets && pack && score, "NULL pointer argument");
  VocabArgs a;
  a.feats = feats;
  a.offsets = offsets;
  a.order = order;
  a.n_utts = n_utts;
  a.total_frames = total_frames;
  a.n_tiles = n_tiles;
  a.D = D;
  a.max_T = max_T;
  a.W = W;
  a.S = S;
  a.pack = pack;
  a.score = score;
  a.blocks = static_cast<unsigned>(blocks);
  a.stream = as_stream(stream);
  int rc;
  switch (sp_of(S)) {
    case 4: rc = launch_vocab_dp<4>(a, vit); break;
    case 10: rc = launch_vocab_dp<10>(a, vit); break;
    default: rc = launch_vocab_dp<18>(a, vit); break;
  }
  if (rc) return rc;
  if (best_word || word_post) {
    SAPR_LAUNCH(vocab_epilogue_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(kBlock), 0, a.stream, n_utts, W,
                score, best_word, word_post);
    SAPR_HIP_TRY(hipGetLastError());
  }
  return 0;
}
