// Scoring over the vocabulary for full-covariance Gaussian HMMs on gfx950 (hmmlearn's GaussianHMM with
// covariance_type "full" or "tied"): score[n_utts][W] — the forward log-likelihood or the Viterbi log-probability of
// every utterance under EVERY word model — the arg-max word and, for forward scores, the posterior over the words.
//
// Extends the full-covariance path of gmm_hmm.hip (fullcov_ops.h), which evaluates an utterance under the ONE model
// of its tile, over the model loop of decoder.py:42, as gmm_vocab.hip does for the mixtures.  CPU restatement:
// tests/_fullcov_ref.py looped over the words.
//
// Mapping: gmm_vocab_kernel's, through the same scan body (vocab_scan.h).  The (utterance tile, word) grid of
// forward_vocab.hip (viterbi_shared.h decode_block: the W workgroups that read the same 256 utterances sit on one XCD,
// so the features cross HBM once), one lane per utterance, the model wavefront-uniform (scalar loads from the pack of
// sapr_full_pack_layout, nothing else is packed).  Per frame the lane walks the model's own S states in a rolled loop:
// the emission of state j (fullcov_emit.h full_log_density: the triangle Winv_j (x - mu_j), one running dot product
// per row) is evaluated where it is consumed, next to the transition term of column j (reduce_finite: a -inf log
// transition is skipped by a uniform branch).  The recursion's state is SP float64 registers per lane: no lattice and
// no logb ever reach memory, and there is no workspace (sapr_full_vocab_workspace_bytes returns 0; the argument pair
// stays in the ABI for a staged path).  Lanes whose utterance has ended idle until the wavefront's longest one ends.
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
#include "vocab_scan.h"

template <int SP, int DP, bool VIT>
__global__ __launch_bounds__(kBlock) void full_vocab_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
    int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, int32_t W, int32_t S,
    const double *__restrict__ pack, double *__restrict__ score) {
  int64_t tile;
  int w;
  decode_block(W, n_tiles, tile, w);
  if (tile >= n_tiles) return;  // grid padding (whole block leaves together)

  // the wavefront-uniform model -> scalar loads
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * static_cast<int64_t>(full_model_doubles(SP, DP));

  using XT = std::conditional_t<(DP >= 26), float, double>;
  // the next frame in flight under this frame's arithmetic where its DP registers do not cost a wavefront per SIMD (the
  // register table of DESIGN 4.3h was taken for both settings of every instantiation)
  constexpr bool kPrefetch = DP < 26 || (DP >= 39 && SP <= 4);
  vocab_scan<SP, DP, VIT, XT, kPrefetch>(
      feats, offsets, order, n_utts, total_frames, tile, w, D, max_T, W, S, mdl, mdl + SP + SP * SP, score,
      [=](auto x, int j) {
        // (the pointers are formed where they are used: formed ahead of the scan they cost <18, 26, false> a spilled
        // vector register)
        const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
        const double *__restrict__ mu = cc + SP;
        const double *__restrict__ wi = mu + SP * DP;
        return full_log_density<DP>(x, mu + j * DP, wi + static_cast<int64_t>(j) * DP * DP, cc[j]);
      });
}

template <int SP, int DP>
int launch_vocab(const VocabArgs &a, bool vit) {
  return launch_vocab_kernel(vit ? full_vocab_kernel<SP, DP, true> : full_vocab_kernel<SP, DP, false>, a);
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
  if (int rc = check_full_shape(S, D)) return rc;
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
  if (int rc = check_full_shape(S, D)) return rc;
  size_t need = 0;
  if (int rc = sapr_full_vocab_workspace_bytes(n_utts, total_frames, W, S, D, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  return vocab_run({feats, offsets, order, n_utts, total_frames, D, max_T, W, S, pack, score, as_stream(stream)},
                   mode == SAPR_FULL_VOCAB_VITERBI, best_word, word_post, [](const VocabArgs &a, bool vit) {
                     switch (sp_of(a.S)) {
                       case 4: return launch_vocab_dp<4>(a, vit);
                       case 10: return launch_vocab_dp<10>(a, vit);
                       default: return launch_vocab_dp<18>(a, vit);
                     }
                   });
}
