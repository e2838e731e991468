// Scoring over the vocabulary for Gaussian-mixture HMMs on gfx950: score[n_utts][W] — the forward log-likelihood
// (hmmlearn _hmmc.cpp forward_log) or the Viterbi log-probability (viterbi) of every utterance under EVERY word model
// over mixture emissions — the arg-max word and, for forward scores, the posterior over the words.
//
// Extends gmm_hmm.hip, which evaluates an utterance under the ONE model of its tile, over the model loop of
// decoder.py:42, as forward_vocab.hip does for the single-Gaussian models.  CPU restatement: tests/_gmmhmm_ref.py
// looped over the words.
//
// Mapping: the (utterance tile, word) grid of forward_vocab.hip (viterbi_shared.h decode_block: the W workgroups that
// read the same 256 utterances sit on one XCD, so the features cross HBM once), one lane per utterance, the model
// wavefront-uniform (scalar loads from the pack of sapr_gmm_pack_layout, nothing else is packed); the scan body is
// vocab_scan.h's, shared with full_vocab.hip.  Per frame the lane walks the model's own S states in a rolled loop: the
// mixture emission of state j (gmm_ops.h mix_log_terms, then lse_all over the components) is evaluated where it is
// consumed, next to the transition term of column j (reduce_finite: a -inf log transition is skipped by a uniform
// branch).  The recursion's state is SP float64 registers per lane: no lattice and no logb ever reach memory, and
// there is no workspace.  Lanes whose utterance has ended idle until the wavefront's longest one ends.
//
// These are the device functions of gmm_emit_kernel and gmm_forward_kernel, called in the same order on the same
// values (the build runs with -ffp-contract=off, the emission's one FMA is an explicit fma(); a float32 frame promoted
// inside the chain is exact): score[u][w] carries the bits sapr_gmm_estep_diag / sapr_gmm_viterbi_diag return for that
// pair.  Every score is a function of its (utterance, model) pair alone; the launch is deterministic.
#include "viterbi_shared.h"

#include <type_traits>

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "vocab_scan.h"

template <int SP, int MP, int DP, bool VIT>
__global__ __launch_bounds__(kBlock) void gmm_vocab_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
    int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, int32_t W, int32_t S,
    const double *__restrict__ pack, double *__restrict__ score) {
  int64_t tile;
  int w;
  decode_block(W, n_tiles, tile, w);
  if (tile >= n_tiles) return;  // grid padding (whole block leaves together)

  // wavefront-uniform model pointers -> scalar loads
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * static_cast<int64_t>(model_doubles(SP, MP, DP));
  const double *__restrict__ cc = mdl + off_cc(SP);
  const double *__restrict__ prm = mdl + off_prm(SP, MP);

  // 39-dimensional frames stay float32 in registers and are promoted inside the chain (exact); the next frame is
  // always in flight under this frame's arithmetic
  using XT = std::conditional_t<(DP >= 39), float, double>;
  vocab_scan<SP, DP, VIT, XT, true>(feats, offsets, order, n_utts, total_frames, tile, w, D, max_T, W, S,
                                    mdl + off_log_start(), mdl + off_log_transT(SP), score, [=](auto x, int j) {
                                      double lc[MP];
                                      mix_log_terms<MP, DP>(x, prm + static_cast<int64_t>(j) * DP * MP * 2,
                                                            cc + j * MP, lc);
                                      if constexpr (MP == 1)
                                        return lc[0];
                                      else
                                        return lse_all<MP>(lc);
                                    });
}

template <int SP, int MP, int DP>
int launch_vocab(const VocabArgs &a, bool vit) {
  return launch_vocab_kernel(vit ? gmm_vocab_kernel<SP, MP, DP, true> : gmm_vocab_kernel<SP, MP, DP, false>, a);
}

template <int SP, int MP>
int launch_vocab_dp(const VocabArgs &a, bool vit) {
  switch (dp_of(a.D)) {
    case 13: return launch_vocab<SP, MP, 13>(a, vit);
    case 26: return launch_vocab<SP, MP, 26>(a, vit);
    default: return launch_vocab<SP, MP, 39>(a, vit);
  }
}

template <int SP>
int launch_vocab_mp(const VocabArgs &a, bool vit, int M) {
  switch (mp_of(M)) {
    case 1: return launch_vocab_dp<SP, 1>(a, vit);
    case 2: return launch_vocab_dp<SP, 2>(a, vit);
    case 4: return launch_vocab_dp<SP, 4>(a, vit);
    default: return launch_vocab_dp<SP, 8>(a, vit);
  }
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_gmm_vocab_diag(const float *feats, const int64_t *offsets, const int32_t *order, int64_t n_utts,
                                   int64_t total_frames, int32_t D, int32_t max_T, const double *pack, int32_t W,
                                   int32_t S, int32_t M, int32_t mode, double *score, int32_t *best_word,
                                   double *word_post, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0 && M > 0 && D > 0 && max_T >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d M=%d D=%d max_T=%d)", (long long)n_utts,
               (long long)total_frames, W, S, M, D, max_T);
  SAPR_REQUIRE(mode == SAPR_GMM_VOCAB_FORWARD || mode == SAPR_GMM_VOCAB_VITERBI, "bad mode %d", mode);
  if (int rc = check_shape(S, M, D)) return rc;
  return vocab_run({feats, offsets, order, n_utts, total_frames, D, max_T, W, S, pack, score, as_stream(stream)},
                   mode == SAPR_GMM_VOCAB_VITERBI, best_word, word_post, [M](const VocabArgs &a, bool vit) {
                     switch (sp_of(a.S)) {
                       case 4: return launch_vocab_mp<4>(a, vit, M);
                       case 10: return launch_vocab_mp<10>(a, vit, M);
                       default: return launch_vocab_mp<18>(a, vit, M);
                     }
                   });
}
