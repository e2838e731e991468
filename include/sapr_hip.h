/* sapr_hip.h — C ABI of libsapr_hip.so, the MI355X (gfx950) implementation of the
 * data-parallel hot path of frankcholula/sapr assignment2 (MFCC front-end +
 * Gaussian-HMM Viterbi / forward-backward).
 *
 * The reference has no FFI layer: its hot path is plain Python (numpy, hmmlearn,
 * librosa).  Each entry point below names the reference call (file:line under
 * /root/reference/assignment2) whose arithmetic it replaces; the ctypes stub a
 * maintainer adds on the reference side is shown in INTEGRATION.md and shipped in
 * sapr_amd/_lib.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - no torch / HIP types in signatures: `stream` is a hipStream_t passed as void*
 *     (NULL = default stream); launches are asynchronous on that stream;
 *   - feature batches are ragged and frame-major: feats[total_frames][D] float32,
 *     offsets[n_utts+1] int64 (utterance u owns frames offsets[u] .. offsets[u+1]-1).
 *     This is the transpose of the reference's per-utterance (D,T) numpy arrays
 *     (mfcc_extract.py:15-24; decoder.py:59 already hands hmmlearn the (T,D) view);
 *   - word models are float64 arrays means[W][S][D], vars[W][S][D], gconst[W][S], log_start[W][S],
 *     log_trans[W][S][S] (W word models, S states), packed once by sapr_diag_pack;
 *   - return value: 0 on success, <0 argument/shape error, >0 hipError_t;
 *     sapr_last_error() returns a thread-local message for the last failure.
 */
#ifndef SAPR_HIP_H
#define SAPR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAPR_ABI_VERSION 2

/* transition topology of a model pack */
#define SAPR_TOPO_DENSE 0  /* any S x S log_trans */
#define SAPR_TOPO_BIDIAG 1 /* only log_trans[i][i] and log_trans[i][i+1] are > -inf
                              (hmmlearn_hmm.py:45-78, custom_hmm.py:94-116) */

/* back-trace tie-break of GaussianHMM.decode (see oracle/hmmlearn_oracle.py) */
#define SAPR_TIE_LOW 0  /* equal scores -> lower predecessor index  (Cython _argmax, hmmlearn <= 0.2.7) */
#define SAPR_TIE_HIGH 1 /* equal scores -> higher predecessor index (std::max over (value,index), 0.3.x) */

/* order of the sum over the D feature dimensions inside the log-density: numpy's reduction
 * order depends on the memory layout of the X array hmmlearn receives (see viterbi.hip) */
#define SAPR_SUM_PAIRWISE 0 /* X is a C-contiguous (T,D) array: fit/score, hmmlearn_hmm.py:80-81 */
#define SAPR_SUM_TVIEW 1    /* X is the transposed view of a (D,T) array, decoder.py:59: left-to-right
                               sum when T > 1, pair-wise when T == 1 */
#define SAPR_SUM_SEQ 2      /* left-to-right sum for every utterance: numpy's order for fewer than 8 dimensions in
                               either layout — what a model narrower than 8 dimensions needs when it runs padded
                               to an instantiated width (sapr_amd/trellis.py kernel_dims) */

/* bits of sapr_diag_pack's *pack_flags output, passed on to the decode entry points */
#define SAPR_PACK_FAST_DIV 1 /* parameters inside the proven domain of the FMA-based exactly-rounded division */
#define SAPR_PACK_BOUND_OK 2 /* variances in [1e-20, 1e20]: the pruned decoder's float32 bounding pass is valid */
#define SAPR_ESTEP_STAGED 256 /* sapr_estep_diag only, OR-ed into its fast_div argument: the workspace still holds the
                                 slot-major feature copy a previous call made for the SAME feats / offsets / slot_utt
                                 (the features do not change between EM iterations) */
#define SAPR_PACK_GEMM_OK 4  /* the bounding pass may run on the matrix cores (finite coefficients; states without a
                                self-loop only at chain positions 0, 4, 8, 12) */
#define SAPR_PACK_BIDIAG 8   /* every log_trans entry off the i -> i, i -> i + 1 band is -inf (hmmlearn_hmm.py:45-78
                                topology): what sapr_viterbi_decode_pruned walks; it refuses packs without this bit */

#define SAPR_PACK_EXACT_ONLY 16 /* INPUT bit of *pack_flags (the caller sets it before the call; it is echoed back): build
                                   the exact-kernel operands only — what sapr_estep_diag, sapr_forward_diag and the
                                   all-vocabulary Viterbi read — and leave out the bounding-pass operands; BOUND_OK and
                                   GEMM_OK stay clear, so the pruned decoder refuses the pack.  A Baum-Welch loop
                                   (hmmlearn_hmm.py:103 -> base.fit) packs a new model every iteration and never
                                   decodes with it */

#define SAPR_ERR_ARG (-1)
#define SAPR_ERR_UNSUPPORTED (-2)
#define SAPR_ERR_WORKSPACE (-3)

int sapr_abi_version(void);
const char *sapr_last_error(void);
/* number of CUs / wave size / gcnArchName of device `dev`; arch buffer may be NULL */
int sapr_device_info(int dev, int *cu_count, int *wave_size, char *arch, size_t arch_len);
/* self-test of the device arithmetic behind the E-step's two-term log-sum-exp (csrc/lse_unit.h; the CPU check of that
 * header cannot see the hardware's reciprocal estimate, v_ldexp_f64 and v_rndne_f64): for d[i] >= 0
 * out = [exp(-d) | 1 / (1 + exp(-d)) | log(1 + exp(-d)) | exp_unit(-d)], four runs of n doubles */
int sapr_selftest_lse(const double *d, int64_t n, double *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Viterbi decode, diagonal Gaussians, every state emitting.
 * Replaces GaussianHMM.decode(X) as called at decoder.py:43 for ALL W word models of
 * decoder.py:42 at once (log-density: hmmlearn stats.py _log_multivariate_normal_density_diag;
 * lattice + back-trace: hmmlearn _hmmc.cpp viterbi).  Scores are bit-identical to the
 * float64 numpy/C++ evaluation (same operation order, IEEE division, no FMA contraction).
 *
 *   pass 1  sapr_viterbi_diag_scores   scores[n_utts][W], last_state[n_utts][W], back-pointer
 *                                      words in `workspace`
 *   pass 2  sapr_viterbi_backtrace     state path of ONE model per utterance: the arg-max word
 *                                      (decoder.py:42-47, strict '>' in model order) when
 *                                      word_sel == NULL, else model word_sel[u]
 *
 * `order` (optional, may be NULL) is a permutation of utterances, normally sorted by length so
 * that the 64 lanes of a wavefront walk trellises of similar T.
 * ---------------------------------------------------------------------------------- */
int sapr_viterbi_workspace_bytes(int64_t n_utts, int32_t W, int32_t S, int32_t max_T,
                                 int32_t topology, size_t *bytes);

/* Model preparation (once per set of word models, not per batch): interleaves the float64
 * arrays  means[W][S][D], vars[W][S][D] (covars floored at DBL_MIN like hmmlearn stats.py),
 * gconst[W][S] = D*log(2*pi) + sum_d log var, log_start[W][S], log_trans[W][S][S]
 * into one device blob {mean, var, RN(1/var), RN(1/var - RN(1/var))} ... that the kernels read with scalar loads.
 * *pack_flags: SAPR_PACK_FAST_DIV is set when every parameter lies in the domain where the FMA-based
 * exactly-rounded division of viterbi.hip is proven equal to IEEE division (pass it on as `fast_div`; 0
 * selects the IEEE-division instantiation — same bits, slower); SAPR_PACK_BOUND_OK when the pruned decoder
 * may be used.  *pack_flags is read on entry as well: initialise it to 0, or to SAPR_PACK_EXACT_ONLY (above).
 * Synchronises `stream`. */
int sapr_diag_pack_bytes(int32_t W, int32_t S, int32_t D, size_t *bytes);
int sapr_diag_pack(const double *means, const double *vars, const double *gconst,
                   const double *log_start, const double *log_trans, int32_t W, int32_t S, int32_t D,
                   void *pack, size_t pack_bytes, int32_t *pack_flags /* host */, void *stream);

int sapr_viterbi_diag_scores(const float *feats, const int64_t *offsets, const int32_t *order,
                             int64_t n_utts, int32_t D, int32_t max_T, const void *pack,
                             int32_t W, int32_t S, int32_t topology, int32_t tie, int32_t sum_order,
                             int32_t fast_div, void *workspace, size_t workspace_bytes,
                             double *scores, int32_t *last_state, void *stream);

int sapr_viterbi_backtrace(const int64_t *offsets, const int32_t *order, int64_t n_utts,
                           int32_t max_T, int32_t W, int32_t S, int32_t topology,
                           const void *workspace, size_t workspace_bytes,
                           const double *scores, const int32_t *last_state,
                           const int32_t *word_sel, /* NULL -> arg-max over words */
                           int32_t *best_word, double *best_score,
                           int32_t *path /* [total_frames] */, void *stream);

/* Pruned decode: Decoder.decode_sequence (decoder.py:35-49) returns only the best word, its score and its
 * state path, so the exact lattice is evaluated only for the words that can still be the arg-max.
 *   pass A  float32 emission sums (3 instead of 7 VALU instructions per state and dimension, at the float32
 *           rate, no back-pointers) give every word an interval [score - eps, score + eps] that provably
 *           contains its exact score (viterbi.hip states the bound);
 *   pass B  a word is dropped when its interval lies strictly below another word's;
 *   pass C  sapr_viterbi_diag_scores' kernel over the remaining (utterance, word) pairs;
 *   pass D  arg-max among them (first strict maximum in model order) and back-trace.
 * best_word / best_score / path are bit-identical to sapr_viterbi_diag_scores + sapr_viterbi_backtrace
 * (word_sel == NULL).  pack_flags & SAPR_PACK_BIDIAG (bidiagonal topology, scanned by sapr_diag_pack) and
 * pack_flags & SAPR_PACK_BOUND_OK required (SAPR_ERR_UNSUPPORTED otherwise: use the two-call form).  sapr_viterbi_pruned_views exposes the intermediate arrays inside
 * `workspace` ([n_utts][W] each; cand_slot < 0 = dropped; cand_count[W]) for tests and diagnostics. */
int sapr_viterbi_pruned_workspace_bytes(int64_t n_utts, int32_t W, int32_t S, int32_t max_T, size_t *bytes);
int sapr_viterbi_decode_pruned(const float *feats, const int64_t *offsets, const int32_t *order, int64_t n_utts,
                               int32_t D, int32_t max_T, const void *pack, int32_t W, int32_t S, int32_t tie,
                               int32_t sum_order, int32_t pack_flags, void *workspace, size_t workspace_bytes,
                               int32_t *best_word, double *best_score, int32_t *path /* [total_frames] */,
                               void *stream);
int sapr_viterbi_pruned_views(int64_t n_utts, int32_t W, int32_t max_T, void *workspace, double **approx_score,
                              double **approx_eps, double **exact_score, int32_t **cand_slot,
                              int32_t **cand_count);

/* ------------------------------------------------------------------------------------
 * Forward scoring and Baum-Welch E-step, diagonal Gaussians, every state emitting.
 * Replace GaussianHMM.score / the E-step of GaussianHMM.fit as called at hmmlearn_hmm.py:103-104
 * (hmmlearn _hmmc.cpp forward_log, backward_log, compute_log_xi_sum; base.py
 * _compute_posteriors_log; hmm.py _accumulate_sufficient_statistics) for a whole batch.
 *
 * Utterances are presented in TILES of 256 slots that share one word model:
 *   slot_utt[n_tiles*256]  utterance index of each slot, -1 = empty
 *   tile_model[n_tiles]    word model of each tile; tiles sorted by model, and
 *   model_tile_off[W+1]    first tile of each model (prefix offsets).
 * Features are consumed as the C-contiguous (T,D) concatenation hmmlearn_hmm.py:80-81 builds
 * (pair-wise numpy summation order inside the log-density).
 *
 *   sapr_forward_diag  loglik[n_utts]: log P(utterance | its tile's model)
 *   sapr_estep_diag    loglik[n_utts] and stats[W][width], width from sapr_stats_width():
 *                      {n_sequences, sum log-prob, start[S], trans[S][S], post[S], obs[S][D], obs2[S][D]}
 *                      = hmmlearn's stats dict {nobs, -, start, trans, post, obs, obs**2}, reduced
 *                      over each model's utterances in a fixed order (deterministic, no atomics).
 *                      Across GPUs the caller all-reduces `stats` (sum) before the M-step.
 *                      The first call on a batch copies the features into slot-major order inside the
 *                      workspace; later calls on the same batch and workspace may pass
 *                      fast_div | SAPR_ESTEP_STAGED to skip that copy.
 * Non-finite features follow numpy's IEEE arithmetic in all entry points of this family, with and without fast_div:
 * a NaN feature makes its utterance's loglik NaN, an infinite one makes it -inf (every log-density of the frame is
 * -inf); the other utterances of the batch keep their bits, the word's summed log-prob and statistics do not.
 * ---------------------------------------------------------------------------------- */
int sapr_fb_workspace_bytes(int64_t n_utts, int64_t n_tiles, int32_t S, int32_t D, int32_t max_T,
                            size_t *bytes);
int sapr_stats_width(int32_t S, int32_t D, int32_t *width);
int sapr_forward_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                      const int32_t *tile_model, int64_t n_tiles, int32_t D, const void *pack,
                      int32_t W, int32_t S, int32_t topology, int32_t fast_div, double *loglik,
                      void *stream);
int sapr_estep_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                    const int32_t *tile_model, const int32_t *model_tile_off, int64_t n_utts,
                    int64_t n_tiles, int32_t D, int32_t max_T, const void *pack, int32_t W, int32_t S,
                    int32_t topology, int32_t fast_div, void *workspace, size_t workspace_bytes,
                    double *loglik, double *stats, void *stream);

/* Forward scoring over the vocabulary: GaussianHMM.score (hmmlearn_hmm.py:104; hmmlearn _hmmc.cpp forward_log)
 * extended over the model loop of decoder.py:42 — every utterance under EVERY word model in one launch, where
 * sapr_forward_diag scores an utterance under the one model of its tile.  No tile layout and no workspace: `order`
 * (optional, may be NULL) is the length-sorted permutation of the Viterbi entry points.  Only the exact-kernel
 * operands of the pack are read (SAPR_PACK_EXACT_ONLY packs work).
 *   loglik[n_utts][W]     log P(utterance | word model w); -inf for an utterance without frames
 *   best_word[n_utts]     optional: first strict maximum of the row in model order, starting from -inf
 *                         (decoder.py:42-47's rule on forward scores); -1 when no score beats -inf.  A NaN score
 *                         is never a strict maximum: an utterance with a non-finite feature, whose scores are NaN
 *                         (a NaN feature) or -inf (an infinite one) under every model, gets -1
 *   word_post[n_utts][W]  optional: exp(loglik - logsumexp_w loglik), the posterior over the words under a uniform
 *                         prior; NaN where the row's maximum is -inf or a score is NaN (nothing is repaired)
 * Log-densities are evaluated in the E-step's quick form ((x - mean)^2 * RN(1/var) accumulated by FMA): scores agree
 * with the float64 CPU evaluation to ~1e-13 relative, not bit for bit.  n_utts == 0 returns 0 at once.  max_T (the
 * longest utterance, as in the Viterbi entry points) is checked to be >= 0 and sizes nothing: there is no workspace. */
int sapr_forward_vocab(const float *feats, const int64_t *offsets, const int32_t *order /* may be NULL */,
                       int64_t n_utts, int32_t D, int32_t max_T, const void *pack, int32_t W, int32_t S,
                       int32_t topology, double *loglik /* [n_utts][W] */,
                       int32_t *best_word /* [n_utts], may be NULL */,
                       double *word_post /* [n_utts][W], may be NULL */, void *stream);

/* State posteriors and MAP decoding: GaussianHMM.score_samples / predict_proba / decode(algorithm="map") (hmmlearn
 * base.py _compute_posteriors_log, _decode_map; _hmmc.cpp forward_log / backward_log) for a whole batch, every
 * utterance under the ONE model of its tile — the tile layout of sapr_forward_diag (slot_utt, tile_model).  Only the
 * exact-kernel operands of the pack are read (SAPR_PACK_EXACT_ONLY packs work).
 *   loglik[n_utts]                     forward log-likelihood; -inf for an utterance without frames (no rows)
 *   post[total_frames][n_out_states]   optional: gamma_t(s) = softmax_s(fwd + bwd), frame-major and ragged along
 *                                      `offsets` — hmmlearn's (n_samples, n_components) layout.  n_out_states <= S
 *                                      cuts the padded states of a model that runs at a larger kernel state count off
 *                                      in the store
 *   path[total_frames]                 optional: argmax_s post[t] over the first n_out_states states; equal values:
 *                                      the lowest state; a row holding NaN: the index of its first NaN (np.argmax)
 * post or path may be NULL, not both; with post == NULL no posterior reaches memory in the caller's layout (4 bytes of
 * output per frame).  Two launches over a slot-major workspace of sapr_state_posteriors_workspace_bytes():
 *   bidiagonal  (max(max_T, 1) + 1) * S * n_tiles * 256 * 8   (stay shares of the forward pass + its last row)
 *   dense        2 * max(max_T, 1)  * S * n_tiles * 256 * 8   (forward lattice + log-densities)
 * max_T must not be smaller than the longest utterance.  Log-densities are evaluated in the E-step's quick form:
 * results agree with the float64 CPU evaluation to ~1e-13 relative, not bit for bit; every utterance is a function of
 * its own (features, model) pair.  Bad sizes, a bad topology, n_out_states outside 1..S, a NULL loglik, both outputs
 * NULL and a workspace that is too small return SAPR_ERR_ARG before anything is launched; n_tiles == 0 returns 0
 * after the size checks without touching any pointer; D > 39 or S > 18 return SAPR_ERR_UNSUPPORTED. */
int sapr_state_posteriors_workspace_bytes(int64_t n_tiles, int32_t S, int32_t max_T, int32_t topology, size_t *bytes);
int sapr_state_posteriors_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                               const int32_t *tile_model, int64_t n_tiles, int32_t D, int32_t max_T,
                               const void *pack, int32_t W, int32_t S, int32_t topology, int32_t n_out_states,
                               void *workspace, size_t workspace_bytes, double *loglik,
                               double *post /* may be NULL */, int32_t *path /* may be NULL */, void *stream);

/* One Lloyd step of k-means for G independent problems ("groups": the frames of one word model each) and R centre
 * sets per group ("restarts") side by side — the k-means of hmmlearn's GaussianHMM._init (sklearn KMeans, n_init=10)
 * batched over the vocabulary.  A frame is loaded once and scored against all R centre sets of its group.  The layout
 * is tiles of 1..256 consecutive frames of ONE group, sorted by group (kmeans.py FrameTiles builds it from the group
 * lengths): tile_begin[n_tiles] (first frame), tile_len[n_tiles], tile_group[n_tiles], group_tile_off[G+1].
 *   stats[G][R][K][2*D+1]       {count, sum_x[D], sqdev[D]} per cluster: the frames whose label is k, their column
 *                               sums and sum (x_d - c_kd)^2 — new centre = sum_x / count, inertia = sum of sqdev over
 *                               k and d.  A cluster or a group without frames gets exact zeros
 *   labels[R][total_frames]     optional: argmin_k sum_d (x_d - c_kd)^2, float64, the difference squared directly
 *                               (never the |x|^2 - 2x.c + |c|^2 expansion: c0 sits near -300 and it cancels); equal
 *                               distances: the lowest k; a frame holding NaN: label 0 (np.argmin) and its NaN flows
 *                               into the sums — nothing is repaired
 * D in {13, 39} (narrower features run zero-padded: zero columns against zero centre columns add +0.0), K in 1..32,
 * R >= 1; other D and K > 32 return SAPR_ERR_UNSUPPORTED.  Two launches: per-tile partial statistics into a workspace
 * of sapr_kmeans_workspace_bytes() = n_tiles * R * K * (2*D+1) * 8, then one sum per group in tile order.  No
 * floating-point atomics: results are bit-identical run to run, and a group's results do not depend on which other
 * groups share the launch.  Tiles whose table entries point outside the batch are served as empty.  Bad sizes, NULL
 * required pointers and a workspace that is too small return SAPR_ERR_ARG before anything is launched; n_tiles == 0
 * zero-fills stats (one memset on the stream; nothing at all when G == 0) and returns 0 without touching any other
 * pointer. */
int sapr_kmeans_workspace_bytes(int64_t n_tiles, int32_t R, int32_t K, int32_t D, size_t *bytes);
int sapr_kmeans_step(const float *feats /* [total_frames][D] */, int64_t total_frames, const int64_t *tile_begin,
                     const int32_t *tile_len /* 1..256 */, const int32_t *tile_group,
                     const int32_t *group_tile_off /* [G+1] */, int64_t n_tiles, int32_t G, int32_t R, int32_t K,
                     int32_t D, const double *centres /* [G][R][K][D] */, void *workspace, size_t workspace_bytes,
                     double *stats /* [G][R][K][2*D+1] */, int32_t *labels /* [R][total_frames], may be NULL */,
                     void *stream);

/* Gaussian-mixture HMMs (hmmlearn's GMMHMM, diagonal covariances): S states, M components per state, D features.
 *   lc[t,s,m] = log w[s,m] - (D log 2 pi + sum_d log var[s,m,d] + sum_d (x[t,d] - mu[s,m,d])^2 / var[s,m,d]) / 2
 *   logb[t,s] = logsumexp_m lc[t,s,m]   (log 0 = -inf flows through: a zero weight switches a component off)
 * and over logb the log-domain recursions of _hmmc.cpp forward_log / backward_log / viterbi with any pattern of zeros
 * in the transition matrix (a -inf log transition is skipped), gamma_t(s) = softmax_s(fwd + bwd) and the
 * responsibilities r[t,s,m] = gamma_t(s) exp(lc[t,s,m] - logb[t,s]).  CPU restatement: tests/_gmmhmm_ref.py.
 *
 * Layout: the tile layout of sapr_estep_diag (256 slots per tile, one model per tile: slot_utt, tile_model,
 * model_tile_off).  S in 1..18, M in 1..8, D in 1..39 are run-time values; the kernels are instantiated for the padded
 * shapes SP in {4, 10, 18}, MP in {1, 2, 4, 8}, DP in {13, 26, 39} that sapr_gmm_pack_layout returns, and the W
 * models' parameters arrive in that padded form, `pack` = W blocks of doubles_per_model float64 values each:
 *   log_start[SP]             log startprob; -inf for a padded state
 *   log_trans[SP][SP]         log transmat;  -inf in the rows and columns of padded states
 *   log_transT[SP][SP]        its transpose
 *   cc[SP][MP]                log w - (D log 2 pi + sum_d log var) / 2; -inf for a padded component or state
 *   prm[SP][DP][MP][2]        {mean, -1 / (2 var)}; {0, 0} for padded states, components and dimensions
 * (gmm_hmm.py pack_models builds it).  feats[total_frames][D] keeps its own row stride D.
 *
 * sapr_gmm_estep_diag — one E-step:
 *   loglik[n_utts]            forward log-likelihood; -inf for an utterance without frames
 *   stats[W][width]           optional; width = sapr_gmm_stats_width = 2 + S + S*S + S + S*M + 2*S*M*D, per model and
 *                             summed over its utterances: n_seq, sum loglik, start[S] = sum gamma_0, trans[S][S] = sum_t
 *                             xi_t, post[S] = sum gamma, post_mix[S][M] = sum r, obs[S][M][D] = sum r x,
 *                             obs2[S][M][D] = sum r x^2 with x^2 rounded to float32 first (as numpy squares a float32
 *                             feature array).  An utterance without frames contributes nothing (n_seq included).
 *                             model_tile_off is read only when stats is given
 *   post[total_frames][S]     optional: gamma, hmmlearn's (n_samples, n_components) layout, ragged along offsets
 *   path[total_frames]        optional: argmax_s gamma_t(s); equal values: the lowest state; a row holding NaN: the
 *                             index of its first NaN (np.argmax)
 * sapr_gmm_viterbi_diag — logprob[n_utts] (-inf without frames) and path[total_frames], hmmlearn's viterbi: the first
 *   maximum of the last row, then argmax_i (lattice[t][i] + log a[i][next]), ties to the first maximum.
 *
 * Launches: frame-parallel emission (logb into the workspace), one lane per utterance for the recursions, frame-
 * parallel accumulation of post_mix / obs / obs2 into four partial rows per tile, then fixed-order reductions (the 256
 * slots of a tile, then the model's tiles in order).  No floating-point atomics: results are bit-identical run to run,
 * a model's statistics do not depend on which other models share the launch, and loglik / post / path of an utterance
 * are a function of its own (features, model) pair.  Non-finite values propagate; nothing is repaired.  Workspace:
 * sapr_gmm_workspace_bytes() = 8 * (2 * max(total_frames, 1) * SP + (2 + S + S*S + S) * 257 * max(n_tiles, 1)
 * + 4 * max(n_tiles, 1) * S*M*(2*D+1)), the same for both entry points.  max_T must not be smaller than the longest
 * utterance (an utterance that is longer, or whose offsets leave the batch, is served as empty) and is at most 65535.
 * Bad sizes, NULL required pointers and a workspace that is too small return SAPR_ERR_ARG before anything is launched;
 * S > 18, M > 8 or D > 39 return SAPR_ERR_UNSUPPORTED (from the size functions too); n_tiles == 0 returns 0 after
 * these checks without touching any pointer. */
int sapr_gmm_stats_width(int32_t S, int32_t M, int32_t D, int32_t *width);
int sapr_gmm_pack_layout(int32_t S, int32_t M, int32_t D, int32_t *SP, int32_t *MP, int32_t *DP,
                         size_t *doubles_per_model);
int sapr_gmm_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t M, int32_t D, size_t *bytes);
int sapr_gmm_estep_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                        const int32_t *tile_model, const int32_t *model_tile_off /* [W+1]; may be NULL without stats */,
                        int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T,
                        const double *pack, int32_t W, int32_t S, int32_t M, void *workspace, size_t workspace_bytes,
                        double *loglik, double *stats /* may be NULL */, double *post /* may be NULL */,
                        int32_t *path /* may be NULL */, void *stream);
int sapr_gmm_viterbi_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                          const int32_t *tile_model, int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D,
                          int32_t max_T, const double *pack, int32_t W, int32_t S, int32_t M, void *workspace,
                          size_t workspace_bytes, double *logprob, int32_t *path, void *stream);

/* Full covariances (hmmlearn's GaussianHMM, covariance_type "full"; a "tied" model is packed as S copies of its one
 * matrix): S states, D features, one Gaussian per state,
 *   logb[t,s] = c_s - 1/2 sum_i (sum_{j<=i} Winv_s[i][j] (x[t,j] - mu_s[j]))^2
 * with Sigma_s = L_s L_s^T, Winv_s = L_s^-1 (lower triangular, computed by the host: nothing is factorised on the
 * device) and c_s = -(D log 2 pi + log|Sigma_s|) / 2.  Over logb run the recursions, posteriors, decoders, xi sums and
 * reductions of the mixture entry points above, unchanged; the tile layout, the arguments, the rules on ties, empty
 * utterances, non-finite values and determinism are theirs.  CPU restatement: tests/_fullcov_ref.py.
 *
 * `pack` = W blocks of doubles_per_model float64 values (sapr_full_pack_layout; SP in {4, 10, 18}, DP in {13, 26, 39}):
 *   log_start[SP], log_trans[SP][SP], log_transT[SP][SP]     as in the mixture pack, at the same offsets
 *   c[SP]                     -inf for a padded state
 *   mu[SP][DP]                0 for padded states and dimensions
 *   Winv[SP][DP][DP]          row-major, 0 above the diagonal and for padded states and dimensions
 * (full_cov.py pack_models builds it).
 *
 * sapr_full_estep — loglik[n_utts], optional post / path as sapr_gmm_estep_diag gives them, and optional
 *   stats[W][width]           width = sapr_full_stats_width = 2 + S + S*S + S + S*D + S*D*D: n_seq, sum loglik, start[S],
 *                             trans[S][S], post[S], obs[S][D] = sum_t gamma_t(s) x_t, oo[S][D][D] = sum_t gamma_t(s) x_t
 *                             x_t^T with x promoted to float64 before the product.  Every oo[s] is exactly symmetric (the
 *                             tiles on or above the diagonal are computed on the float64 matrix cores and written to both
 *                             halves).
 * sapr_full_viterbi — logprob[n_utts] and path[total_frames] as sapr_gmm_viterbi_diag gives them.
 *
 * Workspace: sapr_full_workspace_bytes() = 8 * (2 * max(total_frames, 1) * SP + (2 + S + S*S + S) * 257 * max(n_tiles, 1)
 * + 4 * max(n_tiles, 1) * S*D*(D+1)), the same for both entry points: the four partial rows of obs / oo cost
 * 4 * S*D*(D+1) * 8 bytes per tile, about 0.9 MB at (S, D) = (18, 39).  Bad sizes, NULL required pointers and a
 * workspace that is too small return SAPR_ERR_ARG before anything is launched; S > 18 or D > 39 return
 * SAPR_ERR_UNSUPPORTED (from the size functions too); n_tiles == 0 returns 0 after these checks. */
int sapr_full_pack_layout(int32_t S, int32_t D, int32_t *SP, int32_t *DP, size_t *doubles_per_model);
int sapr_full_stats_width(int32_t S, int32_t D, int32_t *width);
int sapr_full_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t D, size_t *bytes);
int sapr_full_estep(const float *feats, const int64_t *offsets, const int32_t *slot_utt, const int32_t *tile_model,
                    const int32_t *model_tile_off /* [W+1]; may be NULL without stats */, int64_t n_utts,
                    int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, const double *pack, int32_t W,
                    int32_t S, void *workspace, size_t workspace_bytes, double *loglik, double *stats /* may be NULL */,
                    double *post /* may be NULL */, int32_t *path /* may be NULL */, void *stream);
int sapr_full_viterbi(const float *feats, const int64_t *offsets, const int32_t *slot_utt, const int32_t *tile_model,
                      int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T,
                      const double *pack, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                      double *logprob, int32_t *path, void *stream);

/* Scoring over the vocabulary for the Gaussian-mixture HMMs: every utterance under EVERY word model in one launch,
 * where the two entry points above evaluate an utterance under the one model of its tile — what sapr_forward_vocab is
 * to sapr_forward_diag.  `pack` is the operand block of sapr_gmm_pack_layout (W models, nothing new is packed); `order`
 * (optional, may be NULL) is the length-sorted permutation of sapr_forward_vocab.  No tile layout and no workspace: the
 * recursion's state lives in registers, no lattice and no logb reach memory.
 *   score[n_utts][W]      SAPR_GMM_VOCAB_FORWARD: the forward log-likelihood of utterance u under model w — the bits
 *                         sapr_gmm_estep_diag returns as loglik for that pair; SAPR_GMM_VOCAB_VITERBI: the viterbi
 *                         log-probability — the bits of sapr_gmm_viterbi_diag's logprob.  -inf for an utterance without
 *                         frames, for one longer than max_T and for one whose offsets leave the batch (served as empty)
 *   best_word[n_utts]     optional: first strict maximum of the row in model order, starting from -inf
 *                         (decoder.py:42-47's rule); -1 when no score beats -inf
 *   word_post[n_utts][W]  optional, forward mode only: exp(score - logsumexp_w score), the posterior over the words
 *                         under a uniform prior; NaN where the row's maximum is -inf or a score is NaN
 * Non-finite values propagate; nothing is repaired.  Every score is a function of its (utterance, model) pair alone:
 * equal models give equal bits, and the launch is deterministic whatever `order` is.  Bad sizes, NULL required
 * pointers, an unknown mode and a word_post in Viterbi mode (a soft-max of path scores is no posterior) return
 * SAPR_ERR_ARG, S > 18, M > 8 or D > 39 SAPR_ERR_UNSUPPORTED, both before anything is launched and before any HIP
 * call; n_utts == 0 returns 0 after these checks without touching any pointer. */
#define SAPR_GMM_VOCAB_FORWARD 0
#define SAPR_GMM_VOCAB_VITERBI 1
int sapr_gmm_vocab_diag(const float *feats, const int64_t *offsets, const int32_t *order /* may be NULL */,
                        int64_t n_utts, int64_t total_frames, int32_t D, int32_t max_T, const double *pack, int32_t W,
                        int32_t S, int32_t M, int32_t mode, double *score /* [n_utts][W] */,
                        int32_t *best_word /* [n_utts], may be NULL */,
                        double *word_post /* [n_utts][W], may be NULL; FORWARD only */, void *stream);

/* Scoring over the vocabulary for the full-covariance HMMs: every utterance under EVERY word model in one launch —
 * what sapr_gmm_vocab_diag is to the mixtures.  `pack` is the operand block of sapr_full_pack_layout as it is (W
 * models, nothing new is packed); `order` (optional, may be NULL) is the length-sorted permutation of
 * sapr_forward_vocab.  score, best_word, word_post, the rules on empty and unserved utterances, on an `order` entry
 * outside the batch (never followed), on non-finite values and on determinism are sapr_gmm_vocab_diag's, word for word:
 *   score[n_utts][W]      SAPR_FULL_VOCAB_FORWARD: the bits sapr_full_estep returns as loglik with every utterance
 *                         assigned to model w; SAPR_FULL_VOCAB_VITERBI: the bits of sapr_full_viterbi's logprob (first
 *                         maximum of the last row).  -inf for an utterance without frames, for one longer than max_T and
 *                         for one whose offsets leave the batch
 *   best_word[n_utts]     optional: first strict maximum of the row in model order, starting from -inf; -1 if none
 *   word_post[n_utts][W]  optional, forward mode only: exp(score - logsumexp_w score)
 * The emission of a state is evaluated where the recursion consumes it, by the device function full_emit_kernel calls
 * (fullcov_emit.h); the recursion's state lives in registers, no lattice and no logb reach memory.
 *
 * Workspace: sapr_full_vocab_workspace_bytes() is 0 today — every instantiation takes the fused path and `workspace`
 * may be NULL.  The pair is part of the ABI so that a staged path (a frame-parallel emission into a
 * logb[frames of a slice of utterances][W][SP] block, bounded independently of n_utts) can be added without changing
 * it; callers size and pass the workspace as for the other entry points.
 *
 * Bad sizes, NULL required pointers, an unknown mode, a word_post in Viterbi mode and a workspace that is too small
 * return SAPR_ERR_ARG, S > 18 or D > 39 SAPR_ERR_UNSUPPORTED (from the size function too), all before any HIP call;
 * n_utts == 0 returns 0 after these checks without touching any pointer. */
#define SAPR_FULL_VOCAB_FORWARD 0
#define SAPR_FULL_VOCAB_VITERBI 1
int sapr_full_vocab_workspace_bytes(int64_t n_utts, int64_t total_frames, int32_t W, int32_t S, int32_t D,
                                    size_t *bytes);
int sapr_full_vocab(const float *feats, const int64_t *offsets, const int32_t *order /* may be NULL */,
                    int64_t n_utts, int64_t total_frames, int32_t D, int32_t max_T, const double *pack, int32_t W,
                    int32_t S, int32_t mode, void *workspace, size_t workspace_bytes,
                    double *score /* [n_utts][W] */, int32_t *best_word /* [n_utts], may be NULL */,
                    double *word_post /* [n_utts][W], may be NULL; FORWARD only */, void *stream);

/* ------------------------------------------------------------------------------------
 * Connected-word recognition (csrc/connected.hip): one-pass Viterbi over the word loop — the end of any word may be
 * followed by the start of any word — for a recording that holds several words in a row.  The definition is the CPU
 * restatement tests/_connected_ref.py (plain numpy, float64); with b_t(w,s) = logb[t][w * SP + s]:
 *     delta_0(w,j) = log_start[w][j] + b_0(w,j)
 *     E_{t-1}      = max over (w,s) in flat order of (delta_{t-1}(w,s) + log_exit[w][s])
 *     within       = max_i (delta_{t-1}(w,i) + log_trans[w][i][j])            i ascending, the first maximum
 *     entry        = (E_{t-1} + word_penalty) + log_start[w][j]
 *     delta_t(w,j) = max(within, entry) + b_t(w,j)                            entry only where strictly greater
 *     score        = max over (w,s) of (delta_{T-1}(w,s) + log_exit[w][s])    lowest flat index w * SP + s on ties
 * The additions are made in the order written, so the recursion is float64 adds and compares only and its outputs are
 * bit for bit numpy's.  log_exit[w][s] = -inf: a word may not end in state s.
 *
 * Layout: sapr_connected_layout returns the padded shape — SP in {4, 10, 18} states per word, DP in {13, 26, 39}
 * features, R = W * SP flat states (R <= 256: the flat states lie along the lanes of one wavefront, up to 4 per lane).
 * Any of the three outputs may be NULL.
 *
 * Stage 1, sapr_connected_emit_diag: logb[total_frames][R] float64 for diagonal Gaussians, frame-parallel,
 *     logb = -0.5 * (gconst + sum_d ((x_d - mean_d) * (x_d - mean_d)) * (1 / var_d)),  d ascending.
 *   feats  [total_frames][D] float32
 *   ops    [R][1 + 2 DP] float64, the operand block the host builds from the arrays sapr_diag_pack takes
 *          (means[W][S][D], vars, gconst): per flat state {gconst, mean[DP], 1 / var[DP]}.  Padding features carry
 *          mean 0 and coefficient 0 (they add +0.0); a padding state carries gconst = +inf, mean 0, coefficient 0
 *          and comes out as -inf.  (sapr_amd/connected.py emit_operands builds it.)
 * Stage 1 has two more variants, which read a family's own operand block in place (nothing is repacked) and write the
 * same logb[total_frames][R], frame-parallel over a (frame block, word) grid:
 *   sapr_connected_emit_gmm   Gaussian mixtures.  pack [W][doubles per model] as sapr_gmm_pack_layout(S, M, D)
 *          describes it (the block sapr_gmm_vocab_diag takes); read: cc[SP][MP] and prm[SP][DP][MP][2].
 *              logb[t][w * SP + s] = logsumexp_m (cc[s][m] + sum_d (x_d - mean_dm)^2 * (-1 / (2 var_dm)))
 *   sapr_connected_emit_full  full covariances ("full", "tied").  pack [W][doubles per model] as
 *          sapr_full_pack_layout(S, D) describes it (the block sapr_full_vocab takes); read: c[SP], mu[SP][DP],
 *          Winv[SP][DP][DP].
 *              logb[t][w * SP + s] = c[s] - 1/2 |Winv_s (x - mu_s)|^2
 *   Both call the device functions of the per-model emission kernels (sapr_gmm_estep_diag / sapr_full_estep) in the
 *   same order: the values carry the same bits.  A state whose constants are all -inf (the padding states of a pack)
 *   comes out as -inf.  S is the vocabulary's kernel state count (the pack's), M its component count.
 * Stage 2, sapr_connected_viterbi: the recursion over a logb it is given (any emission family may supply one).
 *   logb       [total_frames][R] float64; offsets[n_utts + 1] as everywhere (frames of utterance u:
 *              offsets[u] .. offsets[u + 1]); offsets that leave the batch are served as an empty utterance
 *   log_start  [W][S], log_trans [W][S][S], log_exit [W][S] float64 (the models' own S: the kernel pads to SP with
 *              -inf); word_penalty is added once per word boundary
 *   workspace  sapr_connected_workspace_bytes: back-pointers, one byte per (frame, flat state), rounded up to 16,
 *              then one int32 per frame (the flat arg-max of E_t).  logb is the caller's buffer.
 *   score      [n_utts]; -inf for an utterance without frames
 *   n_words    [n_utts], may be NULL: words on the best path; 0 where the score is not finite
 *   path_word, path_state [total_frames] int32, path_entry [total_frames] uint8, each may be NULL: per frame the
 *              word, its state, and 1 where a word begins (frame 0 and wherever `entry` won; the same word may follow
 *              itself).  Where the score is not finite: -1, -1, 0.
 * No atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of its own frames
 * and the network alone.  Non-finite values propagate, nothing is repaired.
 *
 * Bad sizes, NULL required pointers and a workspace that is too small return SAPR_ERR_ARG, S > 18, D > 39, M > 8 or
 * W * SP > 256 SAPR_ERR_UNSUPPORTED (from the layout and size functions too), all before any launch; n_utts == 0
 * (total_frames == 0 for the emissions) returns 0 after these checks. */
int sapr_connected_layout(int32_t W, int32_t S, int32_t D, int32_t *SP, int32_t *DP, int32_t *R);
int sapr_connected_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S, size_t *bytes);
int sapr_connected_emit_diag(const float *feats, int64_t total_frames, int32_t D, const double *ops, int32_t W,
                             int32_t S, double *logb /* [total_frames][R] */, void *stream);
int sapr_connected_emit_gmm(const float *feats, int64_t total_frames, int32_t D, const double *pack, int32_t W,
                            int32_t S, int32_t M, double *logb /* [total_frames][R] */, void *stream);
int sapr_connected_emit_full(const float *feats, int64_t total_frames, int32_t D, const double *pack, int32_t W,
                             int32_t S, double *logb /* [total_frames][R] */, void *stream);
int sapr_connected_viterbi(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                           const double *log_start, const double *log_trans, const double *log_exit,
                           double word_penalty, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                           double *score, int32_t *n_words /* may be NULL */, int32_t *path_word /* may be NULL */,
                           int32_t *path_state /* may be NULL */, uint8_t *path_entry /* may be NULL */,
                           void *stream);

/* ------------------------------------------------------------------------------------
 * Connected-word recognition under a word-pair language model (csrc/connected_bigram.hip): the word loop in which the
 * step from word v to word w costs lm[v][w] (the same word may follow itself), the first word lm_start[w] and the last
 * word lm_end[v].  The definition is the CPU restatement tests/_bigram_ref.py; with b_t(w,s) = logb[t][w * SP + s]:
 *     delta_0(w,j)  = (lm_start[w] + log_start[w][j]) + b_0(w,j)
 *     X_{t-1}(v)    = max_s (delta_{t-1}(v,s) + log_exit[v][s])        s ascending, the first maximum
 *     N_{t-1}(w)    = max_v (X_{t-1}(v) + lm[v][w])                    v ascending, the first maximum
 *     within        = max_i (delta_{t-1}(w,i) + log_trans[w][i][j])    i ascending, the first maximum
 *     entry         = N_{t-1}(w) + log_start[w][j]
 *     delta_t(w,j)  = max(within, entry) + b_t(w,j)                    entry only where strictly greater
 *     score         = max_v (X_{T-1}(v) + lm_end[v])                   v ascending, the first maximum
 * The additions are made in the order written: float64 adds and compares only, bit for bit numpy's.  -inf in lm,
 * lm_start or lm_end forbids a pair, a first word or a last word — a finite-state word-pair grammar is a table of 0.0
 * and -inf.  There is no separate word_penalty: the caller folds it into lm (sapr_amd/connected.py
 * WordBigram.scaled).  Two identities follow: with lm == p, lm_start == 0 and lm_end == 0 the score is
 * sapr_connected_viterbi's with word_penalty = p bit for bit (every output with p = 0.0); with lm = -inf except
 * lm[w_k][w_{k+1}] = p along a transcript of distinct words, lm_start = -inf except 0.0 at w_0 and lm_end = -inf except
 * 0.0 at w_{K-1}, every output is sapr_connected_align's with word_penalty = p.
 *   logb, offsets, log_start, log_trans, log_exit, W, S: as for sapr_connected_viterbi (same layout, same limits)
 *   lm         [W][W] float64, lm_start [W], lm_end [W]
 *   workspace  sapr_connected_bigram_workspace_bytes:
 *                  a16(total_frames * R) + 2 * a16(total_frames * W) + a16(4 * n_utts)   bytes, a16 rounding up to 16:
 *              back-pointers, one byte per (frame, flat state) — the predecessor state, or 255 for an entry; one byte
 *              per (frame, word), the state that attained X_t(v); one byte per (frame, word), the predecessor word
 *              that attained N_t(w); one int32 per utterance, the final word
 *   score, n_words, path_word, path_state, path_entry: as for sapr_connected_viterbi (each but score may be NULL)
 * No atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of its own frames
 * and the network alone.  Non-finite values propagate; every index of the walk is clamped into its row.
 *
 * Bad sizes, NULL required pointers (lm, lm_start and lm_end among them) and a workspace that is too small return
 * SAPR_ERR_ARG, S > 18 or W * SP > 256 SAPR_ERR_UNSUPPORTED (from the size function too), all before any launch;
 * n_utts == 0 returns 0 after these checks. */
int sapr_connected_bigram_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S, size_t *bytes);
int sapr_connected_bigram(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                          const double *log_start, const double *log_trans, const double *log_exit,
                          const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                          const double *lm_end /* [W] */, int32_t W, int32_t S, void *workspace,
                          size_t workspace_bytes, double *score, int32_t *n_words /* may be NULL */,
                          int32_t *path_word /* may be NULL */, int32_t *path_state /* may be NULL */,
                          uint8_t *path_entry /* may be NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Connected-word recognition with a known or bounded number of words (csrc/connected_levels.hip): level building over
 * the word loop of sapr_connected_bigram.  A path carries, next to (word, state), its level l = 0 .. L - 1 — level l
 * holds the paths that are in their (l + 1)-th word — and one pass returns the best string of exactly k words for
 * every k = 1 .. L.  The definition is the CPU restatement tests/_levels_ref.py; with b_t(w,s) = logb[t][w * SP + s]:
 *     delta_0(0,w,j) = (lm_start[w] + log_start[w][j]) + b_0(w,j)          delta_0(l>0,.,.) = -inf
 *     X_t(l,v)       = max_s (delta_t(l,v,s) + log_exit[v][s])             s ascending, the first maximum
 *     N_t(l,w)       = max_v (X_t(l-1,v) + lm[v][w])   for l >= 1          v ascending, the first maximum;  N_t(0,w) = -inf
 *     within         = max_i (delta_{t-1}(l,w,i) + log_trans[w][i][j])     i ascending, the first maximum
 *     entry          = N_{t-1}(l,w) + log_start[w][j]
 *     delta_t(l,w,j) = max(within, entry) + b_t(w,j)                       entry only where strictly greater
 *     level_score[k-1] = max_v (X_{T-1}(k-1,v) + lm_end[v])   k = 1..L     v ascending, the first maximum
 * float64 adds and compares only, in the order written, b_t last: bit for bit numpy's.  An utterance without frames
 * scores -inf on every level.  Three identities follow from the monotone rounding of add and max: where
 * sapr_connected_bigram on the same logb and tables decodes n <= L words, level_score[n-1] is its score bit for bit and
 * no level scores higher; with L = 1, level_score[0] is sapr_connected_bigram's score with every pair forbidden; with
 * the chain language model of a transcript of K distinct words (see sapr_connected_bigram), level_score[K-1] and its
 * path are sapr_connected_align's outputs and every other level is -inf.
 *
 * The work is split in two so that one recursion serves any number of back-traces over the workspace it left.
 * sapr_connected_levels runs the recursion and writes level_score.  sapr_connected_levels_backtrace selects a count per
 * utterance and walks back: from k = lo it takes a later k <= hi only where level_score[k-1] is strictly greater (on a
 * tie the fewest words win), starts in level k - 1 from the word that attained level_score[k-1] in the state that
 * attained its X, and where entry won at frame t steps to level l - 1, to the word that attained N_{t-1}(l,.) in the
 * state that attained that word's X_{t-1}(l-1,.).
 *   logb, offsets, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S: as for sapr_connected_bigram (same
 *              layout, same limits)
 *   L          the largest number of words, 1 .. 8
 *   workspace  sapr_connected_levels_workspace_bytes:
 *                  a16(total_frames * L * R) + 2 * a16(total_frames * L * W) + a16(4 * n_utts * L)   bytes, a16 rounding
 *              up to 16: per (frame, level) one back-pointer byte per flat state — the predecessor state, or 255 for an
 *              entry —, one byte per word for the state that attained X_t(l,v) and one for the predecessor word that
 *              attained N_t(l,w); one int32 per (utterance, level), the final word.  The back-trace takes the workspace
 *              the recursion wrote, with the same sizes.
 *   level_score [n_utts][L]: written by the recursion, read by the back-trace
 *   count_lo, count_hi  [n_utts] int32, each may be NULL (1 and L): the range of counts per utterance.  lo > hi selects
 *              nothing (score -inf, no path); otherwise both are clamped into 1 .. L.
 *   score      [n_utts]: the selected level's score.  n_words, path_word, path_state, path_entry: as for
 *              sapr_connected_viterbi (each may be NULL); where the selected score is not finite the path rows are -1,
 *              the entry flags 0 and n_words 0, otherwise n_words is the selected k.
 * No atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of its own frames
 * and the tables alone.  Non-finite values propagate; every index of the walk is clamped into its row.
 *
 * Bad sizes, NULL required pointers (lm, lm_start and lm_end among them) and a workspace that is too small return
 * SAPR_ERR_ARG, S > 18, W * SP > 256 or L outside 1 .. 8 SAPR_ERR_UNSUPPORTED (from the size function too), all before
 * any launch; n_utts == 0 returns 0 after these checks. */
int sapr_connected_levels_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S, int32_t L,
                                          size_t *bytes);
int sapr_connected_levels(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                          const double *log_start, const double *log_trans, const double *log_exit,
                          const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                          const double *lm_end /* [W] */, int32_t W, int32_t S, int32_t L, void *workspace,
                          size_t workspace_bytes, double *level_score /* [n_utts][L] */, void *stream);
int sapr_connected_levels_backtrace(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t S,
                                    int32_t L, void *workspace, size_t workspace_bytes,
                                    const double *level_score /* [n_utts][L] */,
                                    const int32_t *count_lo /* may be NULL */, const int32_t *count_hi /* may be NULL */,
                                    double *score, int32_t *n_words /* may be NULL */,
                                    int32_t *path_word /* may be NULL */, int32_t *path_state /* may be NULL */,
                                    uint8_t *path_entry /* may be NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Connected-word N-best (csrc/connected_nbest.hip): the n_best <= 8 best DISTINCT word strings of every utterance with
 * their Viterbi scores, in one recursion over the word loop of sapr_connected_bigram, without a back-pointer workspace.
 * The definition is the CPU restatement tests/_nbest_ref.py.  A hypothesis is a pair (score: float64, code: uint64);
 * code is the word string so far, the current word included: the string w_0 .. w_{k-1} has
 * code = sum (w_i + 1) * B^(k-1-i) with B = W + 1, appending w is code * B + (w + 1), and cap(W) is the largest K with
 * B^K <= 2^64 (sapr_connected_nbest_capacity: 17 at W = 11, 10 at W = 64, 40 at W = 2).  merge_n(cands) is a function
 * of the candidates' values alone: 1. drop every candidate whose score is not > -inf (this drops -inf and NaN);
 * 2. among candidates with equal code keep the largest score; 3. order by score descending, then code ascending;
 * 4. keep the first n = n_best.  With b_t(w,j) = logb[t][w * SP + j], every + applying to each hypothesis's score and
 * leaving its code alone unless said otherwise:
 *     cell_0(w,j) = merge_n{ ((lm_start[w] + log_start[w][j]), w + 1) }                      then + b_0(w,j)
 *     X_t(v)      = merge_n{ h + log_exit[v][s]        : s, h in cell_t(v,s) }
 *     N_t(w)      = merge_n{ (h + lm[v][w], code * B + (w+1)) : v, h in X_t(v), code < B^(cap-1) }     t < T-1
 *     cell_t(w,j) = merge_n( { h + log_trans[w][i][j] : i, h in cell_{t-1}(w,i) }
 *                            U { h + log_start[w][j]  : h in N_{t-1}(w) } )                  then + b_t(w,j)
 *     result      = merge_n{ h + lm_end[v]             : v, h in X_{T-1}(v) }
 * A cell is the set AFTER b_t was added, with no re-sort and no drop; the next merge drops what became -inf.  overflow
 * is 1 iff some candidate of an N_t had h + lm[v][w] > -inf and code >= B^(cap-1): that string would not fit and the
 * candidate was dropped.  T = 0 gives an empty list.  Every addition is made in sapr_connected_bigram's order,
 * ((delta + log_exit) + lm) + log_start, then + b, and adding a constant is monotone under rounding: rank 1 has
 * sapr_connected_bigram's score bit for bit, and where no two of the top n_best + 1 string scores are equal and
 * overflow is 0 the list is exactly the n_best best strings, each with the score of its own best path.
 *   logb, offsets, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S: as for sapr_connected_bigram (same
 *              layout, same limits)
 *   n_best     1 .. 8
 *   score      [n_utts][n_best]: best first, -inf padded
 *   code       [n_utts][n_best]: the strings, 0 padded
 *   n_found    [n_utts] int32, may be NULL: the strings found
 *   overflow   [n_utts] uint8, may be NULL
 * No workspace and no atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of
 * its own frames and the tables alone; a NaN in logb drops hypotheses of its own utterance only.  Word boundaries of a
 * returned string come from sapr_connected_align.
 *
 * Bad sizes and NULL required pointers (lm, lm_start, lm_end, score and code among them) return SAPR_ERR_ARG, S > 18,
 * W * SP > 256 or n_best outside 1 .. 8 SAPR_ERR_UNSUPPORTED, all before any launch; n_utts == 0 returns 0 after the
 * size, shape and language-model checks. */
int sapr_connected_nbest(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                         const double *log_start, const double *log_trans, const double *log_exit,
                         const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                         const double *lm_end /* [W] */, int32_t W, int32_t S, int32_t n_best /* 1..8 */,
                         double *score /* [n_utts][n_best], -inf padded */,
                         uint64_t *code /* [n_utts][n_best], 0 padded */, int32_t *n_found /* may be NULL */,
                         uint8_t *overflow /* may be NULL */, void *stream);
int sapr_connected_nbest_capacity(int32_t W, int32_t *max_words); /* cap(W) */

/* ------------------------------------------------------------------------------------
 * Connected-word lattices (csrc/connected_lattice.hip): one pass over the word loop of sapr_connected_bigram leaves,
 * for every (frame, word), the score of the best path that ends the word there and the frame at which that path
 * entered the word.  That table is a word lattice: it is pruned to a beam around the best path and rescored under any
 * other word-pair language model without emission or recursion.  The definition is the CPU restatement
 * tests/_lattice_ref.py; with delta, X_t(w) and N_t(w) as for sapr_connected_bigram:
 *     wend_score[t][w] = X_t(w)        wend_entry[t][w] = N_t(w)
 *     wend_start[t][w] = B_t(w)        the utterance-relative frame at which the path that attains X_t(w) entered w:
 *         b_0(w,j) = 0;  b_t(w,j) = t where entry won, else b_{t-1}(w,i*), i* the within-word predecessor that won;
 *         B_t(w) = b_t(w, xarg_t(w)), and -1 where X_t(w) is not greater than -inf
 * A record is a pair (w, t) with X_t(w) > -inf and tau = B_t(w) inside 0 .. t; in = lm_start[w] if tau = 0, else
 * N_{tau-1}(w); ac = X_t(w) - in.  The record may follow any word that ends at tau - 1; tau = 0 starts the utterance.
 * The backward pass under any tables (lm', lm_start', lm_end') — the forward pass's own give pruning margins, others
 * rescore —: beta_{T-1}(w) = lm_end'[w], every other beta -inf, next = (-1, 255), root = -inf, first = (-1, 255);
 * records are visited with t' from T - 1 down to 0 and, inside a frame, w' ascending:
 *     g = ac + beta_{t'}(w')
 *     tau > 0:  for every v: c = lm'[v][w'] + g;  where c > beta_{tau-1}(v): beta_{tau-1}(v) = c, next_{tau-1}(v) = (t', w')
 *     tau = 0:               c = lm_start'[w'] + g; where c > root: root = c, first = (t', w')
 * float64 adds, one subtract and strict compares in the order written: bit for bit numpy's.  The walk goes from first
 * along next until a record ends at T - 1; next_end is clamped into (t, T - 1] and next_word below W.
 *   logb, offsets, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S: as for sapr_connected_bigram (same
 *              layout, same limits)
 *   workspace  sapr_connected_lattice_workspace_bytes:  2 * a16(8 * total_frames * W) + a16(4 * total_frames * W)  bytes,
 *              a16 rounding up to 16: the forward tables wend_score and wend_entry [total_frames][W] float64 and
 *              wend_start [total_frames][W] int32, in this order.  The forward pass writes them, the backward pass reads
 *              them; 20 W bytes per frame and no per-state back-pointer.
 *   score      [n_utts]: sapr_connected_bigram's score bit for bit.  final_word [n_utts] int32, may be NULL
 *   forward_lm_start  [W]: the lm_start the forward pass ran under (it defines `in` of a record with tau = 0)
 *   beta       [total_frames][W] float64, next_end [total_frames][W] int32, next_word [total_frames][W] uint8
 *   root       [n_utts] float64: the best complete lattice path under the tables of the backward pass
 *   first      [n_utts][2] int32: (end frame, word) of that path's first record, (-1, 255) without one
 *   n_words, path_word, path_entry: as for sapr_connected_viterbi (each may be NULL); where root is not finite the path
 *              rows are -1, the entry flags 0 and n_words 0
 * No atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of its own frames
 * and the tables alone.  Non-finite values propagate; a NaN never wins a compare, and every index of the walk is
 * clamped into its row.
 *
 * Bad sizes, NULL required pointers (the language-model tables among them) and a workspace that is too small return
 * SAPR_ERR_ARG, S > 18 or W * SP > 256 SAPR_ERR_UNSUPPORTED (from the size function too), all before any launch;
 * n_utts == 0 returns 0 after these checks. */
int sapr_connected_lattice_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S, size_t *bytes);
int sapr_connected_lattice(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                           const double *log_start, const double *log_trans, const double *log_exit,
                           const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                           const double *lm_end /* [W] */, int32_t W, int32_t S, void *workspace,
                           size_t workspace_bytes, double *score, int32_t *final_word /* may be NULL */, void *stream);
int sapr_connected_lattice_backward(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t S,
                                    const void *workspace, size_t workspace_bytes,
                                    const double *forward_lm_start /* [W] */, const double *lm /* [W][W] */,
                                    const double *lm_start /* [W] */, const double *lm_end /* [W] */, double *beta,
                                    int32_t *next_end, uint8_t *next_word, double *root, int32_t *first /* [n_utts][2] */,
                                    void *stream);
int sapr_connected_lattice_walk(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t S,
                                const int32_t *next_end, const uint8_t *next_word, const double *root,
                                const int32_t *first, int32_t *n_words /* may be NULL */,
                                int32_t *path_word /* may be NULL */, uint8_t *path_entry /* may be NULL */,
                                void *stream);

/* ------------------------------------------------------------------------------------
 * Lattice posteriors (csrc/connected_lattice.hip): forward-backward in the sum semiring over the records of a word
 * lattice — link posteriors, word confidences and the likelihood of the lattice under any tables (lm', lm_start',
 * lm_end') and any acoustic scale, without emission or recursion over states.  The definition is the CPU restatement
 * tests/_lattice_post_ref.py over the records, tau, in and ac of tests/_lattice_ref.py.  With a = acoustic_scale * ac,
 * lse the log-sum-exp (the maximum taken out, the exponentials added in ascending order) and alpha, Q, beta, H = -inf:
 *     forward, t ascending:    for every record (w, t): alpha_t(w) = a + (lm_start'[w] if tau = 0 else Q_{tau-1}(w));
 *                              then Q_t(w) = lse_v (alpha_t(v) + lm'[v][w])
 *     backward, t descending:  beta_t(v) = lse_w (lm'[v][w] + H_{t+1}(w)), H_T = -inf; beta_{T-1}(v) = lm_end'[v];
 *                              then for every record (w, t): H_tau(w) = logaddexp(H_tau(w), a + beta_t(w))
 *     loglik[u]         = lse_w (alpha_{T-1}(w) + lm_end'[w]);  -inf for an utterance without frames
 *     record_post[t][w] = exp(alpha_t(w) + beta_t(w) - loglik) for a record, 0 elsewhere
 *     word_post[f][w]   = the sum of record_post[t][w] over the records of w with tau <= f <= t: the posterior that
 *                         frame f lies inside word w.  It is formed as the mass that started at or before f,
 *                         sum over tau <= f of exp(Q_{tau-1}(w) + H_tau(w) - loglik), minus the mass that ended before f
 * A loglik that is not finite gives exact zeros in both tables of that utterance.
 *   lattice_workspace  what sapr_connected_lattice wrote (sapr_connected_lattice_workspace_bytes), read only
 *   forward_lm_start   [W]: the lm_start the lattice was made under (it defines ac)
 *   keep       [total_frames][W] uint8, may be NULL (every record): a record with keep == 0 does not exist for this pass
 *   workspace  sapr_connected_lattice_posteriors_workspace_bytes:  4 * a16(8 * total_frames * W)  bytes: alpha, Q, beta
 *              and H [total_frames][W] float64, in this order (Q_{T-1} is not formed); 32 W bytes per frame
 *   loglik [n_utts], record_post [total_frames][W], word_post [total_frames][W] (may be NULL): float64
 * No atomics, a fixed order of every sum: outputs are bit-identical from run to run, and an utterance's outputs are a
 * function of its own frames, the tables, acoustic_scale and keep alone.
 *
 * Bad sizes, NULL required pointers (the four tables among them), a workspace that is too small and an acoustic_scale
 * that is not finite or not above 0 return SAPR_ERR_ARG, S > 18 or W * SP > 256 SAPR_ERR_UNSUPPORTED (from the size
 * function too), all before any launch; n_utts == 0 returns 0 after these checks. */
int sapr_connected_lattice_posteriors_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                      size_t *bytes);
int sapr_connected_lattice_posteriors(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t S,
                                      const void *lattice_workspace, size_t lattice_workspace_bytes,
                                      const double *forward_lm_start /* [W] */, const double *lm /* [W][W] */,
                                      const double *lm_start /* [W] */, const double *lm_end /* [W] */,
                                      double acoustic_scale, const uint8_t *keep /* may be NULL: every record */,
                                      void *workspace, size_t workspace_bytes, double *loglik /* [n_utts] */,
                                      double *record_post, double *word_post /* may be NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Online connected-word decoding (csrc/connected_online.hip): the recursion of sapr_connected_bigram over recordings
 * that are still arriving.  A session holds n_streams streams over one network; a chunk of frames per stream is
 * consumed by sapr_connected_online_step, and sapr_connected_online_commit hands out the part of the best path that
 * can no longer change (partial traceback).  The definition is the CPU restatement tests/_online_ref.py.  Fixed for a
 * session: window, the back-pointer rows a stream keeps, and max_chunk, the most frames one step consumes,
 * 1 <= max_chunk < window.
 *   state      sapr_connected_online_state_bytes: n_streams blocks of
 *                  64 + a16(8 * (R + 2 W)) + a16(window * R) + 2 * a16(window * W)   bytes, a16 rounding up to 16:
 *              a header (frames consumed, committed, forced, ...), delta[R], X[W] and N[W] float64, and the rows of
 *              sapr_connected_bigram's workspace for the frames t mod window.  Opaque device memory; ALL ZERO is a
 *              session of fresh streams.
 * Step: stream u consumes the frames offsets[u] .. offsets[u+1] of logb — sapr_connected_bigram's recursion continued
 * from the stream's delta and N; the stream's absolute frame 0 takes the lm_start branch.  After the step delta, X, N
 * and the stored rows are bit for bit what the offline recursion has at those frames.  A chunk longer than max_chunk
 * (or than the ring has free, if commit was not called after the step before) has only its first frames consumed and
 * truncated[u] = 1.
 *   logb, offsets, tables, lm, lm_start, lm_end, W, S: as for sapr_connected_bigram (n_streams in the place of n_utts)
 *   reset      [n_streams] uint8, may be NULL: != 0 makes the stream fresh before its chunk
 *   truncated  [n_streams] uint8, may be NULL
 * Commit, with t = frames - 1, c = committed and live = the flat states with finite delta_t: stable is the largest
 * frame tau in [c, t] at which the stored back-traces from every live state hold the same state.  If there is one, rows
 * c .. tau of that back-trace are final and c = tau + 1.  If then frames - c > window - max_chunk, the oldest
 * k = frames - c - (window - max_chunk) pending frames are committed by force along the back-trace from the first
 * maximum of delta_t over the live states in flat order (-1 / -1 / 0 where nothing is live) and forced += k: the next
 * chunk always fits the ring.  A forced commit gives up the continuity of the path across that boundary, never the
 * score.  With flush[u] != 0 the stream is flushed instead: score = max_v (X(v) + lm_end[v]) (-inf without frames); a
 * finite score commits every pending row along the walk from the word that attains it, a score that is not finite
 * commits nothing more and n_words = 0 (rows handed out earlier stand); the stream is then fresh.
 *   flush        [n_streams] uint8, may be NULL (no stream is flushed)
 *   n_new        [n_streams] int32: rows handed out by this call;  first_frame [n_streams] int64: the absolute frame
 *                of the first of them
 *   out_word, out_state [n_streams][window] int32, out_entry [n_streams][window] uint8: row i is frame first_frame + i
 *   score        [n_streams] float64, n_words [n_streams] int32: written where flush[u] != 0 (n_words counts every
 *                entry flag handed out for the recording); required with flush
 *   forced       [n_streams] int64: frames of the recording committed by force so far
 *   hyp_len      [n_streams] int32, hyp_word, hyp_state [n_streams][window] int32, hyp_entry uint8, each may be NULL:
 *                the rows a flush would write now over the frames still pending (0 where the score is not finite)
 * With forced == 0 and a finite score the rows handed out over a recording, n_words and score are
 * sapr_connected_bigram's bit for bit, whatever the chunking.  No atomics; a stream's outputs are a function of its own
 * frames, its own state and the network alone.  Every index read from the ring is clamped into its row.
 *
 * Bad sizes (window < 2, max_chunk outside 1 .. window - 1), NULL required pointers and a state that is too small
 * return SAPR_ERR_ARG, S > 18 or W * SP > 256 SAPR_ERR_UNSUPPORTED (from the size function too), all before any
 * launch; n_streams == 0 returns 0 after these checks. */
int sapr_connected_online_state_bytes(int64_t n_streams, int32_t W, int32_t S, int32_t window, size_t *bytes);
int sapr_connected_online_step(const double *logb, const int64_t *offsets, int64_t n_streams, int64_t total_frames,
                               const double *log_start, const double *log_trans, const double *log_exit,
                               const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                               const double *lm_end /* [W] */, int32_t W, int32_t S, int32_t window, int32_t max_chunk,
                               void *state, size_t state_bytes, const uint8_t *reset /* may be NULL */,
                               uint8_t *truncated /* may be NULL */, void *stream);
int sapr_connected_online_commit(int64_t n_streams, int32_t W, int32_t S, int32_t window, int32_t max_chunk,
                                 void *state, size_t state_bytes, const uint8_t *flush /* may be NULL */,
                                 int32_t *n_new, int64_t *first_frame, int32_t *out_word, int32_t *out_state,
                                 uint8_t *out_entry, double *score, int32_t *n_words, int64_t *forced,
                                 int32_t *hyp_len /* may be NULL */, int32_t *hyp_word /* may be NULL */,
                                 int32_t *hyp_state /* may be NULL */, uint8_t *hyp_entry /* may be NULL */,
                                 void *stream);

/* ------------------------------------------------------------------------------------
 * Connected-word confidence (csrc/connected_loop_fb.hip): forward-backward over the word loop under the word-pair
 * language model of sapr_connected_bigram — the sum over every word string the grammar allows where that function
 * takes the maximum.  The definition is the CPU restatement tests/_loop_fb_ref.py; with b_t(w,s) = logb[t][w * SP + s]
 * and lse the log-sum-exp:
 *     alpha_0(w,j)  = (lm_start[w] + log_start[w][j]) + b_0(w,j)
 *     X_t(v)        = lse_s (alpha_t(v,s) + log_exit[v][s])
 *     N_t(w)        = lse_v (X_t(v) + lm[v][w])
 *     alpha_t(w,j)  = lse( lse_i (alpha_{t-1}(w,i) + log_trans[w][i][j]),  N_{t-1}(w) + log_start[w][j] ) + b_t(w,j)
 *     loglik        = lse_v (X_{T-1}(v) + lm_end[v])
 *
 *     beta_{T-1}(v,s) = log_exit[v][s] + lm_end[v]
 *     E_t(w)        = lse_j (log_start[w][j] + b_t(w,j) + beta_t(w,j))
 *     F_t(v)        = lse_w (lm[v][w] + E_t(w))
 *     beta_t(v,i)   = lse( lse_j (log_trans[v][i][j] + b_{t+1}(v,j) + beta_{t+1}(v,j)),  log_exit[v][i] + F_{t+1}(v) )
 *
 *     post_t(w,s)    = exp(alpha_t(w,s) + beta_t(w,s) - loglik)
 *     word_post_t(w) = sum_s post_t(w,s)                       s ascending
 *     entry_post_0(w) = word_post_0(w)
 *     entry_post_t(w) = exp(N_{t-1}(w) + E_t(w) - loglik)      t >= 1: "a word w begins at frame t"
 * A step inside a word and a step that leaves the word and enters the same word again (lm[w][w]) are different paths;
 * both count.  loglik - (the score of sapr_connected_bigram on the same logb) is >= 0 and its negative is the log
 * posterior of the decoded path.  Two identities follow: the chain language model of a transcript of distinct words
 * (see sapr_connected_bigram) gives sapr_connected_embed's loglik and gamma; every pair forbidden, lm_start = lm_end
 * = 0 and log_exit = 0 give the log-sum over the words of the isolated-word forward likelihoods and their softmax.
 *   logb, offsets, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S: as for sapr_connected_bigram (same
 *              layout, same limits)
 *   workspace  sapr_connected_posteriors_workspace_bytes:
 *                  a16(8 * total_frames * R) + a16(8 * total_frames * W)   bytes, a16 rounding up to 16:
 *              alpha_t and N_t in float64, 8 (R + W) bytes per frame
 *   loglik     [n_utts]: -inf for an utterance without frames or without a path; NaN where a NaN was met anywhere in
 *              the utterance's frames or in the tables
 *   word_post  [total_frames][W], entry_post [total_frames][W], post [total_frames][R], each may be NULL; with all
 *              three NULL only the forward pass is launched.  An utterance whose loglik is not finite gets exact zeros
 *              in its rows (the rule of sapr_connected_embed); a padded state gets 0.0 in post; frames that belong to
 *              no utterance are not written.
 * No atomics and a fixed order in every sum: outputs are bit-identical from run to run, and an utterance's outputs are
 * a function of its own frames and the network alone.
 *
 * Bad sizes, NULL required pointers (lm, lm_start and lm_end among them) and a workspace that is too small return
 * SAPR_ERR_ARG, S > 18 or W * SP > 256 SAPR_ERR_UNSUPPORTED (from the size function too), all before any launch;
 * n_utts == 0 returns 0 after these checks. */
int sapr_connected_posteriors_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                              size_t *bytes);
int sapr_connected_posteriors(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                              const double *log_start, const double *log_trans, const double *log_exit,
                              const double *lm /* [W][W] */, const double *lm_start /* [W] */,
                              const double *lm_end /* [W] */, int32_t W, int32_t S, void *workspace,
                              size_t workspace_bytes, double *loglik /* [n_utts] */,
                              double *word_post /* [total_frames][W] or NULL */,
                              double *entry_post /* [total_frames][W] or NULL */,
                              double *post /* [total_frames][R] or NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Denominator statistics of discriminative (MMI) training (csrc/connected_loop_stats.hip): the state posteriors
 * post[total_frames][R = W * SP] of sapr_connected_posteriors reduced to per-word sufficient statistics.  The
 * definition is the CPU restatement tests/_mmi_ref.py (den_stats); with r = w * SP + s, s < S, x_t the float32 frame
 * and the sums over the frames t of the utterances u with utt_keep[u] != 0 (all of them where utt_keep is NULL):
 *     post[w][s] = sum post_t(r)      obs[w][s] = sum post_t(r) x_t      obs2[w][s] = sum post_t(r) RN32(x_t x_t)
 * in float64 (x_t x_t is the float32 square, widened: sapr_connected_embed's rule).  This is the product
 * post^T [x | x^2 | 1], R rows by 2 D + 1 columns, on the float64 matrix cores.
 *   stats      [W][sapr_connected_embed_stats_width(S, D)], the row of sapr_connected_embed:
 *              {nobs, 0.0, start[S], trans[S][S], post[S], obs[S][D], obs2[S][D]}.  nobs = the number of kept
 *              utterances with at least one frame, the same in every row; the reserved slot, start and trans are exact
 *              zeros (transitions are not trained discriminatively); padded states have no place in a row
 *   offsets    [n_utts + 1]; a range that leaves the batch is served as empty.  A frame outside every kept utterance's
 *              range is never read, neither its row of post nor its features
 *   workspace  sapr_connected_loop_stats_workspace_bytes:  a16(8 * parts * R * (2 D + 1))  bytes with
 *              span = max(256, ceil(ceil(total_frames / 1024) / 128) * 128) frames, parts = ceil(total_frames / span):
 *              one partial row per span of frames, added span ascending
 * No atomics and a fixed order in every sum: the bytes are the same from run to run.
 *
 * Bad sizes (D < 1 among them), NULL required pointers and a workspace that is too small return SAPR_ERR_ARG, S > 18,
 * W * SP > 256 or D > 39 SAPR_ERR_UNSUPPORTED (from the size function too), all before any launch; n_utts == 0 writes
 * a zero stats and returns 0 after these checks. */
int sapr_connected_loop_stats_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S, int32_t D,
                                              size_t *bytes);
int sapr_connected_loop_stats(const double *post /* [total_frames][W*SP] */, const float *feats /* [total_frames][D] */,
                              int32_t D, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                              const uint8_t *utt_keep /* [n_utts] or NULL = all */, int32_t W, int32_t S,
                              void *workspace, size_t workspace_bytes, double *stats /* [W][width] */, void *stream);

/* ------------------------------------------------------------------------------------
 * Forced alignment (csrc/connected_align.hip): Viterbi over the left-to-right chain of the K words an utterance is
 * known to hold — where does each word begin and end, and which state explains each frame.  Word slot k is entered
 * only from the exit of slot k - 1 and the score is read only at the exit of the last slot.  The definition is the CPU
 * restatement tests/_align_ref.py; with the transcript w_0 .. w_{K-1} and b_t(k,s) = logb[t][w_k * SP + s]:
 *     delta_0(0,j)   = log_start[w_0][j] + b_0(0,j)          delta_0(k>0,j) = -inf
 *     X_{t-1}(k)     = max_s (delta_{t-1}(k,s) + log_exit[w_k][s])            s ascending, the first maximum
 *     within         = max_i (delta_{t-1}(k,i) + log_trans[w_k][i][j])        i ascending, the first maximum
 *     entry (k >= 1) = (X_{t-1}(k-1) + word_penalty) + log_start[w_k][j]      (k = 0: -inf)
 *     delta_t(k,j)   = max(within, entry) + b_t(k,j)                          entry only where strictly greater
 *     score          = X_{T-1}(K-1)
 * The additions are made in the order written (the word loop's order): float64 adds and compares only, bit for bit
 * numpy's, and aligning to the string sapr_connected_viterbi decoded gives that call's score bit for bit.
 *   logb          [total_frames][R = W * SP], what the three sapr_connected_emit_* entry points write
 *   offsets       [n_utts + 1] frames, word_offsets [n_utts + 1] transcript positions; a range that leaves its array is
 *                 served as empty
 *   words         [total_words] vocabulary indices, the transcripts one after the other (a word may follow itself)
 *   max_words     the longest transcript the call is sized for: max_words * SP <= 256 chain positions lie along the
 *                 lanes of one wavefront
 *   log_start, log_trans, log_exit, word_penalty: as for sapr_connected_viterbi
 *   workspace     sapr_connected_align_workspace_bytes: back-pointers, one byte per (frame, chain position) in rows of
 *                 max_words * SP, rounded up to 16, then one byte per (frame, word slot) — the state that attained X —
 *                 in rows of max_words, rounded up to 16
 *   score         [n_utts]
 *   path_word (vocabulary indices), path_state [total_frames] int32, path_entry [total_frames] uint8 (1 at frame 0 and
 *                 wherever a word begins), word_start [total_words] int32 (the frame, counted from the utterance's
 *                 start, at which transcript word k begins): each may be NULL
 * An utterance without a path — no frames, no words, more than max_words words, a word index outside 0 .. W - 1, a
 * score that is not finite — scores -inf (or the NaN that propagated); its path rows are -1, its entry flags 0, its
 * word_start -1.  No atomics: outputs are bit-identical from run to run, and an utterance's outputs are a function of
 * its own frames, its own transcript and the network.  Non-finite values propagate; every index of the walk is clamped
 * into its row.
 *
 * Bad sizes, NULL required pointers and a workspace that is too small return SAPR_ERR_ARG, S > 18, W * SP > 256 or
 * max_words * SP > 256 SAPR_ERR_UNSUPPORTED (from the size function too), all before any launch; n_utts == 0 returns 0
 * after these checks. */
int sapr_connected_align_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t max_words, int32_t S,
                                         size_t *bytes);
int sapr_connected_align(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                         const int32_t *words /* [total_words] */, const int64_t *word_offsets /* [n_utts + 1] */,
                         int64_t total_words, int32_t max_words, const double *log_start, const double *log_trans,
                         const double *log_exit, double word_penalty, int32_t W, int32_t S, void *workspace,
                         size_t workspace_bytes, double *score, int32_t *path_word /* may be NULL */,
                         int32_t *path_state /* may be NULL */, uint8_t *path_entry /* may be NULL */,
                         int32_t *word_start /* [total_words], may be NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Embedded Baum-Welch (csrc/connected_embed.hip): forward-backward over the same chain of an utterance's transcript
 * words, and its posteriors reduced to per-word sufficient statistics — training from recordings of several words
 * without cutting them.  The definition is the CPU restatement tests/_embedded_ref.py; with lse the log-sum-exp:
 *     alpha_0(0,j)  = log_start[w_0][j] + b_0(0,j)             alpha_0(k>0,j) = -inf
 *     X_{t-1}(k)    = lse_s (alpha_{t-1}(k,s) + log_exit[w_k][s])
 *     alpha_t(k,j)  = lse( lse_i (alpha_{t-1}(k,i) + log_trans[w_k][i][j]),
 *                          (X_{t-1}(k-1) + word_penalty) + log_start[w_k][j] ) + b_t(k,j)   (k = 0: no entry term)
 *     loglik        = X_{T-1}(K-1)
 *     beta_{T-1}(K-1,s) = log_exit[w_{K-1}][s]                 beta_{T-1}(k<K-1,s) = -inf
 *     E_t(k)        = word_penalty + lse_j (log_start[w_k][j] + b_t(k,j) + beta_t(k,j))     (k >= 1)
 *     beta_t(k,i)   = lse( lse_j (log_trans[w_k][i][j] + b_{t+1}(k,j) + beta_{t+1}(k,j)),
 *                          log_exit[w_k][i] + E_{t+1}(k+1) )                                (k = K-1: no exit term)
 *     gamma_t(k,s)  = exp(alpha_t(k,s) + beta_t(k,s) - loglik)
 * Statistics are kept per word model w and sum over every slot k with w_k = w of every utterance whose loglik is
 * finite: post = sum_t gamma, obs = sum_t gamma x_t, obs2 = sum_t gamma x_t^2 (float64 sums; x_t^2 is the float32
 * square, as in sapr_estep_diag), trans[i][j] = sum_{t>=1}
 * exp(alpha_{t-1}(k,i) + log_trans + b_t(k,j) + beta_t(k,j) - loglik), start[j] = gamma_0(0,j) for slot 0 plus, for
 * k >= 1, sum_{t>=1} exp((X_{t-1}(k-1) + word_penalty) + log_start[w_k][j] + b_t(k,j) + beta_t(k,j) - loglik),
 * nobs = the number of such slots.
 *   logb, offsets, words, word_offsets, max_words, log_start, log_trans, log_exit, word_penalty, W, S: as for
 *                 sapr_connected_align
 *   feats         [total_frames][D] float32, the frames logb was evaluated on; NULL iff D == 0 (the obs blocks then
 *                 have width 0).  D <= 39
 *   workspace     sapr_connected_embed_workspace_bytes: alpha [total_frames][max_words * SP] and X
 *                 [total_frames][max_words] float64, one partial statistics row per transcript word
 *                 (SP * (2 + SP + 2 D) float64), one byte per transcript word, and per 256 transcript words 256 / SP
 *                 statistics rows (the first level of the fold), each block rounded up to 16
 *   loglik        [n_utts]
 *   stats         [W][width], width = sapr_connected_embed_stats_width(S, D) = 2 + S + S*S + S + 2*S*D:
 *                 {nobs, reserved 0.0, start[S], trans[S][S], post[S], obs[S][D], obs2[S][D]} per word model; or NULL
 *   post          [total_frames][max_words * SP]: gamma_t at chain position k * SP + s, 0 behind the utterance's own
 *                 K * SP positions; or NULL.  Frames that belong to no utterance are not written
 * An utterance without a path — no frames, no words, more words than frames or than max_words, a word index outside
 * 0 .. W - 1, a likelihood that is not finite (-inf, or NaN wherever a NaN was met) — contributes exact zeros to every
 * statistic and its posterior rows are 0: one bad recording does not poison a word's statistics (sapr_estep_diag
 * propagates instead).  No atomics: the per-slot sums are folded in slot order, outputs are bit-identical from run to
 * run.  The argument checks, limits and error codes are those of sapr_connected_align, with D > 39 unsupported. */
int sapr_connected_embed_stats_width(int32_t S, int32_t D, int32_t *width);
int sapr_connected_embed_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                         int32_t max_words, int32_t S, int32_t D, size_t *bytes);
int sapr_connected_embed(const double *logb, const float *feats /* [total_frames][D]; NULL iff D == 0 */, int32_t D,
                         const int64_t *offsets, int64_t n_utts, int64_t total_frames, const int32_t *words,
                         const int64_t *word_offsets, int64_t total_words, int32_t max_words,
                         const double *log_start, const double *log_trans, const double *log_exit,
                         double word_penalty, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                         double *loglik /* [n_utts] */, double *stats /* [W][width] or NULL */,
                         double *post /* [total_frames][max_words*SP] or NULL */, void *stream);

/* The same E-step with second-moment matrices, for word models with "full" or "tied" covariances (definition:
 * tests/_embedded_full_ref.py): in place of obs2 the row carries, with x_t the float32 frame widened to float64,
 *     oo[w][s] = sum over the utterances with a finite loglik, the slots k with w_k = w and t of
 *                gamma_t(k,s) x_t x_t^T        (float64 products, as sapr_full_estep)
 * The arguments are those of sapr_connected_embed, in its order; loglik and post are exactly its results, and so is
 * the head of a statistics row, byte for byte (the recursions and their two-level fold are the same launches).
 *   workspace     sapr_connected_embed_full_workspace_bytes: what sapr_connected_embed takes at D = 0, W heads of
 *                 2 + S + S*S + S float64, and one partial row of S*D + S*D*D float64 per (utterance group, word);
 *                 the number of groups is a function of n_utts only (8 utterances each, at most 96 groups, beyond
 *                 which the groups grow), each block rounded up to 16
 *   stats         [W][width], width = sapr_connected_embed_full_stats_width(S, D) = 2 + S + S*S + S + S*D + S*D*D
 *                 (== sapr_full_stats_width): {nobs, reserved 0.0, start[S], trans[S][S], post[S], obs[S][D],
 *                 oo[S][D][D]} per word model, the row of sapr_full_estep; or NULL.  stats != NULL needs D >= 1 and
 *                 feats.  Every oo[w][s] is exactly symmetric (both halves are written from the upper one)
 * The gamma of the slots of one word are added (k ascending) into one weight per frame and state, and sum g x x^T runs
 * as weighted Gram products on the float64 matrix cores, utterances ascending inside a group; the groups' partial rows
 * are added in ascending order.  No atomics: outputs are bit-identical from run to run.  An utterance without a path
 * contributes exact zeros — its posterior rows in the workspace are never read.  Argument checks, limits and error
 * codes are those of sapr_connected_embed. */
int sapr_connected_embed_full_stats_width(int32_t S, int32_t D, int32_t *width);
int sapr_connected_embed_full_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                              int32_t max_words, int32_t W, int32_t S, int32_t D, size_t *bytes);
int sapr_connected_embed_full(const double *logb, const float *feats /* [total_frames][D] */, int32_t D,
                              const int64_t *offsets, int64_t n_utts, int64_t total_frames, const int32_t *words,
                              const int64_t *word_offsets, int64_t total_words, int32_t max_words,
                              const double *log_start, const double *log_trans, const double *log_exit,
                              double word_penalty, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                              double *loglik /* [n_utts] */, double *stats /* [W][width] or NULL */,
                              double *post /* [total_frames][max_words*SP] or NULL */, void *stream);

/* The same E-step with mixture responsibilities, for Gaussian-mixture word models (GMMHMM; definition:
 * tests/_embedded_gmm_ref.py).  With x_t the float32 frame widened to float64, lc[t][w][s][m] the component log-terms
 * of word w (the formula of sapr_gmm_estep_diag) and g_t(w,s) = sum over the slots k with w_k = w of gamma_t(k,s),
 *     r_t(w,s,m)        = g_t(w,s) exp(lc - max_m lc) / sum_m exp(lc - max_m lc)   (0 where every component is off)
 *     post_mix[w][s][m] = sum r     obs[w][s][m] = sum r x_t     obs2[w][s][m] = sum r f64(RN32(x_t x_t))
 * over the utterances with a finite loglik and all their frames.  pack is the [W][sapr_gmm_pack_layout(S, M, D)] block
 * sapr_connected_emit_gmm read, in place; the other arguments are those of sapr_connected_embed, in its order; loglik
 * and post are exactly its results, and so is the head of a statistics row, byte for byte.
 *   workspace     sapr_connected_embed_gmm_workspace_bytes: what sapr_connected_embed takes at D = 0, W heads of
 *                 2 + S + S*S + S float64, and one partial row of S*M*(2 D + 1) float64 per (utterance group, word),
 *                 the groups being those of sapr_connected_embed_full; each block rounded up to 16
 *   stats         [W][width], width = sapr_connected_embed_gmm_stats_width(S, M, D) (== sapr_gmm_stats_width):
 *                 {nobs, reserved 0.0, start[S], trans[S][S], post[S], post_mix[S][M], obs[S][M][D], obs2[S][M][D]}
 *                 per word model, the row of sapr_gmm_estep_diag; or NULL.  stats != NULL needs D >= 1, feats and pack
 * The sums r^T [x, x^2, 1] run on the float64 matrix cores, utterances ascending inside a group; the groups' partial
 * rows are added in ascending order.  No atomics: outputs are bit-identical from run to run.  An utterance without a
 * path contributes exact zeros — its posterior rows in the workspace are never read.  Argument checks, limits and error
 * codes are those of sapr_connected_embed, with M > 8 unsupported. */
int sapr_connected_embed_gmm_stats_width(int32_t S, int32_t M, int32_t D, int32_t *width);
int sapr_connected_embed_gmm_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                             int32_t max_words, int32_t W, int32_t S, int32_t M, int32_t D,
                                             size_t *bytes);
int sapr_connected_embed_gmm(const double *logb, const float *feats /* [total_frames][D] */, int32_t D,
                             const double *pack /* [W][sapr_gmm_pack_layout(S, M, D)] */, int32_t M,
                             const int64_t *offsets, int64_t n_utts, int64_t total_frames, const int32_t *words,
                             const int64_t *word_offsets, int64_t total_words, int32_t max_words,
                             const double *log_start, const double *log_trans, const double *log_exit,
                             double word_penalty, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                             double *loglik /* [n_utts] */, double *stats /* [W][width] or NULL */,
                             double *post /* [total_frames][max_words*SP] or NULL */, void *stream);

/* ------------------------------------------------------------------------------------
 * Optional transcript slots in the two chain units: `optional` [total_words] uint8, laid out like words,
 * marks slots the path may walk through or step over — `sil? w1 sil? w2 ... wK sil?` is silence nobody wrote down.  No
 * two neighbouring slots are optional and at least one slot is mandatory, so a slot has at most two predecessor slots;
 * far(k) holds for k >= 2 with opt_{k-1} = 1: slot k may be entered from slot k - 2.  The definition is the CPU
 * restatement tests/_optional_ref.py.  Alignment, in the notation of sapr_connected_align:
 *     delta_0(0,j) = log_start[w_0][j] + b_0(0,j)
 *     delta_0(1,j) = log_start[w_1][j] + b_0(1,j)   where opt_0 = 1 and K > 1;   every other slot -inf
 *     enter(k)     = X_{t-1}(k-1);  where far(k) and X_{t-1}(k-2) is STRICTLY greater: X_{t-1}(k-2), a "skip entry"
 *     entry        = (enter(k) + word_penalty) + log_start[w_k][j]        (k = 0: -inf)
 *     delta_t(k,j) = max(within, entry) + b_t(k,j)                        entry only where strictly greater
 *     score        = X_{T-1}(K-1);  where opt_{K-1} = 1, K >= 2 and X_{T-1}(K-2) is STRICTLY greater: X_{T-1}(K-2), and
 *                    the path ends in slot K-2
 * The nearer slot wins every tie; word_penalty is paid for every slot entered, optional or not, and never for a slot
 * stepped over; the back-trace steps two slots back over a skip entry and word_start[k] = -1 for a slot the path
 * stepped over.  Forward-backward is the same chain with lse in place of max, in the notation of sapr_connected_embed:
 *     alpha_0                  the two start slots above
 *     alpha_t(k,j) entry term  (lse(X_{t-1}(k-1), X_{t-1}(k-2) where far(k)) + word_penalty) + log_start[w_k][j]
 *     loglik                   lse(X_{T-1}(K-1), X_{T-1}(K-2) where opt_{K-1} = 1 and K >= 2)
 *     beta_{T-1}(k,s)          log_exit for k = K-1, and for k = K-2 where opt_{K-1} = 1;   else -inf
 *     beta_t(k,i) exit term    log_exit[w_k][i] + lse(E_{t+1}(k+1), E_{t+1}(k+2) where far(k+2))
 *     start[k]                 sum_t exp((lse(X_{t-1}(k-1), X_{t-1}(k-2) where far(k)) + word_penalty) + log_start
 *                              + b_t + beta_t - loglik), plus gamma_0 of the start slots
 * gamma, trans, post, the observation sums, the second moments and the mixture responsibilities are per slot exactly
 * as without flags; nobs counts the slots of utterances with a path, whether or not mass went through them.
 *   optional      [total_words] uint8 (0 / 1), between word_offsets and total_words in the argument list; NULL means
 *                 all zero, and the call then IS the entry point without _opt: the same launches, the same bytes
 *   workspace     sapr_connected_align_opt_workspace_bytes: what sapr_connected_align takes, then one byte per
 *                 utterance (the slot its path ends in), rounded up to 16; with optional == NULL the size of
 *                 sapr_connected_align_workspace_bytes is enough.  The three embed entry points keep their size
 *                 functions: their workspaces do not grow
 * Every other argument, output, check and error code is that of the entry point without _opt.  An utterance whose
 * flags break the two rules, or hold a byte other than 0 / 1, has no path (-inf, rows of -1, exact zeros in the
 * statistics) and nothing else in the batch changes.  max_words counts optional slots too. */
int sapr_connected_align_opt_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t max_words, int32_t S,
                                             size_t *bytes);
int sapr_connected_align_opt(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                             const int32_t *words /* [total_words] */, const int64_t *word_offsets /* [n_utts + 1] */,
                             const uint8_t *optional /* [total_words] or NULL */, int64_t total_words,
                             int32_t max_words, const double *log_start, const double *log_trans,
                             const double *log_exit, double word_penalty, int32_t W, int32_t S, void *workspace,
                             size_t workspace_bytes, double *score, int32_t *path_word /* may be NULL */,
                             int32_t *path_state /* may be NULL */, uint8_t *path_entry /* may be NULL */,
                             int32_t *word_start /* [total_words], may be NULL */, void *stream);
int sapr_connected_embed_opt(const double *logb, const float *feats /* [total_frames][D]; NULL iff D == 0 */,
                             int32_t D, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                             const int32_t *words, const int64_t *word_offsets,
                             const uint8_t *optional /* [total_words] or NULL */, int64_t total_words,
                             int32_t max_words, const double *log_start, const double *log_trans,
                             const double *log_exit, double word_penalty, int32_t W, int32_t S, void *workspace,
                             size_t workspace_bytes, double *loglik /* [n_utts] */,
                             double *stats /* [W][width] or NULL */,
                             double *post /* [total_frames][max_words*SP] or NULL */, void *stream);
int sapr_connected_embed_full_opt(const double *logb, const float *feats /* [total_frames][D] */, int32_t D,
                                  const int64_t *offsets, int64_t n_utts, int64_t total_frames, const int32_t *words,
                                  const int64_t *word_offsets, const uint8_t *optional /* [total_words] or NULL */,
                                  int64_t total_words, int32_t max_words, const double *log_start,
                                  const double *log_trans, const double *log_exit, double word_penalty, int32_t W,
                                  int32_t S, void *workspace, size_t workspace_bytes, double *loglik /* [n_utts] */,
                                  double *stats /* [W][width] or NULL */,
                                  double *post /* [total_frames][max_words*SP] or NULL */, void *stream);
int sapr_connected_embed_gmm_opt(const double *logb, const float *feats /* [total_frames][D] */, int32_t D,
                                 const double *pack /* [W][sapr_gmm_pack_layout(S, M, D)] */, int32_t M,
                                 const int64_t *offsets, int64_t n_utts, int64_t total_frames, const int32_t *words,
                                 const int64_t *word_offsets, const uint8_t *optional /* [total_words] or NULL */,
                                 int64_t total_words, int32_t max_words, const double *log_start,
                                 const double *log_trans, const double *log_exit, double word_penalty, int32_t W,
                                 int32_t S, void *workspace, size_t workspace_bytes, double *loglik /* [n_utts] */,
                                 double *stats /* [W][width] or NULL */,
                                 double *post /* [total_frames][max_words*SP] or NULL */, void *stream);

/* Flat start of HMMLearnModel (hmmlearn_hmm.py:83-94: np.mean / np.var over axis 0 of the concatenated float32
 * features): numpy adds row after row in float32, so each column is one sequential float32 chain — reproduced
 * bit for bit.  center == NULL: out[d] = sum_r x[r][d]; else out[d] = sum_r RN32(RN32(x[r][d] - center[d])^2).
 * The divisions by N stay with the caller (numpy's own true_divide). */
int sapr_colsum_f32(const float *x, int64_t n_rows, int32_t D, const float *center /* may be NULL */, float *out,
                    void *stream);

/* ------------------------------------------------------------------------------------
 * The reference's from-scratch HMM (custom_hmm.py): non-emitting entry/exit states, full
 * covariances, the Gram-row-sum emission term — every quirk kept (see custom_*.hip).  Models are
 * float64 arrays prepared on the host exactly as the reference prepares them per call:
 *   means[W][S][D], inv[W][S][D][D] = inv(cov + 1e-6 I), cterm[W][S] = D*log(2*pi) + logdet,
 *   A[W][S][S], logA[W][S][S] = log(A)   (custom_hmm.py:160-165, :191-205).
 *
 *   sapr_custom_estep       custom_hmm.py:146-322,:434-439 per utterance (model utt_model[u], or 0):
 *                           lattices E/alpha/beta/gamma [total_frames][S], optional dense
 *                           xi [total_frames][S][S] (rows t < T-1), and
 *                           utt_out[u] = {LL, scale, agg_gamma[S], agg_xi[S][S]}
 *   sapr_custom_emission_exact  custom_hmm.py:146-174 in the reference's evaluation order (bit-exact)
 *   sapr_custom_decode      custom_hmm.py:462-514 for every (utterance, model): trellis over the first
 *                           Tq frames; scores[n_utts][W], paths[n_utts][W][Tq]
 *   sapr_custom_update_b    custom_hmm.py:366-400 (means, occupancies, raw covariances / occupancy;
 *                           symmetrisation and flooring are host work)
 *   sapr_custom_global_sum / _cov   custom_hmm.py:70-92 (flat-start sums)
 * ---------------------------------------------------------------------------------- */
/* lane_slots: 0 = lattices in the reference's row layout [total_frames][S]; > 0 (>= n_utts) = lattices
 * [max_T][S][lane_slots] with the utterance index fastest (coalesced; gamma then goes to the update_b
 * entry points with the same lane_slots).  In the lane_slots layout with xi == NULL (the batched training path) gamma
 * and utt_out are the outputs: E is filled, the alpha (unshifted) and beta lattices are scratch except for the
 * utterances whose backward half had to run in the reference's own order (custom_estep.hip).
 * An utterance too short to reach the exit state (T < S - 1) has NaN posteriors in EVERY state of every frame and NaN
 * posterior sums, as in the reference (a soft-max over a row of -inf), and no transition counts; the batched path
 * used to return exact zeros for the exit state's posteriors of such an utterance.  An utterance of 0 frames gets a
 * zero utt_out row and nothing else. */
int sapr_custom_estep(const float *feats, const int64_t *offsets, const int32_t *utt_model, int64_t n_utts,
                      int32_t D, int32_t S, int32_t W, const double *means, const double *inv,
                      const double *cterm, const double *A, const double *logA, int64_t lane_slots, double *E,
                      double *alpha, double *beta, double *gamma, double *xi_dense /* may be NULL */,
                      double *utt_out, void *stream);
/* the slot-major copy of the features, feat_t[max_T][D][lane_slots] float32 (zero past each utterance), and the E-step
 * reading from it: one coalesced row per wavefront and value instead of 64 private 4-byte reads — what the batched
 * training shapes of sapr_custom_estep spend most of their time on.  custom_hmm.py:402-460's loop stages once per
 * call of baum_welch (the features do not change between iterations).  frame_sums[D][lane_slots] float64 (may be NULL
 * in both calls): every utterance's sum over its frames, in frame order — the vector custom_hmm.py:168-172's row sum
 * of the Gram matrix needs; given to the E-step it saves every iteration a pass over the features */
int sapr_custom_stage_features(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D, int32_t max_T,
                               int64_t lane_slots, float *feat_t, double *frame_sums /* may be NULL */, void *stream);
int sapr_custom_estep_staged(const float *feats, const int64_t *offsets, const int32_t *utt_model, int64_t n_utts,
                             int32_t D, int32_t S, int32_t W, const double *means, const double *inv,
                             const double *cterm, const double *A, const double *logA, int64_t lane_slots, double *E,
                             double *alpha, double *beta, double *gamma, double *xi /* may be NULL */,
                             double *utt_out, const float *feat_t /* may be NULL */,
                             const double *frame_sums /* may be NULL */, void *stream);
/* single-utterance pieces on caller-supplied lattices (the reference's per-method API: forward(E),
 * backward(E, scale), compute_gamma(alpha, beta), compute_xi(alpha, beta, E)); op: 0 emission,
 * 1 forward (scale -> scalar[0]), 2 backward (scale <- scalar[0]), 3 gamma, 4 xi */
int sapr_custom_piece(int32_t op, const float *x, int32_t T, int32_t D, int32_t S, const double *means,
                      const double *inv, const double *cterm, const double *A, const double *logA, double *E,
                      double *alpha, double *beta, double *gamma, double *xi, double *scalar, void *stream);
/* evaluation-order-faithful emission rows (custom_hmm.py:168-172 as numpy/OpenBLAS evaluate it: two
 * fused-multiply-add chains over the contraction index and numpy's pair-wise row sum of the (T,T) Gram matrix),
 * bit-identical to the reference's compute_emission_matrix on the golden build.  n_rows > 0: the first n_rows
 * frames of every utterance against every model, E[n_utts][W][n_rows][S]; n_rows == 0 (W == 1): all frames,
 * E[total_frames][S]. */
int sapr_custom_emission_exact(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t W, int32_t D,
                               int32_t S, int32_t n_rows, int32_t max_T /* longest utterance; used when n_rows == 0 */,
                               const double *means, const double *inv, const double *cterm, double *E, void *stream);
/* HMM.decode (custom_hmm.py:462-514) for every (utterance, model) and, optionally, Decoder.decode_sequence's
 * arg-max over the models (decoder.py:35-49): e_rows is workspace for n_utts*W*Tq*S doubles; every utterance
 * must hold >= Tq frames; best_word / best_score / best_path[n_utts][Tq] may all be NULL */
int sapr_custom_decode(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t W, int32_t D,
                       int32_t S, int32_t num_states, int32_t Tq, const double *means, const double *inv,
                       const double *cterm, const double *A, const double *logA, double *e_rows, double *scores,
                       int32_t *paths, int32_t *best_word, double *best_score, int32_t *best_path, void *stream);
int sapr_custom_update_b_workspace_bytes(int64_t n_utts, int32_t W, int32_t D, int32_t S, size_t *bytes);
int sapr_custom_update_b(const float *feats, const int64_t *offsets, const int32_t *utt_model, int64_t n_utts,
                         int32_t W, int32_t D, int32_t S, const double *gamma, int64_t lane_slots,
                         double *means_out, double *occ_out, double *covs_out, void *workspace,
                         size_t workspace_bytes, void *stream);
/* the same two passes split so that a sharded run can sum across ranks in between (custom_hmm.py:366-400 is
 * two-pass: covariances are taken about the NEW means): unnormalised sum_x[W][S][D] + occ[W][S], then
 * unnormalised scatter[W][S][D][D] about `means`; sapr_custom_normalise divides by occ where occ > 0 */
int sapr_custom_update_b_sums(const float *feats, const int64_t *offsets, const int32_t *utt_model, int64_t n_utts,
                              int32_t W, int32_t D, int32_t S, const double *gamma, int64_t lane_slots,
                              double *sum_x_out, double *occ_out, void *workspace, size_t workspace_bytes,
                              void *stream);
int sapr_custom_update_b_scatter(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                 int64_t n_utts, int32_t W, int32_t D, int32_t S, const double *gamma,
                                 int64_t lane_slots, const double *means, double *scatter_out, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* both passes as one (one model, D = 13, S <= 16): out[16][112] = posterior-weighted moments about `center`[D] —
 * row s: columns 0..90 the upper triangle of sum g x'x'^T, 91..103 sum g x', 104 sum g (x' = x - center); after the
 * cross-rank sum mean = center + s1/occ, cov = S2/occ - (s1/occ)(s1/occ)^T: custom_hmm.py:366-400's values from one
 * read of the data on the float64 matrix cores */
int sapr_custom_update_b_moments(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D, int32_t S,
                                 const double *gamma, int64_t lane_slots, const double *center, double *out,
                                 void *workspace, size_t workspace_bytes, void *stream);
int sapr_custom_normalise(double *x, const double *occ, int64_t n_states, int32_t per, void *stream);
/* out[K] = sum over rows of part[n_rows][K], rows added one after another in row order — the reference's
 * accumulation over sequences (custom_hmm.py:434-439) applied to sapr_custom_estep's utt_out, on the device */
int sapr_custom_fold_rows(const double *part, int64_t n_rows, int64_t K, double *out, void *stream);
int sapr_custom_global_workspace_bytes(int64_t n_utts, int64_t total_frames, int32_t D, size_t *bytes);
int sapr_custom_global_sum(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D,
                           double *sum_out, void *workspace, size_t workspace_bytes, void *stream);
int sapr_custom_global_cov(const float *feats, int64_t total_frames, int32_t D, const double *mean,
                           double *cov_out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * MFCC front-end.  Replaces librosa.feature.mfcc(y, sr, n_mfcc=13, win_length, hop_length,
 * window="hamming", center=True) as called at mfcc_extract.py:15-23 (librosa defaults:
 * n_fft 2048, 128 Slaney mels, power 2, power_to_db(top_db=80), DCT-II ortho), batched over
 * utterances, plus BASELINE.json's north-star options (pre-emphasis, delta / delta-delta).
 *
 *   plan   host-side tables (Hamming window, FFT twiddles, banded mel filterbank as MFMA
 *          fragments, DCT rows, Savitzky-Golay taps) uploaded once; n_fft is 512 or 2048.
 *          max_frames > 0: FUSED mode — the log-mel matrix of one utterance (at most max_frames
 *          frames) lives in LDS, so the utterance-global top_db maximum costs no second HBM pass;
 *          max_frames == 0 (or a fused layout that does not fit 160 KiB of LDS, or one that fits only one workgroup
 *          per CU where the layout without the log-mel matrix fits two — the reference preset: ask
 *          sapr_mfcc_plan_info / sapr_mfcc_workspace_bytes, do not assume): TWO-PASS mode —
 *          log-mel rows go through a caller-supplied HBM workspace and a second small kernel does
 *          clip / DCT / deltas; utterances of any length.
 *   batch  pcm[total_samples] float32 (librosa.load's mono float32, mfcc_extract.py:12),
 *          sample_offsets[n_utts+1], frame_offsets[n_utts+1] with
 *          frames(u) = 1 + n_samples(u) / hop  (center=True);
 *          out[total_frames][d_out] float32 frame-major, d_out = n_mfcc * (deltas ? 3 : 1)
 *          — the layout sapr_viterbi_diag_scores consumes (transpose of the reference's (13,T)).
 *          HARD PRECONDITION: total_frames == frame_offsets[n_utts] (the value on the device).  `out`, the
 *          workspace and the launch are sized from total_frames; the offsets are only read on the device, so
 *          the call cannot return an error for a mismatch.  The 512-point wave-private core checks it on the
 *          device: offsets that describe MORE frames than total_frames make it write nothing but NaN into all
 *          of `out` (tests/test_capi_errors_gpu.py) instead of running past the buffers.
 *          That core counts frames and utterances in 32 bits: total_frames or n_utts of 2^31 - 16 or more
 *          return SAPR_ERR_ARG before anything is launched (the log-mel workspace of such a batch exceeds the
 *          device's memory by itself).
 *   slices The 512-point wave-private core cuts a large batch into slices of whole utterances and runs the finish
 *          pass of slice k on a low-priority stream the plan owns, under the spectral kernel of slice k + 1
 *          (same bits as the single launch sequence; SAPR_MFCC_SLICES at plan creation: 1 = never, n = always n).
 *          The caller's stream waits for that work before sapr_mfcc_batch returns, so whatever is enqueued on
 *          `stream` afterwards sees complete features; nothing is created per call.  Forced grids
 *          (grid_blocks > 0), a capturing stream and small batches keep the single launch sequence.  The plan's
 *          stream and events are guarded by a mutex: concurrent calls on one plan from several host threads are
 *          serialised at the launch, not undefined.
 *   finish The finish pass of that core has bodies specialised on 40 mels without and with deltas and a generic
 *          body for every other shape (same bits; SAPR_FINISH_GENERIC=1 at plan creation: the generic body for
 *          every plan).
 * ---------------------------------------------------------------------------------- */
int sapr_mfcc_plan_create(double sr, int32_t n_fft, int32_t win_length, int32_t hop,
                          int32_t n_mels, int32_t n_mfcc, double fmin, double fmax /* <=0: sr/2 */,
                          double top_db, double preemph /* 0 = off */, int32_t deltas,
                          int32_t max_frames, void **plan_out);
int sapr_mfcc_plan_destroy(void *plan);
int sapr_mfcc_plan_info(const void *plan, int32_t *d_out, int32_t *max_frames, int64_t *lds_bytes,
                        int32_t *mel_ksteps);
int sapr_mfcc_workspace_bytes(const void *plan, int64_t total_frames, int64_t n_utts, size_t *bytes); /* 0 if fused */
int sapr_mfcc_batch(const void *plan, const float *pcm, const int64_t *sample_offsets,
                    const int64_t *frame_offsets, int64_t n_utts, int64_t total_frames, float *out,
                    int32_t grid_blocks /* <=0: auto */, void *workspace /* may be NULL if fused */,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Sample-rate conversion ahead of the MFCC chain: librosa.load(path) resamples every file to
 * 22 050 Hz (mfcc_extract.py:12).  Polyphase FIR with scipy.signal.resample_poly's definition; the
 * low-pass taps (already scaled by `up` and left-padded as scipy does) and n_pre_remove come from the
 * host (sapr_amd/mfcc_extract.py: resample_design).  out_offsets[u+1]-out_offsets[u] must equal
 * ceil(n_in(u) * up / down).  float32 in/out, float64 accumulation.
 * ---------------------------------------------------------------------------------- */
int sapr_resample_poly(const float *x, const int64_t *in_offsets, const int64_t *out_offsets, int64_t n_utts,
                       int64_t max_out, int32_t up, int32_t down, const float *taps, int32_t n_taps,
                       int32_t n_pre_remove, float *y, void *stream);

/* 16-bit PCM (WAV sample format) -> float32 in [-1, 1) on the device: x / 32768, as the host WAV reader of
 * sapr_amd/mfcc_extract.py does, so that host-resident audio crosses PCIe as 2 bytes per sample */
int sapr_pcm16_to_f32(const int16_t *pcm16, int64_t n_samples, float *out, void *stream);

/* diagnostic build of sapr_mfcc_batch (BENCH-style plans only): stamps[grid_blocks][4][12] receives
 * per-wavefront, per-phase s_memtime sums.  Read the shares, not the run time. */
int sapr_mfcc_batch_stamped(const void *plan, const float *pcm, const int64_t *sample_offsets,
                            const int64_t *frame_offsets, int64_t n_utts, float *out,
                            int32_t grid_blocks, uint64_t *stamps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SAPR_HIP_H */
