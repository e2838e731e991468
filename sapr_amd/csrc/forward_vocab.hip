// Forward scoring over the vocabulary for diagonal-Gaussian HMMs on gfx950: loglik[n_utts][W], the arg-max word and
// the posterior over the words.
//
// Extends GaussianHMM.score (hmmlearn_hmm.py:104; hmmlearn _hmmc.cpp forward_log) over the model loop of
// decoder.py:42: every utterance under EVERY word model in one launch, where sapr_forward_diag (estep.hip) scores an
// utterance under the one model of its tile.  CPU restatement: oracle/c_oracle.decode_batch(which=1).
//
// Mapping: the (utterance tile, word) grid of the Viterbi kernels (viterbi_shared.h decode_block: the W workgroups
// that read the same 256 utterances sit on one XCD, so the features cross HBM once) around quick_forward_walk of
// diag_forward.h, the recursion of the E-step's fb_forward_kernel without the share stores — one lane per utterance, the
// model wavefront-uniform in SGPRs, log-densities in the quick form of emission_quick.h (three float64 instructions
// per state, dimension and frame; only the exact-kernel operands of the pack are read), NF frames per walk over the
// parameters.  The recursion's state is S registers per
// lane: no lattice reaches HBM, there is no workspace, and the grid is W times the single-model forward grid.
// Features are read from the frame-major batch itself (a lane's frame is 4 D contiguous bytes, re-read by the other
// W - 1 models from the XCD's L2), not from a slot-major copy.
//
// Arithmetic is float64; the quick emission form and the lse_unit.h chain agree with the CPU evaluation to ~1e-13
// relative (tests: 1e-11), not bit for bit.  Every (utterance, word) score is a function of that pair alone, so equal
// models give equal bits and the launch is deterministic.
#include "emission_quick.h"
#include "viterbi_shared.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "diag_forward.h"
#include "vocab_epilogue.h"

using namespace emission;

template <int D, int S, bool BIDIAG>
__global__ __launch_bounds__(kBlock) void forward_vocab_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
    int64_t n_utts, int64_t n_tiles, int32_t W, const double4 *__restrict__ prm_all,
    const double *__restrict__ gconst, const double *__restrict__ log_start, const double *__restrict__ log_trans,
    double *__restrict__ loglik) {
  int64_t tile;
  int w;
  decode_block(W, n_tiles, tile, w);
  if (tile >= n_tiles) return;  // grid padding (whole block leaves together)

  const int64_t slot = tile * kBlock + threadIdx.x;
  const Lane ln = lane_of(offsets, slot < n_utts ? (order ? static_cast<int64_t>(order[slot]) : slot) : -1);
  const DiagModel m = diag_model<D, S>(prm_all, gconst, log_start, log_trans, w);
  const float *__restrict__ xp = feats + ln.beg * D;

  double fwd[S];
  quick_forward_walk<D, S, BIDIAG>(
      ln, m, fwd, [&](int t, auto &x) { load_quick_frame<D>(xp + static_cast<int64_t>(t) * D, x); });
  // logsumexp over the last row (unreachable padding states add exp(-inf) = 0); no frames: the C oracle's -inf
  if (ln.live) loglik[ln.u * W + w] = ln.T > 0 ? lse_all<S>(fwd) : neg_inf();
}

struct VocabArgs {
  const float *feats;
  const int64_t *offsets;
  const int32_t *order;
  int64_t n_utts;
  int32_t W;
  PackView pv;
  double *loglik;
  hipStream_t stream;
};

template <int D, int S>
int launch_forward_vocab(const VocabArgs &a, int topology) {
  const int64_t n_tiles = (a.n_utts + kBlock - 1) / kBlock;
  const int64_t blocks = round_up(n_tiles, kXcd) * a.W;
  if (blocks > 0x7fffffffLL) return fail(SAPR_ERR_ARG, "grid too large (%lld blocks)", (long long)blocks);
  dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
  if (topology == SAPR_TOPO_BIDIAG)
    SAPR_LAUNCH((forward_vocab_kernel<D, S, true>), grid, block, 0, a.stream, a.feats, a.offsets, a.order, a.n_utts,
                n_tiles, a.W, a.pv.prm, a.pv.gconst, a.pv.log_start, a.pv.log_trans, a.loglik);
  else
    SAPR_LAUNCH((forward_vocab_kernel<D, S, false>), grid, block, 0, a.stream, a.feats, a.offsets, a.order, a.n_utts,
                n_tiles, a.W, a.pv.prm, a.pv.gconst, a.pv.log_start, a.pv.log_trans, a.loglik);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_forward_vocab(const float *feats, const int64_t *offsets, const int32_t *order, int64_t n_utts,
                                  int32_t D, int32_t max_T, const void *pack, int32_t W, int32_t S, int32_t topology,
                                  double *loglik, int32_t *best_word, double *word_post, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && W > 0 && S > 0 && D > 0 && max_T >= 0, "bad sizes");
  SAPR_REQUIRE(topology == SAPR_TOPO_DENSE || topology == SAPR_TOPO_BIDIAG, "bad topology");
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(feats && offsets && pack && loglik, "NULL pointer argument");
  VocabArgs a;
  a.feats = feats;
  a.offsets = offsets;
  a.order = order;
  a.n_utts = n_utts;
  a.W = W;
  a.pv = pack_view(pack, W, S, D);
  a.loglik = loglik;
  a.stream = as_stream(stream);
  const int rc = dispatch_ds(D, S, [&](auto d, auto s) {
    return launch_forward_vocab<decltype(d)::value, decltype(s)::value>(a, topology);
  });
  if (rc) return rc;
  if (best_word || word_post) return launch_vocab_epilogue(n_utts, W, loglik, best_word, word_post, a.stream);
  return 0;
}
