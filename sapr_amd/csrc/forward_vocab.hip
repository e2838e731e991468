// Forward scoring over the vocabulary for diagonal-Gaussian HMMs on gfx950: loglik[n_utts][W], the arg-max word and
// the posterior over the words.
//
// Extends GaussianHMM.score (hmmlearn_hmm.py:104; hmmlearn _hmmc.cpp forward_log) over the model loop of
// decoder.py:42: every utterance under EVERY word model in one launch, where sapr_forward_diag (estep.hip) scores an
// utterance under the one model of its tile.  CPU restatement: oracle/c_oracle.decode_batch(which=1).
//
// Mapping: the (utterance tile, word) grid of the Viterbi kernels (viterbi_shared.h decode_block: the W workgroups
// that read the same 256 utterances sit on one XCD, so the features cross HBM once) around the forward recursion of
// fb_forward_kernel<..., QEMIT> — one lane per utterance, the model wavefront-uniform in SGPRs, log-densities in the
// quick form of emission_quick.h (three float64 instructions per state, dimension and frame; only the exact-kernel
// operands of the pack are read), NF frames per walk over the parameters.  The recursion's state is S registers per
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
  const bool live = slot < n_utts;
  const int64_t u = live ? (order ? static_cast<int64_t>(order[slot]) : slot) : 0;
  const int64_t beg = live ? offsets[u] : 0;
  const int T = live ? static_cast<int>(offsets[u + 1] - beg) : 0;
  const int Tw = wave_max_i32(T);

  // wavefront-uniform model pointers -> scalar loads
  const double4 *__restrict__ prm = prm_all + static_cast<int64_t>(w) * S * D;
  const double *__restrict__ gc = gconst + static_cast<int64_t>(w) * S;
  const double *__restrict__ ls = log_start + static_cast<int64_t>(w) * S;
  const double *__restrict__ lt = log_trans + static_cast<int64_t>(w) * S * S;
  const float *__restrict__ xp = feats + beg * D;

  double fwd[S];
#pragma unroll
  for (int s = 0; s < S; ++s) fwd[s] = ls[s];

  // one frame of _hmmc.cpp forward_log from its log-densities (fb_forward_kernel's recursion without the share stores)
  auto step = [&](int t, const double (&b)[S]) {
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < S; ++j) fwd[j] += b[j];
    } else if constexpr (BIDIAG) {
      // descending j: fwd[j - 1] is still the previous frame's value when state j reads it
#pragma unroll
      for (int j = S - 1; j >= 1; --j)
        fwd[j] = lse2(fwd[j - 1] + lt[(j - 1) * S + j], fwd[j] + lt[j * S + j]) + b[j];
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
  };

  // 39-dimensional frames stay float32 in registers and are promoted inside the chain (emission_quick.h)
  using XT = std::conditional_t<(D >= 39), float, double>;
  constexpr int NF = (D >= 39 || S > 10) ? 2 : 4;
  for (int t0 = 0; t0 < Tw; t0 += NF) {
    if (t0 < T) {
      XT xq[NF][D];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int t = t0 + f < T ? t0 + f : T - 1;  // frames past the end: evaluated, not used
        if constexpr (D >= 39)
          load_frame_f32<D>(xp + static_cast<int64_t>(t) * D, xq[f]);
        else
          load_frame<D>(xp + static_cast<int64_t>(t) * D, xq[f]);
      }
      double bq[NF][S];
      frame_log_densities_quick<D, S, NF>(xq, prm, gc,
                                          [&](auto jc, int f, double bv) { bq[f][decltype(jc)::value] = bv; });
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (t0 + f < T) step(t0 + f, bq[f]);
    }
  }
  // logsumexp over the last row (unreachable padding states add exp(-inf) = 0); no frames: the C oracle's -inf
  if (live) loglik[u * W + w] = T > 0 ? lse_all<S>(fwd) : neg_inf();
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
  int rc;
  if (D == 13 && S == 10) rc = launch_forward_vocab<13, 10>(a, topology);
#ifndef SAPR_ONLY_13_10
  else if (D == 13 && S == 18) rc = launch_forward_vocab<13, 18>(a, topology);
  else if (D == 39 && S == 10) rc = launch_forward_vocab<39, 10>(a, topology);
  else if (D == 39 && S == 18) rc = launch_forward_vocab<39, 18>(a, topology);
#endif
  else
    rc = fail(SAPR_ERR_UNSUPPORTED, "trellis kernels are instantiated for (D,S) in {13,39}x{10,18}; got D=%d S=%d", D,
              S);
  if (rc) return rc;
  if (best_word || word_post) return launch_vocab_epilogue(n_utts, W, loglik, best_word, word_post, a.stream);
  return 0;
}
