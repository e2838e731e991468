// Connected-word recognition on gfx950: one-pass Viterbi over the word loop (the end of any word may be followed by
// the start of any word), in two stages cut where the dependence changes.  CPU restatement, which is
// the definition: tests/_connected_ref.py.
//
// Stage 1, sapr_connected_emit_diag: logb[total_frames][R = W * SP] for diagonal Gaussians, frame-parallel, one
// thread per frame.  The frame's DP features stay in registers as float64, the lane walks the R flat states in a
// rolled loop and every parameter is wavefront-uniform: the operand block comes in through a __restrict__
// kernel-argument pointer, so the compiler issues scalar loads (as gmm_hmm.hip does; no inline assembly).  The
// operand block is built by the host from the arrays sapr_diag_pack takes (connected.py emit_operands), per flat
// state 1 + 2 DP doubles: {gconst, mean[DP], 1 / var[DP]}; padding features carry mean 0 and coefficient 0 and add
// +0.0, a padding state carries gconst = +inf and comes out as -inf.
//     logb = -0.5 * (gconst + sum_d ((x_d - mean_d) * (x_d - mean_d)) * (1 / var_d)),   d ascending
//
// Stage 1 for the other two families, sapr_connected_emit_gmm and sapr_connected_emit_full: the same geometry over a
// (frame block, word) grid — every (frame, word) pair is independent, and one word's SP states cost up to
// SP * DP^2 / 2 FMAs per frame, so a small batch still fills the device.  The operand is the family's own pack
// ([W][doubles per model] of sapr_gmm_pack_layout / sapr_full_pack_layout, read in place behind the head the
// recursions of the per-model kernels use), the arithmetic the shared device functions of gmm_emit_kernel /
// full_emit_kernel (gmm_ops.h mix_log_terms + lse_ops.h lse_all; fullcov_emit.h full_log_density) called in the same
// order: the emitted bits are the per-model emissions' bits.  A state whose every component constant (whose constant)
// is -inf — the padding states of the pack — is written as -inf by a wavefront-uniform branch, whatever the frame
// holds, and costs no arithmetic.
//
// Stage 2, sapr_connected_viterbi: the recursion over a given logb; it knows nothing about the emission family.
//     connected_viterbi_kernel<RL>: the lane layout of connected_lanes.h over the flat states, four utterances per
//     workgroup, the transition table by source (SP is a run-time value here).  The coupling is this unit's own: any
//     word may follow any word, so E_{t-1} = max_r (delta + log_exit) is one wave-wide butterfly over (value, flat
//     index), the lowest index among equals, and needs no LDS row.
//     Back-pointers: one byte per (frame, flat state) — the predecessor state, or kXEntry where the word entry won —
//     and the flat arg-max of E per frame (int32), both in the workspace.  A second kernel, one lane per utterance,
//     walks back and writes path_word, path_state, path_entry, n_words.
//
// The recursion is float64 adds and compares in the order of the definition (within candidates i ascending, first
// maximum; entry only where strictly greater; the emission added last): bit for bit the reference.  No atomics; an
// utterance's outputs are a function of its own frames and the network alone.  Non-finite values propagate.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "fullcov_emit.h"
#include "connected_lanes.h"

constexpr int cn_sp_of(int S) { return sp_of(S); }  // (the padding rules of every family: gmm_ops.h)
constexpr int cn_dp_of(int D) { return dp_of(D); }

// the emission stages' check: x_check_shape and the feature dimension
inline int cn_check_shape(int32_t W, int32_t S, int32_t D) {
  if (S > kMaxS || D > kMaxD || static_cast<int64_t>(W) * cn_sp_of(S) > kXMaxR)
    return fail(SAPR_ERR_UNSUPPORTED,
                "the connected-word kernels serve S in 1..%d, D in 1..%d and W * SP <= %d; got W=%d S=%d D=%d",
                kMaxS, kMaxD, kXMaxR, W, S, D);
  return 0;
}

// ---------------------------------------------------------------------------------------
// stage 1: diagonal-Gaussian emissions
// ---------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kXBlock) void connected_emit_kernel(const float *__restrict__ feats,
                                                                 int64_t total_frames, int32_t D, int32_t R,
                                                                 const double *__restrict__ ops,
                                                                 double *__restrict__ logb) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  const bool live = t < total_frames;
  double x[DP];
  const float *__restrict__ xp = feats + (live ? t : 0) * D;
#pragma unroll
  for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? static_cast<double>(xp[d]) : 0.0;
  double *__restrict__ out = logb + (live ? t : 0) * R;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const double *__restrict__ o = ops + static_cast<int64_t>(r) * (1 + 2 * DP);  // wavefront-uniform: scalar loads
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const double diff = x[d] - o[1 + d];
      acc += (diff * diff) * o[1 + DP + d];
    }
    const double v = -0.5 * (o[0] + acc);
    if (live) out[r] = v;
  }
}

// ---------------------------------------------------------------------------------------
// stage 1: mixture and full-covariance emissions, grid (frame blocks, W)
// ---------------------------------------------------------------------------------------
template <int MP, int DP>
__global__ __launch_bounds__(kXBlock) void connected_emit_gmm_kernel(const float *__restrict__ feats,
                                                                     int64_t total_frames, int32_t D, int32_t SP,
                                                                     int32_t R, const double *__restrict__ pack,
                                                                     double *__restrict__ logb) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (t >= total_frames) return;
  const int w = blockIdx.y;
  double x[DP];
  load_frame_pad<DP>(feats + t * D, D, true, x);
  // the word's model in the pack of sapr_gmm_pack_layout, wavefront-uniform: scalar loads
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * static_cast<int64_t>(model_doubles(SP, MP, DP));
  const double *__restrict__ cc = mdl + off_cc(SP);
  const double *__restrict__ prm = mdl + off_prm(SP, MP);
  double *__restrict__ out = logb + t * R + w * SP;
#pragma unroll 1
  for (int s = 0; s < SP; ++s) {
    bool off = true;  // (uniform) every component switched off: a padding state
#pragma unroll
    for (int m = 0; m < MP; ++m) off = off && cc[s * MP + m] == neg_inf();
    if (off) {
      out[s] = neg_inf();
      continue;
    }
    double lc[MP];
    mix_log_terms<MP, DP>([&](int d) { return x[d]; }, prm + static_cast<int64_t>(s) * DP * MP * 2, cc + s * MP, lc);
    double v;
    if constexpr (MP == 1)
      v = lc[0];
    else
      v = lse_all<MP>(lc);
    out[s] = v;
  }
}

template <int DP>
__global__ __launch_bounds__(kXBlock) void connected_emit_full_kernel(const float *__restrict__ feats,
                                                                      int64_t total_frames, int32_t D, int32_t SP,
                                                                      int32_t R, const double *__restrict__ pack,
                                                                      double *__restrict__ logb) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (t >= total_frames) return;
  const int w = blockIdx.y;
  double x[DP];
  load_frame_pad<DP>(feats + t * D, D, true, x);
  // the word's model in the pack of sapr_full_pack_layout, wavefront-uniform: scalar loads
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * static_cast<int64_t>(full_model_doubles(SP, DP));
  const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
  const double *__restrict__ mu = cc + SP;
  const double *__restrict__ wi = mu + SP * DP;
  double *__restrict__ out = logb + t * R + w * SP;
#pragma unroll 1
  for (int s = 0; s < SP; ++s) {
    const double c = cc[s];
    if (c == neg_inf()) {
      out[s] = neg_inf();
      continue;
    }
    out[s] = full_log_density<DP>([&](int d) { return x[d]; }, mu + s * DP, wi + static_cast<int64_t>(s) * DP * DP, c);
  }
}

// ---------------------------------------------------------------------------------------
// stage 2: the recursion
// ---------------------------------------------------------------------------------------
struct ValIdx {
  double v;
  int i;
};

// wave-wide first maximum: the greatest value, among equals the lowest flat index; every lane gets the result
__device__ __forceinline__ ValIdx wave_argmax_first(ValIdx a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(a.v, o, kWave);
    const int oi = __shfl_xor(a.i, o, kWave);
    const bool take = ov > a.v || (ov == a.v && oi < a.i);
    a.v = take ? ov : a.v;
    a.i = take ? oi : a.i;
  }
  return a;
}

template <int RL>
__global__ __launch_bounds__(kXBlock) void connected_viterbi_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    double word_penalty, int32_t W, int32_t S, int32_t SP, uint8_t *__restrict__ bp, int32_t *__restrict__ exit_idx,
    double *__restrict__ score) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  extern __shared__ double tab[];  // [SP][RP] by source
  const int R = W * SP;
  x_load_by_source(tab, log_trans, W, S, SP, RP, kXBlock);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + (threadIdx.x / kWave);
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;

  double ls[RL], lx[RL], delta[RL], bn[RL];
  int sk[RL];
  bool ok[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const XState x = x_flat_state(k * kWave + lane, R, SP, S, log_start, log_exit);
    ok[k] = x.ok;
    sk[k] = x.s;
    ls[k] = x.ls;
    lx[k] = x.lx;
    delta[k] = neg_inf();
  }
  const uint64_t dmask = x_mask_by_source<RL>(tab, sk, lane, SP);

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = (ok[k] && T > 0) ? brow[k * kWave + lane] : neg_inf();

  ValIdx E{neg_inf(), 0};
  for (int64_t t = 0; t < T; ++t) {
    double b[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) b[k] = bn[k];
    {  // the next frame's row in flight under this frame's chain
      const int64_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
      for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[tn * R + k * kWave + lane] : neg_inf();
    }
    double v[RL];
    int back[RL];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        v[k] = ls[k];
        back[k] = kXEntry;
      }
    } else {
      double best[RL];
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        best[k] = neg_inf();
        back[k] = 0;
      }
      // predecessors i ascending = distances descending; the first maximum stays (strict compare)
      for (int d = SP - 1; d > -SP; --d) {
        if (!x_live(dmask, d, SP)) continue;  // (uniform)
        x_rotate<RL>(delta, lane, d, [=, &best, &back](int k, double prev) {
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[(in ? i : 0) * RP + k * kWave + lane];
          const double c = prev + (in ? lt : neg_inf());
          const bool take = c > best[k];
          best[k] = take ? c : best[k];
          back[k] = take ? i : back[k];
        });
      }
      const double ep = E.v + word_penalty;
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double entry = ep + ls[k];
        const bool take = entry > best[k];
        v[k] = take ? entry : best[k];
        back[k] = take ? kXEntry : back[k];
      }
    }
    uint8_t *__restrict__ bprow = bp + (beg + t) * R;
    ValIdx e{neg_inf(), lane};
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      delta[k] = v[k] + b[k];
      if (ok[k]) bprow[k * kWave + lane] = static_cast<uint8_t>(back[k]);
      const double c = delta[k] + lx[k];
      const bool take = k == 0 || c > e.v;  // the lane's own states in flat order: the first maximum stays
      e.i = take ? k * kWave + lane : e.i;
      e.v = take ? c : e.v;
    }
    E = wave_argmax_first(e);
    E.i = __builtin_amdgcn_readfirstlane(E.i);
    E.i = E.i < R ? E.i : R - 1;  // (only a NaN lattice can name a lane without a state: keep the walk inside the row)
    if (lane == 0) exit_idx[beg + t] = E.i;
  }
  if (lane == 0) score[u] = T > 0 ? E.v : neg_inf();
}

// one lane per utterance walks back from the best exit of the last frame
__global__ __launch_bounds__(kXBlock) void connected_backtrace_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t SP, int32_t R,
    const uint8_t *__restrict__ bp, const int32_t *__restrict__ exit_idx, const double *__restrict__ score,
    int32_t *__restrict__ n_words, int32_t *__restrict__ path_word, int32_t *__restrict__ path_state,
    uint8_t *__restrict__ path_entry) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (u >= n_utts) return;
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  if (!finite_f64(score[u]) || T == 0) {
    x_no_path(beg, T, path_word, path_state, path_entry);
    if (n_words) n_words[u] = 0;
    return;
  }
  int r = exit_idx[beg + T - 1];
  int nw = 0;
  for (int64_t t = T - 1; t >= 0; --t) {
    const int w = r / SP;
    if (path_word) path_word[beg + t] = w;
    if (path_state) path_state[beg + t] = r - w * SP;
    const int b = bp[(beg + t) * R + r];
    const bool entry = t == 0 || b == kXEntry;
    if (path_entry) path_entry[beg + t] = entry ? 1 : 0;
    if (entry) {
      ++nw;
      if (t > 0) r = exit_idx[beg + t - 1];
    } else {
      r = w * SP + (b < SP ? b : 0);
    }
  }
  if (n_words) n_words[u] = nw;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_layout(int32_t W, int32_t S, int32_t D, int32_t *SP, int32_t *DP, int32_t *R) {
  SAPR_REQUIRE(W > 0 && S > 0 && D > 0, "bad sizes (W=%d S=%d D=%d)", W, S, D);
  if (int rc = cn_check_shape(W, S, D)) return rc;
  if (SP) *SP = cn_sp_of(S);
  if (DP) *DP = cn_dp_of(D);
  if (R) *R = W * cn_sp_of(S);
  return 0;
}

extern "C" int sapr_connected_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                              size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  if (int rc = cn_check_shape(W, S, 1)) return rc;
  const size_t R = static_cast<size_t>(W) * cn_sp_of(S);
  // back-pointers [total_frames][R] bytes (padded to 16), then the exit index of every frame (int32)
  *bytes = x_align16(static_cast<size_t>(total_frames) * R) + static_cast<size_t>(total_frames) * sizeof(int32_t);
  return 0;
}

extern "C" int sapr_connected_emit_diag(const float *feats, int64_t total_frames, int32_t D, const double *ops,
                                        int32_t W, int32_t S, double *logb, void *stream) {
  SAPR_REQUIRE(total_frames >= 0 && W > 0 && S > 0 && D > 0, "bad sizes (total_frames=%lld W=%d S=%d D=%d)",
               (long long)total_frames, W, S, D);
  if (int rc = cn_check_shape(W, S, D)) return rc;
  const int64_t blocks = (total_frames + kXBlock - 1) / kXBlock;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (total_frames == 0) return 0;
  SAPR_REQUIRE(feats && ops && logb, "NULL pointer argument");
  const int32_t R = W * cn_sp_of(S);
  const dim3 grid(static_cast<unsigned>(blocks)), block(kXBlock);
  hipStream_t st = as_stream(stream);
  switch (cn_dp_of(D)) {
    case 13: SAPR_LAUNCH((connected_emit_kernel<13>), grid, block, 0, st, feats, total_frames, D, R, ops, logb); break;
    case 26: SAPR_LAUNCH((connected_emit_kernel<26>), grid, block, 0, st, feats, total_frames, D, R, ops, logb); break;
    default: SAPR_LAUNCH((connected_emit_kernel<39>), grid, block, 0, st, feats, total_frames, D, R, ops, logb); break;
  }
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

namespace sapr {
namespace {

// what both pack-reading emission entry points check before any launch; *blocks: the frame blocks of the grid
int cn_emit_checks(const void *feats, int64_t total_frames, int32_t D, const void *pack, int32_t W, int32_t S,
                   const void *logb, int64_t *blocks) {
  if (int rc = cn_check_shape(W, S, D)) return rc;
  *blocks = (total_frames + kXBlock - 1) / kXBlock;
  SAPR_REQUIRE(*blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)*blocks);
  if (total_frames == 0) return 0;
  SAPR_REQUIRE(feats && pack && logb, "NULL pointer argument");
  return 0;
}

template <int MP>
int launch_emit_gmm(dim3 grid, hipStream_t st, const float *feats, int64_t total_frames, int32_t D, int32_t SP,
                    int32_t R, const double *pack, double *logb) {
  const dim3 block(kXBlock);
  switch (cn_dp_of(D)) {
    case 13:
      SAPR_LAUNCH((connected_emit_gmm_kernel<MP, 13>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
    case 26:
      SAPR_LAUNCH((connected_emit_gmm_kernel<MP, 26>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
    default:
      SAPR_LAUNCH((connected_emit_gmm_kernel<MP, 39>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
  }
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sapr

extern "C" int sapr_connected_emit_gmm(const float *feats, int64_t total_frames, int32_t D, const double *pack,
                                       int32_t W, int32_t S, int32_t M, double *logb, void *stream) {
  SAPR_REQUIRE(total_frames >= 0 && W > 0 && S > 0 && M > 0 && D > 0,
               "bad sizes (total_frames=%lld W=%d S=%d M=%d D=%d)", (long long)total_frames, W, S, M, D);
  if (int rc = check_shape(S, M, D)) return rc;
  int64_t blocks = 0;
  if (int rc = cn_emit_checks(feats, total_frames, D, pack, W, S, logb, &blocks)) return rc;
  if (total_frames == 0) return 0;
  const int32_t SP = cn_sp_of(S), R = W * SP;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(W));
  hipStream_t st = as_stream(stream);
  switch (mp_of(M)) {
    case 1: return launch_emit_gmm<1>(grid, st, feats, total_frames, D, SP, R, pack, logb);
    case 2: return launch_emit_gmm<2>(grid, st, feats, total_frames, D, SP, R, pack, logb);
    case 4: return launch_emit_gmm<4>(grid, st, feats, total_frames, D, SP, R, pack, logb);
    default: return launch_emit_gmm<8>(grid, st, feats, total_frames, D, SP, R, pack, logb);
  }
}

extern "C" int sapr_connected_emit_full(const float *feats, int64_t total_frames, int32_t D, const double *pack,
                                        int32_t W, int32_t S, double *logb, void *stream) {
  SAPR_REQUIRE(total_frames >= 0 && W > 0 && S > 0 && D > 0, "bad sizes (total_frames=%lld W=%d S=%d D=%d)",
               (long long)total_frames, W, S, D);
  int64_t blocks = 0;
  if (int rc = cn_emit_checks(feats, total_frames, D, pack, W, S, logb, &blocks)) return rc;
  if (total_frames == 0) return 0;
  const int32_t SP = cn_sp_of(S), R = W * SP;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(W)), block(kXBlock);
  hipStream_t st = as_stream(stream);
  switch (cn_dp_of(D)) {
    case 13:
      SAPR_LAUNCH((connected_emit_full_kernel<13>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
    case 26:
      SAPR_LAUNCH((connected_emit_full_kernel<26>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
    default:
      SAPR_LAUNCH((connected_emit_full_kernel<39>), grid, block, 0, st, feats, total_frames, D, SP, R, pack, logb);
      break;
  }
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sapr_connected_viterbi(const double *logb, const int64_t *offsets, int64_t n_utts,
                                      int64_t total_frames, const double *log_start, const double *log_trans,
                                      const double *log_exit, double word_penalty, int32_t W, int32_t S,
                                      void *workspace, size_t workspace_bytes, double *score, int32_t *n_words,
                                      int32_t *path_word, int32_t *path_state, uint8_t *path_entry, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = cn_check_shape(W, S, 1)) return rc;
  size_t need = 0;
  if (int rc = sapr_connected_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && score && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = cn_sp_of(S);
  const int32_t R = W * SP;
  uint8_t *bp = static_cast<uint8_t *>(workspace);
  int32_t *exit_idx =
      reinterpret_cast<int32_t *>(bp + x_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(R)));
  hipStream_t st = as_stream(stream);
  if (int rc = x_dispatch(SP, R, [&](auto rl, auto) {  // (the kernel takes SP as a run-time value)
        constexpr int RL = decltype(rl)::value;
        const size_t lds = static_cast<size_t>(SP) * kWave * RL * sizeof(double);
        return x_launch(connected_viterbi_kernel<RL>, blocks, kXBlock, lds, st, logb, offsets, n_utts, total_frames,
                        log_start, log_trans, log_exit, word_penalty, W, S, SP, bp, exit_idx, score);
      }))
    return rc;
  if (n_words || path_word || path_state || path_entry)
    return x_launch(connected_backtrace_kernel, (n_utts + kXBlock - 1) / kXBlock, kXBlock, 0, st, offsets, n_utts,
                    total_frames, SP, R, bp, exit_idx, score, n_words, path_word, path_state, path_entry);
  return 0;
}
