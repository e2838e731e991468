// Connected-word recognition under a word-pair language model on gfx950: one-pass Viterbi over the word loop in which
// the step from word v to word w costs lm[v][w], the first word lm_start[w] and the last word lm_end[v].
// -inf forbids a pair, a first or a last word: a finite-state word-pair grammar is a table of 0.0 and -inf.  CPU
// restatement, which is the definition: tests/_bigram_ref.py.  The input logb[total_frames][R = W * SP] is what the
// three emission stages of connected.hip write; this unit knows nothing about the emission family.
//
// connected_bigram_kernel<RL, SP>: the lane layout of connected_lanes.h over the flat states, four utterances per
// workgroup, the transition table by source.  What is this unit's own is the coupling: the entry score is per word,
// N_{t-1}(w) = max_v (X_{t-1}(v) + lm[v][w]), in three steps through per-wavefront LDS rows:
//   1. every lane writes delta + log_exit to cbuf[r];
//   2. lane v < W takes the first maximum over the SP values of word v (s ascending) and writes X(v) to xbuf[v] and the
//      state that attained it to the workspace;
//   3. lane w < W takes the first maximum over v ascending of xbuf[v] + lm[v][w] and writes N(w) to nbuf[w] and the
//      predecessor word to the workspace; every state lane then reads back the N of its own word.
// lm lies transposed in LDS, lmt[w][v], with lm_end behind it.
// Workspace: back-pointers, one byte per (frame, flat state) — the predecessor state, or kXEntry where the entry won;
// one byte per (frame, word), the state that attained X_t(v); one byte per (frame, word), the word that attained
// N_t(w); one int32 per utterance, the word that attained the score.  connected_bigram_backtrace_kernel, one lane per
// utterance, walks back and writes path_word, path_state, path_entry, n_words.
//
// The recursion is float64 adds and compares in the order of the definition: bit for bit the restatement.  No atomics;
// an utterance's outputs are a function of its own frames and the network alone.  Non-finite values propagate, and
// every index used in the walk is clamped into its row.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

// LDS of one workgroup in doubles: tab[SP][64 RL], lmt[W][W | 1], lm_end[W], then per wavefront cbuf[64 RL], xbuf[64],
// nbuf[64]
constexpr size_t bg_lds_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W +
         static_cast<size_t>(kXWaves) * (kWave * RL + 2 * kWave);
}

template <int RL, int SP>
__global__ __launch_bounds__(kXBlock) void connected_bigram_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, uint8_t *__restrict__ bp, uint8_t *__restrict__ xarg, uint8_t *__restrict__ warg,
    int32_t *__restrict__ fin, double *__restrict__ score) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  extern __shared__ double smem[];
  double *tab = smem;             // [SP][RP] by source
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  double *lmt = tab + SP * RP;    // [W][LS]: lmt[w][v] = lm[v][w]
  double *lme = lmt + W * LS;     // [W]
  x_load_by_source(tab, log_trans, W, S, SP, RP, kXBlock);
  x_load_lm(lmt, lme, lm, lm_end, W, true, kXBlock);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cbuf = lme + W + wave * (RP + 2 * kWave);  // [RP]: delta + log_exit of every flat state
  double *xbuf = cbuf + RP;                          // [64]: X(v)
  double *nbuf = xbuf + kWave;                       // [64]: N(w)
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;

  double ls[RL], ls0[RL], lx[RL], delta[RL], bn[RL], ne[RL];
  int sk[RL], wk[RL];
  bool ok[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const XState x = x_flat_state(k * kWave + lane, R, SP, S, log_start, log_exit);
    ok[k] = x.ok;
    sk[k] = x.s;
    wk[k] = x.w;
    ls[k] = x.ls;
    lx[k] = x.lx;
    ls0[k] = x.real ? lm_start[x.w] + x.ls : neg_inf();
    delta[k] = neg_inf();
    ne[k] = neg_inf();
  }
  nbuf[lane] = neg_inf();
  const uint64_t dmask = x_mask_by_source<RL>(tab, sk, lane, SP);

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = (ok[k] && T > 0) ? brow[k * kWave + lane] : neg_inf();

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
        v[k] = ls0[k];
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
#pragma unroll 1
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
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double entry = ne[k] + ls[k];
        const bool take = entry > best[k];
        v[k] = take ? entry : best[k];
        back[k] = take ? kXEntry : back[k];
      }
    }
    uint8_t *__restrict__ bprow = bp + (beg + t) * R;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      delta[k] = v[k] + b[k];
      if (ok[k]) {
        bprow[k * kWave + lane] = static_cast<uint8_t>(back[k]);
        cbuf[k * kWave + lane] = delta[k] + lx[k];
      }
    }
    wave_lds_sync();
    if (lane < W) {  // X(v): the first maximum over the word's states, s ascending
      int xs;
      xbuf[lane] = x_first_max<SP>(cbuf + lane * SP, &xs);
      xarg[(beg + t) * W + lane] = static_cast<uint8_t>(xs);
    }
    wave_lds_sync();
    if (lane < W) {  // N(w): the first maximum over the predecessor words, v ascending
      int nw;
      nbuf[lane] = x_first_max_pair(xbuf, lmt + lane * LS, W, &nw);
      warg[(beg + t) * W + lane] = static_cast<uint8_t>(nw);
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < RL; ++k) ne[k] = nbuf[wk[k]];
  }
  if (lane == 0) {  // score = max_v (X_{T-1}(v) + lm_end[v]), v ascending, the first maximum
    int fw = 0;
    const double sc = T > 0 ? x_first_max_pair(xbuf, lme, W, &fw) : neg_inf();
    score[u] = sc;
    fin[u] = fw;
  }
}

// one lane per utterance walks back from the last word's best exit at the last frame
__global__ __launch_bounds__(kXBlock) void connected_bigram_backtrace_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t SP,
    const uint8_t *__restrict__ bp, const uint8_t *__restrict__ xarg, const uint8_t *__restrict__ warg,
    const int32_t *__restrict__ fin, const double *__restrict__ score, int32_t *__restrict__ n_words,
    int32_t *__restrict__ path_word, int32_t *__restrict__ path_state, uint8_t *__restrict__ path_entry) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (u >= n_utts) return;
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  if (!finite_f64(score[u]) || T == 0) {
    x_no_path(beg, T, path_word, path_state, path_entry);
    if (n_words) n_words[u] = 0;
    return;
  }
  const int64_t R = static_cast<int64_t>(W) * SP;
  int w = fin[u];
  w = (w >= 0 && w < W) ? w : 0;
  int s = xarg[(beg + T - 1) * W + w];
  s = s < SP ? s : 0;
  int nw = 0;
  for (int64_t t = T - 1; t >= 0; --t) {
    if (path_word) path_word[beg + t] = w;
    if (path_state) path_state[beg + t] = s;
    const int b = bp[(beg + t) * R + w * SP + s];
    const bool entry = t == 0 || b == kXEntry;
    if (path_entry) path_entry[beg + t] = entry ? 1 : 0;
    if (entry) {
      ++nw;
      if (t > 0) {
        w = warg[(beg + t - 1) * W + w];
        w = w < W ? w : 0;
        s = xarg[(beg + t - 1) * W + w];
        s = s < SP ? s : 0;
      }
    } else {
      s = b < SP ? b : 0;
    }
  }
  if (n_words) n_words[u] = nw;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_bigram_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                     size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  if (int rc = x_check_shape(W, S)) return rc;
  const size_t R = static_cast<size_t>(W) * sp_of(S);
  // back-pointers [total_frames][R] bytes, the exit state and the predecessor word of every (frame, word), the final
  // word of every utterance (int32), each padded to 16
  *bytes = x_align16(static_cast<size_t>(total_frames) * R) +
           2 * x_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(W)) +
           x_align16(static_cast<size_t>(n_utts) * sizeof(int32_t));
  return 0;
}

extern "C" int sapr_connected_bigram(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                     const double *log_start, const double *log_trans, const double *log_exit,
                                     const double *lm, const double *lm_start, const double *lm_end, int32_t W,
                                     int32_t S, void *workspace, size_t workspace_bytes, double *score,
                                     int32_t *n_words, int32_t *path_word, int32_t *path_state, uint8_t *path_entry,
                                     void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = x_check_shape(W, S)) return rc;
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_bigram_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && score && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  const size_t frames = static_cast<size_t>(total_frames);
  uint8_t *bp = static_cast<uint8_t *>(workspace);
  uint8_t *xarg = bp + x_align16(frames * static_cast<size_t>(R));
  uint8_t *warg = xarg + x_align16(frames * static_cast<size_t>(W));
  int32_t *fin = reinterpret_cast<int32_t *>(warg + x_align16(frames * static_cast<size_t>(W)));
  hipStream_t st = as_stream(stream);
  if (int rc = x_dispatch(SP, R, [&](auto rl, auto sp) {
        constexpr int RL = decltype(rl)::value, SPc = decltype(sp)::value;
        return x_launch(connected_bigram_kernel<RL, SPc>, blocks, kXBlock, bg_lds_doubles(W, SPc, RL) * sizeof(double),
                        st, logb, offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start, lm_end,
                        W, S, bp, xarg, warg, fin, score);
      }))
    return rc;
  if (n_words || path_word || path_state || path_entry)
    return x_launch(connected_bigram_backtrace_kernel, (n_utts + kXBlock - 1) / kXBlock, kXBlock, 0, st, offsets,
                    n_utts, total_frames, W, SP, bp, xarg, warg, fin, score, n_words, path_word, path_state,
                    path_entry);
  return 0;
}
