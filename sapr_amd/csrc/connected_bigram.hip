// Connected-word recognition under a word-pair language model on gfx950: one-pass Viterbi over the word loop in which
// the step from word v to word w costs lm[v][w], the first word lm_start[w] and the last word lm_end[v].
// -inf forbids a pair, a first or a last word: a finite-state word-pair grammar is a table of 0.0 and -inf.  CPU
// restatement, which is the definition: tests/_bigram_ref.py.  The input logb[total_frames][R = W * SP] is what the
// three emission stages of connected.hip write; this unit knows nothing about the emission family.
//
// connected_bigram_kernel<RL, SP>: one wavefront serves one utterance, four utterances per workgroup.  The R flat states
// lie along the lanes, RL in {1, 2, 4} per lane, exactly as in connected_viterbi_kernel: flat state r = k * 64 + lane
// sits in register k, row t of logb is RL coalesced reads with the next row in flight, the transition table
// tab[i][r] is shared in LDS, and the within-word predecessor at distance d = j - i comes by ds_bpermute, only at the
// distances at which some transition of the vocabulary is finite.  What differs from the word loop is the coupling:
// the entry score is per word, N_{t-1}(w) = max_v (X_{t-1}(v) + lm[v][w]), so the wave-wide butterfly over
// (value, flat index) is replaced by three steps through per-wavefront LDS rows:
//   1. every lane writes delta + log_exit to cbuf[r];
//   2. lane v < W takes the first maximum over the SP values of word v (s ascending) and writes X(v) to xbuf[v] and the
//      state that attained it to the workspace;
//   3. lane w < W takes the first maximum over v ascending of xbuf[v] + lm[v][w] and writes N(w) to nbuf[w] and the
//      predecessor word to the workspace; every state lane then reads back the N of its own word.
// lm lies transposed in LDS, lmt[w][v] in rows of an odd stride (W | 1 doubles), so that the W lanes of step 3 read W
// different banks while xbuf[v] is a broadcast; lm_end lies behind it.  A wavefront's LDS operations complete in
// order (wave_lds_sync, as in connected_align.hip): the frame loop has no workgroup barrier.
// Workspace: back-pointers, one byte per (frame, flat state) — the predecessor state, or kBgEntry where the entry won;
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

constexpr int kBgMaxR = 256;          // flat states one wavefront holds
constexpr int kBgBlock = 256;         // 4 wavefronts per workgroup
constexpr int kBgWaves = kBgBlock / kWave;
constexpr int kBgEntry = 255;         // back-pointer byte: the word was entered at this frame (connected.hip kEntry)

inline int bg_check_shape(int32_t W, int32_t S) {
  if (S > kMaxS || static_cast<int64_t>(W) * sp_of(S) > kBgMaxR)
    return fail(SAPR_ERR_UNSUPPORTED, "the connected-word kernels serve S in 1..%d and W * SP <= %d; got W=%d S=%d",
                kMaxS, kBgMaxR, W, S);
  return 0;
}

inline size_t bg_align16(size_t x) { return (x + 15) / 16 * 16; }

constexpr int bg_lm_stride(int W) { return W | 1; }  // doubles per row of the transposed lm in LDS

// LDS of one workgroup in doubles: tab[SP][64 RL], lmt[W][W | 1], lm_end[W], then per wavefront cbuf[64 RL], xbuf[64],
// nbuf[64]
constexpr size_t bg_lds_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * bg_lm_stride(W) + W +
         static_cast<size_t>(kBgWaves) * (kWave * RL + 2 * kWave);
}

// between the lanes of ONE wavefront: what the lanes wrote to LDS before is what they read after (connected_align.hip)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int RL, int SP>
__global__ __launch_bounds__(kBgBlock) void connected_bigram_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, uint8_t *__restrict__ bp, uint8_t *__restrict__ xarg, uint8_t *__restrict__ warg,
    int32_t *__restrict__ fin, double *__restrict__ score) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  extern __shared__ double smem[];
  double *tab = smem;             // [SP][RP]: tab[i][r] = log_trans[w][i][s], the transition INTO flat state r from i
  const int R = W * SP;
  const int LS = bg_lm_stride(W);
  double *lmt = tab + SP * RP;    // [W][LS]: lmt[w][v] = lm[v][w]
  double *lme = lmt + W * LS;     // [W]
  for (int n = threadIdx.x; n < SP * RP; n += kBgBlock) {
    const int i = n / RP, r = n - i * RP;
    const int w = r / SP, s = r - w * SP;
    double v = neg_inf();
    if (r < R && s < S && i < S) v = log_trans[(static_cast<int64_t>(w) * S + i) * S + s];
    tab[n] = v;
  }
  for (int n = threadIdx.x; n < W * W; n += kBgBlock) {  // (coalesced read of lm[v][w], strided write)
    const int v = n / W, w = n - v * W;
    lmt[w * LS + v] = lm[n];
  }
  for (int n = threadIdx.x; n < W; n += kBgBlock) lme[n] = lm_end[n];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cbuf = lme + W + wave * (RP + 2 * kWave);  // [RP]: delta + log_exit of every flat state
  double *xbuf = cbuf + RP;                          // [64]: X(v)
  double *nbuf = xbuf + kWave;                       // [64]: N(w)
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kBgWaves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  const int64_t T = end - beg;

  double ls[RL], ls0[RL], lx[RL], delta[RL], bn[RL], ne[RL];
  int sk[RL], wk[RL];
  bool ok[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int r = k * kWave + lane;
    const int w = r / SP, s = r - w * SP;  // (w <= 255 / SP <= 63: inside nbuf)
    ok[k] = r < R;
    sk[k] = s;
    wk[k] = w;
    const bool real = ok[k] && s < S;
    ls[k] = real ? log_start[w * S + s] : neg_inf();
    ls0[k] = real ? lm_start[w] + ls[k] : neg_inf();
    lx[k] = real ? log_exit[w * S + s] : neg_inf();
    delta[k] = neg_inf();
    ne[k] = neg_inf();
  }
  nbuf[lane] = neg_inf();
  // the distances d = j - i in -(SP - 1) .. SP - 1 at which some transition of the vocabulary is finite
  // (wavefront-uniform; bit d + SP - 1)
  uint64_t dmask = 0;
#pragma unroll 1
  for (int d = 1 - SP; d < SP; ++d) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      const int i = sk[k] - d;
      const bool in = i >= 0 && i < SP;
      any |= in && !(tab[(in ? i : 0) * RP + k * kWave + lane] == neg_inf());
    }
    if (__ballot(any)) dmask |= 1ull << (d + SP - 1);
  }
  dmask = (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<unsigned>(dmask >> 32))) << 32) |
          __builtin_amdgcn_readfirstlane(static_cast<unsigned>(dmask));

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
        back[k] = kBgEntry;
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
        if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
        // flat state r - d: lane (lane - d) & 63 of register k, of k - 1 where lane < d, of k + 1 where lane - d >= 64
        const int off = lane - d;
        const int src = off & (kWave - 1);
        double rot[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) rot[k] = __shfl(delta[k], src, kWave);
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
          const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
          const double prev = off < 0 ? below : (off >= kWave ? above : rot[k]);
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[(in ? i : 0) * RP + k * kWave + lane];
          const double c = prev + (in ? lt : neg_inf());
          const bool take = c > best[k];
          best[k] = take ? c : best[k];
          back[k] = take ? i : back[k];
        }
      }
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double entry = ne[k] + ls[k];
        const bool take = entry > best[k];
        v[k] = take ? entry : best[k];
        back[k] = take ? kBgEntry : back[k];
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
      double c[SP];
#pragma unroll
      for (int s = 0; s < SP; ++s) c[s] = cbuf[lane * SP + s];
      double xv = c[0];
      int xs = 0;
#pragma unroll
      for (int s = 1; s < SP; ++s) {
        const bool take = c[s] > xv;
        xv = take ? c[s] : xv;
        xs = take ? s : xs;
      }
      xbuf[lane] = xv;
      xarg[(beg + t) * W + lane] = static_cast<uint8_t>(xs);
    }
    wave_lds_sync();
    if (lane < W) {  // N(w): the first maximum over the predecessor words, v ascending
      const double *__restrict__ row = lmt + lane * LS;
      double nv = xbuf[0] + row[0];
      int nw = 0;
#pragma unroll 4
      for (int p = 1; p < W; ++p) {
        const double c = xbuf[p] + row[p];
        const bool take = c > nv;
        nv = take ? c : nv;
        nw = take ? p : nw;
      }
      nbuf[lane] = nv;
      warg[(beg + t) * W + lane] = static_cast<uint8_t>(nw);
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < RL; ++k) ne[k] = nbuf[wk[k]];
  }
  if (lane == 0) {  // score = max_v (X_{T-1}(v) + lm_end[v]), v ascending, the first maximum
    double sc = neg_inf();
    int fw = 0;
    if (T > 0) {
      sc = xbuf[0] + lme[0];
      for (int p = 1; p < W; ++p) {
        const double c = xbuf[p] + lme[p];
        const bool take = c > sc;
        sc = take ? c : sc;
        fw = take ? p : fw;
      }
    }
    score[u] = sc;
    fin[u] = fw;
  }
}

// one lane per utterance walks back from the last word's best exit at the last frame
__global__ __launch_bounds__(kBgBlock) void connected_bigram_backtrace_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t SP,
    const uint8_t *__restrict__ bp, const uint8_t *__restrict__ xarg, const uint8_t *__restrict__ warg,
    const int32_t *__restrict__ fin, const double *__restrict__ score, int32_t *__restrict__ n_words,
    int32_t *__restrict__ path_word, int32_t *__restrict__ path_state, uint8_t *__restrict__ path_entry) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kBgBlock + threadIdx.x;
  if (u >= n_utts) return;
  const int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) {
    if (n_words) n_words[u] = 0;
    return;
  }
  const int64_t T = end - beg;
  const double sc = score[u];
  if (!(sc - sc == 0.0) || T == 0) {  // a non-finite score has no path
    for (int64_t t = 0; t < T; ++t) {
      if (path_word) path_word[beg + t] = -1;
      if (path_state) path_state[beg + t] = -1;
      if (path_entry) path_entry[beg + t] = 0;
    }
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
    const bool entry = t == 0 || b == kBgEntry;
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

template <int RL, int SP>
int launch_bigram(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                  const double *log_start, const double *log_trans, const double *log_exit, const double *lm,
                  const double *lm_start, const double *lm_end, int32_t W, int32_t S, uint8_t *bp, uint8_t *xarg,
                  uint8_t *warg, int32_t *fin, double *score, hipStream_t stream) {
  const size_t lds = bg_lds_doubles(W, SP, RL) * sizeof(double);
  const int64_t blocks = (n_utts + kBgWaves - 1) / kBgWaves;
  SAPR_LAUNCH((connected_bigram_kernel<RL, SP>), dim3(static_cast<unsigned>(blocks)), dim3(kBgBlock), lds, stream, logb,
              offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S, bp, xarg, warg,
              fin, score);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int SP, typename... Args>
int launch_bigram_rl(int R, Args... args) {
  if (R <= kWave) return launch_bigram<1, SP>(args...);
  if (R <= 2 * kWave) return launch_bigram<2, SP>(args...);
  return launch_bigram<4, SP>(args...);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_bigram_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                     size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  if (int rc = bg_check_shape(W, S)) return rc;
  const size_t R = static_cast<size_t>(W) * sp_of(S);
  // back-pointers [total_frames][R] bytes, the exit state and the predecessor word of every (frame, word), the final
  // word of every utterance (int32), each padded to 16
  *bytes = bg_align16(static_cast<size_t>(total_frames) * R) +
           2 * bg_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(W)) +
           bg_align16(static_cast<size_t>(n_utts) * sizeof(int32_t));
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
  if (int rc = bg_check_shape(W, S)) return rc;
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_bigram_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kBgWaves - 1) / kBgWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && score && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  const size_t frames = static_cast<size_t>(total_frames);
  uint8_t *bp = static_cast<uint8_t *>(workspace);
  uint8_t *xarg = bp + bg_align16(frames * static_cast<size_t>(R));
  uint8_t *warg = xarg + bg_align16(frames * static_cast<size_t>(W));
  int32_t *fin = reinterpret_cast<int32_t *>(warg + bg_align16(frames * static_cast<size_t>(W)));
  hipStream_t st = as_stream(stream);
  int rc;
  if (SP == 4)
    rc = launch_bigram_rl<4>(R, logb, offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start,
                             lm_end, W, S, bp, xarg, warg, fin, score, st);
  else if (SP == 10)
    rc = launch_bigram_rl<10>(R, logb, offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start,
                              lm_end, W, S, bp, xarg, warg, fin, score, st);
  else
    rc = launch_bigram_rl<18>(R, logb, offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start,
                              lm_end, W, S, bp, xarg, warg, fin, score, st);
  if (rc) return rc;
  if (n_words || path_word || path_state || path_entry) {
    SAPR_LAUNCH(connected_bigram_backtrace_kernel, dim3(static_cast<unsigned>((n_utts + kBgBlock - 1) / kBgBlock)),
                dim3(kBgBlock), 0, st, offsets, n_utts, total_frames, W, SP, bp, xarg, warg, fin, score, n_words,
                path_word, path_state, path_entry);
    SAPR_HIP_TRY(hipGetLastError());
  }
  return 0;
}
