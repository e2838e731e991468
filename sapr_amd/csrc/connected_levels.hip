// Connected-word recognition with a known or bounded number of words on gfx950: level building over the word loop of
// connected_bigram.hip.  Next to (word, state) a path carries its level l = 0 .. L - 1, the index of the
// word it is in, and the recursion returns the best string of exactly k words for every k = 1 .. L in one pass.  CPU
// restatement, which is the definition: tests/_levels_ref.py.  The input logb[total_frames][R = W * SP] is what the
// three emission stages of connected.hip write; the language model is sapr_connected_bigram's.
//
// connected_levels_kernel<RL, SP, LT>: the lane layout of connected_lanes.h over the flat states, the transition table
// by source and the transposed lm in LDS as in the bigram decoder (written out in the kernel: it keeps the text it was
// timed with, and takes the constants, the X step and the host side from the header) — with delta of all L <= LT levels in registers,
// LT * RL doubles per lane.  Row t of logb is read once and serves every level; inside the distance loop one tab read
// and one lane-address computation serve L candidates, and the L dependent chains of a frame (one per level: they do
// not read each other) fill each other's latency.  Level l needs its own old delta and N_{t-1}(l,.) alone, so the
// update is in place.  The three hand-overs through per-wavefront LDS rows are made for all levels together, three
// wave_lds_sync per frame:
//   1. every lane writes delta(l) + log_exit to cbuf[l][r];
//   2. the L * W (level, word) pairs are spread over the lanes in ceil(L W / 64) passes: pair p = l * W + v takes the
//      first maximum over the SP values of word v on level l and writes X(l,v) to xbuf[l][v], the state to the workspace;
//   3. pair p = l * W + w, l >= 1, takes the first maximum over v ascending of xbuf[l - 1][v] + lm[v][w] and writes
//      N(l,w) to nbuf[l][w], the predecessor word to the workspace; nbuf[0][.] stays -inf.  The state lanes read the N
//      of their own word from nbuf when the next frame compares it.
// Workspace: per (frame, level) what the bigram decoder keeps per frame — one back-pointer byte per flat state
// (kXEntry where the entry won), one byte per word for the state that attained X, one for the word that attained N —
// and one int32 per (utterance, level), the word that attained level_score.  connected_levels_backtrace_kernel, one
// lane per utterance, selects the count and walks back; it may be launched any number of times over one workspace.
//
// The recursion is float64 adds and compares in the order of the definition: bit for bit the restatement.  No atomics;
// an utterance's outputs are a function of its own frames and the tables alone.  Non-finite values propagate, and every
// index used in the walk is clamped into its row.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kLvMaxL = 8;            // levels one wavefront holds

inline int lv_check_shape(int32_t W, int32_t S, int32_t L) {
  if (int rc = x_check_shape(W, S)) return rc;
  if (L < 1 || L > kLvMaxL)
    return fail(SAPR_ERR_UNSUPPORTED, "the level-building kernels serve L in 1..%d words; got L=%d", kLvMaxL, L);
  return 0;
}

// LDS in doubles.  Shared by the workgroup: tab[SP][64 RL], lmt[W][W | 1], lm_end[W]; per wavefront: cbuf[L][64 RL],
// xbuf[L][W], nbuf[L][W]
constexpr size_t lv_shared_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W;
}
constexpr size_t lv_wave_doubles(int W, int RL, int L) { return static_cast<size_t>(L) * (kWave * RL + 2 * W); }

// the workspace of sapr_connected_levels_workspace_bytes, cut up
struct LvWorkspace {
  uint8_t *bp;    // [total_frames][L][R]
  uint8_t *xarg;  // [total_frames][L][W]
  uint8_t *warg;  // [total_frames][L][W]
  int32_t *fin;   // [n_utts][L]
};

inline LvWorkspace lv_cut(void *workspace, int64_t total_frames, int32_t W, int32_t SP, int32_t L) {
  const size_t rows = static_cast<size_t>(total_frames) * static_cast<size_t>(L);
  LvWorkspace ws;
  ws.bp = static_cast<uint8_t *>(workspace);
  ws.xarg = ws.bp + x_align16(rows * static_cast<size_t>(W) * static_cast<size_t>(SP));
  ws.warg = ws.xarg + x_align16(rows * static_cast<size_t>(W));
  ws.fin = reinterpret_cast<int32_t *>(ws.warg + x_align16(rows * static_cast<size_t>(W)));
  return ws;
}

// levels that share one pass of the distance loop: four, two where a lane holds four states on eight levels
constexpr int lv_group(int RL, int LT) { return LT < 4 ? LT : (RL == 4 && LT == 8 ? 2 : 4); }

template <int RL, int SP, int LT>
__global__ __launch_bounds__(kXBlock) void connected_levels_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, int32_t L, uint8_t *__restrict__ bp, uint8_t *__restrict__ xarg, uint8_t *__restrict__ warg,
    int32_t *__restrict__ fin, double *__restrict__ level_score) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  constexpr int LG = lv_group(RL, LT);
  extern __shared__ double smem[];
  double *tab = smem;             // [SP][RP]: tab[i][r] = log_trans[w][i][s], the transition INTO flat state r from i
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  const int LW = L * W;           // (level, word) pairs
  double *lmt = tab + SP * RP;    // [W][LS]: lmt[w][v] = lm[v][w]
  double *lme = lmt + W * LS;     // [W]
  const int nthreads = blockDim.x;
  for (int n = threadIdx.x; n < SP * RP; n += nthreads) {
    const int i = n / RP, r = n - i * RP;
    const int w = r / SP, s = r - w * SP;
    double v = neg_inf();
    if (r < R && s < S && i < S) v = log_trans[(static_cast<int64_t>(w) * S + i) * S + s];
    tab[n] = v;
  }
  for (int n = threadIdx.x; n < W * W; n += nthreads) {  // (coalesced read of lm[v][w], strided write)
    const int v = n / W, w = n - v * W;
    lmt[w * LS + v] = lm[n];
  }
  for (int n = threadIdx.x; n < W; n += nthreads) lme[n] = lm_end[n];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cbuf = lme + W + wave * (L * (RP + 2 * W));  // [L][RP]: delta + log_exit of every flat state
  double *xbuf = cbuf + L * RP;                        // [L][W]: X(l,v), pair p = l * W + v at xbuf[p]
  double *nbuf = xbuf + LW;                            // [L][W]: N(l,w); row 0 stays -inf
  const int64_t u = static_cast<int64_t>(blockIdx.x) * (nthreads / kWave) + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  const int64_t T = end - beg;

  double ls[RL], ls0[RL], lx[RL], delta[LT][RL], bn[RL];
  int sk[RL], wk[RL];
  bool ok[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int r = k * kWave + lane;
    const int w = r / SP, s = r - w * SP;
    ok[k] = r < R;
    sk[k] = s;
    wk[k] = ok[k] ? w : 0;  // (a lane without a state reads word 0's row of nbuf: inside it)
    const bool real = ok[k] && s < S;
    ls[k] = real ? log_start[w * S + s] : neg_inf();
    ls0[k] = real ? lm_start[w] + ls[k] : neg_inf();
    lx[k] = real ? log_exit[w * S + s] : neg_inf();
#pragma unroll
    for (int l = 0; l < LT; ++l) delta[l][k] = neg_inf();
  }
  for (int p = lane; p < LW; p += kWave) nbuf[p] = neg_inf();
  // p / W for a (level, word) pair p = l * W + w < 8 * 64 as a multiply: exact while p * W < 65536
  const int winv = (65536 + W - 1) / W;
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
    {  // the next frame's row in flight under this frame's chains
      const int64_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
      for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[tn * R + k * kWave + lane] : neg_inf();
    }
    // the levels in groups of LG: one tab read per distance serves a group's candidates, and best / back live for one
    // group at a time
#pragma unroll
    for (int g = 0; g < LT; g += LG) {
      if (g >= L) continue;  // (uniform)
      double v[LG][RL];
      int back[LG][RL];
      if (t == 0) {  // only the first word begins at the first frame
#pragma unroll
        for (int j = 0; j < LG; ++j) {
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            v[j][k] = g + j == 0 ? ls0[k] : neg_inf();
            back[j][k] = kXEntry;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < LG; ++j) {
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            v[j][k] = neg_inf();
            back[j][k] = 0;
          }
        }
        // predecessors i ascending = distances descending; the first maximum stays (strict compare)
#pragma unroll 1
        for (int d = SP - 1; d > -SP; --d) {
          if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
          // flat state r - d: lane (lane - d) & 63 of register k, of k - 1 where lane < d, of k + 1 where
          // lane - d >= 64
          const int off = lane - d;
          const int src = off & (kWave - 1);
          double lt[RL];
          int pi[RL];
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            const int i = sk[k] - d;
            const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
            const double e = tab[(in ? i : 0) * RP + k * kWave + lane];
            lt[k] = in ? e : neg_inf();
            pi[k] = i;
          }
#pragma unroll
          for (int j = 0; j < LG; ++j) {
            if (g + j < L) {  // (uniform)
              double rot[RL];
#pragma unroll
              for (int k = 0; k < RL; ++k) rot[k] = __shfl(delta[g + j][k], src, kWave);
#pragma unroll
              for (int k = 0; k < RL; ++k) {
                const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
                const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
                const double prev = off < 0 ? below : (off >= kWave ? above : rot[k]);
                const double c = prev + lt[k];
                const bool take = c > v[j][k];
                v[j][k] = take ? c : v[j][k];
                back[j][k] = take ? pi[k] : back[j][k];
              }
            }
          }
        }
        // the entry into the (l + 1)-th word: N_{t-1}(l, w) of the lane's own word; the first word is never entered
        // here
#pragma unroll
        for (int j = 0; j < LG; ++j) {
          if (g + j > 0 && g + j < L) {  // (uniform)
#pragma unroll
            for (int k = 0; k < RL; ++k) {
              const double entry = nbuf[(g + j) * W + wk[k]] + ls[k];
              const bool take = entry > v[j][k];
              v[j][k] = take ? entry : v[j][k];
              back[j][k] = take ? kXEntry : back[j][k];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < LG; ++j) {
        if (g + j < L) {  // (uniform)
          uint8_t *__restrict__ bprow = bp + ((beg + t) * L + (g + j)) * R;
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            delta[g + j][k] = v[j][k] + b[k];
            if (ok[k]) {
              bprow[k * kWave + lane] = static_cast<uint8_t>(back[j][k]);
              cbuf[(g + j) * RP + k * kWave + lane] = delta[g + j][k] + lx[k];
            }
          }
        }
      }
    }
    wave_lds_sync();
    uint8_t *__restrict__ xrow = xarg + (beg + t) * LW;
    uint8_t *__restrict__ wrow = warg + (beg + t) * LW;
#pragma unroll 1
    for (int p = lane; p < LW; p += kWave) {  // X(l,v): the first maximum over the word's states, s ascending
      const int l = (p * winv) >> 16, w = p - l * W;
      int xs;
      const double xv = x_first_max<SP>(cbuf + l * RP + w * SP, &xs);
      xbuf[p] = xv;
      xrow[p] = static_cast<uint8_t>(xs);
    }
    wave_lds_sync();
#pragma unroll 1
    for (int p = lane; p < LW; p += kWave) {  // N(l,w): the first maximum over the predecessor words, v ascending
      const int l = (p * winv) >> 16, w = p - l * W;
      int nw = 0;
      if (l > 0) {
        const double *__restrict__ row = lmt + w * LS;
        const double *__restrict__ x = xbuf + (l - 1) * W;
        double nv = x[0] + row[0];
#pragma unroll 4
        for (int q = 1; q < W; ++q) {
          const double c = x[q] + row[q];
          const bool take = c > nv;
          nv = take ? c : nv;
          nw = take ? q : nw;
        }
        nbuf[p] = nv;
      }
      wrow[p] = static_cast<uint8_t>(nw);
    }
    wave_lds_sync();
  }
  if (lane < L) {  // level_score[l] = max_v (X_{T-1}(l,v) + lm_end[v]), v ascending, the first maximum
    double sc = neg_inf();
    int fw = 0;
    if (T > 0) {
      const double *__restrict__ x = xbuf + lane * W;
      sc = x[0] + lme[0];
      for (int p = 1; p < W; ++p) {
        const double c = x[p] + lme[p];
        const bool take = c > sc;
        sc = take ? c : sc;
        fw = take ? p : fw;
      }
    }
    level_score[u * L + lane] = sc;
    fin[u * L + lane] = fw;
  }
}

// one lane per utterance selects the count k in lo .. hi — from lo, a later k only where its score is strictly
// greater — and walks back from level k - 1: the last word's best exit at the last frame, down one level at every entry
__global__ __launch_bounds__(kXBlock) void connected_levels_backtrace_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W, int32_t SP, int32_t L,
    const uint8_t *__restrict__ bp, const uint8_t *__restrict__ xarg, const uint8_t *__restrict__ warg,
    const int32_t *__restrict__ fin, const double *__restrict__ level_score, const int32_t *__restrict__ count_lo,
    const int32_t *__restrict__ count_hi, double *__restrict__ score, int32_t *__restrict__ n_words,
    int32_t *__restrict__ path_word, int32_t *__restrict__ path_state, uint8_t *__restrict__ path_entry) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (u >= n_utts) return;
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  int lo = count_lo ? count_lo[u] : 1, hi = count_hi ? count_hi[u] : L;
  const bool none = lo > hi;  // an empty range selects nothing
  lo = lo < 1 ? 1 : (lo > L ? L : lo);
  hi = hi < 1 ? 1 : (hi > L ? L : hi);
  int k = lo;
  double sc = neg_inf();
  if (!none && T > 0) {
    sc = level_score[u * L + lo - 1];
    for (int c = lo + 1; c <= hi; ++c) {
      const double other = level_score[u * L + c - 1];
      const bool take = other > sc;
      sc = take ? other : sc;
      k = take ? c : k;
    }
  }
  score[u] = sc;
  if (!finite_f64(sc)) {
    x_no_path(beg, T, path_word, path_state, path_entry);
    if (n_words) n_words[u] = 0;
    return;
  }
  const int64_t R = static_cast<int64_t>(W) * SP;
  int l = k - 1;
  int w = fin[u * L + l];
  w = (w >= 0 && w < W) ? w : 0;
  int s = xarg[((beg + T - 1) * L + l) * W + w];
  s = s < SP ? s : 0;
  for (int64_t t = T - 1; t >= 0; --t) {
    if (path_word) path_word[beg + t] = w;
    if (path_state) path_state[beg + t] = s;
    const int b = bp[((beg + t) * L + l) * R + w * SP + s];
    const bool entry = t == 0 || b == kXEntry;
    if (path_entry) path_entry[beg + t] = entry ? 1 : 0;
    if (entry) {
      if (t > 0) {
        w = warg[((beg + t - 1) * L + l) * W + w];
        w = w < W ? w : 0;
        l = l > 0 ? l - 1 : 0;
        s = xarg[((beg + t - 1) * L + l) * W + w];
        s = s < SP ? s : 0;
      }
    } else {
      s = b < SP ? b : 0;
    }
  }
  if (n_words) n_words[u] = k;
}

struct LvArgs {
  const double *logb;
  const int64_t *offsets;
  int64_t n_utts, total_frames;
  const double *log_start, *log_trans, *log_exit, *lm, *lm_start, *lm_end;
  int32_t W, S, L;
  LvWorkspace ws;
  double *level_score;
};

template <int RL, int SP, int LT>
int launch_levels(const LvArgs &a, hipStream_t stream) {
  size_t lds = 0;
  const int waves = x_waves(lv_shared_doubles(a.W, SP, RL) * sizeof(double),
                            lv_wave_doubles(a.W, RL, a.L) * sizeof(double), &lds);
  if (lds > static_cast<size_t>(kXLdsMax))
    return fail(SAPR_ERR_UNSUPPORTED, "the level-building kernel needs %zu bytes of LDS, the device offers %d", lds,
                kXLdsMax);
  return x_launch(connected_levels_kernel<RL, SP, LT>, (a.n_utts + waves - 1) / waves, waves * kWave, lds, stream,
                  a.logb, a.offsets, a.n_utts, a.total_frames, a.log_start, a.log_trans, a.log_exit, a.lm, a.lm_start,
                  a.lm_end, a.W, a.S, a.L, a.ws.bp, a.ws.xarg, a.ws.warg, a.ws.fin, a.level_score);
}

template <int RL, int SP>
int launch_levels_lt(const LvArgs &a, hipStream_t stream) {
  if (a.L <= 1) return launch_levels<RL, SP, 1>(a, stream);
  if (a.L <= 2) return launch_levels<RL, SP, 2>(a, stream);
  if (a.L <= 4) return launch_levels<RL, SP, 4>(a, stream);
  return launch_levels<RL, SP, 8>(a, stream);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_levels_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                     int32_t L, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  if (int rc = lv_check_shape(W, S, L)) return rc;
  const size_t R = static_cast<size_t>(W) * sp_of(S);
  const size_t rows = static_cast<size_t>(total_frames) * static_cast<size_t>(L);
  // per (frame, level): back-pointers [R] bytes, the exit state and the predecessor word of every word; per
  // (utterance, level) the final word (int32); each array padded to 16
  *bytes = x_align16(rows * R) + 2 * x_align16(rows * static_cast<size_t>(W)) +
           x_align16(static_cast<size_t>(n_utts) * static_cast<size_t>(L) * sizeof(int32_t));
  return 0;
}

extern "C" int sapr_connected_levels(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                     const double *log_start, const double *log_trans, const double *log_exit,
                                     const double *lm, const double *lm_start, const double *lm_end, int32_t W,
                                     int32_t S, int32_t L, void *workspace, size_t workspace_bytes,
                                     double *level_score, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = lv_check_shape(W, S, L)) return rc;
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_levels_workspace_bytes(total_frames, n_utts, W, S, L, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  SAPR_REQUIRE(n_utts <= 0x7fffffffLL, "grid too large (%lld utterances)", (long long)n_utts);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && level_score && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  const LvArgs a{logb,     offsets, n_utts, total_frames, log_start, log_trans, log_exit,
                 lm,       lm_start, lm_end, W,           S,         L,         lv_cut(workspace, total_frames, W, SP, L),
                 level_score};
  hipStream_t st = as_stream(stream);
  return x_dispatch(SP, R, [&](auto rl, auto sp) {
    return launch_levels_lt<decltype(rl)::value, decltype(sp)::value>(a, st);
  });
}

extern "C" int sapr_connected_levels_backtrace(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W,
                                               int32_t S, int32_t L, void *workspace, size_t workspace_bytes,
                                               const double *level_score, const int32_t *count_lo,
                                               const int32_t *count_hi, double *score, int32_t *n_words,
                                               int32_t *path_word, int32_t *path_state, uint8_t *path_entry,
                                               void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = lv_check_shape(W, S, L)) return rc;
  size_t need = 0;
  if (int rc = sapr_connected_levels_workspace_bytes(total_frames, n_utts, W, S, L, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXBlock - 1) / kXBlock;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && level_score && score, "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const LvWorkspace ws = lv_cut(workspace, total_frames, W, SP, L);
  return x_launch(connected_levels_backtrace_kernel, blocks, kXBlock, 0, as_stream(stream), offsets, n_utts,
                  total_frames, W, SP, L, ws.bp, ws.xarg, ws.warg, ws.fin, level_score, count_lo, count_hi, score,
                  n_words, path_word, path_state, path_entry);
}
