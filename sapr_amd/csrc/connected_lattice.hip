// Connected-word lattices on gfx950: one pass over the word loop of connected_bigram.hip leaves, for
// every (frame, word), the score X_t(w) of the best path that ends word w there, the entry score N_t(w) and the frame
// B_t(w) at which that path entered the word.  That table is a word lattice: it can be pruned to a beam around the best
// path and rescored under any other word-pair language model without touching the acoustics.  CPU restatement, which is
// the definition: tests/_lattice_ref.py (over tests/_bigram_ref.py).
//
// connected_lattice_kernel<RL, SP>: connected_bigram_kernel's mapping, LDS layout and per-frame coupling, plus one int32
// start frame per flat state in the lane's registers.  The integer moves with delta — a second cross-lane move per
// finite distance, selected by the same compare (x_rotate_tagged) — and takes the frame number where entry wins.  Lane
// w < W fetches the start frame of the state that attained X(w) from the lane that holds it (RL more cross-lane reads
// per frame; the LDS is the bigram kernel's to the byte) and writes X, N and B of its word per frame, 20 W bytes; no
// back-pointer, xarg or warg bytes.
//
// connected_lattice_backward_kernel: one wavefront per utterance, lane v owns column v of beta and next, so every global
// read-modify-write is private to a lane and nothing is handed between lanes through global memory.  For frame t' lane
// w' loads its own beta, X, in and tau and forms g; a wave-uniform loop over w' broadcasts (g, tau) by a cross-lane read
// and every lane v updates beta[tau - 1][v] against row v of lm' in LDS.  Lane-uniform registers keep root and first.
// The chain is global round trips: the read-only X, B and in are loaded a frame ahead, and the beta rows of four
// records are loaded together (a row that occurs twice among the four is handed on in registers), and the lane's own
// beta of the next frame is kept in a register beside the memory, so a frame costs ceil(W / 4) dependent round trips
// instead of 3 + W.
//
// connected_lattice_walk_kernel: one lane per utterance, from first along next; every index is clamped into its row.
//
// float64 adds, one subtract and strict compares in the order of the definition: bit for bit the restatement.  No
// atomics; an utterance's outputs are a function of its own frames and the tables alone.  Non-finite values propagate.
//
// Lattice posteriors (the definition is tests/_lattice_post_ref.py): forward-backward in the sum semiring
// over the same records under any tables and an acoustic scale.  lattice_post_forward_kernel and
// lattice_post_backward_kernel keep the backward kernel's mapping — one wavefront per utterance, lane w owning column w
// of alpha, Q, beta and H — and take one W x W log-sum-exp per frame (pair_lse, connected_lanes.h) where the
// max-semiring pass does W read-modify-writes; lattice_post_kernel, one lane per (utterance, word), forms record_post
// and word_post from two running sums per column.  These three match the restatement within the tolerances of the
// word loop's forward-backward, not bit for bit; every sum has a fixed order, so two calls return the same bytes.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kLNoWord = 255;  // next_word / first of a (frame, word) nothing follows
constexpr int kLChunk = 4;     // records the backward pass serves per global round trip

// LDS of one workgroup in doubles, as connected_bigram_kernel's: tab[SP][64 RL], lmt[W][W | 1], lm_end[W], then per
// wavefront cbuf[64 RL], xbuf[64], nbuf[64]
constexpr size_t lt_lds_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W +
         static_cast<size_t>(kXWaves) * (kWave * RL + 2 * kWave);
}

// the forward tables inside the workspace: X[total_frames][W] f64, N[total_frames][W] f64, B[total_frames][W] i32
struct LTables {
  double *X, *N;
  int32_t *B;
};

inline size_t lt_table_bytes(size_t frames, size_t W, size_t elem) { return x_align16(frames * W * elem); }

inline LTables lt_tables(void *workspace, int64_t total_frames, int32_t W) {
  const size_t f = static_cast<size_t>(total_frames), w = static_cast<size_t>(W);
  uint8_t *p = static_cast<uint8_t *>(workspace);
  LTables t;
  t.X = reinterpret_cast<double *>(p);
  t.N = reinterpret_cast<double *>(p + lt_table_bytes(f, w, 8));
  t.B = reinterpret_cast<int32_t *>(p + 2 * lt_table_bytes(f, w, 8));
  return t;
}

template <int RL, int SP>
__global__ __launch_bounds__(kXBlock) void connected_lattice_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, double *__restrict__ wend_score, double *__restrict__ wend_entry, int32_t *__restrict__ wend_start,
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
  int sk[RL], wk[RL], bs[RL];
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
    bs[k] = -1;
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
    int from[RL];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        v[k] = ls0[k];
        from[k] = 0;
      }
    } else {
      double best[RL];
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        best[k] = neg_inf();
        from[k] = -1;
      }
      // predecessors i ascending = distances descending; the first maximum stays (strict compare)
#pragma unroll 1
      for (int d = SP - 1; d > -SP; --d) {
        if (!x_live(dmask, d, SP)) continue;  // (uniform)
        x_rotate_tagged<RL>(delta, bs, lane, d, [=, &best, &from](int k, double prev, int start) {
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[(in ? i : 0) * RP + k * kWave + lane];
          const double c = prev + (in ? lt : neg_inf());
          const bool take = c > best[k];
          best[k] = take ? c : best[k];
          from[k] = take ? start : from[k];
        });
      }
      const int now = static_cast<int>(t);
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double entry = ne[k] + ls[k];
        const bool take = entry > best[k];
        v[k] = take ? entry : best[k];
        from[k] = take ? now : from[k];
      }
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      delta[k] = v[k] + b[k];
      bs[k] = from[k];
      if (ok[k]) cbuf[k * kWave + lane] = delta[k] + lx[k];
    }
    wave_lds_sync();
    double xv = neg_inf();
    int xs = 0;
    if (lane < W) {  // X(v): the first maximum over the word's states, s ascending
      xv = x_first_max<SP>(cbuf + lane * SP, &xs);
      xbuf[lane] = xv;
    }
    // ... and that state's start frame, from register r / 64 of lane r % 64 (every lane takes part in the read)
    const int xr = lane < W ? lane * SP + xs : 0;
    int xb = -1;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      const int got = __shfl(from[k], xr & (kWave - 1), kWave);
      xb = (xr >> 6) == k ? got : xb;
    }
    xb = xv > neg_inf() ? xb : -1;
    wave_lds_sync();
    if (lane < W) {  // N(w): the first maximum over the predecessor words, v ascending
      int nw;
      const double nv = x_first_max_pair(xbuf, lmt + lane * LS, W, &nw);
      nbuf[lane] = nv;
      const int64_t at = (beg + t) * W + lane;
      wend_score[at] = xv;
      wend_entry[at] = nv;
      wend_start[at] = xb;
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < RL; ++k) ne[k] = nbuf[wk[k]];
  }
  if (lane == 0) {  // score = max_v (X_{T-1}(v) + lm_end[v]), v ascending, the first maximum
    int fw = 0;
    const double sc = T > 0 ? x_first_max_pair(xbuf, lme, W, &fw) : neg_inf();
    score[u] = sc;
    if (fin) fin[u] = fw;
  }
}

__device__ __forceinline__ double lt_readlane(double v, int src) {  // lane src's value; src is wavefront-uniform
  const unsigned long long bits = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane(static_cast<unsigned>(bits), src);
  const unsigned hi = __builtin_amdgcn_readlane(static_cast<unsigned>(bits >> 32), src);
  return __longlong_as_double((static_cast<unsigned long long>(hi) << 32) | lo);
}

// LDS of one workgroup in doubles: lmx[W][W | 1] (lmx[v][w] = lm'[v][w]), lm_end'[W], lm_start'[W]
constexpr size_t lb_lds_doubles(int W) { return static_cast<size_t>(W) * x_lm_stride(W) + 2 * W; }

__global__ __launch_bounds__(kXBlock) void connected_lattice_backward_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W,
    const double *__restrict__ wend_score, const double *__restrict__ wend_entry,
    const int32_t *__restrict__ wend_start, const double *__restrict__ fwd_lm_start, const double *__restrict__ lm,
    const double *__restrict__ lm_start, const double *__restrict__ lm_end, double *beta, int32_t *next_end,
    uint8_t *next_word, double *__restrict__ root, int32_t *__restrict__ first) {
  extern __shared__ double smem[];
  const int LS = x_lm_stride(W);
  double *lmx = smem;           // [W][LS]: row v is what lane v reads
  double *lme = lmx + W * LS;   // [W]
  double *lms = lme + W;        // [W]
  x_load_lm(lmx, lme, lm, lm_end, W, false, kXBlock);
  for (int n = threadIdx.x; n < W; n += kXBlock) lms[n] = lm_start[n];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  const bool mine = lane < W;  // lane v owns column v of beta, next_end and next_word
  if (mine)
    for (int64_t t = 0; t < T; ++t) {
      const int64_t at = (beg + t) * W + lane;
      beta[at] = t == T - 1 ? lme[lane] : neg_inf();
      next_end[at] = -1;
      next_word[at] = static_cast<uint8_t>(kLNoWord);
    }
  const double in0 = mine ? fwd_lm_start[lane] : neg_inf();
  double rt = neg_inf();  // (every lane keeps the same root and first: they are formed from broadcast values)
  int fe = -1, fw = kLNoWord;
  // X, B and in of the lane's word are read-only here and loaded a frame ahead of the chain
  double xq = neg_inf(), inq = neg_inf();
  int bq = -1;
  double own = (mine && T > 0) ? lme[lane] : neg_inf();  // beta_t(lane) of the frame at hand, kept in a register
  if (mine && T > 0) {
    const int64_t at = (beg + T - 1) * W + lane;
    xq = wend_score[at];
    bq = wend_start[at];
    inq = bq == 0 ? in0 : (bq >= 1 && bq <= T - 1 ? wend_entry[(beg + bq - 1) * W + lane] : neg_inf());
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const double x = xq, in = inq;
    const int b = bq;
    // beta_{t-1}(lane) as the frames so far left it, in flight under this frame's chain; the records of this frame that
    // start at t (tau = t) update the register beside the memory, so the next frame begins without a round trip
    double prev = neg_inf();
    if (mine && t > 0) {
      const int64_t at = (beg + t - 1) * W + lane;
      xq = wend_score[at];
      bq = wend_start[at];
      prev = beta[at];
    }
    const int now_t = static_cast<int>(t);
    double g = neg_inf();
    int tau = -1;
    if (mine && x > neg_inf() && b >= 0 && b <= t) {  // a record; a tau outside 0 .. t' skips it
      g = (x - in) + own;
      tau = b;
    }
    // kLChunk records per global round trip: their beta rows are loaded together, and a row that occurs twice in a
    // chunk is handed on in registers (the compares on tau are wavefront-uniform)
#pragma unroll 1
    for (int w0 = 0; w0 < W; w0 += kLChunk) {
      int tw[kLChunk];
      double gw[kLChunk], cur[kLChunk];
#pragma unroll
      for (int j = 0; j < kLChunk; ++j) {
        const int w = w0 + j < W ? w0 + j : 0;
        tw[j] = w0 + j < W ? __builtin_amdgcn_readlane(tau, w) : -1;
        gw[j] = lt_readlane(g, w);
      }
#pragma unroll
      for (int j = 0; j < kLChunk; ++j)
        cur[j] = (mine && tw[j] > 0) ? beta[(beg + tw[j] - 1) * W + lane] : neg_inf();
#pragma unroll
      for (int j = 0; j < kLChunk; ++j) {
        const int w = w0 + j;
        if (tw[j] > 0) {
          if (mine) {
            const int64_t at = (beg + tw[j] - 1) * W + lane;
            const double c = lmx[lane * LS + w] + gw[j];
            const bool take = c > cur[j];
            if (take) {
              beta[at] = c;
              next_end[at] = static_cast<int32_t>(t);
              next_word[at] = static_cast<uint8_t>(w);
            }
            const double now = take ? c : cur[j];
#pragma unroll
            for (int i = j + 1; i < kLChunk; ++i) cur[i] = tw[i] == tw[j] ? now : cur[i];
            prev = tw[j] == now_t ? now : prev;
          }
        } else if (tw[j] == 0) {
          const double c = lms[w] + gw[j];
          if (c > rt) {
            rt = c;
            fe = static_cast<int>(t);
            fw = w;
          }
        }
      }
    }
    if (mine && t > 0)
      inq = bq == 0 ? in0 : (bq >= 1 && bq <= t - 1 ? wend_entry[(beg + bq - 1) * W + lane] : neg_inf());
    own = prev;
  }
  if (lane == 0) {
    root[u] = rt;
    first[2 * u] = fe;
    first[2 * u + 1] = fw;
  }
}

// one lane per utterance: from first along next until a record ends at T - 1
__global__ __launch_bounds__(kXBlock) void connected_lattice_walk_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W,
    const int32_t *__restrict__ next_end, const uint8_t *__restrict__ next_word, const double *__restrict__ root,
    const int32_t *__restrict__ first, int32_t *__restrict__ n_words, int32_t *__restrict__ path_word,
    uint8_t *__restrict__ path_entry) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (u >= n_utts) return;
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  if (!finite_f64(root[u]) || T == 0) {
    x_no_path(beg, T, path_word, nullptr, path_entry);
    if (n_words) n_words[u] = 0;
    return;
  }
  int64_t e = first[2 * u];
  e = e < 0 ? 0 : (e > T - 1 ? T - 1 : e);
  int w = first[2 * u + 1];
  w = (w >= 0 && w < W) ? w : 0;
  int64_t a = 0;
  int nw = 0;
  for (;;) {  // (e grows by at least one per step: at most T steps)
    for (int64_t t = a; t <= e; ++t) {
      if (path_word) path_word[beg + t] = w;
      if (path_entry) path_entry[beg + t] = t == a ? 1 : 0;
    }
    ++nw;
    if (e >= T - 1) break;
    a = e + 1;
    const int64_t at = (beg + a - 1) * W + w;
    const int64_t ne = next_end[at];
    const int nx = next_word[at];
    e = ne < a ? a : (ne > T - 1 ? T - 1 : ne);  // clamped into (t, T - 1]
    w = nx < W ? nx : 0;
  }
  if (n_words) n_words[u] = nw;
}

// ---- lattice posteriors: forward-backward in the sum semiring over the records ------------------------
// LDS of one workgroup in doubles: lm'[W][W | 1] (transposed forward, row-major backward), lm_end'[W], lm_start'[W];
// per wavefront xbuf[64], mbuf[64] and the exponentials of pair_lse, ebuf[W][W | 1] — 33 KB at W = 64, where three
// wavefronts share a workgroup (x_waves)
constexpr size_t lp_shared_doubles(int W) { return static_cast<size_t>(W) * x_lm_stride(W) + 2 * W; }
constexpr size_t lp_wave_doubles(int W) { return 2 * kWave + static_cast<size_t>(W) * x_lm_stride(W); }

// the scratch of the posteriors: alpha, Q, beta and H, each [total_frames][W] f64
struct LpTables {
  double *alpha, *Q, *beta, *H;
};

inline LpTables lp_tables(void *workspace, int64_t total_frames, int32_t W) {
  const size_t one = lt_table_bytes(static_cast<size_t>(total_frames), static_cast<size_t>(W), 8);
  uint8_t *p = static_cast<uint8_t *>(workspace);
  LpTables t;
  t.alpha = reinterpret_cast<double *>(p);
  t.Q = reinterpret_cast<double *>(p + one);
  t.beta = reinterpret_cast<double *>(p + 2 * one);
  t.H = reinterpret_cast<double *>(p + 3 * one);
  return t;
}

// what lane w's record at frame t brings into either pass: a = kappa * ac and its start frame; tau = -1 without one
// (X not above -inf, a start outside 0 .. t, or keep == 0).  t lies inside the utterance and lane < W.
struct LpRecord {
  double a;
  int tau;
};

__device__ __forceinline__ LpRecord lp_record(const double *__restrict__ X, const double *__restrict__ N,
                                              const int32_t *__restrict__ B, const uint8_t *__restrict__ keep,
                                              int64_t beg, int64_t t, int W, int lane, double in0, double kappa) {
  const int64_t at = (beg + t) * W + lane;
  const double x = X[at];
  const int b = B[at];
  const bool kept = keep ? keep[at] != 0 : true;
  LpRecord r;
  r.a = neg_inf();
  r.tau = -1;
  if (x > neg_inf() && b >= 0 && b <= t && kept) {
    const double in = b == 0 ? in0 : N[(beg + b - 1) * W + lane];
    r.a = kappa * (x - in);
    r.tau = b;
  }
  return r;
}

// Forward: lane w forms alpha_t(w) = a + Q_{tau-1}(w) from its own column of Q — written frames ago by this very lane,
// loaded a frame ahead; Q_{t-1} is handed on in a register — and the wavefront takes Q_t = the W x W log-sum-exp of
// alpha_t against lm'.  It also leaves H = -inf for the backward pass and loglik[u].
__global__ __launch_bounds__(kXBlock) void lattice_post_forward_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W,
    const double *__restrict__ wend_score, const double *__restrict__ wend_entry,
    const int32_t *__restrict__ wend_start, const double *__restrict__ fwd_lm_start, const double *__restrict__ lm,
    const double *__restrict__ lm_start, const double *__restrict__ lm_end, double kappa,
    const uint8_t *__restrict__ keep, double *__restrict__ alpha, double *Q, double *__restrict__ H,
    double *__restrict__ loglik) {
  extern __shared__ double smem[];
  const int LS = x_lm_stride(W);
  double *lmt = smem;           // [W][LS]: lmt[w][v] = lm'[v][w]
  double *lme = lmt + W * LS;   // [W]
  double *lms = lme + W;        // [W]
  x_load_lm(lmt, lme, lm, lm_end, W, true, blockDim.x);
  for (int n = threadIdx.x; n < W; n += blockDim.x) lms[n] = lm_start[n];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  double *xbuf = lms + W + static_cast<size_t>(wave) * lp_wave_doubles(W);  // [64]: alpha_t(v)
  double *mbuf = xbuf + kWave;                                              // [64]: the maxima
  double *ebuf = mbuf + kWave;                                              // [W][LS]
  const int64_t u = static_cast<int64_t>(blockIdx.x) * waves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  if (T == 0) {
    if (lane == 0) loglik[u] = neg_inf();
    return;
  }
  const bool mine = lane < W;  // lane w owns column w of alpha, Q and H
  const double in0 = mine ? fwd_lm_start[lane] : neg_inf();
  const double q0 = mine ? lms[lane] : neg_inf();
  LpRecord nx;
  nx.a = neg_inf();
  nx.tau = -1;
  if (mine) nx = lp_record(wend_score, wend_entry, wend_start, keep, beg, 0, W, lane, in0, kappa);
  double qn = q0;             // what the next record starts from, where it is in memory already
  double qlast = neg_inf();   // Q_{t-1}(lane)
  for (int64_t t = 0; t < T; ++t) {
    const LpRecord rc = nx;
    const double qp = (rc.tau > 0 && rc.tau == t) ? qlast : qn;
    if (mine && t + 1 < T) {  // the next frame's record in flight under this frame's chain
      nx = lp_record(wend_score, wend_entry, wend_start, keep, beg, t + 1, W, lane, in0, kappa);
      // (tau = t + 1 starts from Q_t, which this frame forms: the register)
      qn = nx.tau == 0 ? q0 : ((nx.tau > 0 && nx.tau <= t) ? Q[(beg + nx.tau - 1) * W + lane] : neg_inf());
    }
    const double al = rc.tau >= 0 ? rc.a + qp : neg_inf();
    const int64_t at = (beg + t) * W + lane;
    if (mine) {
      alpha[at] = al;
      H[at] = neg_inf();
    }
    xbuf[lane] = al;
    wave_lds_sync();
    if (t + 1 < T) {  // (uniform) Q_t(w) on lane w; nothing starts behind the last frame
      const double qv = pair_lse(lmt, xbuf, mbuf, ebuf, lane, W, LS);
      if (mine) Q[at] = qv;
      qlast = qv;
    }
  }
  if (lane == 0) {  // loglik = lse_w (alpha_{T-1}(w) + lm_end'[w]), w ascending
    double m = xbuf[0] + lme[0];
    for (int p = 1; p < W; ++p) {
      const double c = xbuf[p] + lme[p];
      m = c > m ? c : m;
    }
    double ll = m;
    if (!isinf(m)) {
      double acc = 0.0;
      for (int p = 0; p < W; ++p) acc += exp_unit((xbuf[p] + lme[p]) - m);
      ll = log(acc) + m;
    }
    loglik[u] = ll;
  }
}

// Backward: beta_t = the W x W log-sum-exp of H_{t+1} against the rows of lm' (lm_end' at the last frame); lane w then
// folds g = a + beta_t(w) into H[tau][w] with one lse2.  The row it folds into and the lane's own H_t are loaded
// before pair_lse, the next frame's record with them; H_t is kept in a register beside the memory.
__global__ __launch_bounds__(kXBlock) void lattice_post_backward_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W,
    const double *__restrict__ wend_score, const double *__restrict__ wend_entry,
    const int32_t *__restrict__ wend_start, const double *__restrict__ fwd_lm_start, const double *__restrict__ lm,
    const double *__restrict__ lm_end, double kappa, const uint8_t *__restrict__ keep, double *__restrict__ beta,
    double *H) {
  extern __shared__ double smem[];
  const int LS = x_lm_stride(W);
  double *lmx = smem;           // [W][LS]: row v is what lane v reads
  double *lme = lmx + W * LS;   // [W]
  x_load_lm(lmx, lme, lm, lm_end, W, false, blockDim.x);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  double *xbuf = lme + 2 * W + static_cast<size_t>(wave) * lp_wave_doubles(W);  // [64]: H_{t+1}(w)
  double *mbuf = xbuf + kWave;
  double *ebuf = mbuf + kWave;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * waves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  if (T == 0) return;
  const bool mine = lane < W;  // lane w owns column w of beta and H
  const double in0 = mine ? fwd_lm_start[lane] : neg_inf();
  LpRecord nx;
  nx.a = neg_inf();
  nx.tau = -1;
  if (mine) nx = lp_record(wend_score, wend_entry, wend_start, keep, beg, T - 1, W, lane, in0, kappa);
  double hn = neg_inf();  // H_{t+1}(lane), complete: every record that starts at t + 1 ends there or later
  for (int64_t t = T - 1; t >= 0; --t) {
    const LpRecord rc = nx;
    const int64_t at = (beg + t) * W + lane;
    const int64_t to = (beg + (rc.tau >= 0 ? rc.tau : 0)) * W + lane;
    double hs = neg_inf(), cur = neg_inf();
    if (mine) {
      hs = H[at];
      if (rc.tau >= 0) cur = H[to];
    }
    if (mine && t > 0) nx = lp_record(wend_score, wend_entry, wend_start, keep, beg, t - 1, W, lane, in0, kappa);
    double bv;
    if (t == T - 1) {  // (uniform)
      bv = mine ? lme[lane] : neg_inf();
    } else {
      xbuf[lane] = hn;
      wave_lds_sync();
      bv = pair_lse(lmx, xbuf, mbuf, ebuf, lane, W, LS);
    }
    if (mine) {
      beta[at] = bv;
      if (rc.tau >= 0) {
        const double now = lse2(cur, rc.a + bv);
        H[to] = now;
        hs = rc.tau == t ? now : hs;
      }
    }
    hn = hs;
  }
}

// The posterior pass: one lane per (utterance, word), f ascending.  The mass of word w that has started at or before
// f needs no walk over records: the records of w that start at tau share Q_{tau-1}(w), so their posteriors add up to
// exp(Q_{tau-1}(w) + H_tau(w) - loglik).  word_post[f][w] is that running sum minus the running sum of the record
// posteriors that ended before f — two non-decreasing sums per column, each added in frame order.
__global__ __launch_bounds__(kXBlock) void lattice_post_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, int32_t W,
    const double *__restrict__ lm_start, const double *__restrict__ alpha, const double *__restrict__ Q,
    const double *__restrict__ beta, const double *__restrict__ H, const double *__restrict__ loglik,
    double *__restrict__ record_post, double *__restrict__ word_post) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (gid >= n_utts * W) return;
  const int64_t u = gid / W;
  const int w = static_cast<int>(gid - u * W);
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  const double ll = loglik[u];
  if (!finite_f64(ll)) {  // no path, or a NaN on the way: exact zeros
    for (int64_t f = 0; f < T; ++f) {
      record_post[(beg + f) * W + w] = 0.0;
      if (word_post) word_post[(beg + f) * W + w] = 0.0;
    }
    return;
  }
  double started = 0.0, ended = 0.0;
  double qprev = lm_start[w];
  for (int64_t f = 0; f < T; ++f) {
    const int64_t at = (beg + f) * W + w;
    const double al = alpha[at], be = beta[at], h = H[at];
    const double qnext = f + 1 < T ? Q[at] : neg_inf();
    started += exp_unit((qprev + h) - ll);
    if (word_post) {
      const double d = started - ended;
      word_post[at] = d < 0.0 ? 0.0 : d;
    }
    const double rp = al == neg_inf() ? 0.0 : exp_unit((al + be) - ll);
    record_post[at] = rp;
    ended += rp;
    qprev = qnext;
  }
}

int lt_check(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S) {
  SAPR_REQUIRE(total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  return x_check_shape(W, S);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_lattice_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                      size_t *bytes) {
  SAPR_REQUIRE(bytes, "NULL pointer argument (bytes)");
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  // X and N [total_frames][W] float64, B [total_frames][W] int32, each padded to 16
  const size_t f = static_cast<size_t>(total_frames), w = static_cast<size_t>(W);
  *bytes = 2 * lt_table_bytes(f, w, 8) + lt_table_bytes(f, w, 4);
  return 0;
}

extern "C" int sapr_connected_lattice(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                      const double *log_start, const double *log_trans, const double *log_exit,
                                      const double *lm, const double *lm_start, const double *lm_end, int32_t W,
                                      int32_t S, void *workspace, size_t workspace_bytes, double *score,
                                      int32_t *final_word, void *stream) {
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_lattice_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && score && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  const LTables tb = lt_tables(workspace, total_frames, W);
  hipStream_t st = as_stream(stream);
  return x_dispatch(SP, R, [&](auto rl, auto sp) {
    constexpr int RL = decltype(rl)::value, SPc = decltype(sp)::value;
    return x_launch(connected_lattice_kernel<RL, SPc>, blocks, kXBlock, lt_lds_doubles(W, SPc, RL) * sizeof(double),
                    st, logb, offsets, n_utts, total_frames, log_start, log_trans, log_exit, lm, lm_start, lm_end, W, S,
                    tb.X, tb.N, tb.B, final_word, score);
  });
}

extern "C" int sapr_connected_lattice_backward(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W,
                                               int32_t S, const void *workspace, size_t workspace_bytes,
                                               const double *forward_lm_start, const double *lm,
                                               const double *lm_start, const double *lm_end, double *beta,
                                               int32_t *next_end, uint8_t *next_word, double *root, int32_t *first,
                                               void *stream) {
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  SAPR_REQUIRE(forward_lm_start && lm && lm_start && lm_end,
               "NULL language model (forward_lm_start, lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_lattice_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && root && first && (total_frames == 0 || (beta && next_end && next_word)),
               "NULL pointer argument");
  const LTables tb = lt_tables(const_cast<void *>(workspace), total_frames, W);
  return x_launch(connected_lattice_backward_kernel, blocks, kXBlock, lb_lds_doubles(W) * sizeof(double),
                  as_stream(stream), offsets, n_utts, total_frames, W, tb.X, tb.N, tb.B, forward_lm_start, lm, lm_start,
                  lm_end, beta, next_end, next_word, root, first);
}

extern "C" int sapr_connected_lattice_walk(const int64_t *offsets, int64_t n_utts, int64_t total_frames, int32_t W,
                                           int32_t S, const int32_t *next_end, const uint8_t *next_word,
                                           const double *root, const int32_t *first, int32_t *n_words,
                                           int32_t *path_word, uint8_t *path_entry, void *stream) {
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  const int64_t blocks = (n_utts + kXBlock - 1) / kXBlock;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && root && first && (total_frames == 0 || (next_end && next_word)), "NULL pointer argument");
  return x_launch(connected_lattice_walk_kernel, blocks, kXBlock, 0, as_stream(stream), offsets, n_utts, total_frames,
                  W, next_end, next_word, root, first, n_words, path_word, path_entry);
}

extern "C" int sapr_connected_lattice_posteriors_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W,
                                                                 int32_t S, size_t *bytes) {
  SAPR_REQUIRE(bytes, "NULL pointer argument (bytes)");
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  // alpha, Q, beta and H [total_frames][W] float64, each padded to 16
  *bytes = 4 * lt_table_bytes(static_cast<size_t>(total_frames), static_cast<size_t>(W), 8);
  return 0;
}

extern "C" int sapr_connected_lattice_posteriors(const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                                 int32_t W, int32_t S, const void *lattice_workspace,
                                                 size_t lattice_workspace_bytes, const double *forward_lm_start,
                                                 const double *lm, const double *lm_start, const double *lm_end,
                                                 double acoustic_scale, const uint8_t *keep, void *workspace,
                                                 size_t workspace_bytes, double *loglik, double *record_post,
                                                 double *word_post, void *stream) {
  if (int rc = lt_check(total_frames, n_utts, W, S)) return rc;
  SAPR_REQUIRE(forward_lm_start && lm && lm_start && lm_end,
               "NULL language model (forward_lm_start, lm, lm_start, lm_end)");
  SAPR_REQUIRE(acoustic_scale - acoustic_scale == 0.0 && acoustic_scale > 0.0,
               "acoustic_scale must be finite and > 0, got %g", acoustic_scale);
  size_t need = 0;
  if (int rc = sapr_connected_lattice_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(lattice_workspace_bytes >= need && (need == 0 || lattice_workspace),
               "lattice workspace too small: %zu < %zu", lattice_workspace_bytes, need);
  if (int rc = sapr_connected_lattice_posteriors_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  size_t lds = 0;
  const int waves = x_waves(lp_shared_doubles(W) * sizeof(double), lp_wave_doubles(W) * sizeof(double), &lds);
  if (lds > static_cast<size_t>(kXLdsMax))
    return fail(SAPR_ERR_UNSUPPORTED, "the lattice posteriors need %zu bytes of LDS, the device offers %d", lds,
                kXLdsMax);
  const int64_t blocks = (n_utts + waves - 1) / waves;
  const int64_t post_blocks = (n_utts * W + kXBlock - 1) / kXBlock;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL && post_blocks <= 0x7fffffffLL, "grid too large (%lld utterances)",
               (long long)n_utts);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && loglik && (total_frames == 0 || record_post), "NULL pointer argument");
  const LTables tb = lt_tables(const_cast<void *>(lattice_workspace), total_frames, W);
  const LpTables pt = lp_tables(workspace, total_frames, W);
  hipStream_t st = as_stream(stream);
  if (int rc = x_launch(lattice_post_forward_kernel, blocks, waves * kWave, lds, st, offsets, n_utts, total_frames, W,
                        tb.X, tb.N, tb.B, forward_lm_start, lm, lm_start, lm_end, acoustic_scale, keep, pt.alpha, pt.Q,
                        pt.H, loglik))
    return rc;
  if (total_frames == 0) return 0;
  if (int rc = x_launch(lattice_post_backward_kernel, blocks, waves * kWave, lds, st, offsets, n_utts, total_frames, W,
                        tb.X, tb.N, tb.B, forward_lm_start, lm, lm_end, acoustic_scale, keep, pt.beta, pt.H))
    return rc;
  return x_launch(lattice_post_kernel, post_blocks, kXBlock, 0, st, offsets, n_utts, total_frames, W, lm_start,
                  pt.alpha, pt.Q, pt.beta, pt.H, loglik, record_post, word_post);
}
