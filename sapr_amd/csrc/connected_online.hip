// Online connected-word decoding on gfx950: the trellis of connected_bigram.hip carried from chunk to chunk of a
// recording that is still arriving, and partial traceback over a ring of back-pointer rows.  CPU
// restatement, which is the definition: tests/_online_ref.py over tests/_bigram_ref.py.  The input
// logb[total_frames][R = W * SP] is what the three emission stages of connected.hip write for the chunks' frames; this
// unit knows nothing about the emission family.
//
// A session is n_streams blocks of opaque device memory (sapr_connected_online_state_bytes; all zero = fresh):
//   header        frames consumed, frames committed, frames committed by force, entry flags handed out, the score a
//                 flush would return and the word that attains it
//   delta[R], X[W], N[W]   the recursion's whole carried state, float64
//   ring          back-pointer rows bp[window][R], xarg[window][W], warg[window][W], one byte each as in
//                 connected_bigram.hip, the row of absolute frame t at t mod window
//
// connected_online_step_kernel<RL, SP> is connected_bigram_kernel's recursion — lane layout, tab by source, lmt, the
// three-step coupling through cbuf / xbuf / nbuf, the same arithmetic in the same order — with three differences: it
// starts from the stream's delta and N where the stream has frames, the t == 0 branch belongs to the stream's absolute
// frame 0, and the rows go to the ring.  It stores delta, X, N, the score and the final word back after the chunk.
//
// connected_online_commit_kernel<RL>: one wavefront per stream, the flat states on the lanes as in the step kernel.
// Every live lane (finite delta) walks its own back-trace down the ring in lock step; after each frame the wavefront
// asks whether all live lanes hold the same flat state (compared with the first live lane's, one ballot).  The walk
// stops at the first agreement or at the oldest pending frame.  Lane 0 then writes the newly final rows, applies the
// forced rule (the window must keep room for the next chunk), and updates the header; with the stream's flush byte it
// performs the flush instead, and with hypothesis pointers it writes the rows a flush would write now.
//
// No atomics; a stream's outputs are a function of its own frames, its own state and the network alone.  Every index
// read from the ring is clamped into its row, and every ring row is addressed modulo the window.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

struct OnHeader {      // 64 bytes; all zero: a fresh stream
  int64_t frames;      // consumed
  int64_t committed;   // final: the pending frames are [committed, frames)
  int64_t forced;      // of the committed frames, those committed by force
  int64_t entries;     // entry flags among the committed rows
  double score;        // max_v (X(v) + lm_end[v]) at frame frames - 1 (meaningless while frames == 0)
  int32_t fin;         // ... and the word that attains it
  int32_t pad0;
  int64_t pad1[2];
};
static_assert(sizeof(OnHeader) == 64, "the header is 64 bytes");

// one stream's block: header, delta[R], X[W], N[W] (doubles), then the three rings (bytes), each part padded to 16
struct OnLayout {
  size_t carried, bp, xarg, warg, stride;
};

inline OnLayout on_layout(int32_t W, int32_t SP, int32_t window) {
  const size_t R = static_cast<size_t>(W) * SP, win = static_cast<size_t>(window);
  OnLayout l;
  l.carried = sizeof(OnHeader);
  l.bp = l.carried + x_align16((R + 2 * static_cast<size_t>(W)) * sizeof(double));
  l.xarg = l.bp + x_align16(win * R);
  l.warg = l.xarg + x_align16(win * W);
  l.stride = l.warg + x_align16(win * W);
  return l;
}

// LDS of one workgroup in doubles: connected_bigram_kernel's
constexpr size_t on_lds_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W +
         static_cast<size_t>(kXWaves) * (kWave * RL + 2 * kWave);
}

template <int RL, int SP>
__global__ __launch_bounds__(kXBlock) void connected_online_step_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_streams, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, int32_t window, int32_t max_chunk, uint8_t *__restrict__ state, OnLayout lay,
    const uint8_t *__restrict__ reset, uint8_t *__restrict__ truncated) {
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
  if (u >= n_streams) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg;

  uint8_t *__restrict__ base = state + static_cast<size_t>(u) * lay.stride;
  OnHeader *__restrict__ hdr = reinterpret_cast<OnHeader *>(base);
  double *__restrict__ st_delta = reinterpret_cast<double *>(base + lay.carried);  // [R]
  double *__restrict__ st_x = st_delta + R;                                        // [W]
  double *__restrict__ st_n = st_x + W;                                            // [W]
  uint8_t *__restrict__ bp = base + lay.bp;
  uint8_t *__restrict__ xarg = base + lay.xarg;
  uint8_t *__restrict__ warg = base + lay.warg;

  const bool fresh = reset != nullptr && reset[u] != 0;
  int64_t frames0 = fresh ? 0 : hdr->frames;
  int64_t pending = fresh ? 0 : frames0 - hdr->committed;
  if (frames0 < 0 || pending < 0 || pending > window) frames0 = pending = 0;  // (not a state this unit wrote)
  // the chunk: at most max_chunk frames and never more than the ring has free, whatever the caller did before
  int64_t T = fr.T;
  const int64_t room = window - pending < max_chunk ? window - pending : max_chunk;
  const bool cut = T > room;
  T = cut ? room : T;
  wave_lds_sync();  // (every lane has read the header before lane 0 writes it)
  if (lane == 0) {
    if (truncated) truncated[u] = cut ? 1 : 0;
    if (fresh || frames0 != hdr->frames) {
      hdr->frames = 0;
      hdr->committed = 0;
      hdr->forced = 0;
      hdr->entries = 0;
    }
  }
  if (T <= 0) return;

  double ls[RL], ls0[RL], lx[RL], delta[RL], bn[RL], ne[RL];
  int sk[RL], wk[RL];
  bool ok[RL];
  nbuf[lane] = (frames0 > 0 && lane < W) ? st_n[lane] : neg_inf();
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const XState x = x_flat_state(k * kWave + lane, R, SP, S, log_start, log_exit);
    ok[k] = x.ok;
    sk[k] = x.s;
    wk[k] = x.w;
    ls[k] = x.ls;
    lx[k] = x.lx;
    ls0[k] = x.real ? lm_start[x.w] + x.ls : neg_inf();
    delta[k] = (frames0 > 0 && x.ok) ? st_delta[k * kWave + lane] : neg_inf();
    ne[k] = nbuf[wk[k]];
  }
  const uint64_t dmask = x_mask_by_source<RL>(tab, sk, lane, SP);

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[k * kWave + lane] : neg_inf();

  int slot = static_cast<int>(frames0 % window);  // the ring row of absolute frame frames0 + t
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
    if (frames0 + t == 0) {
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
    uint8_t *__restrict__ bprow = bp + static_cast<size_t>(slot) * R;
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
      xarg[static_cast<size_t>(slot) * W + lane] = static_cast<uint8_t>(xs);
    }
    wave_lds_sync();
    if (lane < W) {  // N(w): the first maximum over the predecessor words, v ascending
      int nw;
      nbuf[lane] = x_first_max_pair(xbuf, lmt + lane * LS, W, &nw);
      warg[static_cast<size_t>(slot) * W + lane] = static_cast<uint8_t>(nw);
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < RL; ++k) ne[k] = nbuf[wk[k]];
    slot = slot + 1 == window ? 0 : slot + 1;
  }
  // the carried state of the next chunk, and what a flush needs
#pragma unroll
  for (int k = 0; k < RL; ++k)
    if (ok[k]) st_delta[k * kWave + lane] = delta[k];
  if (lane < W) {
    st_x[lane] = xbuf[lane];
    st_n[lane] = nbuf[lane];
  }
  if (lane == 0) {  // score = max_v (X(v) + lm_end[v]), v ascending, the first maximum
    int fw = 0;
    hdr->score = x_first_max_pair(xbuf, lme, W, &fw);
    hdr->fin = fw;
    hdr->frames = frames0 + T;
  }
}

// ---- the commit ---------------------------------------------------------------------------------------------------
// a stream's rings as the walks read them; every index is clamped into its row
struct OnRing {
  const uint8_t *bp, *xarg, *warg;
  int W, SP, window;
  __device__ __forceinline__ int slot(int64_t t) const { return static_cast<int>(t % window); }
  __device__ __forceinline__ int back(int sl, int w, int s) const {
    return bp[static_cast<size_t>(sl) * (W * SP) + w * SP + s];
  }
  // from (w, s) with back-pointer b at the frame whose predecessor row is `prev`
  __device__ __forceinline__ void step(int b, int prev, int *w, int *s) const {
    if (b == kXEntry) {
      int v = warg[static_cast<size_t>(prev) * W + *w];
      v = v < W ? v : 0;
      int e = xarg[static_cast<size_t>(prev) * W + v];
      *w = v;
      *s = e < SP ? e : 0;
    } else {
      *s = b < SP ? b : 0;
    }
  }
};

// one lane: the walk from (w, s) at frame t down to lo; writes the rows of the frames lo .. hi - 1 at index
// frame - first; returns the entry flags among them
__device__ __forceinline__ int on_walk(const OnRing &ring, int w, int s, int64_t t, int64_t lo, int64_t hi,
                                       int64_t first, int32_t *__restrict__ ow, int32_t *__restrict__ os,
                                       uint8_t *__restrict__ oe) {
  int n = 0;
  int sl = ring.slot(t);
  for (int64_t tau = t; tau >= lo; --tau) {
    const int b = ring.back(sl, w, s);
    const bool entry = tau == 0 || b == kXEntry;
    if (tau < hi) {
      if (ow) ow[tau - first] = w;
      if (os) os[tau - first] = s;
      if (oe) oe[tau - first] = entry ? 1 : 0;
      n += entry ? 1 : 0;
    }
    const int prev = sl == 0 ? ring.window - 1 : sl - 1;
    if (tau > lo) ring.step(b, prev, &w, &s);
    sl = prev;
  }
  return n;
}

template <int RL>
__global__ __launch_bounds__(kXBlock) void connected_online_commit_kernel(
    int64_t n_streams, int32_t W, int32_t S, int32_t SP, int32_t window, int32_t max_chunk,
    uint8_t *__restrict__ state, OnLayout lay, const uint8_t *__restrict__ flush, int32_t *__restrict__ n_new,
    int64_t *__restrict__ first_frame, int32_t *__restrict__ out_word, int32_t *__restrict__ out_state,
    uint8_t *__restrict__ out_entry, double *__restrict__ score, int32_t *__restrict__ n_words,
    int64_t *__restrict__ forced, int32_t *__restrict__ hyp_len, int32_t *__restrict__ hyp_word,
    int32_t *__restrict__ hyp_state, uint8_t *__restrict__ hyp_entry) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + threadIdx.x / kWave;
  if (u >= n_streams) return;
  const int R = W * SP;
  uint8_t *__restrict__ base = state + static_cast<size_t>(u) * lay.stride;
  OnHeader *__restrict__ hdr = reinterpret_cast<OnHeader *>(base);
  const double *__restrict__ st_delta = reinterpret_cast<const double *>(base + lay.carried);
  const OnRing ring{base + lay.bp, base + lay.xarg, base + lay.warg, W, SP, window};
  int32_t *__restrict__ ow = out_word ? out_word + u * window : nullptr;
  int32_t *__restrict__ os = out_state ? out_state + u * window : nullptr;
  uint8_t *__restrict__ oe = out_entry ? out_entry + u * window : nullptr;

  int64_t frames = hdr->frames, c = hdr->committed;
  if (frames < 0 || c < 0 || c > frames || frames - c > window) frames = c = 0;  // (not a state this unit wrote)
  const int64_t c0 = c, t = frames - 1;
  const double sc = frames > 0 ? hdr->score : neg_inf();
  int fin = hdr->fin;
  fin = (fin >= 0 && fin < W) ? fin : 0;
  const bool path = frames > 0 && finite_f64(sc);  // a flush has a path to walk

  if (flush != nullptr && flush[u] != 0) {
    wave_lds_sync();  // (every lane has read the header before lane 0 writes it)
    if (lane == 0) {
      int n = 0;
      if (path) {
        int s = ring.xarg[static_cast<size_t>(ring.slot(t)) * W + fin];
        s = s < SP ? s : 0;
        n = on_walk(ring, fin, s, t, c, frames, c0, ow, os, oe);
      }
      if (n_new) n_new[u] = path ? static_cast<int32_t>(frames - c) : 0;
      if (first_frame) first_frame[u] = c0;
      if (score) score[u] = sc;
      if (n_words) n_words[u] = path ? static_cast<int32_t>(hdr->entries + n) : 0;
      if (forced) forced[u] = hdr->forced;
      if (hyp_len) hyp_len[u] = 0;
      hdr->frames = 0;  // the stream is fresh again
      hdr->committed = 0;
      hdr->forced = 0;
      hdr->entries = 0;
    }
    return;
  }

  // the lock-step walk: cw / cs[k] is the state at frame tau on the back-trace from flat state k * 64 + lane at t
  int cw[RL], cs[RL];
  bool live[RL];
  double dv[RL];
  bool any = false;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int r = k * kWave + lane;
    const int w = r / SP;
    cw[k] = r < R ? w : 0;
    cs[k] = r - w * SP;
    dv[k] = (r < R && frames > 0) ? st_delta[r] : neg_inf();
    live[k] = r < R && cs[k] < S && finite_f64(dv[k]);
    cs[k] = r < R ? cs[k] : 0;
    any |= live[k];
  }
  // the first live flat state: register k0 of lane l0 (wavefront-uniform)
  int k0 = -1, l0 = 0;
#pragma unroll
  for (int k = RL - 1; k >= 0; --k) {
    const uint64_t m = __ballot(live[k]);
    if (m) {
      k0 = k;
      l0 = __ffsll(static_cast<long long>(m)) - 1;
    }
  }
  int64_t tau = -1;  // the stable frame, -1 without one
  int aw = 0, as = 0;
  if (k0 >= 0 && c <= t) {
    int sl = ring.slot(t);
    for (int64_t f = t;; --f) {
      int code = 0;
      bool differ = false;
#pragma unroll
      for (int k = 0; k < RL; ++k) code = k == k0 ? (cw[k] << 8 | cs[k]) : code;
      code = __shfl(code, l0, kWave);
#pragma unroll
      for (int k = 0; k < RL; ++k) differ |= live[k] && (cw[k] << 8 | cs[k]) != code;
      if (__ballot(differ) == 0) {
        tau = f;
        aw = code >> 8;
        as = code & 255;
        break;
      }
      if (f == c) break;
      const int prev = sl == 0 ? window - 1 : sl - 1;
#pragma unroll
      for (int k = 0; k < RL; ++k)
        if (live[k]) ring.step(ring.back(sl, cw[k], cs[k]), prev, &cw[k], &cs[k]);
      sl = prev;
    }
  }

  // the forced rule needs the first maximum of delta over the live states in flat order
  double bv = neg_inf();
  int br = kXMaxR;  // (no live state)
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const bool take = live[k] && (br == kXMaxR || dv[k] > bv);
    bv = take ? dv[k] : bv;
    br = take ? k * kWave + lane : br;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, kWave);
    const int orr = __shfl_xor(br, o, kWave);
    const bool take = orr != kXMaxR && (br == kXMaxR || ov > bv || (ov == bv && orr < br));
    bv = take ? ov : bv;
    br = take ? orr : br;
  }

  wave_lds_sync();  // (every lane has read the header before lane 0 writes it)
  if (lane == 0) {
    int n = 0;
    if (tau >= 0) {  // rows c .. tau of the common back-trace
      n += on_walk(ring, aw, as, tau, c, tau + 1, c0, ow, os, oe);
      c = tau + 1;
    }
    int64_t k = frames - c - (static_cast<int64_t>(window) - max_chunk);
    k = k > 0 ? k : 0;
    if (k > 0) {  // the next chunk must fit the ring: the oldest k pending frames leave by force
      if (br != kXMaxR) {
        const int w = br / SP;
        n += on_walk(ring, w, br - w * SP, t, c, c + k, c0, ow, os, oe);
      } else {
        for (int64_t f = c; f < c + k; ++f) {
          if (ow) ow[f - c0] = -1;
          if (os) os[f - c0] = -1;
          if (oe) oe[f - c0] = 0;
        }
      }
      c += k;
    }
    if (n_new) n_new[u] = static_cast<int32_t>(c - c0);
    if (first_frame) first_frame[u] = c0;
    if (forced) forced[u] = hdr->forced + k;
    hdr->committed = c;
    hdr->forced += k;
    hdr->entries += n;
    if (hyp_len) {  // the rows a flush would write now over the pending frames
      hyp_len[u] = path ? static_cast<int32_t>(frames - c) : 0;
      if (path && frames > c) {
        int s = ring.xarg[static_cast<size_t>(ring.slot(t)) * W + fin];
        s = s < SP ? s : 0;
        on_walk(ring, fin, s, t, c, frames, c, hyp_word ? hyp_word + u * window : nullptr,
                hyp_state ? hyp_state + u * window : nullptr, hyp_entry ? hyp_entry + u * window : nullptr);
      }
    }
  }
}

int on_check(int64_t n_streams, int32_t W, int32_t S, int32_t window) {
  SAPR_REQUIRE(n_streams >= 0 && W > 0 && S > 0 && window >= 2, "bad sizes (n_streams=%lld W=%d S=%d window=%d)",
               (long long)n_streams, W, S, window);
  return x_check_shape(W, S);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_online_state_bytes(int64_t n_streams, int32_t W, int32_t S, int32_t window,
                                                 size_t *bytes) {
  SAPR_REQUIRE(bytes, "NULL bytes");
  if (int rc = on_check(n_streams, W, S, window)) return rc;
  *bytes = static_cast<size_t>(n_streams) * on_layout(W, sp_of(S), window).stride;
  return 0;
}

extern "C" int sapr_connected_online_step(const double *logb, const int64_t *offsets, int64_t n_streams,
                                          int64_t total_frames, const double *log_start, const double *log_trans,
                                          const double *log_exit, const double *lm, const double *lm_start,
                                          const double *lm_end, int32_t W, int32_t S, int32_t window,
                                          int32_t max_chunk, void *state, size_t state_bytes, const uint8_t *reset,
                                          uint8_t *truncated, void *stream) {
  if (int rc = on_check(n_streams, W, S, window)) return rc;
  SAPR_REQUIRE(total_frames >= 0 && max_chunk >= 1 && max_chunk < window,
               "bad sizes (total_frames=%lld, 1 <= max_chunk=%d < window=%d)", (long long)total_frames, max_chunk,
               window);
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  const int32_t SP = sp_of(S);
  const OnLayout lay = on_layout(W, SP, window);
  const size_t need = static_cast<size_t>(n_streams) * lay.stride;
  SAPR_REQUIRE(state_bytes >= need && (need == 0 || state), "state too small: %zu < %zu", state_bytes, need);
  const int64_t blocks = (n_streams + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_streams == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && (total_frames == 0 || logb), "NULL pointer argument");
  return x_dispatch(SP, W * SP, [&](auto rl, auto sp) {
    constexpr int RL = decltype(rl)::value, SPc = decltype(sp)::value;
    return x_launch(connected_online_step_kernel<RL, SPc>, blocks, kXBlock, on_lds_doubles(W, SPc, RL) * sizeof(double),
                    as_stream(stream), logb, offsets, n_streams, total_frames, log_start, log_trans, log_exit, lm,
                    lm_start, lm_end, W, S, window, max_chunk, static_cast<uint8_t *>(state), lay, reset, truncated);
  });
}

extern "C" int sapr_connected_online_commit(int64_t n_streams, int32_t W, int32_t S, int32_t window, int32_t max_chunk,
                                            void *state, size_t state_bytes, const uint8_t *flush, int32_t *n_new,
                                            int64_t *first_frame, int32_t *out_word, int32_t *out_state,
                                            uint8_t *out_entry, double *score, int32_t *n_words, int64_t *forced,
                                            int32_t *hyp_len, int32_t *hyp_word, int32_t *hyp_state,
                                            uint8_t *hyp_entry, void *stream) {
  if (int rc = on_check(n_streams, W, S, window)) return rc;
  SAPR_REQUIRE(max_chunk >= 1 && max_chunk < window, "bad sizes (1 <= max_chunk=%d < window=%d)", max_chunk, window);
  const int32_t SP = sp_of(S);
  const OnLayout lay = on_layout(W, SP, window);
  const size_t need = static_cast<size_t>(n_streams) * lay.stride;
  SAPR_REQUIRE(state_bytes >= need && (need == 0 || state), "state too small: %zu < %zu", state_bytes, need);
  const int64_t blocks = (n_streams + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_streams == 0) return 0;
  SAPR_REQUIRE(n_new && first_frame && out_word && out_state && out_entry && forced, "NULL pointer argument");
  SAPR_REQUIRE(flush == nullptr || (score && n_words), "a flush needs score and n_words");
  SAPR_REQUIRE(hyp_len || !(hyp_word || hyp_state || hyp_entry), "hypothesis rows need hyp_len");
  const int R = W * SP;
  uint8_t *st = static_cast<uint8_t *>(state);
  const auto go = [&](auto rl) {
    constexpr int RL = decltype(rl)::value;
    return x_launch(connected_online_commit_kernel<RL>, blocks, kXBlock, 0, as_stream(stream), n_streams, W, S, SP,
                    window, max_chunk, st, lay, flush, n_new, first_frame, out_word, out_state, out_entry, score,
                    n_words, forced, hyp_len, hyp_word, hyp_state, hyp_entry);
  };
  if (R <= kWave) return go(std::integral_constant<int, 1>{});
  if (R <= 2 * kWave) return go(std::integral_constant<int, 2>{});
  return go(std::integral_constant<int, 4>{});
}
