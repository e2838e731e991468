// Connected-word confidence on gfx950: forward-backward over the word loop under the word-pair language model of
// connected_bigram.hip — the sum over every word string the grammar allows where that unit takes the maximum
// (DESIGN 4.3m).  CPU restatement, which is the definition: tests/_loop_fb_ref.py; it is written out in
// include/sapr_hip.h.  The input logb[total_frames][R = W * SP] is what the three emission stages of connected.hip
// write; this unit knows nothing about the emission family.
//
// The lane layout of connected_lanes.h over the flat states, written out in the two kernels (they keep the text they
// were timed with; the constants, the per-word log-sum-exp and the host side are the header's).  The transition table
// lies in LDS by diagonal, tab[(j - i) mod SP][r of j]: the forward kernel reads diagonal d at its own flat state, the
// backward kernel the same diagonal at flat state r + d (transposed).
// The arithmetic is the sum-product one: lse2 over the live distances, then the entry (exit) term; the per-word
// log-sum-exp over a word's states is x_segment_lse.
//
// The W x W log-sum-exp against lm is pair_lse (connected_lanes.h: the lattice posteriors of connected_lattice.hip
// share it): N_t(w) = lse_v (X_t(v) + lm[v][w]) forward,
// F_t(v) = lse_w (lm[v][w] + E_t(w)) backward.  lm lies in LDS in rows of W | 1 doubles — transposed in the forward
// kernel, row-major in the backward kernel — so that lane q walks its own row while the other operand is a broadcast:
//   1. lane q < W takes the maximum of its W terms (adds and compares, pipelined LDS reads);
//   2. the W * W exponentials exp(term - maximum) are spread over the 64 lanes, item n = q * W + p on lane n mod 64,
//      into a per-wavefront block of W rows of W | 1 doubles;
//   3. lane q adds its row p ascending and takes log(sum) + maximum.
// ceil(W * W / 64) exponential issues per frame instead of W, and a fixed order of summation.
//
// loop_forward_kernel<RL, SP> writes alpha_t (R doubles) and N_t (W doubles) per frame into the workspace and
// loglik[u] at the end; a NaN met anywhere (lse2 and the maxima would drop it) makes the likelihood NaN.
// loop_backward_kernel<RL, SP> walks t downwards with beta in registers and writes post, word_post (the sum over a
// word's states through the coupling row, s ascending) and entry_post where asked; an utterance whose likelihood is
// not finite gets exact zeros.  Both kernels take as many wavefronts per workgroup as the LDS holds next to tab and lm,
// at most four (three at W = 64).
//
// No atomics; an utterance's outputs are a function of its own frames and the network alone, and every sum has a fixed
// order: two calls return the same bytes.  Offsets that leave the batch are served as empty.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

// LDS in doubles: tab[SP][64 RL], lm[W][W | 1], lm_end[W] for the workgroup; cbuf[64 RL], xbuf[64], mbuf[64], nbuf[64]
// and the exponentials ebuf[W][W | 1] for every wavefront
constexpr size_t lf_shared_doubles(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W;
}
constexpr size_t lf_wave_doubles(int W, int RL) {
  return static_cast<size_t>(kWave) * RL + 3 * kWave + static_cast<size_t>(W) * x_lm_stride(W);
}

// tab[dd][r] = log_trans[w][i][s] with r = w * SP + s and i = (s - dd) mod SP; lmx[a][b] = lm[a][b], or lm[b][a] where
// transposed; lme = lm_end (all threads of the workgroup; followed by a barrier)
template <int SP>
__device__ __forceinline__ void lf_load_tables(double *tab, double *lmx, double *lme,
                                               const double *__restrict__ log_trans, const double *__restrict__ lm,
                                               const double *__restrict__ lm_end, int W, int S, int RP,
                                               bool transposed) {
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  for (int n = threadIdx.x; n < SP * RP; n += blockDim.x) {
    const int dd = n / RP, r = n - dd * RP;
    const int w = r / SP, s = r - w * SP;
    const int i = s >= dd ? s - dd : s - dd + SP;
    double v = neg_inf();
    if (r < R && s < S && i < S) v = log_trans[(static_cast<int64_t>(w) * S + i) * S + s];
    tab[n] = v;
  }
  for (int n = threadIdx.x; n < W * W; n += blockDim.x) {  // (coalesced read of lm[a][b])
    const int a = n / W, b = n - a * W;
    lmx[transposed ? b * LS + a : a * LS + b] = lm[n];
  }
  for (int n = threadIdx.x; n < W; n += blockDim.x) lme[n] = lm_end[n];
  __syncthreads();
}

// the distances d = j - i in -(SP - 1) .. SP - 1 at which some transition of the vocabulary is finite (bit d + SP - 1),
// wavefront-uniform; *nan: the table holds a NaN
template <int RL, int SP>
__device__ __forceinline__ uint64_t lf_distance_mask(const double *tab, const int (&sk)[RL], int lane, bool *nan) {
  constexpr int RP = kWave * RL;
  uint64_t dmask = 0;
  bool bad = false;
#pragma unroll 1
  for (int d = 1 - SP; d < SP; ++d) {
    const int dd = d >= 0 ? d : d + SP;
    bool any = false;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      const int i = sk[k] - d;
      const bool in = i >= 0 && i < SP;
      const double v = tab[dd * RP + k * kWave + lane];
      any |= in && !(v == neg_inf());
      bad |= in && v != v;
    }
    if (__ballot(any)) dmask |= 1ull << (d + SP - 1);
  }
  *nan = __ballot(bad) != 0;
  return (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<unsigned>(dmask >> 32))) << 32) |
         __builtin_amdgcn_readfirstlane(static_cast<unsigned>(dmask));
}

template <int RL, int SP>
__global__ __launch_bounds__(kXBlock) void loop_forward_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, double *__restrict__ alpha_ws, double *__restrict__ n_ws, double *__restrict__ loglik) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  extern __shared__ double smem[];
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  double *tab = smem;             // [SP][RP] by diagonals
  double *lmt = tab + SP * RP;    // [W][LS]: lmt[w][v] = lm[v][w]
  double *lme = lmt + W * LS;     // [W]
  lf_load_tables<SP>(tab, lmt, lme, log_trans, lm, lm_end, W, S, RP, true);

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  double *cbuf = lme + W + static_cast<size_t>(wave) * lf_wave_doubles(W, RL);  // [RP]
  double *xbuf = cbuf + RP;       // [64]: X(v)
  double *mbuf = xbuf + kWave;    // [64]: the maxima
  double *nbuf = mbuf + kWave;    // [64]: N(w)
  double *ebuf = nbuf + kWave;    // [W][LS]: the exponentials of pair_lse
  const int64_t u = static_cast<int64_t>(blockIdx.x) * waves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  const int64_t T = end - beg;
  if (T == 0) {
    if (lane == 0) loglik[u] = neg_inf();
    return;
  }

  double ls[RL], ls0[RL], lx[RL], alpha[RL], bn[RL], ne[RL];
  int sk[RL], wk[RL];
  bool ok[RL], real[RL];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int r = k * kWave + lane;
    const int w = r / SP, s = r - w * SP;  // (w <= 255 / SP <= 63: inside nbuf)
    ok[k] = r < R;
    sk[k] = s;
    wk[k] = ok[k] ? w : 0;
    real[k] = ok[k] && s < S;
    ls[k] = real[k] ? log_start[w * S + s] : neg_inf();
    ls0[k] = real[k] ? lm_start[w] + ls[k] : neg_inf();
    lx[k] = real[k] ? log_exit[w * S + s] : neg_inf();
    bad = bad || ls0[k] != ls0[k] || lx[k] != lx[k];
    alpha[k] = neg_inf();
    ne[k] = neg_inf();
  }
  for (int n = lane; n < W * LS; n += kWave) {  // (the pad column of an even W is never written: not looked at)
    const int q = n / LS, p = n - q * LS;
    const double v = lmt[n];
    bad = bad || (p < W && v != v);
  }
  if (lane < W) bad = bad || lme[lane] != lme[lane];
  bool tab_nan;
  const uint64_t dmask = lf_distance_mask<RL, SP>(tab, sk, lane, &tab_nan);
  bad = bad || tab_nan;

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = real[k] ? brow[k * kWave + lane] : neg_inf();

  for (int64_t t = 0; t < T; ++t) {
    double b[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) b[k] = bn[k];
    {  // the next frame's row in flight under this frame's chain
      const int64_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
      for (int k = 0; k < RL; ++k) bn[k] = real[k] ? brow[tn * R + k * kWave + lane] : neg_inf();
    }
    double v[RL];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k) v[k] = ls0[k];
    } else {
#pragma unroll
      for (int k = 0; k < RL; ++k) v[k] = neg_inf();
      bool first = true;  // (uniform) the first live distance is the sum so far: lse2(-inf, x) = x, without its chain
#pragma unroll 1
      for (int d = SP - 1; d > -SP; --d) {
        if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
        // flat state r - d: lane (lane - d) & 63 of register k, of k - 1 where lane < d, of k + 1 where lane - d >= 64
        const int off = lane - d;
        const int src = off & (kWave - 1);
        const int drow = (d >= 0 ? d : d + SP) * RP;
        double rot[RL], term[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) rot[k] = __shfl(alpha[k], src, kWave);
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
          const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
          const double prev = off < 0 ? below : (off >= kWave ? above : rot[k]);
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[drow + k * kWave + lane];
          term[k] = prev + (in ? lt : neg_inf());
        }
        if (first) {
#pragma unroll
          for (int k = 0; k < RL; ++k) v[k] = term[k];
        } else {
#pragma unroll
          for (int k = 0; k < RL; ++k) v[k] = lse2(v[k], term[k]);
        }
        first = false;
      }
#pragma unroll
      for (int k = 0; k < RL; ++k) v[k] = lse2(v[k], ne[k] + ls[k]);
    }
    double *__restrict__ arow = alpha_ws + (beg + t) * R;
    double ex[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      alpha[k] = real[k] ? v[k] + b[k] : neg_inf();
      bad = bad || alpha[k] != alpha[k];
      if (ok[k]) arow[k * kWave + lane] = alpha[k];
      ex[k] = alpha[k] + lx[k];
    }
    const double xv = x_segment_lse<RL, SP>(cbuf, mbuf, ex, ok, wk, lane, W);  // X_t(v) on lane v
    if (lane < W) xbuf[lane] = xv;
    bad = bad || xv != xv;
    wave_lds_sync();
    if (t + 1 < T) {  // (uniform) N_t(w) on lane w; nothing enters behind the last frame
      const double nv = pair_lse(lmt, xbuf, mbuf, ebuf, lane, W, LS);
      bad = bad || nv != nv;
      if (lane < W) {
        nbuf[lane] = nv;
        n_ws[(beg + t) * W + lane] = nv;
      }
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < RL; ++k) ne[k] = nbuf[wk[k]];
    }
  }
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {  // loglik = lse_v (X_{T-1}(v) + lm_end[v]), v ascending
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
    loglik[u] = any_bad ? __builtin_nan("") : ll;
  }
}

template <int RL, int SP>
__global__ __launch_bounds__(kXBlock) void loop_backward_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_end, int32_t W, int32_t S,
    const double *__restrict__ alpha_ws, const double *__restrict__ n_ws, const double *__restrict__ loglik,
    double *__restrict__ word_post, double *__restrict__ entry_post, double *__restrict__ post) {
  constexpr int RP = kWave * RL;
  extern __shared__ double smem[];
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  double *tab = smem;             // [SP][RP] by diagonals
  double *lmr = tab + SP * RP;    // [W][LS]: lmr[v][w] = lm[v][w]
  double *lme = lmr + W * LS;     // [W]
  lf_load_tables<SP>(tab, lmr, lme, log_trans, lm, lm_end, W, S, RP, false);

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  double *cbuf = lme + W + static_cast<size_t>(wave) * lf_wave_doubles(W, RL);  // [RP]
  double *xbuf = cbuf + RP;       // [64]: E(w)
  double *mbuf = xbuf + kWave;    // [64]: the maxima
  double *nbuf = mbuf + kWave;    // [64]: F(v)
  double *ebuf = nbuf + kWave;    // [W][LS]: the exponentials of pair_lse
  const int64_t u = static_cast<int64_t>(blockIdx.x) * waves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  const int64_t T = end - beg;
  if (T == 0) return;
  const double ll = loglik[u];
  if (!finite_f64(ll)) {  // no path, or a NaN on the way: exact zeros
    for (int64_t t = 0; t < T; ++t) {
      if (post)
        for (int r = lane; r < R; r += kWave) post[(beg + t) * R + r] = 0.0;
      if (lane < W) {
        if (word_post) word_post[(beg + t) * W + lane] = 0.0;
        if (entry_post) entry_post[(beg + t) * W + lane] = 0.0;
      }
    }
    return;
  }

  double ls[RL], lx[RL], beta[RL], acur[RL], bcur[RL];
  int sk[RL], wk[RL];
  bool ok[RL], real[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int r = k * kWave + lane;
    const int w = r / SP, s = r - w * SP;
    ok[k] = r < R;
    sk[k] = s;
    wk[k] = ok[k] ? w : 0;
    real[k] = ok[k] && s < S;  // (a padded state carries nothing, whatever its column of logb holds)
    ls[k] = real[k] ? log_start[w * S + s] : neg_inf();
    lx[k] = real[k] ? log_exit[w * S + s] : neg_inf();
    beta[k] = real[k] ? lx[k] + lme[wk[k]] : neg_inf();
  }
  bool tab_nan;  // (a NaN in the table made the likelihood NaN: not reached)
  const uint64_t dmask = lf_distance_mask<RL, SP>(tab, sk, lane, &tab_nan);
  (void)tab_nan;

  const double *__restrict__ brow = logb + beg * R;
  const double *__restrict__ abase = alpha_ws + beg * R;
  const double *__restrict__ nbase = n_ws + beg * W;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    acur[k] = ok[k] ? abase[(T - 1) * R + k * kWave + lane] : neg_inf();
    bcur[k] = real[k] ? brow[(T - 1) * R + k * kWave + lane] : neg_inf();
  }
  const bool want_words = word_post != nullptr || entry_post != nullptr;

  for (int64_t t = T - 1; t >= 0; --t) {
    double c[RL], g[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      c[k] = bcur[k] + beta[k];
      g[k] = real[k] ? exp_unit((acur[k] + beta[k]) - ll) : 0.0;
      if (post && ok[k]) post[(beg + t) * R + k * kWave + lane] = g[k];
    }
    if (word_post || (entry_post && t == 0)) {  // (uniform) word_post_t(w): the word's states added s ascending
#pragma unroll
      for (int k = 0; k < RL; ++k)
        if (ok[k]) cbuf[k * kWave + lane] = g[k];
      wave_lds_sync();
      if (lane < W) {
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < SP; ++s) acc += cbuf[lane * SP + s];
        if (word_post) word_post[(beg + t) * W + lane] = acc;
        if (entry_post && t == 0) entry_post[beg * W + lane] = acc;
      }
      wave_lds_sync();
    }
    if (t == 0) break;
    double ap[RL], bp[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {  // frame t - 1 in flight under this frame's chain
      ap[k] = ok[k] ? abase[(t - 1) * R + k * kWave + lane] : neg_inf();
      bp[k] = real[k] ? brow[(t - 1) * R + k * kWave + lane] : neg_inf();
    }
    const double nprev = (want_words && lane < W) ? nbase[(t - 1) * W + lane] : neg_inf();
    double en[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) en[k] = ls[k] + c[k];
    const double ev = x_segment_lse<RL, SP>(cbuf, mbuf, en, ok, wk, lane, W);  // E_t(w) on lane w
    if (lane < W) {
      xbuf[lane] = ev;
      if (entry_post) entry_post[(beg + t) * W + lane] = exp_unit((nprev + ev) - ll);
    }
    wave_lds_sync();
    const double fv = pair_lse(lmr, xbuf, mbuf, ebuf, lane, W, LS);  // F_t(v) on lane v
    if (lane < W) nbuf[lane] = fv;
    wave_lds_sync();
    double nb[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) nb[k] = neg_inf();
    bool first = true;  // (uniform) as in the forward kernel
#pragma unroll 1
    for (int d = SP - 1; d > -SP; --d) {
      if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
      // flat state r + d: lane (lane + d) & 63 of register k, of k + 1 where lane + d >= 64, of k - 1 below lane 0
      const int off = lane + d;
      const int src = off & (kWave - 1);
      const int drow = (d >= 0 ? d : d + SP) * RP;
      double rot[RL], term[RL];
#pragma unroll
      for (int k = 0; k < RL; ++k) rot[k] = __shfl(c[k], src, kWave);
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
        const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
        const double next = off < 0 ? below : (off >= kWave ? above : rot[k]);
        const int j = sk[k] + d;
        const bool in = ok[k] && j >= 0 && j < SP;  // (outside the word: no such successor)
        const double lt = tab[in ? drow + k * kWave + lane + d : 0];  // the diagonal, transposed
        term[k] = in ? lt + next : neg_inf();
      }
      if (first) {
#pragma unroll
        for (int k = 0; k < RL; ++k) nb[k] = term[k];
      } else {
#pragma unroll
        for (int k = 0; k < RL; ++k) nb[k] = lse2(nb[k], term[k]);
      }
      first = false;
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      beta[k] = real[k] ? lse2(nb[k], lx[k] + nbuf[wk[k]]) : neg_inf();
      acur[k] = ap[k];
      bcur[k] = bp[k];
    }
  }
}

struct LfArgs {
  const double *logb;
  const int64_t *offsets;
  int64_t n_utts, total_frames;
  const double *log_start, *log_trans, *log_exit, *lm, *lm_start, *lm_end;
  int32_t W, S;
  double *alpha, *N, *loglik, *word_post, *entry_post, *post;
  bool backward;
};

// the exponentials take W * (W | 1) doubles per wavefront, 33 KB at W = 64: three wavefronts per workgroup there
template <int RL, int SP>
int launch_loop(const LfArgs &a, hipStream_t stream) {
  size_t lds = 0;
  const int waves =
      x_waves(lf_shared_doubles(a.W, SP, RL) * sizeof(double), lf_wave_doubles(a.W, RL) * sizeof(double), &lds);
  if (lds > static_cast<size_t>(kXLdsMax))
    return fail(SAPR_ERR_UNSUPPORTED, "the word-loop kernels need %zu bytes of LDS, the device offers %d", lds,
                kXLdsMax);
  const int64_t blocks = (a.n_utts + waves - 1) / waves;
  if (int rc = x_launch(loop_forward_kernel<RL, SP>, blocks, waves * kWave, lds, stream, a.logb, a.offsets, a.n_utts,
                        a.total_frames, a.log_start, a.log_trans, a.log_exit, a.lm, a.lm_start, a.lm_end, a.W, a.S,
                        a.alpha, a.N, a.loglik))
    return rc;
  if (!a.backward) return 0;
  return x_launch(loop_backward_kernel<RL, SP>, blocks, waves * kWave, lds, stream, a.logb, a.offsets, a.n_utts,
                  a.total_frames, a.log_start, a.log_trans, a.log_exit, a.lm, a.lm_end, a.W, a.S, a.alpha, a.N,
                  a.loglik, a.word_post, a.entry_post, a.post);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_posteriors_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                         size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d)", (long long)total_frames, (long long)n_utts, W, S);
  if (int rc = x_check_shape(W, S)) return rc;
  const size_t R = static_cast<size_t>(W) * sp_of(S);
  // alpha [total_frames][R] and N [total_frames][W], float64, each padded to 16
  *bytes = x_align16(static_cast<size_t>(total_frames) * R * sizeof(double)) +
           x_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(W) * sizeof(double));
  return 0;
}

extern "C" int sapr_connected_posteriors(const double *logb, const int64_t *offsets, int64_t n_utts,
                                         int64_t total_frames, const double *log_start, const double *log_trans,
                                         const double *log_exit, const double *lm, const double *lm_start,
                                         const double *lm_end, int32_t W, int32_t S, void *workspace,
                                         size_t workspace_bytes, double *loglik, double *word_post, double *entry_post,
                                         double *post, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = x_check_shape(W, S)) return rc;
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  size_t need = 0;
  if (int rc = sapr_connected_posteriors_workspace_bytes(total_frames, n_utts, W, S, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  SAPR_REQUIRE(n_utts <= 0x7fffffffLL, "grid too large (%lld utterances)", (long long)n_utts);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && loglik && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  LfArgs a;
  a.logb = logb;
  a.offsets = offsets;
  a.n_utts = n_utts;
  a.total_frames = total_frames;
  a.log_start = log_start;
  a.log_trans = log_trans;
  a.log_exit = log_exit;
  a.lm = lm;
  a.lm_start = lm_start;
  a.lm_end = lm_end;
  a.W = W;
  a.S = S;
  a.alpha = static_cast<double *>(workspace);
  a.N = reinterpret_cast<double *>(static_cast<uint8_t *>(workspace) +
                                   x_align16(static_cast<size_t>(total_frames) * R * sizeof(double)));
  a.loglik = loglik;
  a.word_post = word_post;
  a.entry_post = entry_post;
  a.post = post;
  a.backward = word_post || entry_post || post;
  hipStream_t st = as_stream(stream);
  return x_dispatch(SP, R, [&](auto rl, auto sp) {
    return launch_loop<decltype(rl)::value, decltype(sp)::value>(a, st);
  });
}
