// Gaussian-mixture HMMs (hmmlearn's GMMHMM, diagonal covariances) on gfx950: one E-step over a batch — loglik[u], the
// statistics rows stats[W][width], optionally the state posteriors post[total_frames][S] and their per-frame arg-max —
// and Viterbi decoding, every utterance under the ONE model of its tile (the tile layout of sapr_estep_diag: 256 slots
// per tile, slot_utt, tile_model, model_tile_off).  CPU restatement: tests/_gmmhmm_ref.py.
//
//   lc[t,s,m] = log w[s,m] - (D log 2 pi + sum_d log var[s,m,d] + sum_d (x[t,d] - mu[s,m,d])^2 / var[s,m,d]) / 2
//   logb[t,s] = logsumexp_m lc[t,s,m]          gamma_t(s) = softmax_s(fwd + bwd)
//   r[t,s,m]  = gamma_t(s) exp(lc[t,s,m] - logb[t,s])
//
// The mixture emission costs S M D subtract / multiply / FMA triples per frame and has no recurrence; the recursions
// are sequential in t and cost S^2 exponentials per frame.  So the work is cut where its dependence changes:
//   1  gmm_emit_kernel<MP, DP>       FRAME-parallel.  A tile's utterances are laid end to end ("flat" frames, slot
//        after slot: a scan of the 256 lengths in LDS and a binary search per thread), one workgroup per 256 flat
//        frames, the frame as DP doubles in registers, the tile's model wavefront-uniform (scalar loads).  Writes
//        logb[frame][SP].  The difference is squared directly (c0 sits near -300: the expanded form cancels).
//   2  gmm_forward_kernel<SP, VIT>   one lane per utterance over logb: _hmmc.cpp forward_log (VIT: viterbi, the max
//        semiring, and its back-trace over the stored lattice).  Transitions whose log is -inf are skipped by a
//        wavefront-uniform branch (a bidiagonal matrix is just a sparse dense one: 2 S - 1 terms instead of S^2).
//      gmm_backward_kernel<SP>       backward_log, gamma (replaces the forward lattice in place; post / path are
//        written from the same registers), start, sum gamma and the xi sums in the linear domain, kept slot-major
//        (coalesced read-modify-write of the finite transitions only).
//   3  gmm_accum_kernel<MP, DP>      FRAME-parallel again: chunks of 64 flat frames of a tile; phase A recomputes lc
//        (state per wavefront, frame per lane) and puts r into LDS, phase B is the product r^T [x, x^2, 1] with threads
//        owning (state, component, dimension) accumulators in registers over the workgroup's chunks (vector ALU,
//        float64; x^2 rounded to float32 first, as numpy squares a float32 feature array).  kSub partial rows per tile.
//      gmm_tile_reduce_kernel / gmm_reduce_kernel   the 256 slots of a tile in a fixed shape, then a model's partial
//        rows in tile order.
// No floating-point atomics; every sum has one fixed order that depends only on the model's own tiles, so results are
// bit-identical run to run and independent of which other models share the launch; loglik, post and path of an
// utterance are a function of its own (features, model) pair.
//
// Shapes are run-time values padded to a few instantiations: SP in {4, 10, 18} states (a padded state has log start
// and log transitions -inf and every component switched off), MP in {1, 2, 4, 8} components (a padded component has
// the constant -inf: exp(-inf) adds +0.0), DP in {13, 26, 39} dimensions (zero features against zero means and zero
// inverse variances add +0.0).  The pack (sapr_gmm_pack_layout) is built by the host in this padded form.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"

constexpr int kBlock = 256;   // slots per tile
constexpr int kSub = 4;       // partial rows of the observation sums per tile
constexpr int kChunk = 64;    // flat frames per chunk of the accumulation pass
constexpr int kMaxT = 65535;  // (the emission grid's second dimension)

constexpr int stats_k1(int S) { return 2 + S + S * S + S; }                 // n_seq, loglik, start, trans, post
constexpr int stats_p(int S, int M, int D) { return S * M * (2 * D + 1); }  // post_mix, obs, obs2

struct Ws {
  double *logb, *lat, *ustat, *tile_stats, *part;
  size_t bytes;
};

Ws carve(void *base, int64_t total_frames, int64_t n_tiles, int S, int M, int D) {
  const size_t fr = static_cast<size_t>(total_frames > 0 ? total_frames : 1) * sp_of(S);
  const size_t nt = static_cast<size_t>(n_tiles > 0 ? n_tiles : 1);
  Ws w;
  w.logb = static_cast<double *>(base);
  w.lat = w.logb + fr;
  w.ustat = w.lat + fr;
  w.tile_stats = w.ustat + static_cast<size_t>(stats_k1(S)) * nt * kBlock;
  w.part = w.tile_stats + nt * stats_k1(S);
  w.bytes = (2 * fr + static_cast<size_t>(stats_k1(S)) * nt * kBlock + nt * stats_k1(S) +
             nt * kSub * stats_p(S, M, D)) * sizeof(double);
  return w;
}

struct Batch {
  const float *feats;
  const int64_t *offsets;
  const int32_t *slot_utt, *tile_model;
  int64_t n_utts, total_frames, n_slots;
  int32_t D, max_T, W, S, M;
  int64_t stride;  // doubles per model of the pack
};

// the utterance of a slot: T = 0 for an empty slot and for anything that points outside the batch (never followed)
__device__ __forceinline__ Span slot_span(const Batch &b, int64_t slot, bool tile_ok) {
  return utt_span(b.offsets, b.slot_utt[slot], tile_ok, b.n_utts, b.total_frames, b.max_T);
}

// A tile's utterances end to end: s_cum[i] = frames of the slots before slot i (s_cum[256] = all), s_beg[i] = first
// frame of slot i in the batch.  Every thread of the 256-thread workgroup must call it.
__device__ __forceinline__ int tile_scan(const Batch &b, int64_t tile, bool tile_ok, int32_t *s_cum, int64_t *s_beg,
                                         int32_t *s_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const Span sp = slot_span(b, tile * kBlock + tid, tile_ok);
  s_beg[tid] = sp.beg;
  int incl = sp.T;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    incl += lane >= o ? up : 0;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) base += w < wv ? s_wave[w] : 0;
  s_cum[tid + 1] = base + incl;
  if (tid == 0) s_cum[0] = 0;
  __syncthreads();
  return s_cum[kBlock];
}

// the slot that owns flat frame `flat` (0 <= flat < s_cum[256]): s_cum[slot] <= flat < s_cum[slot + 1]
__device__ __forceinline__ int find_slot(const int32_t *s_cum, int flat) {
  int lo = 0, hi = kBlock;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int mid = (lo + hi) >> 1;
    const bool up = s_cum[mid] <= flat;
    lo = up ? mid : lo;
    hi = up ? hi : mid;
  }
  return lo;
}

// -------------------------------------------------------------------------------------------
// pass 1: logb[frame][SP]
// -------------------------------------------------------------------------------------------
template <int MP, int DP>
__global__ __launch_bounds__(kBlock) void gmm_emit_kernel(Batch b, const double *__restrict__ pack, int SP,
                                                          double *__restrict__ logb) {
  __shared__ int32_t s_cum[kBlock + 1];
  __shared__ int64_t s_beg[kBlock];
  __shared__ int32_t s_wave[kBlock / 64];
  const int64_t tile = blockIdx.x;
  const int w = b.tile_model[tile];
  const bool tile_ok = w >= 0 && w < b.W;
  const int total = tile_scan(b, tile, tile_ok, s_cum, s_beg, s_wave);
  const int64_t flat64 = static_cast<int64_t>(blockIdx.y) * kBlock + threadIdx.x;
  if (flat64 >= total) return;
  const int flat = static_cast<int>(flat64);
  const int slot = find_slot(s_cum, flat);
  const int64_t frame = s_beg[slot] + (flat - s_cum[slot]);
  double x[DP];
  load_frame_pad<DP>(b.feats + frame * b.D, b.D, true, x);
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * b.stride;  // wavefront-uniform
  const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
  const double *__restrict__ prm = cc + SP * MP;
  double *__restrict__ out = logb + frame * SP;
  for (int s = 0; s < SP; ++s) {
    double lc[MP];
    mix_log_terms<MP, DP>([&](int d) { return x[d]; }, prm + static_cast<int64_t>(s) * DP * MP * 2, cc + s * MP, lc);
    if constexpr (MP == 1)
      out[s] = lc[0];
    else
      out[s] = lse_all<MP>(lc);
  }
}

// -------------------------------------------------------------------------------------------
// pass 2: the recursions, one lane per utterance, one wavefront per workgroup
// -------------------------------------------------------------------------------------------
template <int SP, bool VIT>
__global__ __launch_bounds__(64) void gmm_forward_kernel(Batch b, const double *__restrict__ pack,
                                                         const double *__restrict__ logb,
                                                         double *__restrict__ lat, double *__restrict__ loglik,
                                                         int32_t *__restrict__ path) {
  const int64_t tile = blockIdx.x / (kBlock / 64);
  const int64_t slot = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
  const int w = b.tile_model[tile];
  const bool tile_ok = w >= 0 && w < b.W;
  const Span sp = slot_span(b, slot, tile_ok);
  if (sp.u < 0) return;
  const int T = sp.T;
  if (T <= 0) {
    loglik[sp.u] = neg_inf();
    return;
  }
  const double *__restrict__ mdl = pack + static_cast<int64_t>(tile_ok ? w : 0) * b.stride;  // wavefront-uniform
  const double *__restrict__ ls = mdl;
  const double *__restrict__ lt = mdl + SP;
  const double *__restrict__ ltT = lt + SP * SP;
  const double *__restrict__ lb = logb + sp.beg * SP;
  double *__restrict__ la = lat + sp.beg * SP;
  const int S = b.S;

  double fwd[SP], bn[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    fwd[s] = ls[s] + lb[s];
    la[s] = fwd[s];
  }
  if (T > 1) {
#pragma unroll
    for (int s = 0; s < SP; ++s) bn[s] = lb[SP + s];
  }
  for (int t = 1; t < T; ++t) {
    double bt[SP], prev[SP];
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      bt[s] = bn[s];
      prev[s] = fwd[s];
    }
    const int tn = t + 1 < T ? t + 1 : t;  // the next frame's row in flight under this frame's exponentials
#pragma unroll
    for (int s = 0; s < SP; ++s) bn[s] = lb[static_cast<int64_t>(tn) * SP + s];
    // state after state in a rolled loop over the model's own S states (a padded state keeps its -inf): column j of
    // the transition matrix is one run of scalar loads, and the value lands in register j by a uniform select
#pragma unroll 1
    for (int j = 0; j < S; ++j) {
      const double *__restrict__ col = ltT + j * SP;
      const double v = reduce_finite<SP, VIT>([&](int i) { return prev[i]; }, [&](int i) { return col[i]; });
#pragma unroll
      for (int k = 0; k < SP; ++k) fwd[k] = k == j ? v + bt[k] : fwd[k];
    }
#pragma unroll
    for (int s = 0; s < SP; ++s) la[static_cast<int64_t>(t) * SP + s] = fwd[s];
  }
  if constexpr (!VIT) {
    loglik[sp.u] = lse_all<SP>(fwd);
  } else {
    // _hmmc.cpp viterbi: the first maximum of the last row, then argmax_i (lattice[t][i] + log a[i][next]), first
    // maximum — the next state differs from lane to lane: its column is gathered from memory
    int st = argmax_first<SP>(fwd, S);
    double best = fwd[0];
#pragma unroll
    for (int s = 1; s < SP; ++s) best = s == st ? fwd[s] : best;
    loglik[sp.u] = best;
    int32_t *__restrict__ po = path + sp.beg;
    po[T - 1] = st;
    for (int t = T - 2; t >= 0; --t) {
      double cand[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) cand[i] = la[static_cast<int64_t>(t) * SP + i] + lt[i * SP + st];
      st = argmax_first<SP>(cand, S);
      po[t] = st;
    }
  }
}

template <int SP>
__global__ __launch_bounds__(64) void gmm_backward_kernel(Batch b, const double *__restrict__ pack,
                                                          const double *__restrict__ logb,
                                                          double *__restrict__ lat,
                                                          const double *__restrict__ loglik,
                                                          double *__restrict__ ustat, double *__restrict__ post,
                                                          int32_t *__restrict__ path) {
  const int S = b.S;
  const int K1 = stats_k1(S);
  const int64_t tile = blockIdx.x / (kBlock / 64);
  const int64_t slot = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
  const int w = b.tile_model[tile];
  const bool tile_ok = w >= 0 && w < b.W;
  const Span sp = slot_span(b, slot, tile_ok);
  double *__restrict__ us = ustat ? ustat + slot : nullptr;  // statistic k of this slot: us[k * n_slots]
  const int64_t ns = b.n_slots;
  if (us) {
    for (int k = 0; k < K1; ++k) us[k * ns] = 0.0;  // (an empty slot contributes zeros)
  }
  const int T = sp.T;
  if (T <= 0) return;
  const double *__restrict__ lt = pack + static_cast<int64_t>(w) * b.stride + SP;  // wavefront-uniform
  const double *__restrict__ lb = logb + sp.beg * SP;
  double *__restrict__ la = lat + sp.beg * SP;
  const double logprob = loglik[sp.u];

  double bwd[SP], psum[SP], fw[SP], g[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    bwd[s] = 0.0;
    psum[s] = 0.0;
    fw[s] = la[static_cast<int64_t>(T - 1) * SP + s];
  }
  for (int t = T - 1; t >= 0; --t) {
    // the rows of the step to t - 1 in flight under this frame's exponentials
    double bt[SP], fp[SP];
    const int tp = t >= 1 ? t - 1 : 0;
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      bt[s] = lb[static_cast<int64_t>(t) * SP + s];
      fp[s] = la[static_cast<int64_t>(tp) * SP + s];
    }
    // base.py _compute_posteriors_log: row soft-max of fwd + bwd as exp(lg - max) / sum
    double mx = fw[0] + bwd[0];
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      g[s] = fw[s] + bwd[s];
      mx = g[s] > mx ? g[s] : mx;
    }
    double den = 0.0;
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      g[s] = exp_unit(g[s] - mx);  // all -inf: NaN, as exp(lg - (-inf)) is in the reference
      den += g[s];
    }
    const double inv = 1.0 / den;
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      g[s] *= inv;
      psum[s] += g[s];
      la[static_cast<int64_t>(t) * SP + s] = g[s];  // gamma replaces the forward lattice in place
      if (t == 0 && us && s < S) us[static_cast<int64_t>(2 + s) * ns] = g[s];  // stats['start'] += posteriors[0]
    }
    if (post) {
      double *__restrict__ pr = post + (sp.beg + t) * S;
#pragma unroll
      for (int s = 0; s < SP; ++s)
        if (s < S) pr[s] = g[s];
    }
    if (path) path[sp.beg + t] = argmax_first<SP>(g, S);
    if (t == 0) break;
    // _hmmc.cpp backward_log: bwd_(t-1)[i] = logsumexp_j(log a_ij + b_t[j] + bwd_t[j]); xi_t(i, j) beside it
    double nb[SP];
#pragma unroll
    for (int j = 0; j < SP; ++j) {
      bt[j] += bwd[j];  // b_t[j] + bwd_t[j], the part of every term that depends on j alone
      nb[j] = neg_inf();
    }
    // row after row in a rolled loop over the model's own S states (as in the forward kernel)
#pragma unroll 1
    for (int i = 0; i < S; ++i) {
      const double *__restrict__ row = lt + i * SP;
      const double v = reduce_finite<SP, false>([&](int j) { return bt[j]; }, [&](int j) { return row[j]; });
      double fpi = fp[0];
#pragma unroll
      for (int k = 0; k < SP; ++k) {
        nb[k] = k == i ? v : nb[k];
        fpi = k == i ? fp[k] : fpi;
      }
      if (us) {
        const double base = fpi - logprob;
#pragma unroll
        for (int j = 0; j < SP; ++j) {
          const double a = row[j];
          if (j < S && a > neg_inf()) {  // (a padded state's column is -inf in a well-formed pack: never trusted)
            double *__restrict__ x = us + static_cast<int64_t>(2 + S + i * S + j) * ns;
            *x += exp_unit(base + a + bt[j]);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      bwd[s] = nb[s];
      fw[s] = fp[s];
    }
  }
  if (us) {
    us[0] = 1.0;
    us[ns] = logprob;
#pragma unroll
    for (int s = 0; s < SP; ++s)
      if (s < S) us[static_cast<int64_t>(2 + S + S * S + s) * ns] = psum[s];
  }
}

// -------------------------------------------------------------------------------------------
// pass 3: post_mix, obs, obs2 — kSub partial rows per tile
// -------------------------------------------------------------------------------------------
template <int MP>
constexpr int kStatesPerWave = MP >= 8 ? 1 : 8 / MP;  // a group of 4 * kStatesPerWave states = 32 (state, component) rows

template <int MP, int DP>
__global__ __launch_bounds__(kBlock) void gmm_accum_kernel(Batch b, const double *__restrict__ pack, int SP,
                                                           const double *__restrict__ gam,
                                                           double *__restrict__ part) {
  constexpr int NS = kStatesPerWave<MP>;
  constexpr int SG = 4 * NS;                       // states per group
  constexpr int RW = SG * MP;                      // = 32 rows of r per group
  constexpr int RS = RW | 1;                       // LDS row stride (doubles), odd
  constexpr int XS = DP + 2;                       // LDS row stride (floats): x[0..D), 1 at column D
  constexpr int QI = (RW * (DP + 1) + kBlock - 1) / kBlock;  // (row, column) accumulators per thread and group
  __shared__ int32_t s_cum[kBlock + 1];
  __shared__ int64_t s_beg[kBlock];
  __shared__ int32_t s_wave[kBlock / 64];
  __shared__ double s_r[kChunk * RS];
  __shared__ float s_x[kChunk * XS];

  const int S = b.S, M = b.M, D = b.D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (tells the compiler that a wavefront's state is uniform)
  const int64_t tile = blockIdx.x;
  const int w = b.tile_model[tile];
  const bool tile_ok = w >= 0 && w < b.W;
  const int total = tile_scan(b, tile, tile_ok, s_cum, s_beg, s_wave);
  const double *__restrict__ mdl = pack + static_cast<int64_t>(tile_ok ? w : 0) * b.stride;
  const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
  const double *__restrict__ prm = cc + SP * MP;

  // One group of SG states at a time over all of the workgroup's chunks (the features are read once per group: a
  // few times D float32 per frame, from L2): the accumulators of ONE group live in registers
  const int cols = D + 1;
  const int n_chunks = (total + kChunk - 1) / kChunk;
  double *__restrict__ out = part + (tile * kSub + blockIdx.y) * static_cast<int64_t>(stats_p(S, M, D));
  const float *__restrict__ xrow = s_x + lane * XS;
  for (int g = 0; g * SG < S; ++g) {  // (uniform trip counts: every thread reaches the barriers)
    double acc[QI], acc2[QI];
#pragma unroll
    for (int q = 0; q < QI; ++q) acc[q] = acc2[q] = 0.0;
    for (int c = blockIdx.y; c < n_chunks; c += kSub) {
      const int flat = c * kChunk + lane;
      const bool live = flat < total;
      int64_t frame = 0;
      if (live) {
        const int slot = find_slot(s_cum, flat);
        frame = s_beg[slot] + (flat - s_cum[slot]);
      }
      // the chunk's frames into LDS, float32 as they are: columns [0, D) the features, column D the ones behind
      // post_mix (against a padded dimension's zero mean and zero inverse variance it adds +0.0), zeros after it;
      // wavefront wv moves every fourth column of the 64 frames
      {
        const float *__restrict__ xp = b.feats + frame * D;
        for (int d = wv; d <= DP; d += kBlock / 64) {
          float v = 0.0f;
          if (live) v = d < D ? xp[d] : (d == D ? 1.0f : 0.0f);
          s_x[lane * XS + d] = v;
        }
      }
      __syncthreads();
      // ---- phase A: r of SG states for the chunk's 64 frames; wavefront wv owns NS of them --------------------
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        const int s = g * SG + wv * NS + n;
        double r[MP];
#pragma unroll
        for (int m = 0; m < MP; ++m) r[m] = 0.0;
        if (s < S) {  // (uniform)
          double lc[MP];
          mix_log_terms<MP, DP, 16 / MP>([&](int d) { return static_cast<double>(xrow[d]); },
                                prm + static_cast<int64_t>(s) * DP * MP * 2, cc + s * MP, lc);
          const double gm = live ? gam[frame * SP + s] : 0.0;
          double mx = lc[0];
#pragma unroll
          for (int m = 1; m < MP; ++m) mx = lc[m] > mx ? lc[m] : mx;
          double den = 0.0;
#pragma unroll
          for (int m = 0; m < MP; ++m) {
            r[m] = exp_unit(lc[m] - mx);
            den += r[m];
          }
          const double scale = gm / den;
          const bool off = mx == neg_inf() || !live;  // every component switched off: no responsibility
#pragma unroll
          for (int m = 0; m < MP; ++m) r[m] = off ? 0.0 : r[m] * scale;
        }
#pragma unroll
        for (int m = 0; m < MP; ++m) s_r[lane * RS + (wv * NS + n) * MP + m] = r[m];
      }
      __syncthreads();
      // ---- phase B: acc[row][col] += r[f][row] * x[f][col] over the chunk's frames, in frame order --------------
#pragma unroll
      for (int q = 0; q < QI; ++q) {
        const int item = tid + q * kBlock;
        if (item < RW * cols) {
          const int row = item / cols, col = item - row * cols;
          double a = acc[q], a2 = acc2[q];
#pragma unroll 8
          for (int f = 0; f < kChunk; ++f) {
            const double rv = s_r[f * RS + row];
            const float xf = s_x[f * XS + col];
            a = fma(rv, static_cast<double>(xf), a);
            a2 = fma(rv, static_cast<double>(xf * xf), a2);  // X**2 in float32, as numpy squares the array
          }
          acc[q] = a;
          acc2[q] = a2;
        }
      }
      __syncthreads();
    }
    // the group's part of the workgroup's partial row: post_mix[S][M], obs[S][M][D], obs2[S][M][D]
#pragma unroll
    for (int q = 0; q < QI; ++q) {
      const int item = tid + q * kBlock;
      if (item < RW * cols) {
        const int row = item / cols, col = item - row * cols;
        const int s = g * SG + row / MP, m = row % MP;
        if (s < S && m < M) {
          const int sm = s * M + m;
          if (col == D) {
            out[sm] = acc[q];
          } else {
            out[S * M + sm * D + col] = acc[q];
            out[S * M + S * M * D + sm * D + col] = acc2[q];
          }
        }
      }
    }
  }
}

// tile_stats[tile][k] = the statistic's 256 slot values added in one fixed shape: four per lane in slot order, then
// the butterfly over the wavefront's lanes.  One wavefront per statistic at a time, coalesced.
__global__ __launch_bounds__(kBlock) void gmm_tile_reduce_kernel(int K1, int64_t n_slots,
                                                                 const double *__restrict__ ustat,
                                                                 double *__restrict__ tile_stats) {
  const int64_t tile = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = wv; k < K1; k += kBlock / 64) {
    const double *__restrict__ src = ustat + static_cast<int64_t>(k) * n_slots + tile * kBlock + lane;
    double v = src[0];
    v += src[64];
    v += src[128];
    v += src[192];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) tile_stats[tile * K1 + k] = v;
  }
}

// stats[w] = {n_seq, loglik, start[S], trans[S][S], post[S], post_mix[S][M], obs[S][M][D], obs2[S][M][D]} summed over
// the model's partial rows in tile order (kSub rows per tile for the observation sums); eight rows in flight
__global__ void gmm_reduce_kernel(const int32_t *__restrict__ model_tile_off, int W, int K1, int P, int64_t n_tiles,
                                  const double *__restrict__ tile_stats, const double *__restrict__ part,
                                  double *__restrict__ stats) {
  const int Kw = K1 + P;
  const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (idx >= static_cast<int64_t>(W) * Kw) return;
  const int w = static_cast<int>(idx / Kw), k = static_cast<int>(idx - static_cast<int64_t>(w) * Kw);
  int64_t t0 = model_tile_off[w], t1 = model_tile_off[w + 1];
  t0 = t0 < 0 ? 0 : t0;  // (a table that points past the workspace's rows is cut, never followed)
  t1 = t1 > n_tiles ? n_tiles : t1;
  const int sub = k < K1 ? 1 : kSub;
  const double *__restrict__ src = k < K1 ? tile_stats + k : part + (k - K1);
  const int64_t stride = k < K1 ? K1 : P;
  double acc = 0.0;
  int64_t r = t0 * sub;
  const int64_t r1 = t1 * sub;
  for (; r + 8 <= r1; r += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = src[(r + i) * stride];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += v[i];
  }
  for (; r < r1; ++r) acc += src[r * stride];
  stats[idx] = acc;
}

// -------------------------------------------------------------------------------------------
// launches
// -------------------------------------------------------------------------------------------
template <int MP, int DP>
int launch_emit(const Batch &b, const double *pack, int64_t n_tiles, double *logb, hipStream_t stream) {
  SAPR_LAUNCH((gmm_emit_kernel<MP, DP>), dim3(static_cast<unsigned>(n_tiles), static_cast<unsigned>(b.max_T)),
              dim3(kBlock), 0, stream, b, pack, sp_of(b.S), logb);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int MP, int DP>
int launch_accum(const Batch &b, const double *pack, int64_t n_tiles, const double *gam, double *part, hipStream_t stream) {
  SAPR_LAUNCH((gmm_accum_kernel<MP, DP>), dim3(static_cast<unsigned>(n_tiles), kSub), dim3(kBlock), 0, stream, b,
              pack, sp_of(b.S), gam, part);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int MP>
int launch_frames_dp(bool emit, const Batch &b, const double *pack, int64_t n_tiles, double *a, double *c, hipStream_t stream) {
  switch (dp_of(b.D)) {
    case 13: return emit ? launch_emit<MP, 13>(b, pack, n_tiles, a, stream) : launch_accum<MP, 13>(b, pack, n_tiles, a, c, stream);
    case 26: return emit ? launch_emit<MP, 26>(b, pack, n_tiles, a, stream) : launch_accum<MP, 26>(b, pack, n_tiles, a, c, stream);
    default: return emit ? launch_emit<MP, 39>(b, pack, n_tiles, a, stream) : launch_accum<MP, 39>(b, pack, n_tiles, a, c, stream);
  }
}

// emit: a = logb; accumulate: a = gamma lattice, c = partial rows
int launch_frames(bool emit, const Batch &b, const double *pack, int64_t n_tiles, double *a, double *c, hipStream_t stream) {
  switch (mp_of(b.M)) {
    case 1: return launch_frames_dp<1>(emit, b, pack, n_tiles, a, c, stream);
    case 2: return launch_frames_dp<2>(emit, b, pack, n_tiles, a, c, stream);
    case 4: return launch_frames_dp<4>(emit, b, pack, n_tiles, a, c, stream);
    default: return launch_frames_dp<8>(emit, b, pack, n_tiles, a, c, stream);
  }
}

template <int SP>
int launch_trellis(bool vit, const Batch &b, const double *pack, int64_t n_tiles, const Ws &ws, double *loglik, double *ustat,
                   double *post, int32_t *path, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(n_tiles * (kBlock / 64))), block(64);
  if (vit) {
    SAPR_LAUNCH((gmm_forward_kernel<SP, true>), grid, block, 0, stream, b, pack, ws.logb, ws.lat, loglik, path);
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  SAPR_LAUNCH((gmm_forward_kernel<SP, false>), grid, block, 0, stream, b, pack, ws.logb, ws.lat, loglik,
              static_cast<int32_t *>(nullptr));
  SAPR_HIP_TRY(hipGetLastError());
  if (!ustat && !post && !path) return 0;  // scores only
  SAPR_LAUNCH((gmm_backward_kernel<SP>), grid, block, 0, stream, b, pack, ws.logb, ws.lat, loglik, ustat, post,
              path);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

int run(bool vit, const float *feats, const int64_t *offsets, const int32_t *slot_utt, const int32_t *tile_model,
        const int32_t *model_tile_off, int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T,
        const double *pack, int32_t W, int32_t S, int32_t M, void *workspace, size_t workspace_bytes, double *loglik,
        double *stats, double *post, int32_t *path, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && n_tiles >= 0 && W > 0 && S > 0 && M > 0 && D > 0 && max_T >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld n_tiles=%lld W=%d S=%d M=%d D=%d max_T=%d)", (long long)n_utts,
               (long long)total_frames, (long long)n_tiles, W, S, M, D, max_T);
  if (int rc = check_shape(S, M, D)) return rc;
  SAPR_REQUIRE(max_T <= kMaxT, "bad sizes: max_T = %d exceeds %d", max_T, kMaxT);
  SAPR_REQUIRE(n_tiles * (kBlock / 64) <= 0x7fffffffLL, "grid too large (%lld tiles)", (long long)n_tiles);
  if (n_tiles == 0) return 0;
  SAPR_REQUIRE(feats && offsets && slot_utt && tile_model && pack && workspace && loglik, "NULL pointer argument");
  SAPR_REQUIRE(!vit || path, "NULL pointer argument (path)");
  SAPR_REQUIRE(!stats || model_tile_off, "NULL pointer argument (model_tile_off)");
  const Ws ws = carve(workspace, total_frames, n_tiles, S, M, D);
  SAPR_REQUIRE(workspace_bytes >= ws.bytes, "workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
  Batch b;
  b.feats = feats;
  b.offsets = offsets;
  b.slot_utt = slot_utt;
  b.tile_model = tile_model;
  b.n_utts = n_utts;
  b.total_frames = total_frames;
  b.n_slots = n_tiles * kBlock;
  b.D = D;
  b.max_T = max_T;
  b.W = W;
  b.S = S;
  b.M = M;
  b.stride = static_cast<int64_t>(model_doubles(sp_of(S), mp_of(M), dp_of(D)));
  hipStream_t st = as_stream(stream);
  if (max_T > 0 && total_frames > 0) {
    if (int rc = launch_frames(true, b, pack, n_tiles, ws.logb, nullptr, st)) return rc;
  }
  double *ustat = stats ? ws.ustat : nullptr;
  int rc;
  switch (sp_of(S)) {
    case 4: rc = launch_trellis<4>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    case 10: rc = launch_trellis<10>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    default: rc = launch_trellis<18>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
  }
  if (rc || !stats) return rc;
  if (int rc2 = launch_frames(false, b, pack, n_tiles, ws.lat, ws.part, st)) return rc2;
  const int K1 = stats_k1(S), P = stats_p(S, M, D);
  SAPR_LAUNCH(gmm_tile_reduce_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(kBlock), 0, st, K1, b.n_slots,
              ws.ustat, ws.tile_stats);
  SAPR_HIP_TRY(hipGetLastError());
  const int64_t total = static_cast<int64_t>(W) * (K1 + P);
  SAPR_LAUNCH(gmm_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, model_tile_off, W,
              K1, P, n_tiles, ws.tile_stats, ws.part, stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_gmm_stats_width(int32_t S, int32_t M, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && M > 0 && D > 0, "bad sizes (S=%d M=%d D=%d)", S, M, D);
  if (int rc = check_shape(S, M, D)) return rc;
  *width = stats_k1(S) + stats_p(S, M, D);
  return 0;
}

extern "C" int sapr_gmm_pack_layout(int32_t S, int32_t M, int32_t D, int32_t *SP, int32_t *MP, int32_t *DP,
                                    size_t *doubles_per_model) {
  SAPR_REQUIRE(SP && MP && DP && doubles_per_model && S > 0 && M > 0 && D > 0, "bad sizes (S=%d M=%d D=%d)", S, M, D);
  if (int rc = check_shape(S, M, D)) return rc;
  *SP = sp_of(S);
  *MP = mp_of(M);
  *DP = dp_of(D);
  *doubles_per_model = model_doubles(*SP, *MP, *DP);
  return 0;
}

extern "C" int sapr_gmm_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t M, int32_t D,
                                        size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_tiles >= 0 && S > 0 && M > 0 && D > 0,
               "bad sizes (total_frames=%lld n_tiles=%lld S=%d M=%d D=%d)", (long long)total_frames, (long long)n_tiles,
               S, M, D);
  if (int rc = check_shape(S, M, D)) return rc;
  *bytes = carve(nullptr, total_frames, n_tiles, S, M, D).bytes;
  return 0;
}

extern "C" int sapr_gmm_estep_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                   const int32_t *tile_model, const int32_t *model_tile_off, int64_t n_utts,
                                   int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, const double *pack,
                                   int32_t W, int32_t S, int32_t M, void *workspace, size_t workspace_bytes,
                                   double *loglik, double *stats, double *post, int32_t *path, void *stream) {
  return run(false, feats, offsets, slot_utt, tile_model, model_tile_off, n_utts, total_frames, n_tiles, D, max_T, pack,
             W, S, M, workspace, workspace_bytes, loglik, stats, post, path, stream);
}

extern "C" int sapr_gmm_viterbi_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                     const int32_t *tile_model, int64_t n_utts, int64_t total_frames, int64_t n_tiles,
                                     int32_t D, int32_t max_T, const double *pack, int32_t W, int32_t S, int32_t M,
                                     void *workspace, size_t workspace_bytes, double *logprob, int32_t *path,
                                     void *stream) {
  return run(true, feats, offsets, slot_utt, tile_model, nullptr, n_utts, total_frames, n_tiles, D, max_T, pack, W, S,
             M, workspace, workspace_bytes, logprob, nullptr, nullptr, path, stream);
}

// -------------------------------------------------------------------------------------------
// full covariances (hmmlearn's GaussianHMM, covariance_type "full" / "tied"): the emission and the accumulation pass
// of fullcov_ops.h around the recursions above
// -------------------------------------------------------------------------------------------
namespace sapr {
namespace {

#include "fullcov_ops.h"

Ws carve_full(void *base, int64_t total_frames, int64_t n_tiles, int S, int D) {
  const size_t fr = static_cast<size_t>(total_frames > 0 ? total_frames : 1) * sp_of(S);
  const size_t nt = static_cast<size_t>(n_tiles > 0 ? n_tiles : 1);
  Ws w;
  w.logb = static_cast<double *>(base);
  w.lat = w.logb + fr;
  w.ustat = w.lat + fr;
  w.tile_stats = w.ustat + static_cast<size_t>(stats_k1(S)) * nt * kBlock;
  w.part = w.tile_stats + nt * stats_k1(S);
  w.bytes = (2 * fr + static_cast<size_t>(stats_k1(S)) * nt * kBlock + nt * stats_k1(S) +
             nt * kSub * full_stats_p(S, D)) * sizeof(double);
  return w;
}

template <int DP>
int launch_full_emit(const Batch &b, const double *pack, int64_t n_tiles, double *logb, hipStream_t stream) {
  SAPR_LAUNCH((full_emit_kernel<DP>), dim3(static_cast<unsigned>(n_tiles), static_cast<unsigned>(b.max_T)),
              dim3(kBlock), 0, stream, b, pack, sp_of(b.S), logb);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int DP>
int launch_full_accum(const Batch &b, int64_t n_tiles, const double *gam, double *part, hipStream_t stream) {
  SAPR_LAUNCH((full_accum_kernel<DP>), dim3(static_cast<unsigned>(n_tiles), kSub), dim3(kBlock), 0, stream, b,
              sp_of(b.S), gam, part);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

int run_full(bool vit, const float *feats, const int64_t *offsets, const int32_t *slot_utt, const int32_t *tile_model,
             const int32_t *model_tile_off, int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D,
             int32_t max_T, const double *pack, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
             double *loglik, double *stats, double *post, int32_t *path, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && n_tiles >= 0 && W > 0 && S > 0 && D > 0 && max_T >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld n_tiles=%lld W=%d S=%d D=%d max_T=%d)", (long long)n_utts,
               (long long)total_frames, (long long)n_tiles, W, S, D, max_T);
  if (int rc = check_full_shape(S, D)) return rc;
  SAPR_REQUIRE(max_T <= kMaxT, "bad sizes: max_T = %d exceeds %d", max_T, kMaxT);
  SAPR_REQUIRE(n_tiles * (kBlock / 64) <= 0x7fffffffLL, "grid too large (%lld tiles)", (long long)n_tiles);
  if (n_tiles == 0) return 0;
  SAPR_REQUIRE(feats && offsets && slot_utt && tile_model && pack && workspace && loglik, "NULL pointer argument");
  SAPR_REQUIRE(!vit || path, "NULL pointer argument (path)");
  SAPR_REQUIRE(!stats || model_tile_off, "NULL pointer argument (model_tile_off)");
  const Ws ws = carve_full(workspace, total_frames, n_tiles, S, D);
  SAPR_REQUIRE(workspace_bytes >= ws.bytes, "workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
  Batch b;
  b.feats = feats;
  b.offsets = offsets;
  b.slot_utt = slot_utt;
  b.tile_model = tile_model;
  b.n_utts = n_utts;
  b.total_frames = total_frames;
  b.n_slots = n_tiles * kBlock;
  b.D = D;
  b.max_T = max_T;
  b.W = W;
  b.S = S;
  b.M = 1;
  b.stride = static_cast<int64_t>(full_model_doubles(sp_of(S), dp_of(D)));
  hipStream_t st = as_stream(stream);
  if (max_T > 0 && total_frames > 0) {
    int rc;
    switch (dp_of(D)) {
      case 13: rc = launch_full_emit<13>(b, pack, n_tiles, ws.logb, st); break;
      case 26: rc = launch_full_emit<26>(b, pack, n_tiles, ws.logb, st); break;
      default: rc = launch_full_emit<39>(b, pack, n_tiles, ws.logb, st); break;
    }
    if (rc) return rc;
  }
  double *ustat = stats ? ws.ustat : nullptr;
  int rc;
  switch (sp_of(S)) {
    case 4: rc = launch_trellis<4>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    case 10: rc = launch_trellis<10>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    default: rc = launch_trellis<18>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
  }
  if (rc || !stats) return rc;
  switch (dp_of(D)) {
    case 13: rc = launch_full_accum<13>(b, n_tiles, ws.lat, ws.part, st); break;
    case 26: rc = launch_full_accum<26>(b, n_tiles, ws.lat, ws.part, st); break;
    default: rc = launch_full_accum<39>(b, n_tiles, ws.lat, ws.part, st); break;
  }
  if (rc) return rc;
  const int K1 = stats_k1(S), P = full_stats_p(S, D);
  SAPR_LAUNCH(gmm_tile_reduce_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(kBlock), 0, st, K1, b.n_slots,
              ws.ustat, ws.tile_stats);
  SAPR_HIP_TRY(hipGetLastError());
  const int64_t total = static_cast<int64_t>(W) * (K1 + P);
  SAPR_LAUNCH(gmm_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, model_tile_off, W,
              K1, P, n_tiles, ws.tile_stats, ws.part, stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sapr

extern "C" int sapr_full_pack_layout(int32_t S, int32_t D, int32_t *SP, int32_t *DP, size_t *doubles_per_model) {
  SAPR_REQUIRE(SP && DP && doubles_per_model && S > 0 && D > 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = check_full_shape(S, D)) return rc;
  *SP = sp_of(S);
  *DP = dp_of(D);
  *doubles_per_model = full_model_doubles(*SP, *DP);
  return 0;
}

extern "C" int sapr_full_stats_width(int32_t S, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && D > 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = check_full_shape(S, D)) return rc;
  *width = stats_k1(S) + full_stats_p(S, D);
  return 0;
}

extern "C" int sapr_full_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_tiles >= 0 && S > 0 && D > 0,
               "bad sizes (total_frames=%lld n_tiles=%lld S=%d D=%d)", (long long)total_frames, (long long)n_tiles, S,
               D);
  if (int rc = check_full_shape(S, D)) return rc;
  *bytes = carve_full(nullptr, total_frames, n_tiles, S, D).bytes;
  return 0;
}

extern "C" int sapr_full_estep(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                               const int32_t *tile_model, const int32_t *model_tile_off, int64_t n_utts,
                               int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, const double *pack,
                               int32_t W, int32_t S, void *workspace, size_t workspace_bytes, double *loglik,
                               double *stats, double *post, int32_t *path, void *stream) {
  return run_full(false, feats, offsets, slot_utt, tile_model, model_tile_off, n_utts, total_frames, n_tiles, D, max_T,
                  pack, W, S, workspace, workspace_bytes, loglik, stats, post, path, stream);
}

extern "C" int sapr_full_viterbi(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                 const int32_t *tile_model, int64_t n_utts, int64_t total_frames, int64_t n_tiles,
                                 int32_t D, int32_t max_T, const double *pack, int32_t W, int32_t S, void *workspace,
                                 size_t workspace_bytes, double *logprob, int32_t *path, void *stream) {
  return run_full(true, feats, offsets, slot_utt, tile_model, nullptr, n_utts, total_frames, n_tiles, D, max_T, pack, W,
                  S, workspace, workspace_bytes, logprob, nullptr, nullptr, path, stream);
}
