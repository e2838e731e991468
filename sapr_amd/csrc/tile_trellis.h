// The emission-agnostic half of the per-model trellis (gmm_hmm.hip): every utterance under the ONE model of its tile
// (256 slots per tile: slot_utt, tile_model, model_tile_off — the layout of sapr_estep_diag), the recursions over
// logb[frame][SP] and the reductions of the statistics.  A family of emissions (the mixtures of gmm_hmm.hip, the full
// covariances of fullcov_ops.h) adds its two frame-parallel kernels on top of the tile helpers below; nothing here
// knows what an emission is.  Needs sapr_common.h; included INSIDE the unit's `namespace sapr { namespace {` like
// lse_ops.h and gmm_ops.h, which it includes itself.  The kernels are instantiated where launch_trellis is called: one
// translation unit only.
//
//   gmm_forward_kernel<SP, VIT>   one lane per utterance over logb: _hmmc.cpp forward_log (VIT: viterbi, the max
//        semiring, and its back-trace over the stored lattice).  Transitions whose log is -inf are skipped by a
//        wavefront-uniform branch (a bidiagonal matrix is just a sparse dense one: 2 S - 1 terms instead of S^2).
//   gmm_backward_kernel<SP>       backward_log, gamma (replaces the forward lattice in place; post / path are
//        written from the same registers), start, sum gamma and the xi sums in the linear domain, kept slot-major
//        (coalesced read-modify-write of the finite transitions only).
//   gmm_tile_reduce_kernel / gmm_reduce_kernel   the 256 slots of a tile in a fixed shape, then a model's partial
//        rows in tile order (kSub rows per tile for the family's observation sums).
// No floating-point atomics; every sum has one fixed order that depends only on the model's own tiles.
#pragma once

#include "lse_ops.h"
#include "gmm_ops.h"

constexpr int kBlock = 256;   // slots per tile
constexpr int kSub = 4;       // partial rows of the observation sums per tile
constexpr int kChunk = 64;    // flat frames per chunk of the accumulation pass
constexpr int kMaxT = 65535;  // (the emission grid's second dimension)

constexpr int stats_k1(int S) { return 2 + S + S * S + S; }  // n_seq, loglik, start, trans, post

struct Ws {
  double *logb, *lat, *ustat, *tile_stats, *part;
  size_t bytes;
};

// P: the width of the family's observation statistics
Ws carve(void *base, int64_t total_frames, int64_t n_tiles, int S, int P) {
  const size_t fr = static_cast<size_t>(total_frames > 0 ? total_frames : 1) * sp_of(S);
  const size_t nt = static_cast<size_t>(n_tiles > 0 ? n_tiles : 1);
  Ws w;
  w.logb = static_cast<double *>(base);
  w.lat = w.logb + fr;
  w.ustat = w.lat + fr;
  w.tile_stats = w.ustat + static_cast<size_t>(stats_k1(S)) * nt * kBlock;
  w.part = w.tile_stats + nt * stats_k1(S);
  w.bytes = (2 * fr + static_cast<size_t>(stats_k1(S)) * nt * kBlock + nt * stats_k1(S) + nt * kSub * P) *
            sizeof(double);
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

// the frame in the batch of flat frame `flat` of a scanned tile (0 <= flat < s_cum[256])
__device__ __forceinline__ int64_t flat_frame(const int32_t *s_cum, const int64_t *s_beg, int flat) {
  const int slot = find_slot(s_cum, flat);
  return s_beg[slot] + (flat - s_cum[slot]);
}

// -------------------------------------------------------------------------------------------
// the recursions, one lane per utterance, one wavefront per workgroup
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
// the reductions
// -------------------------------------------------------------------------------------------
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

// stats[w] = {n_seq, loglik, start[S], trans[S][S], post[S], the family's P observation sums} summed over the
// model's partial rows in tile order (kSub rows per tile for the observation sums); eight rows in flight
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
