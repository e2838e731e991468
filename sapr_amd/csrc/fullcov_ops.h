// The full-covariance family of the per-model trellis (hmmlearn's GaussianHMM with covariance_type "full" or "tied"; a
// tied model is packed as S copies of its one matrix): its two frame-parallel kernels over the tile helpers of
// tile_trellis.h and its family description (Full) for run<Family> of gmm_hmm.hip.  Needs sapr_common.h; included
// INSIDE the unit's `namespace sapr { namespace {` like the headers it includes.  CPU restatement:
// tests/_fullcov_ref.py.
//
//   Sigma_s = L_s L_s^T        Winv_s = L_s^-1 (lower triangular, from the host)
//   logb[t,s] = c_s - 1/2 sum_i (sum_{j<=i} Winv_s[i][j] (x_j - mu_s[j]))^2       c_s = -(D log 2 pi + log|Sigma_s|) / 2
//
// The pack keeps the head every family's pack has (log_start[SP], log_trans[SP][SP], its transpose), so the recursions,
// the posteriors, both decoders, the xi sums and the reductions of tile_trellis.h run unchanged over logb; the two
// frame-parallel passes are the family's own:
//   full_emit_kernel<DP>    one thread per flat frame, the frame as DP doubles in registers, the tile's model
//                           wavefront-uniform (scalar loads); row after row of Winv_s with one running dot product
//   full_accum_kernel<DP>   obs[s] = sum_t gamma_t(s) x_t and oo[s] = sum_t gamma_t(s) x_t x_t^T as weighted Gram
//                           products on the float64 matrix cores, four frames per v_mfma_f64_16x16x4_f64: A = gamma x[a],
//                           B = x[b], the constant 1 in column DP of B carries obs.  Only the 16 x 16 tiles on or above
//                           the diagonal are computed; both halves of oo are written from the upper one.
#pragma once

#include "tile_trellis.h"
#include "fullcov_emit.h"

typedef double f64x4_full __attribute__((ext_vector_type(4)));

constexpr int full_stats_p(int S, int D) { return S * D + S * D * D; }  // obs, oo

// -------------------------------------------------------------------------------------------
// pass 1: logb[frame][SP]
// -------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kBlock) void full_emit_kernel(Batch b, const double *__restrict__ pack, int SP,
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
  const int64_t frame = flat_frame(s_cum, s_beg, static_cast<int>(flat64));
  double x[DP];
  load_frame_pad<DP>(b.feats + frame * b.D, b.D, true, x);
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * b.stride;  // wavefront-uniform
  const double *__restrict__ cc = mdl + SP + 2 * SP * SP;
  const double *__restrict__ mu = cc + SP;
  const double *__restrict__ wi = mu + SP * DP;
  double *__restrict__ out = logb + frame * SP;
#pragma unroll 1
  for (int s = 0; s < SP; ++s) {
    // row after row of Winv_s with one running dot product (fullcov_emit.h, shared with full_vocab.hip)
    out[s] = full_log_density<DP>([&](int d) { return x[d]; }, mu + s * DP, wi + static_cast<int64_t>(s) * DP * DP,
                                  cc[s]);
  }
}

// -------------------------------------------------------------------------------------------
// pass 3: obs[S][D], oo[S][D][D] — kSub partial rows per tile
// -------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(kBlock) void full_accum_kernel(Batch b, int SP, const double *__restrict__ gam,
                                                            double *__restrict__ part) {
  constexpr int NT = (DP + 1 + 15) / 16;       // 16-wide tiles per side: x[0..DP) and the constant 1 at column DP
  constexpr int NTU = NT * (NT + 1) / 2;       // tiles on or above the diagonal
  constexpr int XS = NT == 2 ? 48 : 16 * NT;   // LDS row stride (doubles): four consecutive rows on distinct banks
  constexpr int GS = kMaxS + 1;                // LDS row stride of gamma (doubles), odd
  constexpr int T1 = DP / 16, N1 = DP % 16;    // where the constant 1 sits
  constexpr int NI = kChunk * XS / kBlock;     // staged values per thread and chunk: features ...
  constexpr int NG = (kChunk * kMaxS + kBlock - 1) / kBlock;  // ... and gamma
  static_assert(NI * kBlock == kChunk * XS, "the staging loop covers the chunk exactly");
  __shared__ int32_t s_cum[kBlock + 1];
  __shared__ int64_t s_beg[kBlock];
  __shared__ int32_t s_wave[kBlock / 64];
  __shared__ int64_t s_frame[kChunk];
  __shared__ double s_x[kChunk * XS];
  __shared__ double s_g[kChunk * GS];

  const int S = b.S, D = b.D;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, k = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t tile = blockIdx.x;
  const int w = b.tile_model[tile];
  const bool tile_ok = w >= 0 && w < b.W;
  const int total = tile_scan(b, tile, tile_ok, s_cum, s_beg, s_wave);
  const int n_chunks = (total + kChunk - 1) / kChunk;
  int64_t frame0 = 0;  // the tile's first frame: an address that is always valid while a chunk is staged
  if (total > 0) frame0 = s_beg[find_slot(s_cum, 0)];
  double *__restrict__ out = part + (tile * kSub + blockIdx.y) * static_cast<int64_t>(full_stats_p(S, D));
  double *__restrict__ out_oo = out + S * D;

  // four states at a time, one per wavefront, over all of the workgroup's chunks: the accumulators of ONE state live in
  // a wavefront's registers (the features are staged again for every group, from L2)
  for (int g = 0; g * 4 < S; ++g) {  // (uniform trip counts: every thread reaches the barriers)
    const int s = g * 4 + wv;
    f64x4_full acc[NTU];
#pragma unroll
    for (int tau = 0; tau < NTU; ++tau) acc[tau] = f64x4_full{0.0, 0.0, 0.0, 0.0};
    for (int c = blockIdx.y; c < n_chunks; c += kSub) {
      if (tid < kChunk) {
        const int flat = c * kChunk + tid;
        int64_t frame = -1;
        if (flat < total) frame = flat_frame(s_cum, s_beg, flat);
        s_frame[tid] = frame;
      }
      __syncthreads();
      // the chunk's frames into LDS as float64: columns [0, D) the features, column DP the ones behind obs, zeros
      // elsewhere and in the rows past the tile's last frame.  Every load is issued before the first value is used
      // (a dead item reads the tile's first frame instead of branching), so a chunk costs one round trip, not NI
      float xv[NI];
      double gv[NG];
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int item = tid + q * kBlock, f = item / XS, col = item - f * XS;
        const int64_t frame = s_frame[f];
        xv[q] = b.feats[(frame >= 0 && col < D) ? frame * D + col : frame0 * D];
      }
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const int item = tid + q * kBlock, f = item / SP, st = item - f * SP;
        const int64_t frame = item < kChunk * SP ? s_frame[f] : -1;
        gv[q] = gam[(frame >= 0 ? frame : frame0) * SP + (frame >= 0 ? st : 0)];
      }
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int item = tid + q * kBlock, f = item / XS, col = item - f * XS;
        const bool live = s_frame[f] >= 0;
        s_x[item] = live ? (col < D ? static_cast<double>(xv[q]) : (col == DP ? 1.0 : 0.0)) : 0.0;
      }
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const int item = tid + q * kBlock, f = item / SP, st = item - f * SP;
        if (item < kChunk * SP) s_g[f * GS + st] = s_frame[f] >= 0 ? gv[q] : 0.0;
      }
      __syncthreads();
      if (s < S) {  // (uniform)
#pragma unroll 2
        for (int step = 0; step < kChunk / 4; ++step) {
          // A and B of the float64 MFMA: lane & 15 = row (column), lane >> 4 = the K index, here the frame
          const int f = 4 * step + k;
          const double gm = s_g[f * GS + s];
          double xa[NT], xb[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            xb[t] = s_x[f * XS + 16 * t + n];
            xa[t] = gm * xb[t];
          }
          int tau = 0;
#pragma unroll
          for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = ti; tj < NT; ++tj, ++tau)
              acc[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[ti], xb[tj], acc[tau], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    if (s < S) {
      // C of the float64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register.  The entries on or above the
      // diagonal go to both halves of oo[s]; column DP of the last tile column is obs[s]
      int tau = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = ti; tj < NT; ++tj, ++tau)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 16 * ti + k + 4 * r, bc = 16 * tj + n;
            const double v = acc[tau][r];
            if (a < D) {
              if (bc < D && a <= bc) {
                out_oo[(static_cast<int64_t>(s) * D + a) * D + bc] = v;
                out_oo[(static_cast<int64_t>(s) * D + bc) * D + a] = v;
              }
              if (tj == T1 && n == N1) out[s * D + a] = v;
            }
          }
    }
  }
}

// -------------------------------------------------------------------------------------------
// the family description (gmm_hmm.hip: run<Family>); there are no components: M is passed as 1 and ignored
// -------------------------------------------------------------------------------------------
struct Full {
  static int check(int32_t S, int32_t, int32_t D) { return check_full_shape(S, D); }
  static size_t model_doubles(int S, int, int D) { return full_model_doubles(sp_of(S), dp_of(D)); }
  static int stats_p(int S, int, int D) { return full_stats_p(S, D); }
  static int launch_emit(const Batch &b, const double *pack, int64_t n_tiles, double *logb, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(n_tiles), static_cast<unsigned>(b.max_T));
    switch (dp_of(b.D)) {
      case 13: SAPR_LAUNCH(full_emit_kernel<13>, grid, dim3(kBlock), 0, stream, b, pack, sp_of(b.S), logb); break;
      case 26: SAPR_LAUNCH(full_emit_kernel<26>, grid, dim3(kBlock), 0, stream, b, pack, sp_of(b.S), logb); break;
      default: SAPR_LAUNCH(full_emit_kernel<39>, grid, dim3(kBlock), 0, stream, b, pack, sp_of(b.S), logb); break;
    }
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  static int launch_accum(const Batch &b, const double *, int64_t n_tiles, const double *gam, double *part,
                          hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(n_tiles), kSub);
    switch (dp_of(b.D)) {
      case 13: SAPR_LAUNCH(full_accum_kernel<13>, grid, dim3(kBlock), 0, stream, b, sp_of(b.S), gam, part); break;
      case 26: SAPR_LAUNCH(full_accum_kernel<26>, grid, dim3(kBlock), 0, stream, b, sp_of(b.S), gam, part); break;
      default: SAPR_LAUNCH(full_accum_kernel<39>, grid, dim3(kBlock), 0, stream, b, sp_of(b.S), gam, part); break;
    }
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
};
