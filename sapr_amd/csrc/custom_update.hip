// The training accumulators of the reference's from-scratch HMM: update_B's means and full covariances
// (assignment2/custom_hmm.py:366-400), the sums over sequences baum_welch keeps (:434-439) and the flat-start
// statistics (:70-92).  CPU restatement: oracle/custom_hmm_oracle.py.
//
//   folds       update_b_fold_kernel (list order), ordered_fold_lds_kernel (list order through LDS: the flat
//               start), update_b_fold_tree_kernel (fixed tree: the default; SAPR_CUSTOM_FOLD=ordered picks list order)
//   update_B    update_b_utt_sums_kernel + update_b_scatter_kernel: any shape, several models;
//               update_b_sums_lane_kernel + update_b_scatter_lane_kernel: one model, D = 13;
//               update_b_moments_mfma_kernel: both passes as one on the matrix cores (one model, D = 13, S <= 16)
//   flat start  custom_global_sum_kernel; custom_global_cov_kernel, or global_cov_mfma_kernel at D = 13
// Each entry point picks by (utt_model, W, D) and the fold switch: the branch table of DESIGN.md section 5.2.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "sapr_common.h"

namespace sapr {
namespace {

#include "custom_np.h"

// update_B (custom_hmm.py:366-400) is two-pass: means first, then covariances about the NEW means.
// Both passes are split into a part that is parallel over utterances and an ordered combination, so
// that they scale to 10^5 utterances and can be summed across ranks between the passes:
//
//   pass 1   update_b_utt_sums_kernel   one lane per (utterance, state, dim): the reference's
//                                       np.sum(gamma[:, j:j+1] * features.T, axis=0) of ONE sequence
//                                       (frames in order) -> part[u][j][d], occ_part[u][j]
//            update_b_fold_kernel       one lane per (model, state, dim): adds the per-sequence sums in
//                                       LIST ORDER, exactly like the reference's loop over sequences
//                                       -> unnormalised sum_x[w][j][d], occ[w][j]
//   pass 2   update_b_scatter_kernel    one lane per (chunk of >= 32 utterances, model, state, a, b):
//                                       sum gamma * (x_a - mu_a)(x_b - mu_b) over the chunk
//            update_b_fold_kernel       chunks in order -> unnormalised scatter[w][j][a][b]
//   custom_normalise_kernel             x / occ where occ > 0 (host: symmetrise, floor the diagonal)
// utterances per pass-2 chunk: 32, or more when that would exceed the 65535 (chunk, model) rows of one grid
__host__ __device__ inline int64_t chunk_utts(int64_t n_utts, int W) {
  const int64_t need = (n_utts * W + 65534) / 65535;
  return need > 32 ? need : 32;
}

// gamma (t, j) of utterance u: reference row layout [total_frames][S] (lane_slots == 0) or the batched
// E-step's lane-contiguous [max_T][S][lane_slots]
// one frame-major feature row as 16-byte pieces (rows are 4-byte aligned: D floats back to back)
struct __attribute__((packed, aligned(4))) RowQuad {
  float a, b, c, d;
};
template <int D>
__device__ __forceinline__ void load_row_f32(const float *__restrict__ p, float (&f)[D]) {
  constexpr int Q = D / 4;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const RowQuad v = *reinterpret_cast<const RowQuad *>(p + 4 * q);
    f[4 * q] = v.a, f[4 * q + 1] = v.b, f[4 * q + 2] = v.c, f[4 * q + 3] = v.d;
  }
#pragma unroll
  for (int d = 4 * Q; d < D; ++d) f[d] = p[d];
}

__device__ __forceinline__ double gamma_at(const double *__restrict__ gamma, int64_t lane_slots, int64_t u, int64_t beg,
                                           int t, int j, int S) {
  return lane_slots ? gamma[(static_cast<int64_t>(t) * S + j) * lane_slots + u] : gamma[(beg + t) * S + j];
}

__global__ void update_b_utt_sums_kernel(const float *__restrict__ feats, const int64_t *__restrict__ offsets,
                                         int64_t n_utts, int D, int S, const double *__restrict__ gamma,
                                         int64_t lane_slots, double *__restrict__ part,
                                         double *__restrict__ occ_part) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (idx >= n_utts * S * D) return;
  const int64_t u = idx / (S * D);
  const int j = static_cast<int>((idx / D) % S), d = static_cast<int>(idx % D);
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  double mu = 0.0, ou = 0.0;
  if (j != 0 && j != S - 1) {
    for (int t = 0; t < T; ++t) {
      const double g = gamma_at(gamma, lane_slots, u, beg, t, j, S);
      mu += g * static_cast<double>(feats[(beg + t) * D + d]);
      ou += g;
    }
  }
  part[idx] = mu;
  if (d == 0) occ_part[u * S + j] = ou;
}

// out[w][k] = sum over rows r (in order) with row_model(r) == w of part[r][k].  Rows are utterances
// (row_model = utt_model, or model 0 when NULL) or, `interleaved`, (chunk, model) pairs: row r belongs
// to model r % W.
template <bool ALL>
__device__ __forceinline__ double fold_rows(const double *__restrict__ part, const int32_t *__restrict__ row_model,
                                            int64_t r, int64_t step, int64_t n_rows, int w, int64_t K, int64_t k) {
  // the adds stay in row order; the loads of kAhead rows are issued together so the loop runs at the add
  // latency instead of the memory latency (a row is its own cache line: 64 of them in flight per lane)
  constexpr int kAhead = ALL ? 64 : 16;
  double acc = 0.0;
  for (; r + (kAhead - 1) * step < n_rows; r += kAhead * step) {
    double v[kAhead];
    int mw[ALL ? 1 : kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int64_t ri = r + i * step;
      v[i] = part[ri * K + k];
      if constexpr (!ALL) mw[i] = row_model[ri];
    }
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the first add waits on one
#pragma unroll
    for (int i = 0; i < kAhead; ++i) acc = (ALL || mw[ALL ? 0 : i] == w) ? acc + v[i] : acc;
  }
  for (; r < n_rows; r += step)
    if (ALL || row_model[r] == w) acc += part[r * K + k];
  return acc;
}

__global__ __launch_bounds__(64) void update_b_fold_kernel(const double *__restrict__ part,
                                                           const int32_t *__restrict__ row_model, int64_t n_rows,
                                                           int W, int64_t K, int interleaved,
                                                           double *__restrict__ out) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (idx >= W * K) return;
  const int w = static_cast<int>(idx / K);
  const int64_t k = idx - static_cast<int64_t>(w) * K;
  if (interleaved)
    out[idx] = fold_rows<true>(part, row_model, w, W, n_rows, w, K, k);
  else if (row_model == nullptr)  // model 0 owns every row when there is no map
    out[idx] = w == 0 ? fold_rows<true>(part, row_model, 0, 1, n_rows, w, K, k) : 0.0;
  else
    out[idx] = fold_rows<false>(part, row_model, 0, 1, n_rows, w, K, k);
}

// The list-order fold of ONE model's rows with the rows staged through LDS (round 4): out[k] = sum_r part[r][k], rows
// added one after another in row order — the chain of update_b_fold_kernel, bit for bit — but the chain's wavefront
// reads its rows from LDS while the other fifteen wavefronts of the workgroup copy the next tile of rows in with
// 16-byte loads.  update_b_fold_kernel's one wavefront fetched its own rows (13 of 64 lanes, 16 rows in flight) and
// ran at the memory latency: 1.30 ms per 100 000 rows of 13 sums; here the chain of dependent float64 additions is
// the critical path.  K <= 64 columns, one workgroup.
constexpr int kFoldLdsDoubles = 6144;  // per buffer (48 KB); two buffers
__global__ __launch_bounds__(1024) void ordered_fold_lds_kernel(const double *__restrict__ part, int64_t n_rows, int K,
                                                                double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) double buf[2][kFoldLdsDoubles];
  const int tid = threadIdx.x;
  const int tile_rows = (kFoldLdsDoubles / K) & ~1;  // even: a tile starts on a 16-byte boundary of `part`
  const int64_t n_tiles = (n_rows + tile_rows - 1) / tile_rows;
  auto stage = [&](int64_t tile, int b, int first_thread, int n_threads) {
    const int64_t r0 = tile * tile_rows;
    const int64_t rows = (r0 + tile_rows <= n_rows) ? tile_rows : (n_rows - r0);
    const int64_t n = rows * K, n2 = n >> 1;
    const double2 *src = reinterpret_cast<const double2 *>(part + r0 * K);
    double2 *dst = reinterpret_cast<double2 *>(buf[b]);
    int64_t i = tid - first_thread;
    for (; i + 3 * n_threads < n2; i += 4 * n_threads) {  // four 16-byte loads in flight per thread
      const double2 v0 = src[i], v1 = src[i + n_threads], v2 = src[i + 2 * n_threads], v3 = src[i + 3 * n_threads];
      dst[i] = v0;
      dst[i + n_threads] = v1;
      dst[i + 2 * n_threads] = v2;
      dst[i + 3 * n_threads] = v3;
    }
    for (; i < n2; i += n_threads) dst[i] = src[i];
    if ((n & 1) && tid == first_thread) buf[b][n - 1] = part[r0 * K + n - 1];
  };
  double acc = 0.0;
  if (n_tiles > 0) stage(0, 0, 0, 1024);
  __syncthreads();
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    const int b = static_cast<int>(tile & 1);
    if (tid >= 64) {  // wavefronts 1-15: next tile -> the other buffer
      if (tile + 1 < n_tiles) stage(tile + 1, b ^ 1, 64, 960);
    } else if (tid < K) {  // wavefront 0, one lane per column: the sequential chain
      const int64_t r0 = tile * tile_rows;
      const int rows = static_cast<int>((r0 + tile_rows <= n_rows) ? tile_rows : (n_rows - r0));
      const double *p = buf[b] + tid;
      int r = 0;
      for (; r + 16 <= rows; r += 16) {
        double v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = p[(r + i) * K];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc += v[i];
      }
      for (; r < rows; ++r) acc += p[r * K];
    }
    __syncthreads();
  }
  if (tid < K) out[tid] = acc;
}
// list-order fold of all rows (one model): the LDS-staged chain where it applies
inline void launch_ordered_fold(hipStream_t st, const double *part, int64_t n_rows, int64_t K, double *out) {
  if (K <= 64 && (reinterpret_cast<uintptr_t>(part) & 15) == 0)
    SAPR_LAUNCH(ordered_fold_lds_kernel, dim3(1), dim3(1024), 0, st, part, n_rows, static_cast<int>(K), out);
  else
    SAPR_LAUNCH(update_b_fold_kernel, dim3(static_cast<unsigned>((K + 63) / 64)), dim3(64), 0, st, part,
                static_cast<const int32_t *>(nullptr), n_rows, 1, K, 0, out);
}

// The same sums as a FIXED-SHAPE TREE (round 3, the default of the per-iteration folds): a workgroup owns eight
// neighbouring columns of one model (one 64-byte line per row); its 32 row lanes each add every 32nd row of the model
// (four accumulators, rows r, r + 32, r + 64, r + 96 of a lane's sequence), then the 4 x 32 partial sums meet in a
// fixed LDS tree.  The shape depends on (n_rows, W, K) only, so the result is deterministic and the same on every
// rank — but its roundings are not the list-order chain's: differences of a few ulp, far inside the 1e-7 the golden
// Baum-Welch histories are compared at (north star: 1e-5 on log-likelihoods).  The ordered kernel above stays for
// the flat-start sums (bit-identical global mean) and behind SAPR_CUSTOM_FOLD=ordered.
__global__ __launch_bounds__(256) void update_b_fold_tree_kernel(const double *__restrict__ part,
                                                                 const int32_t *__restrict__ row_model, int64_t n_rows,
                                                                 int W, int64_t K, int interleaved,
                                                                 double *__restrict__ out) {
  __shared__ double red[256];
  const int kk = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int64_t kblocks = (K + 7) / 8;
  const int w = static_cast<int>(blockIdx.x / kblocks);
  const int64_t k = (blockIdx.x - static_cast<int64_t>(w) * kblocks) * 8 + kk;
  if (gridDim.y > 1) {  // two-level fold (launch_fold): this block takes the blockIdx.y-th run of rows -> out[run][W][K]
    const int64_t per = (n_rows + gridDim.y - 1) / gridDim.y, lo = per * blockIdx.y;
    const int64_t hi = lo + per < n_rows ? lo + per : n_rows;
    part += lo * K;
    n_rows = hi > lo ? hi - lo : 0;
    out += static_cast<int64_t>(blockIdx.y) * W * K;
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (k < K && (interleaved || row_model != nullptr || w == 0)) {
    // rows of this model: interleaved -> r % W == w; mapped -> row_model[r] == w; neither -> all rows (model 0)
    const int64_t first = interleaved ? w + static_cast<int64_t>(rg) * W : rg;
    const int64_t step = interleaved ? 32 * static_cast<int64_t>(W) : 32;
    const bool mapped = !interleaved && row_model != nullptr;
    int64_t r = first;
    for (; r + 3 * step < n_rows; r += 4 * step) {
      const double v0 = part[r * K + k], v1 = part[(r + step) * K + k];
      const double v2 = part[(r + 2 * step) * K + k], v3 = part[(r + 3 * step) * K + k];
      if (mapped) {
        a0 += row_model[r] == w ? v0 : 0.0;
        a1 += row_model[r + step] == w ? v1 : 0.0;
        a2 += row_model[r + 2 * step] == w ? v2 : 0.0;
        a3 += row_model[r + 3 * step] == w ? v3 : 0.0;
      } else {
        a0 += v0;
        a1 += v1;
        a2 += v2;
        a3 += v3;
      }
    }
    for (; r < n_rows; r += step)
      if (!mapped || row_model[r] == w) a0 += part[r * K + k];
  }
  red[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
#pragma unroll
  for (int sft = 128; sft >= 8; sft >>= 1) {
    if (threadIdx.x < sft) red[threadIdx.x] += red[threadIdx.x + sft];
    __syncthreads();
  }
  if (threadIdx.x < 8 && k < K) out[static_cast<int64_t>(w) * K + k] = red[threadIdx.x];
}

// per-iteration folds: the tree unless SAPR_CUSTOM_FOLD=ordered asks for the reference's list order
inline bool fold_ordered() {
  const char *e = std::getenv("SAPR_CUSTOM_FOLD");
  return e && std::strcmp(e, "ordered") == 0;
}
inline void launch_fold(hipStream_t st, const double *part, const int32_t *row_model, int64_t n_rows, int W, int64_t K,
                        int interleaved, double *out) {
  if (fold_ordered()) {
    SAPR_LAUNCH(update_b_fold_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(W) * K + 63) / 64)), dim3(64), 0, st,
                part, row_model, n_rows, W, K, interleaved, out);
  } else {
    const unsigned gx = static_cast<unsigned>(static_cast<int64_t>(W) * ((K + 7) / 8));
    // many rows, few columns (the E-step's 100 000 per-utterance rows of 112 sums: 14 workgroups read 90 MB, 0.39 ms):
    // 128 runs of rows first, on a stream-ordered scratch buffer, then the 128 partial rows — same fixed shape for
    // every rank, 0.39 -> see DESIGN 4.4
    void *scratch = nullptr;
    constexpr unsigned kRuns = 128;
    if (n_rows >= 8192 && gx < 64 && W == 1 && row_model == nullptr && !interleaved &&
        hipMallocAsync(&scratch, static_cast<size_t>(kRuns) * K * sizeof(double), st) == hipSuccess) {
      SAPR_LAUNCH(update_b_fold_tree_kernel, dim3(gx, kRuns), dim3(256), 0, st, part, row_model, n_rows, W, K, 0,
                  static_cast<double *>(scratch));
      SAPR_LAUNCH(update_b_fold_tree_kernel, dim3(gx), dim3(256), 0, st, static_cast<const double *>(scratch), row_model,
                  static_cast<int64_t>(kRuns), W, K, 0, out);
      (void)hipFreeAsync(scratch, st);
      return;
    }
    SAPR_LAUNCH(update_b_fold_tree_kernel, dim3(gx), dim3(256), 0, st, part, row_model, n_rows, W, K, interleaved, out);
  }
}

__global__ void update_b_scatter_kernel(const float *__restrict__ feats, const int64_t *__restrict__ offsets,
                                        const int32_t *__restrict__ utt_model, int64_t n_utts, int64_t per_chunk,
                                        int W, int D, int S, const double *__restrict__ gamma, int64_t lane_slots,
                                        const double *__restrict__ means, double *__restrict__ part) {
  // blockIdx.y = chunk * W + w ; blockIdx.x / threadIdx.x walk (j, a, b)
  const int K = S * D * D;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int64_t chunk = blockIdx.y / W;
  const int w = static_cast<int>(blockIdx.y % W);
  const int j = k / (D * D), a = (k / D) % D, b = k % D;
  double c = 0.0;
  if (j != 0 && j != S - 1) {
    const double ma = means[(w * S + j) * D + a], mb = means[(w * S + j) * D + b];
    const int64_t u0 = chunk * per_chunk, u1 = u0 + per_chunk < n_utts ? u0 + per_chunk : n_utts;
    for (int64_t u = u0; u < u1; ++u) {
      if ((utt_model ? utt_model[u] : 0) != w) continue;
      const int64_t beg = offsets[u];
      const int T = static_cast<int>(offsets[u + 1] - beg);
      for (int t = 0; t < T; ++t) {
        const double da = static_cast<double>(feats[(beg + t) * D + a]) - ma;
        const double db = static_cast<double>(feats[(beg + t) * D + b]) - mb;
        c += gamma_at(gamma, lane_slots, u, beg, t, j, S) * (da * db);
      }
    }
  }
  part[static_cast<int64_t>(blockIdx.y) * K + k] = c;
}

// pass 2 for ONE model (utt_model == NULL) and compile-time D: one lane per utterance, one state per
// workgroup row, the D (D + 1) / 2 distinct entries of the symmetric scatter matrix in registers; the
// 256 lanes of a tile are then combined in a fixed order (xor-butterfly inside the wavefront, wavefronts
// in sequence).  Each term is gamma * (da * db) exactly as in update_b_scatter_kernel; only the order of
// the additions differs (the reference's own order is that of a BLAS matmul).
__device__ __forceinline__ double wave_sum_f64c(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The two lane kernels below: block (tile of 256 utterances, emitting state), one lane per utterance of the tile.
struct LaneTile {
  int64_t tile, u, beg;  // the tile, this lane's utterance and its first frame
  int j, T;              // emitting state 1 .. S-2; frames of the utterance (0 past the last utterance)
};
__device__ __forceinline__ LaneTile lane_tile(const int64_t *__restrict__ offsets, int64_t n_utts) {
  LaneTile lt;
  lt.tile = blockIdx.x;
  lt.j = blockIdx.y + 1;
  lt.u = lt.tile * 256 + threadIdx.x;
  const bool live = lt.u < n_utts;
  lt.beg = live ? offsets[lt.u] : 0;
  lt.T = live ? static_cast<int>(offsets[lt.u + 1] - lt.beg) : 0;
  return lt;
}
// N per-lane values -> per-tile values in a fixed order: butterfly inside the wavefront, then (after the barrier this
// ends on) tile_sum adds the four wavefronts in sequence
template <int N>
__device__ __forceinline__ void tile_reduce(const double (&v)[N], double (&red)[4][N]) {
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double s = wave_sum_f64c(v[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
}
template <int N>
__device__ __forceinline__ double tile_sum(const double (&red)[4][N], int i) {
  return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}
// rows 0 and S - 1 (the non-emitting states) of one tile's [S][per] block of partial sums
__device__ __forceinline__ void zero_end_rows(double *__restrict__ block, int S, int per) {
  for (int k = threadIdx.x; k < per; k += 256) {
    block[k] = 0.0;
    block[static_cast<int64_t>(S - 1) * per + k] = 0.0;
  }
}

template <int D>
__global__ __launch_bounds__(256) void update_b_scatter_lane_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, int64_t n_utts, int S,
    const double *__restrict__ gamma, int64_t lane_slots, const double *__restrict__ means,
    double *__restrict__ part) {
  constexpr int kTri = D * (D + 1) / 2;
  __shared__ double red[4][kTri];
  const auto [tile, u, beg, j, T] = lane_tile(offsets, n_utts);
  double mu[D];
#pragma unroll
  for (int d = 0; d < D; ++d) mu[d] = means[j * D + d];
  double acc[kTri];
#pragma unroll
  for (int i = 0; i < kTri; ++i) acc[i] = 0.0;
  // The next frame's row and posterior are in flight under the 104 float64 operations of the current one (at two
  // wavefronts per SIMD — 182 accumulator registers — nothing else covers the loads).  acc += (g dx_a) dx_b: one
  // multiplication per dimension and one fused multiply-add per entry, where g (dx_a dx_b) took two operations per
  // entry; same value to a rounding (the reference rounds the product, then the scaling, then the sum).
  float xf[D];
  double g = 0.0;
  if (T > 0) {
    load_row_f32<D>(feats + beg * D, xf);
    g = gamma_at(gamma, lane_slots, u, beg, 0, j, S);
  }
  for (int t = 0; t < T; ++t) {
    double dx[D], gdx[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      dx[d] = static_cast<double>(xf[d]) - mu[d];
      gdx[d] = g * dx[d];
    }
    if (t + 1 < T) {
      load_row_f32<D>(feats + (beg + t + 1) * D, xf);
      g = gamma_at(gamma, lane_slots, u, beg, t + 1, j, S);
    }
    int i = 0;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a; b < D; ++b) {
        acc[i] = __builtin_fma(gdx[a], dx[b], acc[i]);
        ++i;
      }
  }
  tile_reduce(acc, red);
  // part[tile][j][a][b] (rows of the fold kernel are tiles; states 0 and S-1 stay zero)
  double *dst = part + static_cast<int64_t>(tile) * S * D * D + static_cast<int64_t>(j) * D * D;
  for (int k = threadIdx.x; k < D * D; k += 256) {
    const int a = k / D, b = k % D;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    dst[k] = tile_sum(red, lo * D - lo * (lo - 1) / 2 + (hi - lo));
  }
  if (blockIdx.y == 0) zero_end_rows(part + static_cast<int64_t>(tile) * S * D * D, S, D * D);
}

// x[w][j][...] /= occ[w][j] where occ > 0 (`per` trailing values per state)
__global__ void custom_normalise_kernel(double *__restrict__ x, const double *__restrict__ occ, int64_t n_states,
                                        int per) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (idx >= n_states * per) return;
  const double o = occ[idx / per];
  if (o > 0) x[idx] /= o;
}

// flat start (custom_hmm.py:70-92): per-utterance float32 row sums in numpy's pair-wise order, then a
// float64 accumulation in utterance order; and sum of centred outer products.

// part[u][d] = np.sum(feature, axis=1)[d] of ONE (D,T) float32 array: float32 pair-wise over the T values
// (parallel over utterances); update_b_fold_kernel then adds the utterances in list order in float64
__global__ void custom_global_sum_kernel(const float *__restrict__ feats, const int64_t *__restrict__ offsets,
                                         int64_t n_utts, int D, double *__restrict__ part) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (idx >= n_utts * D) return;
  const int64_t u = idx / D;
  const int d = static_cast<int>(idx - u * D);
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  part[idx] = static_cast<double>(np_pairwise<float, 8>(feats + beg * D + d, T, D));
}

// part[chunk][a][b] = sum over the chunk's frames of (x_a - mean_a)(x_b - mean_b); chunks are folded in order
constexpr int kChunkFrames = 4096;
__global__ void custom_global_cov_kernel(const float *__restrict__ feats, int64_t total_frames, int D,
                                         const double *__restrict__ mean, double *__restrict__ part) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= D * D) return;
  const int a = idx / D, b = idx % D;
  const double ma = mean[a], mb = mean[b];
  const int64_t f0 = static_cast<int64_t>(blockIdx.y) * kChunkFrames;
  const int64_t f1 = f0 + kChunkFrames < total_frames ? f0 + kChunkFrames : total_frames;
  double c = 0.0;
  for (int64_t f = f0; f < f1; ++f)
    c += (static_cast<double>(feats[f * D + a]) - ma) * (static_cast<double>(feats[f * D + b]) - mb);
  part[static_cast<int64_t>(blockIdx.y) * D * D + idx] = c;
}

// pass 1 for one model and D-dimensional features, lane per utterance (the layout the gamma lattice wants: one
// coalesced 512-byte row per wavefront and frame; update_b_utt_sums_kernel's lane per (utterance, state, dimension)
// touches five rows of it per wavefront load): block (tile of 256 utterances, emitting state) -> part[tile][S][D],
// occ_part[tile][S]; the fold then runs over tiles.  Fixed-shape sums (butterfly inside a wavefront, the four
// wavefronts in order): deterministic, a few ulp from the per-utterance chain, which SAPR_CUSTOM_FOLD=ordered keeps.
template <int D>
__global__ __launch_bounds__(256) void update_b_sums_lane_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, int64_t n_utts, int S,
    const double *__restrict__ gamma, int64_t lane_slots, double *__restrict__ part, double *__restrict__ occ_part) {
  __shared__ double red[4][D + 1];
  const auto [tile, u, beg, j, T] = lane_tile(offsets, n_utts);
  double acc[D + 1];  // [D]: the occupancy
#pragma unroll
  for (int d = 0; d <= D; ++d) acc[d] = 0.0;
  for (int t = 0; t < T; ++t) {
    const double g = gamma_at(gamma, lane_slots, u, beg, t, j, S);
    float xf[D];
    load_row_f32<D>(feats + (beg + t) * D, xf);
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] += g * static_cast<double>(xf[d]);
    acc[D] += g;
  }
  tile_reduce(acc, red);
  double *dst = part + (static_cast<int64_t>(tile) * S + j) * D;
  if (threadIdx.x < D) dst[threadIdx.x] = tile_sum(red, threadIdx.x);
  if (threadIdx.x == D) occ_part[tile * S + j] = tile_sum(red, D);
  if (blockIdx.y == 0) {
    zero_end_rows(part + static_cast<int64_t>(tile) * S * D, S, D);
    zero_end_rows(occ_part + tile * S, S, 1);
  }
}

// ---------------------------------------------------------------------------------------
// update_B as ONE pass of weighted moments on the float64 matrix cores (round 3b; single model, D = 13).
// custom_hmm.py:366-400 is two passes over the data — means, then covariances about the NEW means; both are
// functions of the posterior-weighted moments of the frames about any fixed centre c (x' = x - c):
//     occ_s = sum g_s,   s1_s = sum g_s x',   S2_s = sum g_s x' x'^T
//     mean_s = c + s1_s / occ_s,   cov_s = S2_s / occ_s - d d^T  with  d = s1_s / occ_s
// (algebraically the reference's values; with c = the global mean the subtraction loses about one digit of sixteen).
// All states at once: Gamma (states x rows) times Y (rows x 105), Y = [the 91 products x'_a x'_b (a <= b) | x' | 1],
// one row per (utterance, frame).  v_mfma_f64_16x16x4_f64: M = state, N = column of Y (7 tiles), K = 4 rows — the
// same frame of four neighbouring utterances, so a wavefront's posterior reads of a (frame, state) fall into one
// 128-byte line of the slot-major lattice and every feature row is read once, 52 bytes at a time in sequence.
// The lane-per-utterance kernels this replaces (update_b_sums_lane / update_b_scatter_lane: 1.4 + 1.7 ms per
// 100 000 utterances) re-read the rows once per state through an L1 that 64 private rows per wavefront thrash.
// A wavefront owns 16 utterances at a time (persistent, strided), stages the four rows of a step in its own 2 KB
// of LDS as float64 and forms Y's entries from two ds_read_b64 each.  Partial tiles -> part[wavefront][16][112].
// ---------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kMomCols = 112;  // 7 tiles of 16: 91 pairs, 13 linear, the constant, 7 unused
template <int D>
__global__ __launch_bounds__(256) void update_b_moments_mfma_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, int64_t n_utts, int S,
    const double *__restrict__ gamma, int64_t lane_slots, const double *__restrict__ center,
    double *__restrict__ part) {
  static_assert(D * (D + 1) / 2 + D + 1 <= kMomCols && D <= 13, "column layout");
  constexpr int kTri = D * (D + 1) / 2, NTile = kMomCols / 16;
  __shared__ double s_rows[4][4][4][16];  // [wavefront][group][k][x' (D), 1, 0, 0]
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, n = lane & 15, k = lane >> 4;
  // the two factors of this lane's column in every tile: indices into a staged row (13 = the constant 1, 14 = 0)
  int ia[NTile], ib[NTile];
#pragma unroll
  for (int tau = 0; tau < NTile; ++tau) {
    const int c = 16 * tau + n;
    int a = 14, b = 14;
    if (c < kTri) {
      int rest = c;
      a = 0;
      while (rest >= D - a) {  // row a of the upper triangle holds D - a entries
        rest -= D - a;
        ++a;
      }
      b = a + rest;
    } else if (c < kTri + D) {
      a = c - kTri;
      b = 13;
    } else if (c == kTri + D) {
      a = b = 13;
    }
    ia[tau] = a;
    ib[tau] = b;
  }
  const double cen = n < D ? center[n] : 0.0;
  f64x4 acc[NTile];
#pragma unroll
  for (int tau = 0; tau < NTile; ++tau) acc[tau] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t n_blocks = (n_utts + 15) / 16;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * 4, wid = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  const bool emitting = n >= 1 && n <= S - 2;  // A rows: the state is the lane's n
  for (int64_t blk = wid; blk < n_blocks; blk += n_waves) {
    int64_t beg[4], utt[4];
    int T[4];
    int Tmax = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      utt[g] = blk * 16 + 4 * g + k;
      const bool live = utt[g] < n_utts;
      beg[g] = live ? offsets[utt[g]] : 0;
      T[g] = live ? static_cast<int>(offsets[utt[g] + 1] - beg[g]) : 0;
      Tmax = T[g] > Tmax ? T[g] : Tmax;
    }
    Tmax = wave_max_i32(Tmax);
    // the next step's feature values and posteriors are fetched before this step's products: at three wavefronts
    // per SIMD nothing else covers the round trip between a step's loads and its 28 MFMAs
    float xn[4];
    double an[4];
    auto fetch = [&](int t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        xn[g] = (n < D && t < T[g]) ? feats[(beg[g] + t) * D + n] : 0.0f;
        an[g] = (emitting && t < T[g]) ? gamma_at(gamma, lane_slots, utt[g], beg[g], t, n, S) : 0.0;
      }
    };
    if (Tmax > 0) fetch(0);
    for (int t = 0; t < Tmax; ++t) {
      // stage: row (group g, k) = frame t of utterance 16 blk + 4 g + k, as x' with the constants behind it
      double a[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        s_rows[wave][g][k][n] = n < D ? static_cast<double>(xn[g]) - cen : (n == 13 ? 1.0 : 0.0);
        a[g] = an[g];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (t + 1 < Tmax) fetch(t + 1);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double *row = s_rows[wave][g][k];
#pragma unroll
        for (int tau = 0; tau < NTile; ++tau)
          acc[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g], row[ia[tau]] * row[ib[tau]], acc[tau], 0, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  // C/D of the float64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
  double *dst = part + wid * 16 * kMomCols;
#pragma unroll
  for (int tau = 0; tau < NTile; ++tau)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(k + 4 * r) * kMomCols + 16 * tau + n] = acc[tau][r];
}

// Flat-start covariance sum (custom_hmm.py:81-92) as a Gram product on the float64 matrix cores: with x' = x - mean,
// C[a][b] = sum over frames of x'_a x'_b is A^T A for A = (frames x D), so ONE v_mfma_f64_16x16x4_f64 takes four
// frames: lane (n, k) loads x[4 g + k][n] once — 52 contiguous bytes per frame — and hands x' to the instruction as
// BOTH operands.  (custom_global_cov_kernel reads two values per entry and frame: 338 loads per frame.)  Persistent
// wavefronts, two accumulators in flight, partial 16 x 16 tiles -> part[wavefront][256].
template <int D>
__global__ __launch_bounds__(256) void global_cov_mfma_kernel(const float *__restrict__ feats, int64_t total_frames,
                                                              const double *__restrict__ mean,
                                                              double *__restrict__ part) {
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, n = lane & 15, k = lane >> 4;
  const double mu = n < D ? mean[n] : 0.0;
  const int64_t n_groups = (total_frames + 3) / 4;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * 4, wid = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  auto fetch = [&](int64_t g) {
    const int64_t f = 4 * g + k;
    return (n < D && g < n_groups && f < total_frames) ? static_cast<double>(feats[f * D + n]) - mu : 0.0;
  };
  for (int64_t g = wid; g < n_groups; g += 2 * n_waves) {
    const double v0 = fetch(g), v1 = fetch(g + n_waves);
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v1, acc1, 0, 0, 0);
  }
  double *dst = part + wid * 256;
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[(k + 4 * r) * 16 + n] = acc0[r] + acc1[r];  // row = (lane >> 4) + 4 r, column = lane & 15
}
__global__ void global_cov_unpack_kernel(const double *__restrict__ tile, int D, double *__restrict__ cov_out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < D * D) cov_out[idx] = tile[(idx / D) * 16 + idx % D];
}

}  // namespace
}  // namespace sapr

using namespace sapr;

constexpr int kMomWaves = 4096;  // persistent wavefronts of the moments kernel = rows of its fold
static size_t update_b_ws_doubles(int64_t n_utts, int W, int D, int S) {
  const int64_t n = n_utts > 0 ? n_utts : 1;
  const int64_t per = chunk_utts(n, W);
  const int64_t chunks = (n + per - 1) / per;
  const size_t pass1 = static_cast<size_t>(n) * S * D + static_cast<size_t>(n) * S;
  const size_t pass2 = static_cast<size_t>(chunks) * W * S * D * D;  // also covers the (fewer) 256-utterance tiles
  const size_t mom = static_cast<size_t>(kMomWaves) * 16 * kMomCols;  // sapr_custom_update_b_moments
  const size_t m = pass1 > pass2 ? pass1 : pass2;
  return m > mom ? m : mom;
}

static int check_update_b_ws(size_t ws_bytes, int64_t n_utts, int W, int D, int S) {
  const size_t need = update_b_ws_doubles(n_utts, W, D, S) * sizeof(double);
  if (ws_bytes < need) return fail(SAPR_ERR_WORKSPACE, "workspace too small: %zu < %zu", ws_bytes, need);
  return 0;
}

extern "C" int sapr_custom_update_b_workspace_bytes(int64_t n_utts, int32_t W, int32_t D, int32_t S, size_t *bytes) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(bytes && n_utts >= 0 && W > 0, "bad arguments");
  *bytes = update_b_ws_doubles(n_utts, W, D, S) * sizeof(double);
  return 0;
}

// pass 1, unnormalised: sum_x[W][S][D] and occ[W][S] of this rank's utterances (reference order)
extern "C" int sapr_custom_update_b_sums(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                         int64_t n_utts, int32_t W, int32_t D, int32_t S, const double *gamma,
                                         int64_t lane_slots, double *sum_x_out, double *occ_out, void *workspace,
                                         size_t ws_bytes, void *stream) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0 && W > 0, "bad sizes");
  SAPR_REQUIRE(feats && offsets && gamma && sum_x_out && occ_out && workspace, "NULL pointer argument");
  if (int rc = check_update_b_ws(ws_bytes, n_utts, W, D, S)) return rc;
  hipStream_t st = as_stream(stream);
  double *part = static_cast<double *>(workspace);
  double *occ_part = part + static_cast<size_t>(n_utts) * S * D;
  if (utt_model == nullptr && W == 1 && D == 13 && n_utts > 0 && S > 2 && !fold_ordered()) {
    const int64_t tiles = (n_utts + 255) / 256;
    double *occ_tiles = part + static_cast<size_t>(tiles) * S * D;
    SAPR_LAUNCH((update_b_sums_lane_kernel<13>), dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(S - 2)),
                dim3(256), 0, st, feats, offsets, n_utts, S, gamma, lane_slots, part, occ_tiles);
    launch_fold(st, part, nullptr, tiles, 1, static_cast<int64_t>(S) * D, 0, sum_x_out);
    launch_fold(st, occ_tiles, nullptr, tiles, 1, static_cast<int64_t>(S), 0, occ_out);
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  const int64_t n1 = n_utts * S * D;
  if (n1 > 0)
    SAPR_LAUNCH(update_b_utt_sums_kernel, dim3(static_cast<unsigned>((n1 + 255) / 256)), dim3(256), 0, st, feats,
                offsets, n_utts, D, S, gamma, lane_slots, part, occ_part);
  const int64_t k1 = static_cast<int64_t>(S) * D, k2 = S;
  launch_fold(st, part, utt_model, n_utts, W, k1, 0, sum_x_out);
  launch_fold(st, occ_part, utt_model, n_utts, W, k2, 0, occ_out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// both passes as one: out[16][112] = posterior-weighted moments about `center` of this rank's utterances for ONE
// model with 13-dimensional features — row s (states 1 .. S-2, other rows zero): columns 0..90 the upper triangle of
// sum g x'x'^T (row by row), 91..103 sum g x', 104 sum g.  The caller sums across ranks, then
// mean = center + s1 / occ, cov = S2 / occ - (s1 / occ)(s1 / occ)^T.
extern "C" int sapr_custom_update_b_moments(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D,
                                            int32_t S, const double *gamma, int64_t lane_slots, const double *center,
                                            double *out, void *workspace, size_t ws_bytes, void *stream) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0, "bad sizes");
  SAPR_REQUIRE(feats && offsets && gamma && center && out && workspace, "NULL pointer argument");
  if (D != 13 || S > 16) return fail(SAPR_ERR_UNSUPPORTED, "moments kernel: D = 13 and at most 16 states (got %d, %d)", D, S);
  if (int rc = check_update_b_ws(ws_bytes, n_utts, 1, D, S)) return rc;
  hipStream_t st = as_stream(stream);
  double *part = static_cast<double *>(workspace);
  const int64_t n_blocks = (n_utts + 15) / 16;
  int64_t waves = n_blocks < kMomWaves ? n_blocks : kMomWaves;
  if (waves < 1) waves = 1;
  const unsigned grid = static_cast<unsigned>((waves + 3) / 4);
  SAPR_LAUNCH((update_b_moments_mfma_kernel<13>), dim3(grid), dim3(256), 0, st, feats, offsets, n_utts, S, gamma,
              lane_slots, center, part);
  launch_fold(st, part, nullptr, static_cast<int64_t>(grid) * 4, 1, static_cast<int64_t>(16) * kMomCols, 0, out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// pass 2, unnormalised: scatter[W][S][D][D] = sum gamma * outer(x - means, x - means) of this rank's utterances
extern "C" int sapr_custom_update_b_scatter(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                            int64_t n_utts, int32_t W, int32_t D, int32_t S, const double *gamma,
                                            int64_t lane_slots, const double *means, double *scatter_out,
                                            void *workspace, size_t ws_bytes, void *stream) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0 && W > 0, "bad sizes");
  SAPR_REQUIRE(feats && offsets && gamma && means && scatter_out && workspace, "NULL pointer argument");
  if (int rc = check_update_b_ws(ws_bytes, n_utts, W, D, S)) return rc;
  hipStream_t st = as_stream(stream);
  double *part = static_cast<double *>(workspace);
  const int64_t per = chunk_utts(n_utts, W);
  const int64_t chunks = (n_utts + per - 1) / per;
  const int K = S * D * D;
  if (utt_model == nullptr && W == 1 && D == 13 && n_utts > 0) {
    // single model, 13-dimensional features: lane-per-utterance kernel, rows of the fold are 256-utterance tiles
    const int64_t tiles = (n_utts + 255) / 256;
    SAPR_LAUNCH((update_b_scatter_lane_kernel<13>), dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(S - 2)),
                dim3(256), 0, st, feats, offsets, n_utts, S, gamma, lane_slots, means, part);
    launch_fold(st, part, nullptr, tiles, 1, static_cast<int64_t>(K), 1, scatter_out);
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  if (chunks > 0)
    SAPR_LAUNCH(update_b_scatter_kernel, dim3(static_cast<unsigned>((K + 255) / 256), static_cast<unsigned>(chunks * W)),
                dim3(256), 0, st, feats, offsets, utt_model, n_utts, per, W, D, S, gamma, lane_slots, means, part);
  launch_fold(st, part, nullptr, chunks * W, W, static_cast<int64_t>(K), 1, scatter_out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// out[k] = part[0][k] + part[1][k] + ... in row order (the reference's accumulation over sequences,
// custom_hmm.py:434-439: aggregated_gamma / aggregated_xi / total log-likelihood), on the device
extern "C" int sapr_custom_fold_rows(const double *part, int64_t n_rows, int64_t K, double *out, void *stream) {
  SAPR_REQUIRE(part && out && n_rows >= 0 && K > 0, "bad arguments");
  launch_fold(as_stream(stream), part, nullptr, n_rows, 1, K, 0, out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// in place: x[n_states][per] /= occ[n_states] where occ > 0 (after the cross-rank sum, if any)
extern "C" int sapr_custom_normalise(double *x, const double *occ, int64_t n_states, int32_t per, void *stream) {
  SAPR_REQUIRE(x && occ && n_states >= 0 && per > 0, "bad arguments");
  const int64_t n = n_states * per;
  if (n > 0)
    SAPR_LAUNCH(custom_normalise_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                x, occ, n_states, per);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// single-process convenience: both passes and both normalisations
extern "C" int sapr_custom_update_b(const float *feats, const int64_t *offsets, const int32_t *utt_model,
                                    int64_t n_utts, int32_t W, int32_t D, int32_t S, const double *gamma,
                                    int64_t lane_slots, double *means_out, double *occ_out, double *covs_out,
                                    void *workspace, size_t ws_bytes, void *stream) {
  SAPR_REQUIRE(means_out && occ_out && covs_out, "NULL pointer argument");
  if (int rc = sapr_custom_update_b_sums(feats, offsets, utt_model, n_utts, W, D, S, gamma, lane_slots, means_out,
                                         occ_out, workspace, ws_bytes, stream))
    return rc;
  if (int rc = sapr_custom_normalise(means_out, occ_out, static_cast<int64_t>(W) * S, D, stream)) return rc;
  if (int rc = sapr_custom_update_b_scatter(feats, offsets, utt_model, n_utts, W, D, S, gamma, lane_slots, means_out,
                                            covs_out, workspace, ws_bytes, stream))
    return rc;
  return sapr_custom_normalise(covs_out, occ_out, static_cast<int64_t>(W) * S, D * D, stream);
}

constexpr int kCovWaves = 8192;  // persistent wavefronts of global_cov_mfma_kernel = rows of its fold
extern "C" int sapr_custom_global_workspace_bytes(int64_t n_utts, int64_t total_frames, int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && n_utts >= 0 && total_frames >= 0 && D > 0 && D <= kMaxD, "bad arguments");
  const size_t s1 = static_cast<size_t>(n_utts > 0 ? n_utts : 1) * D;
  const size_t s2 = static_cast<size_t>((total_frames + kChunkFrames - 1) / kChunkFrames + 1) * D * D;
  const size_t s3 = static_cast<size_t>(kCovWaves + 1) * 256;  // partial tiles of the matrix-core covariance + their sum
  const size_t m = s1 > s2 ? s1 : s2;
  *bytes = (m > s3 ? m : s3) * sizeof(double);
  return 0;
}

extern "C" int sapr_custom_global_sum(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t D,
                                      double *sum_out, void *workspace, size_t ws_bytes, void *stream) {
  SAPR_REQUIRE(feats && offsets && sum_out && workspace && D > 0 && D <= kMaxD && n_utts >= 0, "bad arguments");
  SAPR_REQUIRE(ws_bytes >= static_cast<size_t>(n_utts) * D * sizeof(double), "workspace too small");
  double *part = static_cast<double *>(workspace);
  const int64_t n = n_utts * D;
  if (n > 0)
    SAPR_LAUNCH(custom_global_sum_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                feats, offsets, n_utts, D, part);
  launch_ordered_fold(as_stream(stream), part, n_utts, D, sum_out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sapr_custom_global_cov(const float *feats, int64_t total_frames, int32_t D, const double *mean,
                                      double *cov_out, void *workspace, size_t ws_bytes, void *stream) {
  SAPR_REQUIRE(feats && mean && cov_out && workspace && D > 0 && D <= kMaxD && total_frames >= 0, "bad arguments");
  if (D == 13 && total_frames > 0 && !fold_ordered() && ws_bytes >= static_cast<size_t>(kCovWaves + 1) * 256 * sizeof(double)) {
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(workspace);
    const int64_t n_groups = (total_frames + 3) / 4;
    int64_t waves = n_groups < kCovWaves ? n_groups : kCovWaves;
    const unsigned grid = static_cast<unsigned>((waves + 3) / 4);
    double *tile = part + static_cast<size_t>(grid) * 4 * 256;
    SAPR_LAUNCH((global_cov_mfma_kernel<13>), dim3(grid), dim3(256), 0, st, feats, total_frames, mean, part);
    launch_fold(st, part, nullptr, static_cast<int64_t>(grid) * 4, 1, 256, 0, tile);
    SAPR_LAUNCH(global_cov_unpack_kernel, dim3(1), dim3(256), 0, st, tile, D, cov_out);
    SAPR_HIP_TRY(hipGetLastError());
    return 0;
  }
  const int64_t chunks = (total_frames + kChunkFrames - 1) / kChunkFrames;
  SAPR_REQUIRE(ws_bytes >= static_cast<size_t>(chunks) * D * D * sizeof(double), "workspace too small");
  SAPR_REQUIRE(chunks <= 65535, "too many frames for one launch: shard the feature list");
  double *part = static_cast<double *>(workspace);
  if (chunks > 0)
    SAPR_LAUNCH(custom_global_cov_kernel, dim3((D * D + 63) / 64, static_cast<unsigned>(chunks)), dim3(64), 0,
                as_stream(stream), feats, total_frames, D, mean, part);
  SAPR_LAUNCH(update_b_fold_kernel, dim3((D * D + 63) / 64), dim3(64), 0, as_stream(stream), part,
              static_cast<const int32_t *>(nullptr), chunks, 1, static_cast<int64_t>(D) * D, 1, cov_out);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
