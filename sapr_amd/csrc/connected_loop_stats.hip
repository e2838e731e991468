// Denominator statistics of discriminative (MMI) training on gfx950: the state posteriors of the word loop
// (sapr_connected_posteriors' post[total_frames][R = W * SP]) reduced to per-word sufficient statistics in the row
// layout of sapr_connected_embed.  CPU restatement, which is the definition: tests/_mmi_ref.py
// (den_stats); it is written out in include/sapr_hip.h.
//
// The work is one product, post^T [x | RN32(x x) | 1]: R <= 256 rows by NC = 2 D + 1 <= 79 columns, summed over the
// frames of the kept utterances, on the float64 matrix cores (v_mfma_f64_16x16x4_f64, the operand layout of
// embed_gmm_accum_kernel's phase B): the frame is the K index, A = post (16 consecutive flat states of a row, read
// from global memory as they are: a row of post ends at R, the rows behind it are selected 0.0), B = the frame's
// columns, formed from the staged float32 frame as it is read (x, its float32 square, the constant 1, 0.0 behind NC).
//
// loop_stats_accum_kernel<NT>  (NT = ceil(NC / 16) column tiles): workgroup g covers the frames
//   [g * span, (g + 1) * span) of the batch's numbering in chunks of 128, ascending; span is a function of
//   total_frames alone (ls_span).  Wavefront v owns the row tiles v, v + 4, v + 8, v + 12.  Per chunk the first
//   128 threads find each frame's utterance (a cursor walks offsets[] forward from the one the span begins in) and
//   marks the frame live where it lies inside a well-formed [offsets[u], offsets[u + 1]) of a kept utterance; a frame
//   that is not live is never read, neither its row of post nor its features: its A operand is selected 0.0 and its
//   staged features are 0.0f.  A chunk without a live frame is skipped.  The workgroup writes every element of its
//   partial row part[g][R][NC].
// loop_stats_fold_kernel: stats[w][e] = the sum over the partial rows, g ascending, for the post / obs / obs2 elements
//   of the model's own states s < S; nobs = the kept utterances with at least one frame (an integer count); the
//   reserved slot, start and trans are 0.0.  Padded states are not written (a row has no place for them).
//
// No atomics; the order of every sum is fixed by (total_frames, the frame's number): two calls return the same bytes.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kLsMaxD = 39;
constexpr int kLsChunk = 128;      // frames staged at once (a multiple of 16; at most kXBlock: a thread per frame)
constexpr int kLsMinSpan = 256;    // frames of one workgroup's span ...
constexpr int kLsMaxParts = 1024;  // ... beyond 256 * 1024 frames the spans grow instead of their number
constexpr int kLsRowTiles = 4;     // row tiles of one wavefront: 4 wavefronts x 4 tiles x 16 rows = 256 flat states
static_assert(kLsChunk % 16 == 0 && kLsChunk <= kXBlock, "a thread per frame of a chunk");
constexpr int kLsXF = 41;          // LDS row stride of the staged frames (floats), odd, >= kLsMaxD

typedef double f64x4_ls __attribute__((ext_vector_type(4)));

inline int ls_check_dims(int32_t D) {
  if (D > kLsMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "the word-loop statistics serve D in 1..%d; got D=%d", kLsMaxD, D);
  return 0;
}

inline int64_t ls_span(int64_t total_frames) {
  const int64_t spread = (total_frames + kLsMaxParts - 1) / kLsMaxParts;
  const int64_t span = (spread + kLsChunk - 1) / kLsChunk * kLsChunk;
  return span > kLsMinSpan ? span : kLsMinSpan;
}

inline int64_t ls_parts(int64_t total_frames) {
  const int64_t span = ls_span(total_frames);
  return (total_frames + span - 1) / span;
}

// utterance u is counted and read: a well-formed range inside the batch, and kept
__device__ __forceinline__ bool ls_kept(const int64_t *__restrict__ offsets, int64_t total_frames,
                                        const uint8_t *__restrict__ keep, int64_t u, int64_t *beg, int64_t *end) {
  *beg = offsets[u];
  *end = offsets[u + 1];
  return *beg >= 0 && *end >= *beg && *end <= total_frames && (!keep || keep[u] != 0);
}

template <int NT>
__global__ __launch_bounds__(kXBlock) void loop_stats_accum_kernel(
    const double *__restrict__ post, const float *__restrict__ feats, int32_t D, const int64_t *__restrict__ offsets,
    int64_t n_utts, int64_t total_frames, const uint8_t *__restrict__ keep, int32_t R, int64_t span,
    double *__restrict__ part) {
  __shared__ float s_x[kLsChunk * kLsXF];
  __shared__ int s_live[kLsChunk];
  __shared__ int64_t s_cur;

  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, k = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NC = 2 * D + 1;
  const int RT = (R + 15) / 16;
  const int64_t g = blockIdx.x;
  const int64_t f_lo = g * span;
  const int64_t f_hi = f_lo + span < total_frames ? f_lo + span : total_frames;

  if (tid == 0) {  // the last utterance that begins at or before the span's first frame (0 where none does)
    int64_t lo = 0, hi = n_utts - 1;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (offsets[mid] <= f_lo)
        lo = mid;
      else
        hi = mid - 1;
    }
    s_cur = lo;
  }

  // column 16 t + n of B: feature ci[t] as it is (kind 0), its float32 square (1), the constant 1 (2), nothing (3)
  int ci[NT], kind[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * t + n;
    kind[t] = c < D ? 0 : (c < 2 * D ? 1 : (c == 2 * D ? 2 : 3));
    ci[t] = c < D ? c : (c < 2 * D ? c - D : 0);
  }
  int row[kLsRowTiles];
  bool row_ok[kLsRowTiles];
#pragma unroll
  for (int j = 0; j < kLsRowTiles; ++j) {
    row[j] = 16 * (wv + kXWaves * j) + n;
    row_ok[j] = row[j] < R;
  }
  f64x4_ls acc[kLsRowTiles][NT];
#pragma unroll
  for (int j = 0; j < kLsRowTiles; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[j][t] = f64x4_ls{0.0, 0.0, 0.0, 0.0};

  for (int64_t c0 = f_lo; c0 < f_hi; c0 += kLsChunk) {  // (uniform trip counts: every thread reaches the barriers)
    __syncthreads();  // the cursor is written; the chunk before this one is read
    bool live = false;
    int64_t u = 0;
    if (tid < kLsChunk) {
      u = s_cur;
      const int64_t f = c0 + tid;
      if (f < f_hi) {
        while (u + 1 < n_utts && offsets[u + 1] <= f) ++u;  // (offsets that do not ascend: ends, at n_utts - 1)
        int64_t beg, end;
        live = ls_kept(offsets, total_frames, keep, u, &beg, &end) && beg <= f && f < end;
      }
      s_live[tid] = live ? 1 : 0;
    }
    const bool any = __syncthreads_or(live);
    if (tid == kLsChunk - 1) s_cur = u;  // (read again behind the barrier at the head of the loop)
    if (!any) continue;                  // (uniform) a chunk of frames that belong to no kept utterance
    // A and B of the float64 MFMA: lane & 15 = row (column), lane >> 4 = the K index, here the frame.  Four steps of
    // four frames at a time: the 16 loads of A (four row tiles x four steps) of the NEXT 16 frames are issued before
    // the matrix instructions of these 16 — at the wide shapes a wavefront is alone on its SIMD and hides its own
    // loads — and those of the first 16 frames before the features are staged.
    double an[kLsRowTiles][4];
    const auto load_a = [&](int sb) {
#pragma unroll
      for (int j = 0; j < kLsRowTiles; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = 16 * sb + 4 * q + k;
          an[j][q] = 0.0;
          if (row_ok[j] && s_live[f]) an[j][q] = post[(c0 + f) * R + row[j]];
        }
    };
    load_a(0);
    for (int item = tid; item < kLsChunk * D; item += kXBlock) {
      const int f = item / D, d = item - f * D;
      float v = 0.0f;
      if (s_live[f]) v = feats[(c0 + f) * D + d];
      s_x[f * kLsXF + d] = v;
    }
    __syncthreads();
#pragma unroll
    for (int sb = 0; sb < kLsChunk / 16; ++sb) {
      double a[kLsRowTiles][4];
#pragma unroll
      for (int j = 0; j < kLsRowTiles; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[j][q] = an[j][q];
      if (sb + 1 < kLsChunk / 16) load_a(sb + 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = 16 * sb + 4 * q + k;
        double xb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float xf = s_x[f * kLsXF + ci[t]];
          const float v = kind[t] == 1 ? xf * xf : xf;  // X**2 in float32, as numpy squares the array
          xb[t] = kind[t] < 2 ? static_cast<double>(v) : (kind[t] == 2 ? 1.0 : 0.0);
        }
#pragma unroll
        for (int j = 0; j < kLsRowTiles; ++j) {
          if (wv + kXWaves * j >= RT) continue;  // (wavefront-uniform) no such row tile
#pragma unroll
          for (int t = 0; t < NT; ++t)
            acc[j][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][q], xb[t], acc[j][t], 0, 0, 0);
        }
      }
    }
  }

  // C of the float64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
  double *__restrict__ out = part + g * static_cast<int64_t>(R) * NC;
#pragma unroll
  for (int j = 0; j < kLsRowTiles; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ro = 16 * (wv + kXWaves * j) + k + 4 * r, c = 16 * t + n;
        if (ro < R && c < NC) out[static_cast<int64_t>(ro) * NC + c] = acc[j][t][r];
      }
}

// stats[w][e]: {nobs, 0.0, start[S] = 0, trans[S][S] = 0, post[S], obs[S][D], obs2[S][D]}; one thread per element, the
// partial rows added g ascending
__global__ __launch_bounds__(kXBlock) void loop_stats_fold_kernel(
    const double *__restrict__ part, int64_t parts, const int64_t *__restrict__ offsets, int64_t n_utts,
    int64_t total_frames, const uint8_t *__restrict__ keep, int32_t W, int32_t S, int32_t SP, int32_t D, int32_t width,
    double *__restrict__ stats) {
  __shared__ long long s_cnt[kXBlock];
  const int e = blockIdx.x * kXBlock + threadIdx.x;
  const int w = blockIdx.y;
  if (blockIdx.x == 0) {  // (uniform) element 0 lives here: the kept utterances with a frame, an integer count
    long long cnt = 0;
    for (int64_t u = threadIdx.x; u < n_utts; u += kXBlock) {
      int64_t beg, end;
      if (ls_kept(offsets, total_frames, keep, u, &beg, &end) && end > beg) ++cnt;
    }
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = kXBlock / 2; h > 0; h >>= 1) {
      if (static_cast<int>(threadIdx.x) < h) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
      __syncthreads();
    }
  }
  if (e >= width) return;
  const int R = W * SP, NC = 2 * D + 1;
  double sum = 0.0;
  int r = e - 2 - S - S * S;
  if (e == 0) {
    sum = static_cast<double>(s_cnt[0]);
  } else if (r >= 0) {
    int s, col;
    if (r < S) {
      s = r;
      col = 2 * D;
    } else if ((r -= S) < S * D) {
      s = r / D;
      col = r - s * D;
    } else {
      r -= S * D;
      s = r / D;
      col = D + (r - s * D);
    }
    const double *__restrict__ src = part + static_cast<int64_t>(w * SP + s) * NC + col;
    const int64_t stride = static_cast<int64_t>(R) * NC;
    constexpr int NF = 8;  // loads in flight; the additions stay in the order g ascending
    int64_t g = 0;
    for (; g + NF <= parts; g += NF) {
      double v[NF];
#pragma unroll
      for (int q = 0; q < NF; ++q) v[q] = src[(g + q) * stride];
#pragma unroll
      for (int q = 0; q < NF; ++q) sum += v[q];
    }
    for (; g < parts; ++g) sum += src[g * stride];
  }
  stats[static_cast<int64_t>(w) * width + e] = sum;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_loop_stats_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t W, int32_t S,
                                                         int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && W > 0 && S > 0 && D > 0,
               "bad sizes (total_frames=%lld n_utts=%lld W=%d S=%d D=%d)", (long long)total_frames, (long long)n_utts,
               W, S, D);
  if (int rc = x_check_shape(W, S)) return rc;
  if (int rc = ls_check_dims(D)) return rc;
  // the partial rows [parts][R][2 D + 1], float64
  *bytes = x_align16(static_cast<size_t>(ls_parts(total_frames)) * static_cast<size_t>(W) * sp_of(S) *
                     static_cast<size_t>(2 * D + 1) * sizeof(double));
  return 0;
}

extern "C" int sapr_connected_loop_stats(const double *post, const float *feats, int32_t D, const int64_t *offsets,
                                         int64_t n_utts, int64_t total_frames, const uint8_t *utt_keep, int32_t W,
                                         int32_t S, void *workspace, size_t workspace_bytes, double *stats,
                                         void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0 && D > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d D=%d)", (long long)n_utts, (long long)total_frames,
               W, S, D);
  if (int rc = x_check_shape(W, S)) return rc;
  if (int rc = ls_check_dims(D)) return rc;
  size_t need = 0;
  if (int rc = sapr_connected_loop_stats_workspace_bytes(total_frames, n_utts, W, S, D, &need)) return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  SAPR_REQUIRE(n_utts <= 0x7fffffffLL, "grid too large (%lld utterances)", (long long)n_utts);
  SAPR_REQUIRE(stats, "NULL pointer argument (stats)");
  SAPR_REQUIRE(n_utts == 0 || (offsets && (total_frames == 0 || (post && feats))), "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  const int32_t width = 2 + S + S * S + S + 2 * S * D;
  hipStream_t st = as_stream(stream);
  if (n_utts == 0 || total_frames == 0) {  // nothing to add up: no utterance has a frame
    SAPR_HIP_TRY(hipMemsetAsync(stats, 0, static_cast<size_t>(W) * width * sizeof(double), st));
    return 0;
  }
  const int64_t span = ls_span(total_frames), parts = ls_parts(total_frames);
  double *part = static_cast<double *>(workspace);
#define SAPR_LS_ACCUM(NT)                                                                                          \
  SAPR_LAUNCH(loop_stats_accum_kernel<NT>, dim3(static_cast<unsigned>(parts)), dim3(kXBlock), 0, st, post, feats, D, \
              offsets, n_utts, total_frames, utt_keep, R, span, part)
  switch ((2 * D + 1 + 15) / 16) {
    case 1: SAPR_LS_ACCUM(1); break;
    case 2: SAPR_LS_ACCUM(2); break;
    case 3: SAPR_LS_ACCUM(3); break;
    case 4: SAPR_LS_ACCUM(4); break;
    default: SAPR_LS_ACCUM(5); break;
  }
#undef SAPR_LS_ACCUM
  SAPR_HIP_TRY(hipGetLastError());
  const unsigned tiles = static_cast<unsigned>((width + kXBlock - 1) / kXBlock);
  SAPR_LAUNCH(loop_stats_fold_kernel, dim3(tiles, static_cast<unsigned>(W)), dim3(kXBlock), 0, st, part, parts,
              offsets, n_utts, total_frames, utt_keep, W, S, SP, D, width, stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
