// One batched Lloyd step of k-means on gfx950: for every frame the nearest of the K centres of its group, for every
// one of R centre sets ("restarts") evaluated side by side, and per (group, restart, cluster) the statistics
// {count, sum_x[D], sqdev[D]} that the host turns into the next centres (sum / count) and the inertia (sum of sqdev).
//
// Replaces the k-means inside hmmlearn's GaussianHMM._init (sklearn.cluster.KMeans(n_clusters, n_init=10) over all
// frames of a word model) for every word model and every restart in one launch.  CPU restatement: tests/_kmeans_ref.py.
//
// A group is one k-means problem (the frames of one word model).  Frames are independent, so the layout is TILES of at
// most 256 consecutive frames of one group, sorted by group (kmeans.py FrameTiles).  Two kernels:
//   kmeans_tile_kernel<D>   one 256-thread workgroup per tile.  Thread i loads frame i ONCE and keeps it as D doubles in
//        registers.  Then, restart after restart:
//          assign   thread i walks the K centres of (group, r) — workgroup-uniform addresses, i.e. scalar loads — and
//                   takes label = argmin_k sum_d (x_d - c_kd)^2 in float64, the difference squared directly (c0 sits
//                   near -300: the |x|^2 - 2 x.c + |c|^2 expansion cancels); np.argmin's rules: the lowest k on equal
//                   distances, the first NaN distance wins (a frame holding NaN gets label 0)
//          sort     a stable counting sort of the tile's frames by label: per wavefront K ballots give every frame its
//                   rank among the wavefront's frames of its label, the four wavefronts' counts (scanned by shuffles)
//                   give the rest, and thread i writes its frame as float32 into ITS ROW of the sorted copy in LDS
//                   (39 KB at D = 39)
//          gather   threads own (k, d) accumulator pairs (K D of them, up to five per thread) and walk THEIR cluster's
//                   rows — consecutive, so four loads are in flight — in frame order: D * tile_len additions per
//                   restart in all, not K * D * tile_len
//        and the tile's partial statistics go to workspace[tile][r][k][2 D + 1].
//   kmeans_reduce_kernel    stats[g][r][k][:] = the partial rows of the group's tiles added in tile order: eight runs of
//        equal length per value (one lane each, eight loads in flight), the runs' sums added in run order.
// No floating-point atomics; every sum has one fixed order that depends only on the group's own tiles, so results are
// bit-identical run to run and do not depend on which other groups share the launch.
#include "sapr_common.h"

namespace sapr {
namespace {

constexpr int kBlock = 256;     // frames per tile = threads per workgroup
constexpr int kMaxK = 32;

__host__ __device__ constexpr int stat_width(int D) { return 2 * D + 1; }

size_t km_ws_bytes(int64_t n_tiles, int R, int K, int D) {
  return static_cast<size_t>(n_tiles) * static_cast<size_t>(R) * static_cast<size_t>(K) * stat_width(D) * sizeof(double);
}

// (four workgroups per CU is what 40 KB of LDS admits at D = 39: the register budget is set to match)
template <int D>
__global__ __launch_bounds__(kBlock, D >= 39 ? 4 : 6) void kmeans_tile_kernel(
    const float *__restrict__ feats, int64_t total_frames, const int64_t *__restrict__ tile_begin,
    const int32_t *__restrict__ tile_len, const int32_t *__restrict__ tile_group, int G, int R, int K,
    const double *__restrict__ centres, double *__restrict__ partial, int32_t *__restrict__ labels) {
  constexpr int W = stat_width(D);
  // the tile's frames SORTED by (label, frame), float32, row stride D (odd): rewritten for every restart
  __shared__ float s_x[(kBlock + 3) * D];        // (+ 3 rows: the gather reads four rows at a time)
  __shared__ int16_t s_cnt[kBlock / 64][kMaxK];  // frames of label k in wavefront w (int16: the whole block is
                                                 // 40 726 B at D = 39, four workgroups per CU)
  __shared__ int16_t s_base[kMaxK + 1];          // first row of label k in s_x

  const int64_t tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t beg = tile_begin[tile];
  int len = tile_len[tile];
  const int g = tile_group[tile];
  // a table that points outside the batch is served as an empty tile (zeros), never followed
  if (len < 0 || len > kBlock || beg < 0 || beg > total_frames - len || g < 0 || g >= G) len = 0;
  const bool live = tid < len;

  double x[D];
  if (live) {
    const float *__restrict__ xp = feats + (beg + tid) * D;
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = static_cast<double>(xp[d]);
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = 0.0;
  }
  for (int i = tid; i < 3 * D; i += kBlock) s_x[kBlock * D + i] = 0.0f;  // the over-read rows: defined, never added

  const int gg = len > 0 ? g : 0;
  for (int r = 0; r < R; ++r) {
    const double *__restrict__ c = centres + (static_cast<int64_t>(gg) * R + r) * K * D;  // workgroup-uniform
    // ---- assign ------------------------------------------------------------------------------------------
    int label = 0;
    double bv = __builtin_huge_val();
    for (int k = 0; k < K; ++k) {
      const double *__restrict__ ck = c + k * D;
      double dist = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double diff = x[d] - ck[d];
        dist = fma(diff, diff, dist);
      }
      // np.argmin: the first minimum (every distance +inf: 0); a NaN, once met, is kept
      const bool take = !(bv != bv) && (dist < bv || dist != dist);
      bv = take ? dist : bv;
      label = take ? k : label;
    }
    if (live && labels) labels[static_cast<int64_t>(r) * total_frames + beg + tid] = label;

    // ---- sort: stable by (label, frame) ------------------------------------------------------------------
    int rank = 0;
    for (int k = 0; k < K; ++k) {  // (uniform trip count)
      const unsigned long long m = __ballot(live && label == k);
      if (label == k) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_cnt[wv][k] = static_cast<int16_t>(__popcll(m));
    }
    __syncthreads();
    // every wavefront scans the K totals itself (lane k holds label k): base = first row of the label
    int tot = 0, before = 0;  // frames of label `lane` in the tile / in the wavefronts before this one
    if (lane < K) {
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) {
        const int n = s_cnt[w][lane];
        before += w < wv ? n : 0;
        tot += n;
      }
    }
    int incl = tot;
#pragma unroll
    for (int o = 1; o < kMaxK; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      incl += lane >= o ? up : 0;
    }
    const int row = __shfl(incl - tot + before, label, 64) + rank;
    const int all = __shfl(incl, K - 1, 64);
    if (wv == 0 && lane <= K) s_base[lane] = static_cast<int16_t>(lane < K ? incl - tot : all);
    if (live) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        // (opaque copy: the conversions stay inside the restart loop instead of living in D more registers)
        double xd = x[d];
        asm volatile("" : "+v"(xd));
        s_x[row * D + d] = static_cast<float>(xd);
      }
    }
    __syncthreads();

    // ---- gather: (k, d) accumulators over the cluster's rows, in frame order -------------------------------
    double *__restrict__ out = partial + (tile * R + r) * K * W;
    for (int item = tid; item < K * D; item += kBlock) {
      const int k = item / D, d = item - k * D;
      const int b0 = s_base[k], n = s_base[k + 1] - b0;
      const double ckd = c[k * D + d];
      const float *__restrict__ col = s_x + b0 * D + d;
      double sum = 0.0, sq = 0.0;
      for (int j = 0; j < n; j += 4) {  // four rows in flight, added one after the other
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = col[(j + i) * D];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (j + i < n) {
            const double vd = static_cast<double>(v[i]);
            const double diff = vd - ckd;
            sum += vd;
            sq = fma(diff, diff, sq);
          }
        }
      }
      out[k * W + 1 + d] = sum;
      out[k * W + 1 + D + d] = sq;
      if (d == 0) out[k * W] = static_cast<double>(n);
    }
    __syncthreads();  // s_x / s_cnt / s_base are rewritten by the next restart
  }
}

// stats[g][r][k][:] = sum over the group's tiles, in tile order, of partial[tile][r][k][:].  A workgroup serves 32
// values; the group's tiles are cut into kSeg runs of equal length (a function of the group's own tile count alone),
// one lane per (value, run) adds its run in tile order with eight loads in flight, and the runs' sums are added in
// run order — a fixed shape.
constexpr int kSeg = 8;

__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const int32_t *__restrict__ group_tile_off, int64_t row,
                                                            int64_t n_tiles, const double *__restrict__ partial,
                                                            double *__restrict__ stats) {
  __shared__ double part[kSeg][32];
  const int g = blockIdx.y;
  const int col = threadIdx.x & 31, seg = threadIdx.x >> 5;
  const int64_t k = blockIdx.x * 32LL + col;
  int64_t t0 = group_tile_off[g], t1 = group_tile_off[g + 1];
  t0 = t0 < 0 ? 0 : t0;  // (a table that points past the workspace's rows is cut, never followed)
  t1 = t1 > n_tiles ? n_tiles : t1;
  const int64_t n = t1 > t0 ? t1 - t0 : 0;
  const int64_t chunk = (n + kSeg - 1) / kSeg;
  int64_t r = t0 + seg * chunk, r1 = r + chunk;
  r1 = r1 > t1 ? t1 : r1;
  double acc = 0.0;
  if (k < row) {
    const double *__restrict__ src = partial + k;
    for (; r + 8 <= r1; r += 8) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[(r + i) * row];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += v[i];
    }
    for (; r < r1; ++r) acc += src[r * row];
  }
  part[seg][col] = acc;
  __syncthreads();
  if (seg == 0 && k < row) {
    double tot = part[0][col];
#pragma unroll
    for (int s2 = 1; s2 < kSeg; ++s2) tot += part[s2][col];
    stats[g * row + k] = tot;
  }
}

struct KmArgs {
  const float *feats;
  int64_t total_frames;
  const int64_t *tile_begin;
  const int32_t *tile_len, *tile_group, *group_tile_off;
  int64_t n_tiles;
  int G, R, K;
  const double *centres;
  double *partial, *stats;
  int32_t *labels;
  hipStream_t stream;
};

template <int D>
int launch_kmeans(const KmArgs &a) {
  SAPR_LAUNCH((kmeans_tile_kernel<D>), dim3(static_cast<unsigned>(a.n_tiles)), dim3(kBlock), 0, a.stream, a.feats,
              a.total_frames, a.tile_begin, a.tile_len, a.tile_group, a.G, a.R, a.K, a.centres, a.partial, a.labels);
  SAPR_HIP_TRY(hipGetLastError());
  const int64_t row = static_cast<int64_t>(a.R) * a.K * stat_width(D);
  SAPR_LAUNCH(kmeans_reduce_kernel, dim3(static_cast<unsigned>((row + 31) / 32), static_cast<unsigned>(a.G)), dim3(256),
              0, a.stream, a.group_tile_off, row, a.n_tiles, a.partial, a.stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_kmeans_workspace_bytes(int64_t n_tiles, int32_t R, int32_t K, int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && n_tiles >= 0 && R >= 1 && K >= 1 && D >= 1, "bad arguments");
  *bytes = km_ws_bytes(n_tiles, R, K, D);
  return 0;
}

extern "C" int sapr_kmeans_step(const float *feats, int64_t total_frames, const int64_t *tile_begin,
                                const int32_t *tile_len, const int32_t *tile_group, const int32_t *group_tile_off,
                                int64_t n_tiles, int32_t G, int32_t R, int32_t K, int32_t D, const double *centres,
                                void *workspace, size_t workspace_bytes, double *stats, int32_t *labels, void *stream) {
  SAPR_REQUIRE(total_frames >= 0 && n_tiles >= 0 && G >= 0 && R >= 1 && K >= 1 && D >= 1,
               "bad sizes (total_frames=%lld n_tiles=%lld G=%d R=%d K=%d D=%d)", (long long)total_frames,
               (long long)n_tiles, G, R, K, D);
  SAPR_REQUIRE(n_tiles == 0 || G >= 1, "bad sizes: %lld tiles but no group", (long long)n_tiles);
  if (D != 13 && D != 39)
    return fail(SAPR_ERR_UNSUPPORTED, "the k-means kernel is instantiated for D in {13, 39}; got D=%d", D);
  if (K > kMaxK) return fail(SAPR_ERR_UNSUPPORTED, "the k-means kernel serves K in 1..%d; got K=%d", kMaxK, K);
  const int64_t row = static_cast<int64_t>(R) * K * stat_width(D);
  SAPR_REQUIRE(row <= 0x7fffffffLL && (G == 0 || row <= 0x7fffffffffLL / G), "statistics too large (G=%d R=%d K=%d)", G,
               R, K);
  SAPR_REQUIRE(G == 0 || stats, "NULL pointer argument (stats)");
  if (n_tiles == 0) {  // no frames anywhere: every cluster of every group is empty
    if (G > 0) SAPR_HIP_TRY(hipMemsetAsync(stats, 0, static_cast<size_t>(G * row) * sizeof(double), as_stream(stream)));
    return 0;
  }
  SAPR_REQUIRE(feats && tile_begin && tile_len && tile_group && group_tile_off && centres && workspace,
               "NULL pointer argument");
  SAPR_REQUIRE(n_tiles <= 0x7fffffffLL, "grid too large (%lld workgroups)", (long long)n_tiles);
  const size_t need = km_ws_bytes(n_tiles, R, K, D);
  SAPR_REQUIRE(workspace_bytes >= need, "workspace too small: %zu < %zu", workspace_bytes, need);
  KmArgs a;
  a.feats = feats;
  a.total_frames = total_frames;
  a.tile_begin = tile_begin;
  a.tile_len = tile_len;
  a.tile_group = tile_group;
  a.group_tile_off = group_tile_off;
  a.n_tiles = n_tiles;
  a.G = G;
  a.R = R;
  a.K = K;
  a.centres = centres;
  a.partial = static_cast<double *>(workspace);
  a.stats = stats;
  a.labels = labels;
  a.stream = as_stream(stream);
  return D == 13 ? launch_kmeans<13>(a) : launch_kmeans<39>(a);
}
