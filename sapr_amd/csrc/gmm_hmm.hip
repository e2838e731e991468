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
//   2  gmm_forward_kernel<SP, VIT>, gmm_backward_kernel<SP>   one lane per utterance over logb: the recursions, the
//        posteriors, both decoders, start and the xi sums (tile_trellis.h; they never look at an emission parameter).
//   3  gmm_accum_kernel<MP, DP>      FRAME-parallel again: chunks of 64 flat frames of a tile; phase A recomputes lc
//        (state per wavefront, frame per lane) and puts r into LDS, phase B is the product r^T [x, x^2, 1] with threads
//        owning (state, component, dimension) accumulators in registers over the workgroup's chunks (vector ALU,
//        float64; x^2 rounded to float32 first, as numpy squares a float32 feature array).  kSub partial rows per tile.
//      gmm_tile_reduce_kernel / gmm_reduce_kernel   (tile_trellis.h) the 256 slots of a tile in a fixed shape, then a
//        model's partial rows in tile order.
// No floating-point atomics; every sum has one fixed order that depends only on the model's own tiles, so results are
// bit-identical run to run and independent of which other models share the launch; loglik, post and path of an
// utterance are a function of its own (features, model) pair.
//
// Shapes are run-time values padded to a few instantiations: SP in {4, 10, 18} states (a padded state has log start
// and log transitions -inf and every component switched off), MP in {1, 2, 4, 8} components (a padded component has
// the constant -inf: exp(-inf) adds +0.0), DP in {13, 26, 39} dimensions (zero features against zero means and zero
// inverse variances add +0.0).  The pack (sapr_gmm_pack_layout) is built by the host in this padded form.
//
// What is specific to the mixtures is here: the two frame-parallel kernels and the family description (Mix).  The
// recursions, the reductions and the tile helpers are tile_trellis.h; the full-covariance family (Full: hmmlearn's
// GaussianHMM, covariance_type "full" / "tied") is fullcov_ops.h; run<Family> below is the one host engine behind both.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "tile_trellis.h"
#include "fullcov_ops.h"

constexpr int stats_p(int S, int M, int D) { return S * M * (2 * D + 1); }  // post_mix, obs, obs2

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
  const int64_t frame = flat_frame(s_cum, s_beg, static_cast<int>(flat64));
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
        frame = flat_frame(s_cum, s_beg, flat);
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

// -------------------------------------------------------------------------------------------
// A family of emissions is four things: its shape check, its pack stride, the width of its observation statistics and
// its two frame-parallel launches (emit: logb; accumulate: the partial rows from the gamma lattice).  Full
// (fullcov_ops.h) has no M: it is passed 1.  Everything else is the engine.
// -------------------------------------------------------------------------------------------
struct Mix {
  static int check(int32_t S, int32_t M, int32_t D) { return check_shape(S, M, D); }
  static size_t model_doubles(int S, int M, int D) { return sapr::model_doubles(sp_of(S), mp_of(M), dp_of(D)); }
  static int stats_p(int S, int M, int D) { return sapr::stats_p(S, M, D); }
  static int launch_emit(const Batch &b, const double *pack, int64_t n_tiles, double *logb, hipStream_t stream) {
    return launch_frames(true, b, pack, n_tiles, logb, nullptr, stream);
  }
  static int launch_accum(const Batch &b, const double *pack, int64_t n_tiles, double *gam, double *part,
                          hipStream_t stream) {
    return launch_frames(false, b, pack, n_tiles, gam, part, stream);
  }
};

template <class Family>
int run(bool vit, const float *feats, const int64_t *offsets, const int32_t *slot_utt, const int32_t *tile_model,
        const int32_t *model_tile_off, int64_t n_utts, int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T,
        const double *pack, int32_t W, int32_t S, int32_t M, void *workspace, size_t workspace_bytes, double *loglik,
        double *stats, double *post, int32_t *path, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && n_tiles >= 0 && W > 0 && S > 0 && M > 0 && D > 0 && max_T >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld n_tiles=%lld W=%d S=%d M=%d D=%d max_T=%d)", (long long)n_utts,
               (long long)total_frames, (long long)n_tiles, W, S, M, D, max_T);
  if (int rc = Family::check(S, M, D)) return rc;
  SAPR_REQUIRE(max_T <= kMaxT, "bad sizes: max_T = %d exceeds %d", max_T, kMaxT);
  SAPR_REQUIRE(n_tiles * (kBlock / 64) <= 0x7fffffffLL, "grid too large (%lld tiles)", (long long)n_tiles);
  if (n_tiles == 0) return 0;
  SAPR_REQUIRE(feats && offsets && slot_utt && tile_model && pack && workspace && loglik, "NULL pointer argument");
  SAPR_REQUIRE(!vit || path, "NULL pointer argument (path)");
  SAPR_REQUIRE(!stats || model_tile_off, "NULL pointer argument (model_tile_off)");
  const int K1 = stats_k1(S), P = Family::stats_p(S, M, D);
  const Ws ws = carve(workspace, total_frames, n_tiles, S, P);
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
  b.stride = static_cast<int64_t>(Family::model_doubles(S, M, D));
  hipStream_t st = as_stream(stream);
  if (max_T > 0 && total_frames > 0) {
    if (int rc = Family::launch_emit(b, pack, n_tiles, ws.logb, st)) return rc;
  }
  double *ustat = stats ? ws.ustat : nullptr;
  int rc;
  switch (sp_of(S)) {
    case 4: rc = launch_trellis<4>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    case 10: rc = launch_trellis<10>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
    default: rc = launch_trellis<18>(vit, b, pack, n_tiles, ws, loglik, ustat, post, path, st); break;
  }
  if (rc || !stats) return rc;
  if (int rc2 = Family::launch_accum(b, pack, n_tiles, ws.lat, ws.part, st)) return rc2;
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
  if (int rc = Mix::check(S, M, D)) return rc;
  *width = stats_k1(S) + Mix::stats_p(S, M, D);
  return 0;
}

extern "C" int sapr_gmm_pack_layout(int32_t S, int32_t M, int32_t D, int32_t *SP, int32_t *MP, int32_t *DP,
                                    size_t *doubles_per_model) {
  SAPR_REQUIRE(SP && MP && DP && doubles_per_model && S > 0 && M > 0 && D > 0, "bad sizes (S=%d M=%d D=%d)", S, M, D);
  if (int rc = Mix::check(S, M, D)) return rc;
  *SP = sp_of(S);
  *MP = mp_of(M);
  *DP = dp_of(D);
  *doubles_per_model = Mix::model_doubles(S, M, D);
  return 0;
}

extern "C" int sapr_gmm_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t M, int32_t D,
                                        size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_tiles >= 0 && S > 0 && M > 0 && D > 0,
               "bad sizes (total_frames=%lld n_tiles=%lld S=%d M=%d D=%d)", (long long)total_frames, (long long)n_tiles,
               S, M, D);
  if (int rc = Mix::check(S, M, D)) return rc;
  *bytes = carve(nullptr, total_frames, n_tiles, S, Mix::stats_p(S, M, D)).bytes;
  return 0;
}

extern "C" int sapr_gmm_estep_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                   const int32_t *tile_model, const int32_t *model_tile_off, int64_t n_utts,
                                   int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, const double *pack,
                                   int32_t W, int32_t S, int32_t M, void *workspace, size_t workspace_bytes,
                                   double *loglik, double *stats, double *post, int32_t *path, void *stream) {
  return run<Mix>(false, feats, offsets, slot_utt, tile_model, model_tile_off, n_utts, total_frames, n_tiles, D, max_T,
                  pack, W, S, M, workspace, workspace_bytes, loglik, stats, post, path, stream);
}

extern "C" int sapr_gmm_viterbi_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                     const int32_t *tile_model, int64_t n_utts, int64_t total_frames, int64_t n_tiles,
                                     int32_t D, int32_t max_T, const double *pack, int32_t W, int32_t S, int32_t M,
                                     void *workspace, size_t workspace_bytes, double *logprob, int32_t *path,
                                     void *stream) {
  return run<Mix>(true, feats, offsets, slot_utt, tile_model, nullptr, n_utts, total_frames, n_tiles, D, max_T, pack, W, S,
                  M, workspace, workspace_bytes, logprob, nullptr, nullptr, path, stream);
}

extern "C" int sapr_full_pack_layout(int32_t S, int32_t D, int32_t *SP, int32_t *DP, size_t *doubles_per_model) {
  SAPR_REQUIRE(SP && DP && doubles_per_model && S > 0 && D > 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = Full::check(S, 1, D)) return rc;
  *SP = sp_of(S);
  *DP = dp_of(D);
  *doubles_per_model = Full::model_doubles(S, 1, D);
  return 0;
}

extern "C" int sapr_full_stats_width(int32_t S, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && D > 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = Full::check(S, 1, D)) return rc;
  *width = stats_k1(S) + Full::stats_p(S, 1, D);
  return 0;
}

extern "C" int sapr_full_workspace_bytes(int64_t total_frames, int64_t n_tiles, int32_t S, int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_tiles >= 0 && S > 0 && D > 0,
               "bad sizes (total_frames=%lld n_tiles=%lld S=%d D=%d)", (long long)total_frames, (long long)n_tiles, S,
               D);
  if (int rc = Full::check(S, 1, D)) return rc;
  *bytes = carve(nullptr, total_frames, n_tiles, S, Full::stats_p(S, 1, D)).bytes;
  return 0;
}

extern "C" int sapr_full_estep(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                               const int32_t *tile_model, const int32_t *model_tile_off, int64_t n_utts,
                               int64_t total_frames, int64_t n_tiles, int32_t D, int32_t max_T, const double *pack,
                               int32_t W, int32_t S, void *workspace, size_t workspace_bytes, double *loglik,
                               double *stats, double *post, int32_t *path, void *stream) {
  return run<Full>(false, feats, offsets, slot_utt, tile_model, model_tile_off, n_utts, total_frames, n_tiles, D, max_T,
                   pack, W, S, 1, workspace, workspace_bytes, loglik, stats, post, path, stream);
}

extern "C" int sapr_full_viterbi(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                 const int32_t *tile_model, int64_t n_utts, int64_t total_frames, int64_t n_tiles,
                                 int32_t D, int32_t max_T, const double *pack, int32_t W, int32_t S, void *workspace,
                                 size_t workspace_bytes, double *logprob, int32_t *path, void *stream) {
  return run<Full>(true, feats, offsets, slot_utt, tile_model, nullptr, n_utts, total_frames, n_tiles, D, max_T, pack, W,
                   S, 1, workspace, workspace_bytes, logprob, nullptr, nullptr, path, stream);
}
