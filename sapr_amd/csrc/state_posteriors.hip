// State posteriors and MAP decoding for diagonal-Gaussian HMMs on gfx950: loglik[u], post[total_frames][n_out_states]
// (hmmlearn's (n_samples, n_components) layout, ragged along `offsets`) and path[total_frames] = argmax_s post[t].
//
// Replaces GaussianHMM.score_samples / predict_proba / decode(algorithm="map") (hmmlearn base.py _score_log,
// _compute_posteriors_log, _decode_map; _hmmc.cpp forward_log / backward_log) for a whole batch, every utterance under
// the one model of its tile, as sapr_forward_diag scores it.  CPU restatement: oracle/hmmlearn_oracle.py
// (log_density_diag, forward_log, backward_log, posteriors).
//
// Two passes over a slot-major workspace, one lane per utterance, the model wavefront-uniform in SGPRs:
//   pass 1 (sp_forward_kernel)  quick_forward_walk of diag_forward.h (the body of forward_vocab_kernel, the
//          recursion of the E-step's fb_forward_kernel) with one model per tile: features from the frame-major batch itself (one-shot call: no
//          slot-major staging copy to amortise), log-densities in the quick form of emission_quick.h.  Bidiagonal models
//          keep the STAY SHARES, stay[t][s][slot], and the last forward row; dense models keep the forward lattice and
//          the log-densities (stored, not recomputed: pass 2 would otherwise walk the S D parameters again for every
//          frame, and the dense path is the rare one).
//   pass 2 (sp_smooth_kernel)   smooth_ops.h, as the E-step: bidiagonal, smooth_step from softmax(last forward row)
//          backwards; dense, dense_backward_row and softmax_row of fwd + bwd.
//
// The store is the new part.  A lane owns an utterance, so a direct write of post would put 64 rows of 8 n_out_states
// bytes at 64 unrelated addresses every frame.  Pass 2 runs ONE wavefront per workgroup (no workgroup barrier, 4 x the
// workgroups to spread) and buffers kPostChunk frames of every lane in the wavefront's own LDS (row stride odd in
// doubles: conflict-free in both directions); when the recursion — which walks t downwards — completes a chunk of
// frames [t0, t0 + kPostChunk), the wavefront writes each utterance's chunk as ONE contiguous run of
// frames * n_out_states * 8 bytes with the lanes along the run.  n_out_states <= S cuts the padded states off in this
// store.  The path is the arg-max of the same registers (first maximum; a row holding NaN gives its first NaN:
// np.argmax), buffered kPathChunk frames per lane and written as runs of int32 the same way.  With post == NULL no
// posterior leaves the registers: MAP decoding costs 4 bytes of output per frame.
//
// Arithmetic is float64; every utterance is a function of its own (features, model) pair — lanes never exchange
// values — so results do not depend on the batch order, on which outputs are requested or on the pack's flavour.
#include "emission_quick.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "diag_forward.h"
#include "smooth_ops.h"

using namespace emission;

constexpr int kBlock = 256;
constexpr int kPathChunk = 32;  // frames of path per lane and flush: runs of up to 128 bytes
// frames of posteriors per lane and flush: runs of 4 * 10 * 8 = 320 resp. 2 * 18 * 8 = 288 bytes; with the path's
// buffer 30 resp. 28 KB of LDS per wavefront (five workgroups per CU)
template <int S>
constexpr int kPostChunk = S > 10 ? 2 : 4;

// workspace (doubles): bidiagonal  stay[max_T][S][n_slots] then last[S][n_slots]
//                      dense       fwd[max_T][S][n_slots]  then b[max_T][S][n_slots]
size_t sp_ws_bytes(int64_t n_tiles, int S, int max_T, int topology) {
  const size_t rows = static_cast<size_t>(max_T > 0 ? max_T : 1);
  const size_t row = static_cast<size_t>(S) * static_cast<size_t>(n_tiles) * kBlock * sizeof(double);
  return topology == SAPR_TOPO_BIDIAG ? (rows + 1) * row : 2 * rows * row;
}

// -------------------------------------------------------------------------------------------
// pass 1
// -------------------------------------------------------------------------------------------
template <int D, int S, bool BIDIAG>
__global__ __launch_bounds__(kBlock) void sp_forward_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, const int32_t *__restrict__ slot_utt,
    const int32_t *__restrict__ tile_model, int64_t n_slots, const double4 *__restrict__ prm_all,
    const double *__restrict__ gconst, const double *__restrict__ log_start, const double *__restrict__ log_trans,
    double *__restrict__ lat_a, double *__restrict__ lat_c, double *__restrict__ loglik) {
  const int64_t tile = blockIdx.x;
  const int64_t slot = tile * kBlock + threadIdx.x;
  const Lane ln = lane_of(offsets, slot_utt[slot]);
  const DiagModel m = diag_model<D, S>(prm_all, gconst, log_start, log_trans, tile_model[tile]);
  const float *__restrict__ xp = feats + ln.beg * D;
  auto load = [&](int t, auto &x) { load_quick_frame<D>(xp + static_cast<int64_t>(t) * D, x); };

  double fwd[S];
  if constexpr (BIDIAG) {
    // the stay shares, and the last forward row: the posteriors of the last frame start from it
    quick_forward_walk<D, S, true>(ln, m, fwd, load, [&](int t, int j, double stay) {
      lat_a[(static_cast<int64_t>(t) * S + j) * n_slots + slot] = stay;
    });
    if (ln.T > 0) {
#pragma unroll
      for (int j = 0; j < S; ++j) lat_c[static_cast<int64_t>(j) * n_slots + slot] = fwd[j];
    }
  } else {
    // the forward lattice and the log-densities
    auto rows = [&](int t, const double (&b)[S], const double (&f)[S]) {
      const int64_t row = static_cast<int64_t>(t) * S;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        lat_a[(row + j) * n_slots + slot] = f[j];
        lat_c[(row + j) * n_slots + slot] = b[j];
      }
    };
    quick_forward_walk<D, S, false>(ln, m, fwd, load, NoShares{}, rows);
  }
  // logsumexp over the last row (unreachable padding states add exp(-inf) = 0); no frames: -inf
  if (ln.live) loglik[ln.u] = ln.T > 0 ? lse_all<S>(fwd) : neg_inf();
}

// -------------------------------------------------------------------------------------------
// pass 2
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Frames [t0, t0 + chunk) of every lane's utterance, `width` values each, buffered at buf[lane * stride + (t - t0) *
// width + s]: each utterance's rows go out as one contiguous run, lanes along the run.  Utterance l owns rows
// t0 .. min(T_l, t0 + chunk) - 1 of the chunk (none: nothing stored), i.e. out[(beg_l + t0) * width ...].  A run is at
// most 64 values (the callers' static_asserts), so a lane moves at most one value per utterance, and the LDS read is
// unconditional (the buffer is padded by 64 values for lanes past the last row): eight utterances' reads are in flight
// before the first of their stores, instead of one LDS round trip per utterance.
template <class V>
__device__ __forceinline__ void flush_runs(const V *buf, int stride, V *__restrict__ out, int64_t beg, int T, int t0,
                                           int chunk, int width, int lane) {
  wave_lds_sync();
  const int beg_lo = static_cast<int>(beg & 0xffffffffLL), beg_hi = static_cast<int>(beg >> 32);
#pragma unroll 8
  for (int l = 0; l < 64; ++l) {
    const V v = buf[l * stride + lane];
    const int Tl = __builtin_amdgcn_readlane(T, l);
    int rows = Tl - t0;
    rows = rows < chunk ? rows : chunk;
    const int n = rows > 0 ? rows * width : 0;
    const int64_t bl = (static_cast<int64_t>(__builtin_amdgcn_readlane(beg_hi, l)) << 32) |
                       static_cast<uint32_t>(__builtin_amdgcn_readlane(beg_lo, l));
    if (lane < n) out[(bl + t0) * width + lane] = v;
  }
  wave_lds_sync();
}

// first maximum of the first n values; a NaN, once met, is kept (np.argmax)
template <int S>
__device__ __forceinline__ int argmax_first(const double (&g)[S], int n) {
  int best = 0;
  double bv = g[0];
#pragma unroll
  for (int s = 1; s < S; ++s) {
    const bool take = s < n && !(bv != bv) && (g[s] > bv || g[s] != g[s]);
    bv = take ? g[s] : bv;
    best = take ? s : best;
  }
  return best;
}

template <int S, bool BIDIAG>
__global__ __launch_bounds__(64) void sp_smooth_kernel(
    const int64_t *__restrict__ offsets, const int32_t *__restrict__ slot_utt, const int32_t *__restrict__ tile_model,
    int64_t n_slots, const double *__restrict__ log_trans, const double *__restrict__ lat_a,
    const double *__restrict__ lat_c, int32_t n_out, double *__restrict__ post, int32_t *__restrict__ path) {
  constexpr int CH = kPostChunk<S>;
  constexpr int kPs = (CH * S) | 1;     // row strides, odd: lanes land on different banks
  constexpr int kQs = kPathChunk | 1;
  static_assert(CH * S <= 64 && kPathChunk <= 64, "flush_runs: a run is at most one value per lane");
  __shared__ double s_post[64 * kPs + 64];  // (+ 64: flush_runs reads a full wavefront's width from every row)
  __shared__ int32_t s_path[64 * kQs + 64];
  const int lane = threadIdx.x;
  const int64_t wq = blockIdx.x;
  const int64_t slot = wq * 64 + lane;
  const Lane ln = lane_of(offsets, slot_utt[slot]);
  const int64_t beg = ln.beg;
  const int T = ln.T, Tw = ln.Tw;

  double g[S];
#pragma unroll
  for (int s = 0; s < S; ++s) g[s] = 0.0;

  // the rows of one frame that the recursion reads: bidiagonal, the stay shares of the step INTO frame t; dense, the
  // forward values and log-densities of frame t.  Frames t, t-1 in registers, t-2 in flight.  Lanes whose utterance has
  // ended (t >= T) load defined addresses of undefined content: masked below.
  constexpr int R = BIDIAG ? S : 2 * S;
  double r0[R], r1[R];
  auto load_rows = [&](int t, double (&r)[R]) {
    const int64_t row = static_cast<int64_t>(t) * S;
    if constexpr (BIDIAG) {
      r[0] = 1.0;
#pragma unroll
      for (int s = 1; s < S; ++s) r[s] = lat_a[(row + s) * n_slots + slot];
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        r[s] = lat_a[(row + s) * n_slots + slot];
        r[S + s] = lat_c[(row + s) * n_slots + slot];
      }
    }
  };
  if (Tw >= 1) load_rows(Tw - 1, r0);
  if (Tw >= 2) load_rows(Tw - 2, r1);

  // dense: log beta of the current frame and the transition matrix of the tile's model (wavefront-uniform)
  double bwd[BIDIAG ? 1 : S];
  const double *__restrict__ lt = log_trans + static_cast<int64_t>(tile_model[wq / (kBlock / 64)]) * S * S;

  for (int t = Tw - 1; t >= 0; --t) {
    double r2[R];
    if (t >= 2) load_rows(t - 2, r2);
    const bool active = t < T;
    if constexpr (BIDIAG) {
      if (t == T - 1) softmax_last_row<S>(lat_c, n_slots, slot, 1, g);  // (the one row of `last`)
    } else {
      if (t == T - 1) {
#pragma unroll
        for (int s = 0; s < S; ++s) bwd[s] = 0.0;
      }
      if (active) {
        double lg[S];  // base.py _compute_posteriors_log: row soft-max of fwd + bwd
#pragma unroll
        for (int s = 0; s < S; ++s) lg[s] = r0[s] + bwd[s];
        softmax_row<S>(lg, g);
      }
    }

    // lane = utterance -> LDS (lanes past their last frame write rows that no run covers)
    if (post) {
      double *row = s_post + lane * kPs + (t % CH) * n_out;
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < n_out) row[s] = g[s];
      if (t % CH == 0) flush_runs<double>(s_post, kPs, post, beg, T, t, CH, n_out, lane);
    }
    if (path) {
      s_path[lane * kQs + t % kPathChunk] = argmax_first<S>(g, n_out);
      if (t % kPathChunk == 0) flush_runs<int32_t>(s_path, kQs, path, beg, T, t, kPathChunk, 1, lane);
    }

    if (active && t >= 1) {
      if constexpr (BIDIAG) {
        double xs[2 * S];  // the xi sums of the E-step: not wanted here, dropped by the compiler
#pragma unroll
        for (int i = 0; i < 2 * S; ++i) xs[i] = 0.0;
        smooth_step<S>(g, r0, xs);
      } else {
        double nb[S];
        dense_backward_row<S>(lt, r0 + S, bwd, nb);
#pragma unroll
        for (int i = 0; i < S; ++i) bwd[i] = nb[i];
      }
    }
#pragma unroll
    for (int s = 0; s < R; ++s) {
      r0[s] = r1[s];
      r1[s] = r2[s];
    }
  }
}

struct SpArgs {
  const float *feats;
  const int64_t *offsets;
  const int32_t *slot_utt, *tile_model;
  int64_t n_tiles, n_slots;
  PackView pv;
  double *lat_a, *lat_c, *loglik, *post;
  int32_t *path;
  int32_t n_out;
  hipStream_t stream;
};

template <int D, int S, bool BIDIAG>
int launch_sp_topo(const SpArgs &a) {
  const int64_t waves = a.n_tiles * (kBlock / 64);
  if (waves > 0x7fffffffLL) return fail(SAPR_ERR_ARG, "grid too large (%lld workgroups)", (long long)waves);
  SAPR_LAUNCH((sp_forward_kernel<D, S, BIDIAG>), dim3(static_cast<unsigned>(a.n_tiles)), dim3(kBlock), 0, a.stream,
              a.feats, a.offsets, a.slot_utt, a.tile_model, a.n_slots, a.pv.prm, a.pv.gconst, a.pv.log_start,
              a.pv.log_trans, a.lat_a, a.lat_c, a.loglik);
  SAPR_HIP_TRY(hipGetLastError());
  SAPR_LAUNCH((sp_smooth_kernel<S, BIDIAG>), dim3(static_cast<unsigned>(waves)), dim3(64), 0, a.stream, a.offsets,
              a.slot_utt, a.tile_model, a.n_slots, a.pv.log_trans, a.lat_a, a.lat_c, a.n_out, a.post, a.path);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

template <int D, int S>
int launch_sp(const SpArgs &a, int topology) {
  return topology == SAPR_TOPO_BIDIAG ? launch_sp_topo<D, S, true>(a) : launch_sp_topo<D, S, false>(a);
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_state_posteriors_workspace_bytes(int64_t n_tiles, int32_t S, int32_t max_T, int32_t topology,
                                                     size_t *bytes) {
  SAPR_REQUIRE(bytes && n_tiles >= 0 && S > 0 && max_T >= 0, "bad arguments");
  SAPR_REQUIRE(topology == SAPR_TOPO_DENSE || topology == SAPR_TOPO_BIDIAG, "bad topology");
  *bytes = sp_ws_bytes(n_tiles, S, max_T, topology);
  return 0;
}

extern "C" int sapr_state_posteriors_diag(const float *feats, const int64_t *offsets, const int32_t *slot_utt,
                                          const int32_t *tile_model, int64_t n_tiles, int32_t D, int32_t max_T,
                                          const void *pack, int32_t W, int32_t S, int32_t topology,
                                          int32_t n_out_states, void *workspace, size_t workspace_bytes,
                                          double *loglik, double *post, int32_t *path, void *stream) {
  SAPR_REQUIRE(n_tiles >= 0 && W > 0 && S > 0 && D > 0 && max_T >= 0, "bad sizes");
  SAPR_REQUIRE(topology == SAPR_TOPO_DENSE || topology == SAPR_TOPO_BIDIAG, "bad topology");
  SAPR_REQUIRE(n_out_states >= 1 && n_out_states <= S, "n_out_states must lie in 1..S (got %d, S=%d)", n_out_states, S);
  if (n_tiles == 0) return 0;
  SAPR_REQUIRE(feats && offsets && slot_utt && tile_model && pack && workspace && loglik, "NULL pointer argument");
  SAPR_REQUIRE(post || path, "post and path are both NULL: nothing to compute");
  const size_t need = sp_ws_bytes(n_tiles, S, max_T, topology);
  SAPR_REQUIRE(workspace_bytes >= need, "workspace too small: %zu < %zu", workspace_bytes, need);
  SpArgs a;
  a.feats = feats;
  a.offsets = offsets;
  a.slot_utt = slot_utt;
  a.tile_model = tile_model;
  a.n_tiles = n_tiles;
  a.n_slots = n_tiles * kBlock;
  a.pv = pack_view(pack, W, S, D);
  const size_t lat = static_cast<size_t>(max_T > 0 ? max_T : 1) * S * static_cast<size_t>(a.n_slots);
  a.lat_a = static_cast<double *>(workspace);
  a.lat_c = a.lat_a + lat;
  a.loglik = loglik;
  a.post = post;
  a.path = path;
  a.n_out = n_out_states;
  a.stream = as_stream(stream);
  return dispatch_ds(D, S, [&](auto d, auto s) {
    return launch_sp<decltype(d)::value, decltype(s)::value>(a, topology);
  });
}
