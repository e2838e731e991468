// Embedded Baum-Welch on gfx950: forward-backward over the left-to-right chain of an utterance's K transcript words and
// the reduction of its posteriors into per-word sufficient statistics.  CPU restatement, which is the
// definition: tests/_embedded_ref.py.  The input logb[total_frames][R = W * SP] is what the three emission stages of
// connected.hip write; the recursion knows nothing about the emission family.
//
// The recursions use the lane layout of connected_lanes.h over the chain positions, with the vocabulary's table by word
// in LDS and the coupling between the slots through a per-wavefront LDS row.  The two kernels lay out the positions and
// rotate in code of their own (they keep the text they were timed with); the table loader, its mask, the utterance
// span, the segmented log-sum-exp, the constants and the host side are the header's.
//
// embed_forward_kernel<RL, SP>  (four wavefronts per workgroup): the alignment recursion with the two-term log-sum-exp
//   of lse_ops.h in place of the strict maximum and a segmented log-sum-exp (x_segment_lse: the lanes of slot q evaluate
//   its SP exponentials, lane q takes the maximum before and the sum after) in place of the segmented maximum.  Per
//   frame it writes alpha[t][max_words * SP] and X[t][max_words] into the workspace; at the end loglik[u].  A NaN met
//   anywhere (lse2 would drop it) makes the likelihood NaN.
// embed_backward_kernel<RL, SP>  (as many wavefronts per workgroup as the LDS holds, at most four): walks t downwards
//   with beta in registers.  c_t(p) = b_t(p) + beta_t(p) is rotated to the lane of position p - d — the lane of state i
//   reads its successor j = i + d at position p + d, with the transposed diagonal tab[w][d mod SP][i + d] — and one
//   rotation serves both the recursion and the transition share exp(alpha_{t-1}(i) + lt(i,j) + c_t(j) - loglik).
//   The shares are accumulated where they are formed: lane (slot, i) owns trans[slot][i][*], one double per
//   (d mod SP, position) in a per-wavefront LDS block of SP * 64 * RL doubles that only its own lane touches.
//   gamma_t overwrites alpha_t in the workspace (alpha_t is dead once frame t is done) and goes to post[] when asked;
//   the per-position sums of gamma and of the entry shares stay in registers.  At the end the wavefront writes its
//   slots' {start[SP], trans[SP][SP], post[SP]} into the per-slot partial rows and marks the slots as counted.
// embed_obs_kernel: one workgroup per utterance, sum_t gamma_t(p) [x, x^2] in float64 over the float32 features (x^2
//   is the float32 square, as in estep.hip), t ascending, into the per-slot partial rows.
// embed_fold_chunk_kernel, embed_fold_kernel: stats[w][e] = the sum over the counted slots n with words[n] == w, in two
//   levels with fixed boundaries (chunks of 256 slots, n ascending; then the chunks, ascending).
// embed_full_accum_kernel<DP>, embed_full_fold_kernel (sapr_connected_embed_full): the second moments sum gamma x x^T
//   per word model on the float64 matrix cores, behind the same recursions; described where they stand.
// embed_gmm_accum_kernel<MP, DP> (sapr_connected_embed_gmm): the mixture statistics sum r [x, x^2, 1] per word model
//   with r = the chain's gamma shared out among a state's components, the product again on the float64 matrix cores;
//   described where it stands.
//
// No atomics anywhere; an utterance's outputs are a function of its own frames, its own transcript and the network, and
// the fold adds in slot order: two calls return the same bytes.  Every index is clamped into its row and offsets that
// leave the batch are served as empty.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kEmXRow = kWave + 2;    // coupling row of one wavefront: [0] = -inf (nothing enters slot 0), [q + 1]
constexpr int kEmRows = kEmXRow + kWave;  // ... and the row of the slots' maxima behind it
constexpr int kEmMaxD = 39;
constexpr int kEmFoldChunk = 256;     // slots one block of the first fold level adds up (fixed: it fixes the order)

inline int em_check_shape(int32_t W, int32_t S, int32_t max_words) {
  return x_check_chain_shape("embedded Baum-Welch", W, S, max_words);
}

inline int em_check_dims(int32_t D) {
  if (D > kEmMaxD)
    return fail(SAPR_ERR_UNSUPPORTED, "the embedded Baum-Welch kernels serve D in 0..%d; got D=%d", kEmMaxD, D);
  return 0;
}

// doubles of one slot's partial row: {start[SP], trans[SP][SP], post[SP], obs[SP][D], obs2[SP][D]}
inline size_t em_part_width(int SP, int D) { return static_cast<size_t>(SP) * (2 + SP + 2 * D); }

struct EmWorkspace {
  double *alpha;     // [total_frames][max_words * SP]; gamma after the backward pass
  double *X;         // [total_frames][max_words]
  double *part;      // [total_words][em_part_width]
  uint8_t *slot_ok;  // [total_words]: the slot belongs to an utterance with a path
  double *fold;      // [chunks of kEmFoldChunk slots][W <= 256 / SP][stats width]: the first fold level
  size_t bytes;
};

inline int64_t em_chunks(int64_t total_words) { return (total_words + kEmFoldChunk - 1) / kEmFoldChunk; }

inline EmWorkspace em_carve(void *base, int64_t total_frames, int64_t total_words, int32_t max_words, int S, int D) {
  const int SP = sp_of(S);
  EmWorkspace w;
  uint8_t *p = static_cast<uint8_t *>(base);
  const size_t a = x_align16(static_cast<size_t>(total_frames) * max_words * SP * sizeof(double));
  const size_t x = x_align16(static_cast<size_t>(total_frames) * max_words * sizeof(double));
  const size_t s = x_align16(static_cast<size_t>(total_words) * em_part_width(SP, D) * sizeof(double));
  const size_t o = x_align16(static_cast<size_t>(total_words));
  const size_t f = x_align16(static_cast<size_t>(em_chunks(total_words)) * (kXMaxR / SP) *
                              (2 + S + S * S + S + 2 * S * D) * sizeof(double));
  w.alpha = reinterpret_cast<double *>(p);
  w.X = reinterpret_cast<double *>(p + a);
  w.part = reinterpret_cast<double *>(p + a + x);
  w.slot_ok = p + a + x + s;
  w.fold = reinterpret_cast<double *>(p + a + x + s + o);
  w.bytes = a + x + s + o + f;
  return w;
}

// OPT (both recursion kernels): optional[] marks transcript slots that may be stepped over.  bit q of
// `om` = slot q is optional; far = the slot may be entered from slot q - 2; the coupling rows get a second leading
// -inf so that no index is conditional.  Flags that are not 0 / 1, two optional neighbours or no mandatory slot: no
// path.  The OPT = false instantiations are the kernels as they were.
__device__ __forceinline__ bool em_flags(const uint8_t *__restrict__ optional, int64_t wbeg, int K, int lane,
                                         uint64_t *om) {
  const int o = lane < K ? optional[wbeg + lane] : 0;
  *om = __ballot(o == 1);
  const uint64_t all = K >= kWave ? ~0ull : (1ull << K) - 1;
  return !(__ballot(o > 1) || (*om & (*om >> 1)) || *om == all);
}

template <int RL, int SP, bool OPT>
__global__ __launch_bounds__(kXBlock) void embed_forward_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const int32_t *__restrict__ words, const int64_t *__restrict__ word_offsets, int64_t total_words, int32_t max_words,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    double word_penalty, int32_t W, int32_t S, double *__restrict__ alpha_ws, double *__restrict__ x_ws,
    double *__restrict__ loglik, const uint8_t *__restrict__ optional) {
  constexpr int PP = kWave * RL;
  extern __shared__ double smem[];
  double *tab = smem;
  const int n_tab = W * SP * SP;
  x_load_by_word<SP>(tab, log_trans, W, S);

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cbuf = smem + n_tab + wave * (PP + kEmRows);
  double *xbuf = cbuf + PP;
  double *mbuf = xbuf + kEmXRow;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
  bool path = ut.path;
  const int K = ut.K;
  {  // a word outside the vocabulary: no path, and nothing of it is used as an index
    const int w = lane < K ? words[ut.wbeg + lane] : 0;
    if (__ballot(w < 0 || w >= W)) path = false;
  }
  [[maybe_unused]] uint64_t om = 0;
  if constexpr (OPT)
    if (!em_flags(optional, ut.wbeg, K, lane, &om)) path = false;
  if (!path) {
    if (lane == 0) loglik[u] = neg_inf();
    return;
  }
  const int64_t beg = ut.beg, T = ut.T;
  const int P = K * SP;
  const int R = W * SP;
  const int MP = max_words * SP;

  bool tab_nan;
  const uint64_t dmask = x_mask_by_word<SP>(tab, n_tab, lane, &tab_nan);

  double ls[RL], lx[RL], alpha[RL], bn[RL];
  int sk[RL], qk[RL], col[RL], tb[RL];
  bool ok[RL], real[RL];
  [[maybe_unused]] bool far[RL], first[RL];
  bool bad = tab_nan || word_penalty != word_penalty;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int p = k * kWave + lane;
    const int q = p / SP, s = p - q * SP;
    ok[k] = p < P;
    const int w = ok[k] ? words[ut.wbeg + q] : 0;  // (checked above: 0 .. W - 1)
    sk[k] = s;
    qk[k] = ok[k] ? q : 0;
    if constexpr (OPT) {
      far[k] = ok[k] && q >= 2 && ((om >> (q - 1)) & 1ull);
      first[k] = qk[k] == 0 || (qk[k] == 1 && (om & 1ull));  // the start slots (qk = 1 only where K > 1)
    }
    col[k] = w * SP + s;
    tb[k] = w * (SP * SP) + s;
    real[k] = ok[k] && s < S;
    ls[k] = real[k] ? log_start[w * S + s] : neg_inf();
    lx[k] = real[k] ? log_exit[w * S + s] : neg_inf();
    bad = bad || ls[k] != ls[k] || lx[k] != lx[k];
    alpha[k] = neg_inf();
  }

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[col[k]] : neg_inf();
  if (lane == 0) xbuf[0] = neg_inf();
  if constexpr (OPT)  // [q + 2] = X(q): slot q reads [q + 1] (near) and [q] (far)
    if (lane == 0) xbuf[1] = neg_inf();

  double xv = neg_inf();  // lane q: X(q) of the frame just finished
  for (int64_t t = 0; t < T; ++t) {
    double b[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) b[k] = bn[k];
    {  // the next frame's values in flight under this frame's chain
      const int64_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
      for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[tn * R + col[k]] : neg_inf();
    }
    double v[RL];
    if (t == 0) {
      if constexpr (OPT) {
#pragma unroll
        for (int k = 0; k < RL; ++k) v[k] = first[k] ? ls[k] : neg_inf();
      } else {
#pragma unroll
        for (int k = 0; k < RL; ++k) v[k] = qk[k] == 0 ? ls[k] : neg_inf();
      }
    } else {
      double xe[RL];  // X_{t-1} of the slot before the lane's own (-inf in front of slot 0)
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        if constexpr (OPT)  // ... joined with that of the slot two before it where the one between is optional
          xe[k] = lse2(xbuf[qk[k] + 1], far[k] ? xbuf[qk[k]] : neg_inf());
        else
          xe[k] = xbuf[qk[k]];
        v[k] = neg_inf();
      }
#pragma unroll 1
      for (int d = SP - 1; d > -SP; --d) {
        if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
        // position p - d: lane (lane - d) & 63 of register k, of k - 1 where lane < d, of k + 1 where lane - d >= 64
        const int off = lane - d;
        const int src = off & (kWave - 1);
        const int drow = (d >= 0 ? d : d + SP) * SP;
        double rot[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) rot[k] = __shfl(alpha[k], src, kWave);
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
          const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
          const double prev = off < 0 ? below : (off >= kWave ? above : rot[k]);
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[tb[k] + drow];
          v[k] = lse2(v[k], prev + (in ? lt : neg_inf()));
        }
      }
#pragma unroll
      for (int k = 0; k < RL; ++k) v[k] = lse2(v[k], (xe[k] + word_penalty) + ls[k]);
    }
    double *__restrict__ arow = alpha_ws + (beg + t) * MP;
    double ex[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      alpha[k] = real[k] ? v[k] + b[k] : neg_inf();
      bad = bad || alpha[k] != alpha[k];
      if (ok[k]) arow[k * kWave + lane] = alpha[k];
      ex[k] = alpha[k] + lx[k];
    }
    xv = x_segment_lse<RL, SP>(cbuf, mbuf, ex, ok, qk, lane, K);  // the log-sum-exp over the slot's states
    if (lane < K) {
      xbuf[lane + (OPT ? 2 : 1)] = xv;
      x_ws[(beg + t) * max_words + lane] = xv;
    }
    wave_lds_sync();
  }
  const bool any_bad = __ballot(bad) != 0;
  if constexpr (OPT) {  // an optional last slot: the chain may also end in the slot before it
    const double before = __shfl(xv, (lane - 1) & (kWave - 1), kWave);
    if (lane == K - 1) {
      const bool two = K >= 2 && ((om >> (K - 1)) & 1ull);
      loglik[u] = any_bad ? __builtin_nan("") : lse2(xv, two ? before : neg_inf());
    }
  } else {
    if (lane == K - 1) loglik[u] = any_bad ? __builtin_nan("") : xv;
  }
}

template <int RL, int SP, bool OPT>
__global__ __launch_bounds__(kXBlock) void embed_backward_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const int32_t *__restrict__ words, const int64_t *__restrict__ word_offsets, int64_t total_words, int32_t max_words,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    double word_penalty, int32_t W, int32_t S, int32_t part_width, double *__restrict__ alpha_ws,
    const double *__restrict__ x_ws, const double *__restrict__ loglik, double *__restrict__ part,
    uint8_t *__restrict__ slot_ok, double *__restrict__ post, const uint8_t *__restrict__ optional) {
  constexpr int PP = kWave * RL;
  constexpr int kPerWave = PP + kEmRows + SP * PP;  // cbuf, ebuf, mbuf, the transition accumulators [SP][PP]
  extern __shared__ double smem[];
  double *tab = smem;
  const int n_tab = W * SP * SP;
  x_load_by_word<SP>(tab, log_trans, W, S);

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  double *cbuf = smem + n_tab + static_cast<size_t>(wave) * kPerWave;
  double *ebuf = cbuf + PP;
  double *mbuf = ebuf + kEmXRow;
  double *acc = mbuf + kWave;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * waves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
  const int64_t beg = ut.beg, T = ut.T;
  const int MP = max_words * SP;
  const double ll = loglik[u];
  // (a finite likelihood was written only for 0 < K <= max_words, T > 0 and words inside the vocabulary)
  bool path = ut.path && finite_f64(ll);
  const int K = ut.K;
  {
    const int w = lane < K ? words[ut.wbeg + lane] : 0;
    if (__ballot(w < 0 || w >= W)) path = false;
  }
  [[maybe_unused]] uint64_t om = 0;
  if constexpr (OPT)
    if (!em_flags(optional, ut.wbeg, K, lane, &om)) path = false;  // (their likelihood is -inf: not reached)
  if (!path) {  // zero posterior rows; the slots stay uncounted
    if (post)
      for (int64_t t = 0; t < T; ++t)
        for (int p = lane; p < MP; p += kWave) post[(beg + t) * MP + p] = 0.0;
    return;
  }
  const int P = K * SP;
  const int R = W * SP;

  bool tab_nan;  // (a NaN in the table made the likelihood NaN: not reached)
  const uint64_t dmask = x_mask_by_word<SP>(tab, n_tab, lane, &tab_nan);
  (void)tab_nan;

  double ls[RL], lx[RL], beta[RL], acur[RL], bcur[RL], gsum[RL], sacc[RL];
  int sk[RL], qk[RL], col[RL], tb[RL];
  bool ok[RL], real[RL];
  [[maybe_unused]] bool far[RL], first[RL], over[RL];  // OPT: over = slot q + 2 may be entered from this one
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int p = k * kWave + lane;
    const int q = p / SP, s = p - q * SP;
    ok[k] = p < P;
    const int w = ok[k] ? words[ut.wbeg + q] : 0;
    sk[k] = s;
    qk[k] = ok[k] ? q : 0;
    col[k] = w * SP + s;
    tb[k] = w * (SP * SP) + s;
    real[k] = ok[k] && s < S;  // (a padded state carries nothing, whatever its column of logb holds)
    ls[k] = real[k] ? log_start[w * S + s] : neg_inf();
    lx[k] = real[k] ? log_exit[w * S + s] : neg_inf();
    if constexpr (OPT) {
      far[k] = ok[k] && q >= 2 && ((om >> (q - 1)) & 1ull);
      first[k] = ok[k] && (q == 0 || (q == 1 && (om & 1ull)));
      over[k] = ok[k] && q + 2 < K && ((om >> (q + 1)) & 1ull);
      const bool last = q == K - 1 || (q == K - 2 && ((om >> (K - 1)) & 1ull));  // the slots the chain may end in
      beta[k] = (ok[k] && last) ? lx[k] : neg_inf();
    } else {
      beta[k] = (ok[k] && q == K - 1) ? lx[k] : neg_inf();
    }
    gsum[k] = 0.0;
    sacc[k] = 0.0;
#pragma unroll 1
    for (int dd = 0; dd < SP; ++dd) acc[dd * PP + p] = 0.0;
  }
  ebuf[lane] = neg_inf();
  if (lane + kWave < kEmXRow) ebuf[lane + kWave] = neg_inf();

  const double *__restrict__ brow = logb + beg * R;
  double *__restrict__ abase = alpha_ws + beg * MP;
  const double *__restrict__ xbase = x_ws + beg * max_words;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    acur[k] = ok[k] ? abase[(T - 1) * MP + k * kWave + lane] : neg_inf();
    bcur[k] = real[k] ? brow[(T - 1) * R + col[k]] : neg_inf();
  }

  for (int64_t t = T - 1; t >= 0; --t) {
    double c[RL], g[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      const int p = k * kWave + lane;
      c[k] = bcur[k] + beta[k];
      g[k] = ok[k] ? exp_unit((acur[k] + beta[k]) - ll) : 0.0;
      gsum[k] += g[k];
      if (ok[k]) abase[t * MP + p] = g[k];  // alpha_t is dead from here on: the observation sums read gamma_t
      if (post && p < MP) post[(beg + t) * MP + p] = g[k];
    }
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        if constexpr (OPT)
          sacc[k] += first[k] ? g[k] : 0.0;
        else
          sacc[k] += (ok[k] && qk[k] == 0) ? g[k] : 0.0;
      }
      break;
    }
    double ap[RL], bn[RL], xe[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      ap[k] = ok[k] ? abase[(t - 1) * MP + k * kWave + lane] : neg_inf();
      bn[k] = real[k] ? brow[(t - 1) * R + col[k]] : neg_inf();
      xe[k] = (ok[k] && qk[k] > 0) ? xbase[(t - 1) * max_words + qk[k] - 1] : neg_inf();
      if constexpr (OPT) xe[k] = lse2(xe[k], far[k] ? xbase[(t - 1) * max_words + qk[k] - 2] : neg_inf());
    }
    // the entry share of slot q >= 1 at frame t, and E_t(q) through the coupling row
    double en[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      en[k] = ls[k] + c[k];
      sacc[k] += exp_unit(((xe[k] + word_penalty) + en[k]) - ll);
    }
    {
      const double e = x_segment_lse<RL, SP>(cbuf, mbuf, en, ok, qk, lane, K);
      if (lane >= 1 && lane < K) ebuf[lane] = word_penalty + e;
    }
    wave_lds_sync();
    double nb[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      if constexpr (OPT)  // (ebuf[K], ebuf[K + 1] stay -inf)
        nb[k] = lx[k] + lse2(ebuf[qk[k] + 1], over[k] ? ebuf[qk[k] + 2] : neg_inf());
      else
        nb[k] = lx[k] + ebuf[qk[k] + 1];  // (ebuf[K] stays -inf: nothing follows the last slot)
    }
#pragma unroll 1
    for (int d = SP - 1; d > -SP; --d) {
      if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
      // position p + d: lane (lane + d) & 63 of register k, of k + 1 where lane + d >= 64, of k - 1 where lane + d < 0
      const int off = lane + d;
      const int src = off & (kWave - 1);
      const int dd = d >= 0 ? d : d + SP;
      double rot[RL];
#pragma unroll
      for (int k = 0; k < RL; ++k) rot[k] = __shfl(c[k], src, kWave);
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
        const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
        const double next = off < 0 ? below : (off >= kWave ? above : rot[k]);
        const int j = sk[k] + d;
        const bool in = j >= 0 && j < SP;  // (outside the word: no such successor)
        const double lt = tab[in ? tb[k] + dd * SP + d : 0];
        const double term = in ? lt + next : neg_inf();
        nb[k] = lse2(nb[k], term);
        double *a = acc + dd * PP + k * kWave + lane;
        *a += exp_unit((ap[k] + term) - ll);
      }
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      beta[k] = nb[k];
      acur[k] = ap[k];
      bcur[k] = bn[k];
    }
  }

  if (lane < K) slot_ok[ut.wbeg + lane] = 1;
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    if (!ok[k]) continue;
    const int p = k * kWave + lane;
    double *__restrict__ row = part + (ut.wbeg + qk[k]) * static_cast<int64_t>(part_width);
    const int s = sk[k];
    row[s] = sacc[k];
    row[SP + SP * SP + s] = gsum[k];
#pragma unroll 1
    for (int dd = 0; dd < SP; ++dd) {
      const int j = s + dd < SP ? s + dd : s + dd - SP;
      row[SP + s * SP + j] = acc[dd * PP + p];
    }
  }
}

// sum_t gamma_t(p) [x_t, x_t^2]: one workgroup per utterance, thread (p, d) with d fastest
__global__ __launch_bounds__(kXBlock) void embed_obs_kernel(
    const double *__restrict__ gamma, const float *__restrict__ feats, int32_t D, const int64_t *__restrict__ offsets,
    int64_t n_utts, int64_t total_frames, const int64_t *__restrict__ word_offsets, int64_t total_words,
    int32_t max_words, int32_t SP, int32_t part_width, const double *__restrict__ loglik, double *__restrict__ part) {
  const int64_t u = blockIdx.x;
  if (u >= n_utts) return;
  const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
  if (!ut.path || !finite_f64(loglik[u])) return;
  const int MP = max_words * SP;
  const int n = ut.K * SP * D;
  const double *__restrict__ g = gamma + ut.beg * MP;
  const float *__restrict__ x = feats + ut.beg * D;
  constexpr int NP = 4;  // (position, feature) pairs a thread carries at once: independent chains, each t ascending
  for (int base = threadIdx.x; base < n; base += kXBlock * NP) {
    int p[NP], d[NP];
    double a1[NP], a2[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int idx = base + j * kXBlock < n ? base + j * kXBlock : n - 1;  // (behind the end: computed, not stored)
      p[j] = idx / D;
      d[j] = idx - p[j] * D;
      a1[j] = a2[j] = 0.0;
    }
    for (int64_t t = 0; t < ut.T; ++t) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const double gt = g[t * MP + p[j]];
        const float xf = x[t * D + d[j]];
        a1[j] += gt * static_cast<double>(xf);
        a2[j] += gt * static_cast<double>(xf * xf);  // float32 square, then widened (estep.hip, hmmlearn's X**2)
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (base + j * kXBlock >= n) continue;
      const int q = p[j] / SP, s = p[j] - q * SP;
      double *__restrict__ row = part + (ut.wbeg + q) * static_cast<int64_t>(part_width) + SP * (2 + SP);
      row[s * D + d[j]] = a1[j];
      row[SP * D + s * D + d[j]] = a2[j];
    }
  }
}

// stats[w][e]: {nobs, 0.0, start[S], trans[S][S], post[S], obs[S][D], obs2[S][D]} over the counted slots of word w, in
// two levels with fixed boundaries: fold[c][w][e] = the sum over the slots n of chunk c (kEmFoldChunk of them), n
// ascending; then stats[w][e] = the sum over the chunks, c ascending
__global__ __launch_bounds__(kXBlock) void embed_fold_chunk_kernel(const double *__restrict__ part,
                                                                    const uint8_t *__restrict__ slot_ok,
                                                                    const int32_t *__restrict__ words,
                                                                    int64_t total_words, int32_t W, int32_t S,
                                                                    int32_t SP, int32_t D, int32_t part_width,
                                                                    int32_t width, double *__restrict__ fold) {
  const int e = blockIdx.x * kXBlock + threadIdx.x;
  const int w = blockIdx.y;
  const int64_t c = blockIdx.z;
  if (e >= width) return;
  int po = -1;  // the element's place in a slot's partial row
  int r = e - 2;
  if (r >= 0) {
    if (r < S) {
      po = r;
    } else if ((r -= S) < S * S) {
      po = SP + (r / S) * SP + r % S;
    } else if ((r -= S * S) < S) {
      po = SP + SP * SP + r;
    } else if ((r -= S) < S * D) {
      po = SP * (2 + SP) + r;  // (s * D + d in both layouts)
    } else {
      r -= S * D;
      po = SP * (2 + SP) + SP * D + r;
    }
  }
  const int64_t lo = c * kEmFoldChunk;
  const int64_t hi = lo + kEmFoldChunk < total_words ? lo + kEmFoldChunk : total_words;
  double sum = 0.0;
  for (int64_t n = lo; n < hi; ++n) {
    if (!slot_ok[n] || words[n] != w) continue;  // (uniform)
    sum += e == 0 ? 1.0 : (po >= 0 ? part[n * part_width + po] : 0.0);
  }
  fold[(c * W + w) * width + e] = sum;
}

__global__ __launch_bounds__(kXBlock) void embed_fold_kernel(const double *__restrict__ fold, int64_t chunks,
                                                              int32_t W, int32_t width, double *__restrict__ stats) {
  const int e = blockIdx.x * kXBlock + threadIdx.x;
  const int w = blockIdx.y;
  if (e >= width) return;
  double sum = 0.0;
  for (int64_t c = 0; c < chunks; ++c) sum += fold[(c * W + w) * width + e];
  stats[static_cast<int64_t>(w) * width + e] = sum;
}

struct EmArgs {
  const double *logb;
  const int64_t *offsets;
  int64_t n_utts, total_frames;
  const int32_t *words;
  const int64_t *word_offsets;
  int64_t total_words;
  int32_t max_words;
  const double *log_start, *log_trans, *log_exit;
  double word_penalty;
  int32_t W, S;
  const uint8_t *optional;  // [total_words] or NULL: the OPT = false kernels
};

// the forward kernel, then (backward) the backward kernel with as many wavefronts per workgroup as the LDS holds next
// to the vocabulary's table: its transition accumulators take SP * 64 * RL doubles per wavefront (36 KB at SP = 18,
// RL = 4)
template <int RL, int SP, bool OPT>
int launch_recursions(const EmArgs &a, const EmWorkspace &ws, int32_t part_width, double *loglik, double *post,
                      bool backward, hipStream_t stream) {
  const size_t tab = static_cast<size_t>(a.W) * SP * SP * sizeof(double);
  if (int rc = x_launch(embed_forward_kernel<RL, SP, OPT>, (a.n_utts + kXWaves - 1) / kXWaves, kXBlock,
                        tab + static_cast<size_t>(kXWaves) * (kWave * RL + kEmRows) * sizeof(double), stream, a.logb,
                        a.offsets, a.n_utts, a.total_frames, a.words, a.word_offsets, a.total_words, a.max_words,
                        a.log_start, a.log_trans, a.log_exit, a.word_penalty, a.W, a.S, ws.alpha, ws.X, loglik,
                        a.optional))
    return rc;
  if (!backward) return 0;
  size_t lds = 0;
  const int waves = x_waves(tab, static_cast<size_t>(kWave * RL + kEmRows + SP * kWave * RL) * sizeof(double), &lds);
  if (lds > static_cast<size_t>(kXLdsMax))
    return fail(SAPR_ERR_UNSUPPORTED, "the backward kernel needs %zu bytes of LDS, the device offers %d", lds,
                kXLdsMax);
  return x_launch(embed_backward_kernel<RL, SP, OPT>, (a.n_utts + waves - 1) / waves, waves * kWave, lds, stream, a.logb,
                  a.offsets, a.n_utts, a.total_frames, a.words, a.word_offsets, a.total_words, a.max_words, a.log_start,
                  a.log_trans, a.log_exit, a.word_penalty, a.W, a.S, part_width, ws.alpha, ws.X, loglik, ws.part,
                  ws.slot_ok, post, a.optional);
}

// ---- second moments over the chain posteriors (sapr_connected_embed_full) ----------------------------------------
// embed_full_accum_kernel<DP>: obs[w][s] = sum gamma_t(k, s) x_t and oo[w][s] = sum gamma_t(k, s) x_t x_t^T over the
//   slots k with w_k = w, as the weighted Gram products of full_accum_kernel (fullcov_ops.h) on the float64 matrix
//   cores: four frames per v_mfma_f64_16x16x4_f64, A = g x[a], B = x[b], the constant 1 in column DP of B carries obs;
//   only the 16 x 16 tiles on or above the diagonal.  Grid (utterance group, word w); the workgroup walks its group's
//   utterances in ascending order and leaves out, uniformly, those without a path, with a likelihood that is not
//   finite (their gamma rows were never written: nothing of them is read) and those whose transcript lacks w.  Four
//   states per pass, one per wavefront; per chunk of 64 frames the weights g_t(w, s) = sum_{k: w_k = w, k ascending}
//   gamma_t(k, s) of the pass's four states are collapsed while they are staged into LDS; a chunk, and inside it a
//   4-frame step, whose weights are all exactly 0.0 is skipped (adding +0.0 changes no bit of a sum that started at
//   +0.0) — slot k's posterior mass sits in its own stretch of the recording.  One partial row {obs[S][D],
//   oo[S][D][D]} per (group, w), every element of it written.
// embed_full_fold_kernel: stats[w] = {the head sapr_connected_embed folded, the partial rows added group ascending}.
constexpr int kEmFullGroupUtts = 8;    // utterances of one group (fixed: with kEmFullMaxGroups it fixes the order)
constexpr int kEmFullMaxGroups = 96;   // beyond 8 * 96 utterances the groups grow instead of their number
constexpr int kEmFullChunk = 64;       // frames staged at once
constexpr int kEmFullGS = 5;           // LDS row stride of the staged weights (doubles), odd

typedef double f64x4_em __attribute__((ext_vector_type(4)));

inline int64_t em_full_group_utts(int64_t n_utts) {
  const int64_t spread = (n_utts + kEmFullMaxGroups - 1) / kEmFullMaxGroups;
  return spread > kEmFullGroupUtts ? spread : kEmFullGroupUtts;
}

inline int64_t em_full_groups(int64_t n_utts) {
  const int64_t per = em_full_group_utts(n_utts);
  return (n_utts + per - 1) / per;
}

inline size_t em_head_width(int S) { return static_cast<size_t>(2 + S + S * S + S); }
inline size_t em_full_p(int S, int D) { return static_cast<size_t>(S) * D + static_cast<size_t>(S) * D * D; }

struct EmFullWorkspace {
  size_t base_bytes;  // what sapr_connected_embed takes at D = 0 (alpha / gamma first)
  double *head;       // [W][2 + S + S * S + S]
  double *part;       // [groups][W][P]: P = S * D + S * D * D (second moments) or S * M * (2 D + 1) (mixtures)
  size_t bytes;
};

inline EmFullWorkspace em_full_carve(void *base, int64_t total_frames, int64_t n_utts, int64_t total_words,
                                     int32_t max_words, int W, int S, size_t P) {
  EmFullWorkspace w;
  uint8_t *p = static_cast<uint8_t *>(base);
  w.base_bytes = em_carve(nullptr, total_frames, total_words, max_words, S, 0).bytes;
  const size_t h = x_align16(static_cast<size_t>(W) * em_head_width(S) * sizeof(double));
  const size_t f = x_align16(static_cast<size_t>(em_full_groups(n_utts)) * W * P * sizeof(double));
  w.head = reinterpret_cast<double *>(p + w.base_bytes);
  w.part = reinterpret_cast<double *>(p + w.base_bytes + h);
  w.bytes = w.base_bytes + h + f;
  return w;
}

template <int DP>
__global__ __launch_bounds__(kXBlock) void embed_full_accum_kernel(
    const double *__restrict__ gamma, const float *__restrict__ feats, int32_t D, const int64_t *__restrict__ offsets,
    int64_t n_utts, int64_t total_frames, const int32_t *__restrict__ words, const int64_t *__restrict__ word_offsets,
    int64_t total_words, int32_t max_words, int32_t W, int32_t S, int32_t SP, int64_t group_utts,
    const double *__restrict__ loglik, double *__restrict__ part) {
  constexpr int NT = (DP + 1 + 15) / 16;       // 16-wide tiles per side: x[0..DP) and the constant 1 at column DP
  constexpr int NTU = NT * (NT + 1) / 2;       // tiles on or above the diagonal
  constexpr int XS = NT == 2 ? 48 : 16 * NT;   // LDS row stride (doubles): four consecutive rows on distinct banks
  constexpr int GS = kEmFullGS;
  constexpr int T1 = DP / 16, N1 = DP % 16;    // where the constant 1 sits
  constexpr int NI = kEmFullChunk * XS / kXBlock;  // staged features per thread and chunk
  static_assert(NI * kXBlock == kEmFullChunk * XS, "the staging loop covers the chunk exactly");
  static_assert(kEmFullChunk * 4 == kXBlock, "one staged weight per thread: 64 frames x the pass's four states");
  __shared__ double s_x[kEmFullChunk * XS];
  __shared__ double s_g[kEmFullChunk * GS];

  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, k = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t grp = blockIdx.x;
  const int w = blockIdx.y;
  const int64_t u_lo = grp * group_utts;
  const int64_t u_hi = u_lo + group_utts < n_utts ? u_lo + group_utts : n_utts;
  const int MP = max_words * SP;
  const int sf = tid >> 2, sj = tid & 3;  // the weight this thread stages: frame of the chunk, state of the pass
  double *__restrict__ out = part + (grp * W + w) * static_cast<int64_t>(S * D + S * D * D);
  double *__restrict__ out_oo = out + S * D;

  // four states at a time, one per wavefront, over all of the group's utterances: the accumulators of ONE state live
  // in a wavefront's registers (the features are staged again for every pass, from L2)
  for (int g = 0; g * 4 < S; ++g) {  // (uniform trip counts: every thread reaches the barriers)
    const int s = g * 4 + wv;
    f64x4_em acc[NTU];
#pragma unroll
    for (int tau = 0; tau < NTU; ++tau) acc[tau] = f64x4_em{0.0, 0.0, 0.0, 0.0};
    for (int64_t u = u_lo; u < u_hi; ++u) {
      const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
      // (a finite likelihood was written only for 0 < K <= max_words, T > 0 and words inside the vocabulary; the
      // gamma rows of every other utterance hold whatever the workspace held: left out, not multiplied by zero)
      if (!ut.path || !finite_f64(loglik[u])) continue;  // (uniform)
      const int wd = lane < ut.K ? words[ut.wbeg + lane] : -1;
      const uint64_t slots = __ballot(wd == w);  // the slots of word w (the same in every wavefront)
      if (slots == 0) continue;
      const double *__restrict__ gu = gamma + ut.beg * MP;
      const float *__restrict__ xu = feats + ut.beg * D;
      for (int64_t c0 = 0; c0 < ut.T; c0 += kEmFullChunk) {
        {  // g_t(w, s) of the pass's states, the slots collapsed k ascending; 0.0 selected behind the utterance's end
          const int64_t t = c0 + sf;
          const int st = g * 4 + sj;
          const bool live = t < ut.T && st < S;
          const double *__restrict__ src = gu + (live ? t : 0) * MP + (live ? st : 0);  // (dead: a valid address)
          double gw = 0.0;
          for (uint64_t m = slots; m; m &= m - 1) gw += src[__builtin_ctzll(m) * SP];
          gw = live ? gw : 0.0;
          s_g[sf * GS + sj] = gw;
          if (!__syncthreads_or(gw != 0.0)) continue;  // (uniform) nothing of word w in these frames
        }
        // the chunk's frames into LDS as float64: columns [0, D) the features, column DP the ones behind obs, zeros
        // elsewhere and in the rows past the utterance's last frame; every load is issued before the first is used
        float xv[NI];
#pragma unroll
        for (int q = 0; q < NI; ++q) {
          const int item = tid + q * kXBlock, f = item / XS, col = item - f * XS;
          const int64_t t = c0 + f;
          xv[q] = xu[(t < ut.T && col < D) ? t * D + col : 0];
        }
#pragma unroll
        for (int q = 0; q < NI; ++q) {
          const int item = tid + q * kXBlock, f = item / XS, col = item - f * XS;
          const bool live = c0 + f < ut.T;
          s_x[item] = live ? (col < D ? static_cast<double>(xv[q]) : (col == DP ? 1.0 : 0.0)) : 0.0;
        }
        __syncthreads();
        if (s < S) {  // (uniform)
          for (int step = 0; step < kEmFullChunk / 4; ++step) {
            // A and B of the float64 MFMA: lane & 15 = row (column), lane >> 4 = the K index, here the frame
            const int f = 4 * step + k;
            const double gm = s_g[f * GS + wv];
            if (__ballot(gm != 0.0) == 0) continue;  // (wavefront-uniform) four frames that add exact zeros
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

// stats[w][e]: the head as sapr_connected_embed folded it, then {obs[S][D], oo[S][D][D]} = the sum over the groups'
// partial rows, group ascending; one thread per element
__global__ __launch_bounds__(kXBlock) void embed_full_fold_kernel(const double *__restrict__ head,
                                                                   const double *__restrict__ part, int64_t groups,
                                                                   int32_t W, int32_t head_width, int32_t P,
                                                                   double *__restrict__ stats) {
  const int e = blockIdx.x * kXBlock + threadIdx.x;
  const int w = blockIdx.y;
  const int width = head_width + P;
  if (e >= width) return;
  double sum;
  if (e < head_width) {
    sum = head[static_cast<int64_t>(w) * head_width + e];
  } else {
    sum = 0.0;
    for (int64_t g = 0; g < groups; ++g) sum += part[(g * W + w) * static_cast<int64_t>(P) + (e - head_width)];
  }
  stats[static_cast<int64_t>(w) * width + e] = sum;
}

// ---- mixture statistics over the chain posteriors (sapr_connected_embed_gmm) ---------------------------------------
// embed_gmm_accum_kernel<MP, DP>: with g_t(w, s) = sum_{k: w_k = w, k ascending} gamma_t(k, s) and lc the component
//   log-terms of word w's block of the GmmPack (mix_log_terms, gmm_ops.h),
//     r_t(w, s, m) = g_t(w, s) exp(lc[m] - max lc) / sum_m exp(lc[m] - max lc)       (gmm_accum_kernel's rule)
//     post_mix[w][s][m] = sum r     obs[w][s][m] = sum r x_t     obs2[w][s][m] = sum r RN32(x_t x_t)
//   The grid, the utterance groups, the utterances left out and the collapse of the slots are those of
//   embed_full_accum_kernel.  A pass serves SG = min(64 / MP, 18) states, i.e. at most 64 (state, component) rows.
//   Per chunk of 64 frames, phase A (lane = frame, the pass's states dealt round to the wavefronts) recomputes lc from
//   the staged float32 frame and writes r into LDS as r[row][frame]; a state whose 64 weights are all 0.0 writes
//   zeros without evaluating lc.  Phase B is the product r^T [x | RN32(x x) | 1] on the float64 matrix cores, four
//   frames per v_mfma_f64_16x16x4_f64: wavefront v owns rows 16 v .. 16 v + 15 of the pass and all NT column tiles;
//   the B operand is formed from the staged float32 frame as it is read.  A chunk, and a 4-frame step of a row tile,
//   whose weights are all exactly 0.0 is skipped.  One partial row {post_mix[S][M], obs[S][M][D], obs2[S][M][D]} per
//   (group, w), every element of it written; embed_full_fold_kernel adds the groups behind the head.
constexpr int kEmGmmFS = kEmFullChunk + 2;  // LDS stride of r[row][frame] (doubles): the 16 rows x 2 frames of a
                                            // half-wavefront's A operand on 32 distinct bank pairs
constexpr int kEmGmmGF = kEmFullChunk + 1;  // LDS stride of g[state][frame] (doubles), odd

template <int MP>
constexpr int kEmGmmStates = 64 / MP > kMaxS ? kMaxS : 64 / MP;  // states of one pass

inline size_t em_gmm_p(int S, int M, int D) { return static_cast<size_t>(S) * M * (2 * D + 1); }

template <int MP, int DP>
__global__ __launch_bounds__(kXBlock) void embed_gmm_accum_kernel(
    const double *__restrict__ gamma, const float *__restrict__ feats, int32_t D, const double *__restrict__ pack,
    int64_t pack_stride, int32_t M, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const int32_t *__restrict__ words, const int64_t *__restrict__ word_offsets, int64_t total_words,
    int32_t max_words, int32_t W, int32_t S, int32_t SP, int64_t group_utts, const double *__restrict__ loglik,
    double *__restrict__ part) {
  constexpr int SG = kEmGmmStates<MP>;
  constexpr int RW = SG * MP;                  // rows of r in a pass
  constexpr int RT = (RW + 15) / 16;           // 16-row tiles of a pass: one wavefront each
  constexpr int NT = (2 * DP + 1 + 15) / 16;   // 16-wide column tiles: x[0..D), RN32(x x)[0..D), the constant 1
  constexpr int FS = kEmGmmFS, GF = kEmGmmGF;
  constexpr int XF = DP | 1;                   // LDS row stride of the staged frames (floats), odd
  static_assert(RT <= kXWaves && RW <= 16 * RT, "a row tile per wavefront");
  __shared__ double s_r[16 * RT * FS];
  __shared__ double s_g[SG * GF];
  __shared__ float s_x[kEmFullChunk * XF];

  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, k = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t grp = blockIdx.x;
  const int w = blockIdx.y;
  const int64_t u_lo = grp * group_utts;
  const int64_t u_hi = u_lo + group_utts < n_utts ? u_lo + group_utts : n_utts;
  const int MPW = max_words * SP;
  const double *__restrict__ mdl = pack + static_cast<int64_t>(w) * pack_stride;  // (uniform)
  const double *__restrict__ cc = mdl + off_cc(SP);
  const double *__restrict__ prm = mdl + off_prm(SP, MP);
  double *__restrict__ out = part + (grp * W + w) * static_cast<int64_t>(S * M * (2 * D + 1));

  // column 16 t + n of B: feature ci[t] as it is (kind 0), its float32 square (1), the constant 1 (2), nothing (3)
  int ci[NT], kind[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * t + n;
    kind[t] = c < D ? 0 : (c < 2 * D ? 1 : (c == 2 * D ? 2 : 3));
    ci[t] = c < D ? c : (c < 2 * D ? c - D : 0);
  }
  // (the rows of the last tile behind RW are read by phase B and never written by phase A)
  for (int i = tid; i < 16 * RT * FS; i += kXBlock) s_r[i] = 0.0;

  for (int g = 0; g * SG < S; ++g) {  // (uniform trip counts: every thread reaches the barriers)
    f64x4_em acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4_em{0.0, 0.0, 0.0, 0.0};
    for (int64_t u = u_lo; u < u_hi; ++u) {
      const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
      // (as in embed_full_accum_kernel: the gamma rows of an utterance without a finite likelihood were never written
      // and may hold NaN; a frame that is read belongs to an utterance whose every logb, hence every feature, is finite)
      if (!ut.path || !finite_f64(loglik[u])) continue;  // (uniform)
      const int wd = lane < ut.K ? words[ut.wbeg + lane] : -1;
      const uint64_t slots = __ballot(wd == w);  // the slots of word w (the same in every wavefront)
      if (slots == 0) continue;
      const double *__restrict__ gu = gamma + ut.beg * MPW;
      const float *__restrict__ xu = feats + ut.beg * D;
      for (int64_t c0 = 0; c0 < ut.T; c0 += kEmFullChunk) {
        {  // g_t(w, s) of the pass's states, the slots collapsed k ascending; 0.0 selected behind the utterance's end
          bool nz = false;
          for (int item = tid; item < kEmFullChunk * SG; item += kXBlock) {
            const int f = item / SG, sj = item - f * SG;
            const int64_t t = c0 + f;
            const int st = g * SG + sj;
            const bool live = t < ut.T && st < S;
            const double *__restrict__ src = gu + (live ? t : 0) * MPW + (live ? st : 0);  // (dead: a valid address)
            double gw = 0.0;
            for (uint64_t m = slots; m; m &= m - 1) gw += src[__builtin_ctzll(m) * SP];
            gw = live ? gw : 0.0;
            s_g[sj * GF + f] = gw;
            nz = nz || gw != 0.0;
          }
          if (!__syncthreads_or(nz)) continue;  // (uniform) nothing of word w in these frames
        }
        // the chunk's frames into LDS, float32 as they are; zeros in the padded dimensions (against their zero mean
        // and zero coefficient they add +0.0) and in the rows past the utterance's last frame
        for (int item = tid; item < kEmFullChunk * DP; item += kXBlock) {
          const int f = item / DP, d = item - f * DP;
          const int64_t t = c0 + f;
          s_x[f * XF + d] = (t < ut.T && d < D) ? xu[t * D + d] : 0.0f;
        }
        __syncthreads();
        // ---- phase A: r of the pass's states for the chunk's 64 frames, lane = frame -----------------------------
        {
          const float *__restrict__ xrow = s_x + lane * XF;
          for (int j = wv; j < SG; j += kXWaves) {
            const int s = g * SG + j;
            const double gm = s_g[j * GF + lane];
            double r[MP];
#pragma unroll
            for (int m = 0; m < MP; ++m) r[m] = 0.0;
            if (s < S && __ballot(gm != 0.0) != 0) {  // (wavefront-uniform)
              double lc[MP];
              mix_log_terms<MP, DP, 16 / MP>([&](int d) { return static_cast<double>(xrow[d]); },
                                             prm + static_cast<int64_t>(s) * DP * MP * 2, cc + s * MP, lc);
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
              const bool off = mx == neg_inf() || gm == 0.0;  // every component switched off, or no weight
#pragma unroll
              for (int m = 0; m < MP; ++m) r[m] = off ? 0.0 : r[m] * scale;
            }
#pragma unroll
            for (int m = 0; m < MP; ++m) s_r[(j * MP + m) * FS + lane] = r[m];
          }
        }
        __syncthreads();
        // ---- phase B: acc[row][col] += r[f][row] * B[f][col] on the matrix cores, four frames per instruction ----
        if (wv < RT) {  // (uniform)
          for (int step = 0; step < kEmFullChunk / 4; ++step) {
            // A and B of the float64 MFMA: lane & 15 = row (column), lane >> 4 = the K index, here the frame
            const int f = 4 * step + k;
            const double ra = s_r[(16 * wv + n) * FS + f];
            if (__ballot(ra != 0.0) == 0) continue;  // (wavefront-uniform) 16 rows x 4 frames that add exact zeros
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const float xf = s_x[f * XF + ci[t]];
              const float v = kind[t] == 1 ? xf * xf : xf;  // X**2 in float32, as numpy squares the array
              const double xb = kind[t] < 2 ? static_cast<double>(v) : (kind[t] == 2 ? 1.0 : 0.0);
              acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra, xb, acc[t], 0, 0, 0);
            }
          }
        }
        __syncthreads();
      }
    }
    if (wv < RT) {
      // C of the float64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * wv + k + 4 * r, c = 16 * t + n;
          const int s = g * SG + row / MP, m = row % MP;
          if (row < RW && s < S && m < M && c <= 2 * D) {
            const int sm = s * M + m;
            const double v = acc[t][r];
            if (c == 2 * D)
              out[sm] = v;
            else if (c < D)
              out[S * M + sm * D + c] = v;
            else
              out[S * M + S * M * D + sm * D + (c - D)] = v;
          }
        }
    }
  }
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_embed_stats_width(int32_t S, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && D >= 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = em_check_shape(1, S, 1)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  *width = 2 + S + S * S + S + 2 * S * D;
  return 0;
}

extern "C" int sapr_connected_embed_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                                    int32_t max_words, int32_t S, int32_t D, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && total_words >= 0 && max_words > 0 && S > 0 && D >= 0,
               "bad sizes (total_frames=%lld n_utts=%lld total_words=%lld max_words=%d S=%d D=%d)",
               (long long)total_frames, (long long)n_utts, (long long)total_words, max_words, S, D);
  if (int rc = em_check_shape(1, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  *bytes = em_carve(nullptr, total_frames, total_words, max_words, S, D).bytes;
  return 0;
}

extern "C" int sapr_connected_embed_opt(const double *logb, const float *feats, int32_t D, const int64_t *offsets,
                                        int64_t n_utts, int64_t total_frames, const int32_t *words,
                                        const int64_t *word_offsets, const uint8_t *optional, int64_t total_words,
                                        int32_t max_words, const double *log_start, const double *log_trans,
                                        const double *log_exit, double word_penalty, int32_t W, int32_t S,
                                        void *workspace, size_t workspace_bytes, double *loglik, double *stats,
                                        double *post, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0 && D >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld total_words=%lld max_words=%d W=%d S=%d D=%d)",
               (long long)n_utts, (long long)total_frames, (long long)total_words, max_words, W, S, D);
  if (int rc = em_check_shape(W, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  size_t need = 0;
  if (int rc = sapr_connected_embed_workspace_bytes(total_frames, n_utts, total_words, max_words, S, D, &need))
    return rc;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  SAPR_REQUIRE((n_utts + 0) <= 0x7fffffffLL, "grid too large (%lld utterances)", (long long)n_utts);
  SAPR_REQUIRE(em_chunks(total_words) <= 65535, "too many transcript words for one call (%lld; at most %d)",
               (long long)total_words, 65535 * kEmFoldChunk);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && word_offsets && log_start && log_trans && log_exit && loglik && (total_frames == 0 || logb) &&
                   (total_words == 0 || words) && (D == 0 || total_frames == 0 || !stats || feats),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const EmWorkspace ws = em_carve(workspace, total_frames, total_words, max_words, S, D);
  const int32_t part_width = static_cast<int32_t>(em_part_width(SP, D));
  hipStream_t st = as_stream(stream);
  const EmArgs a{logb, offsets, n_utts, total_frames, words, word_offsets, total_words, max_words,
                 log_start, log_trans, log_exit, word_penalty, W, S, optional};
  const bool backward = stats || post;
  if (backward && total_words > 0) SAPR_HIP_TRY(hipMemsetAsync(ws.slot_ok, 0, static_cast<size_t>(total_words), st));
  const int rc = x_dispatch(SP, max_words * SP, [&](auto rl, auto sp) {
    constexpr int RL = decltype(rl)::value, SPc = decltype(sp)::value;
    return optional ? launch_recursions<RL, SPc, true>(a, ws, part_width, loglik, post, backward, st)
                    : launch_recursions<RL, SPc, false>(a, ws, part_width, loglik, post, backward, st);
  });
  if (rc || !stats) return rc;
  if (D > 0 && total_frames > 0) {
    SAPR_LAUNCH(embed_obs_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(kXBlock), 0, st, ws.alpha, feats, D,
                offsets, n_utts, total_frames, word_offsets, total_words, max_words, SP, part_width, loglik, ws.part);
    SAPR_HIP_TRY(hipGetLastError());
  }
  const int32_t width = 2 + S + S * S + S + 2 * S * D;
  const int64_t chunks = em_chunks(total_words);
  const unsigned tiles = static_cast<unsigned>((width + kXBlock - 1) / kXBlock);
  if (chunks > 0) {
    SAPR_LAUNCH(embed_fold_chunk_kernel, dim3(tiles, static_cast<unsigned>(W), static_cast<unsigned>(chunks)),
                dim3(kXBlock), 0, st, ws.part, ws.slot_ok, words, total_words, W, S, SP, D, part_width, width, ws.fold);
    SAPR_HIP_TRY(hipGetLastError());
  }
  SAPR_LAUNCH(embed_fold_kernel, dim3(tiles, static_cast<unsigned>(W)), dim3(kXBlock), 0, st, ws.fold, chunks, W,
              width, stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sapr_connected_embed(const double *logb, const float *feats, int32_t D, const int64_t *offsets,
                                    int64_t n_utts, int64_t total_frames, const int32_t *words,
                                    const int64_t *word_offsets, int64_t total_words, int32_t max_words,
                                    const double *log_start, const double *log_trans, const double *log_exit,
                                    double word_penalty, int32_t W, int32_t S, void *workspace, size_t workspace_bytes,
                                    double *loglik, double *stats, double *post, void *stream) {
  return sapr_connected_embed_opt(logb, feats, D, offsets, n_utts, total_frames, words, word_offsets, nullptr,
                                  total_words, max_words, log_start, log_trans, log_exit, word_penalty, W, S, workspace,
                                  workspace_bytes, loglik, stats, post, stream);
}

extern "C" int sapr_connected_embed_full_stats_width(int32_t S, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && D >= 0, "bad sizes (S=%d D=%d)", S, D);
  if (int rc = em_check_shape(1, S, 1)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  *width = static_cast<int32_t>(em_head_width(S) + em_full_p(S, D));
  return 0;
}

extern "C" int sapr_connected_embed_full_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                                         int32_t max_words, int32_t W, int32_t S, int32_t D,
                                                         size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0 &&
                   D >= 0,
               "bad sizes (total_frames=%lld n_utts=%lld total_words=%lld max_words=%d W=%d S=%d D=%d)",
               (long long)total_frames, (long long)n_utts, (long long)total_words, max_words, W, S, D);
  if (int rc = em_check_shape(W, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  *bytes = em_full_carve(nullptr, total_frames, n_utts, total_words, max_words, W, S, em_full_p(S, D)).bytes;
  return 0;
}

// The host body the two entries with wider rows share ("full": obs*obs.T, "gmm": the per-component sums), after each
// entry's own size and shape checks: the workspace and pointer checks, the carve, sapr_connected_embed itself on the
// front of the workspace, one accumulation kernel over (groups, W) and the fold.  P: the doubles of a row behind its
// head; what: the word for the D >= 1 message; missing: an entry's own NULL-pointer refusal, or NULL; launch(grid, st,
// gamma, SP, per, part) launches the entry's accumulation kernel.
template <typename Launch>
static int embed_wide_rows(const double *logb, const float *feats, int32_t D, const int64_t *offsets, int64_t n_utts,
                           int64_t total_frames, const int32_t *words, const int64_t *word_offsets,
                           const uint8_t *optional, int64_t total_words, int32_t max_words, const double *log_start,
                           const double *log_trans, const double *log_exit, double word_penalty, int32_t W, int32_t S,
                           void *workspace, size_t workspace_bytes, double *loglik, double *stats, double *post,
                           void *stream, size_t P, const char *what, const char *missing, Launch &&launch) {
  const size_t need = em_full_carve(nullptr, total_frames, n_utts, total_words, max_words, W, S, P).bytes;
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  SAPR_REQUIRE(!stats || D >= 1, "the %s need D >= 1 (got D=%d)", what, D);
  SAPR_REQUIRE(!missing, "%s", missing);
  SAPR_REQUIRE(!stats || n_utts == 0 || total_frames == 0 || feats, "NULL pointer argument");
  const EmFullWorkspace ws = em_full_carve(workspace, total_frames, n_utts, total_words, max_words, W, S, P);
  // the recursions, loglik, post and the head of the row: sapr_connected_embed itself on the front of the workspace,
  // without features (the head does not depend on them); gamma stays behind in the workspace
  if (int rc = sapr_connected_embed_opt(logb, nullptr, 0, offsets, n_utts, total_frames, words, word_offsets, optional,
                                        total_words, max_words, log_start, log_trans, log_exit, word_penalty, W, S,
                                        workspace, ws.base_bytes, loglik, stats ? ws.head : nullptr, post, stream))
    return rc;
  if (n_utts == 0 || !stats) return 0;
  hipStream_t st = as_stream(stream);
  const int64_t groups = em_full_groups(n_utts), per = em_full_group_utts(n_utts);
  launch(dim3(static_cast<unsigned>(groups), static_cast<unsigned>(W)), st, static_cast<const double *>(workspace),
         sp_of(S), per, ws.part);
  SAPR_HIP_TRY(hipGetLastError());
  const int32_t hw = static_cast<int32_t>(em_head_width(S));
  const unsigned tiles = static_cast<unsigned>((hw + P + kXBlock - 1) / kXBlock);
  SAPR_LAUNCH(embed_full_fold_kernel, dim3(tiles, static_cast<unsigned>(W)), dim3(kXBlock), 0, st, ws.head, ws.part,
              groups, W, hw, static_cast<int32_t>(P), stats);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sapr_connected_embed_full_opt(const double *logb, const float *feats, int32_t D,
                                             const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                             const int32_t *words, const int64_t *word_offsets,
                                             const uint8_t *optional, int64_t total_words, int32_t max_words,
                                             const double *log_start, const double *log_trans, const double *log_exit,
                                             double word_penalty, int32_t W, int32_t S, void *workspace,
                                             size_t workspace_bytes, double *loglik, double *stats, double *post,
                                             void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0 && D >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld total_words=%lld max_words=%d W=%d S=%d D=%d)",
               (long long)n_utts, (long long)total_frames, (long long)total_words, max_words, W, S, D);
  if (int rc = em_check_shape(W, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  return embed_wide_rows(
      logb, feats, D, offsets, n_utts, total_frames, words, word_offsets, optional, total_words, max_words, log_start,
      log_trans, log_exit, word_penalty, W, S, workspace, workspace_bytes, loglik, stats, post, stream,
      em_full_p(S, D), "second moments", nullptr,
      [&](dim3 grid, hipStream_t st, const double *gamma, int32_t SP, int64_t per, double *part) {
#define SAPR_EM_FULL_ACCUM(DP)                                                                                        \
  SAPR_LAUNCH(embed_full_accum_kernel<DP>, grid, dim3(kXBlock), 0, st, gamma, feats, D, offsets, n_utts,            \
              total_frames, words, word_offsets, total_words, max_words, W, S, SP, per, loglik, part)
        switch (dp_of(D)) {
          case 13: SAPR_EM_FULL_ACCUM(13); break;
          case 26: SAPR_EM_FULL_ACCUM(26); break;
          default: SAPR_EM_FULL_ACCUM(39); break;
        }
#undef SAPR_EM_FULL_ACCUM
      });
}

extern "C" int sapr_connected_embed_full(const double *logb, const float *feats, int32_t D, const int64_t *offsets,
                                         int64_t n_utts, int64_t total_frames, const int32_t *words,
                                         const int64_t *word_offsets, int64_t total_words, int32_t max_words,
                                         const double *log_start, const double *log_trans, const double *log_exit,
                                         double word_penalty, int32_t W, int32_t S, void *workspace,
                                         size_t workspace_bytes, double *loglik, double *stats, double *post,
                                         void *stream) {
  return sapr_connected_embed_full_opt(logb, feats, D, offsets, n_utts, total_frames, words, word_offsets, nullptr,
                                       total_words, max_words, log_start, log_trans, log_exit, word_penalty, W, S,
                                       workspace, workspace_bytes, loglik, stats, post, stream);
}

extern "C" int sapr_connected_embed_gmm_stats_width(int32_t S, int32_t M, int32_t D, int32_t *width) {
  SAPR_REQUIRE(width && S > 0 && M > 0 && D > 0, "bad sizes (S=%d M=%d D=%d)", S, M, D);
  if (int rc = em_check_shape(1, S, 1)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  if (int rc = check_shape(S, M, D)) return rc;
  *width = static_cast<int32_t>(em_head_width(S) + em_gmm_p(S, M, D));
  return 0;
}

extern "C" int sapr_connected_embed_gmm_workspace_bytes(int64_t total_frames, int64_t n_utts, int64_t total_words,
                                                        int32_t max_words, int32_t W, int32_t S, int32_t M, int32_t D,
                                                        size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0 &&
                   M > 0 && D >= 0,
               "bad sizes (total_frames=%lld n_utts=%lld total_words=%lld max_words=%d W=%d S=%d M=%d D=%d)",
               (long long)total_frames, (long long)n_utts, (long long)total_words, max_words, W, S, M, D);
  if (int rc = em_check_shape(W, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  if (int rc = check_shape(S, M, D)) return rc;
  *bytes = em_full_carve(nullptr, total_frames, n_utts, total_words, max_words, W, S, em_gmm_p(S, M, D)).bytes;
  return 0;
}

extern "C" int sapr_connected_embed_gmm_opt(const double *logb, const float *feats, int32_t D, const double *pack,
                                            int32_t M, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                            const int32_t *words, const int64_t *word_offsets,
                                            const uint8_t *optional, int64_t total_words, int32_t max_words,
                                            const double *log_start, const double *log_trans, const double *log_exit,
                                            double word_penalty, int32_t W, int32_t S, void *workspace,
                                            size_t workspace_bytes, double *loglik, double *stats, double *post,
                                            void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0 && M > 0 &&
                   D >= 0,
               "bad sizes (n_utts=%lld total_frames=%lld total_words=%lld max_words=%d W=%d S=%d M=%d D=%d)",
               (long long)n_utts, (long long)total_frames, (long long)total_words, max_words, W, S, M, D);
  if (int rc = em_check_shape(W, S, max_words)) return rc;
  if (int rc = em_check_dims(D)) return rc;
  if (int rc = check_shape(S, M, D)) return rc;
  const char *missing = !stats || n_utts == 0 || pack ? nullptr : "NULL pointer argument (pack)";
  const int64_t stride = static_cast<int64_t>(model_doubles(sp_of(S), mp_of(M), dp_of(D)));
  return embed_wide_rows(
      logb, feats, D, offsets, n_utts, total_frames, words, word_offsets, optional, total_words, max_words, log_start,
      log_trans, log_exit, word_penalty, W, S, workspace, workspace_bytes, loglik, stats, post, stream,
      em_gmm_p(S, M, D), "mixture statistics", missing,
      [&](dim3 grid, hipStream_t st, const double *gamma, int32_t SP, int64_t per, double *part) {
#define SAPR_EM_GMM_ACCUM(MP, DP)                                                                                     \
  SAPR_LAUNCH((embed_gmm_accum_kernel<MP, DP>), grid, dim3(kXBlock), 0, st, gamma, feats, D, pack, stride, M,        \
              offsets, n_utts, total_frames, words, word_offsets, total_words, max_words, W, S, SP, per, loglik, part)
#define SAPR_EM_GMM_ACCUM_DP(MP)                                                                                      \
  switch (dp_of(D)) {                                                                                                 \
    case 13: SAPR_EM_GMM_ACCUM(MP, 13); break;                                                                        \
    case 26: SAPR_EM_GMM_ACCUM(MP, 26); break;                                                                        \
    default: SAPR_EM_GMM_ACCUM(MP, 39); break;                                                                        \
  }
        switch (mp_of(M)) {
          case 1: SAPR_EM_GMM_ACCUM_DP(1); break;
          case 2: SAPR_EM_GMM_ACCUM_DP(2); break;
          case 4: SAPR_EM_GMM_ACCUM_DP(4); break;
          default: SAPR_EM_GMM_ACCUM_DP(8); break;
        }
#undef SAPR_EM_GMM_ACCUM_DP
#undef SAPR_EM_GMM_ACCUM
      });
}

extern "C" int sapr_connected_embed_gmm(const double *logb, const float *feats, int32_t D, const double *pack,
                                        int32_t M, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                        const int32_t *words, const int64_t *word_offsets, int64_t total_words,
                                        int32_t max_words, const double *log_start, const double *log_trans,
                                        const double *log_exit, double word_penalty, int32_t W, int32_t S,
                                        void *workspace, size_t workspace_bytes, double *loglik, double *stats,
                                        double *post, void *stream) {
  return sapr_connected_embed_gmm_opt(logb, feats, D, pack, M, offsets, n_utts, total_frames, words, word_offsets,
                                      nullptr, total_words, max_words, log_start, log_trans, log_exit, word_penalty, W,
                                      S, workspace, workspace_bytes, loglik, stats, post, stream);
}
