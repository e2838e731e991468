// Forced alignment on gfx950: Viterbi over the left-to-right chain of an utterance's K transcript words.
// Word slot k is entered only from the exit of slot k - 1 and the score is read only at the exit of the last slot.
// CPU restatement, which is the definition: tests/_align_ref.py.  The input logb[total_frames][R = W * SP] is what the
// three emission stages of connected.hip write; this unit knows nothing about the emission family.
//
// connected_align_kernel<RL, SP>: the lane layout of connected_lanes.h over the P = K * SP chain positions, four
// utterances per workgroup (written out in the kernel: it keeps the text it was timed with, and takes the constants,
// the X step and the host side from the header).  What differs from the word loop:
//   * the network differs per utterance, so the workgroup shares the vocabulary's table by word in LDS
//     (<= 256 * 18 doubles = 36 KB) and every lane indexes it through its own word;
//   * the emission row is a gather: the lane reads logb[t][w_k * SP + s] (consecutive doubles within a slot; the next
//     frame's values are in flight under the current frame's chain);
//   * the coupling is a segmented exit maximum through a per-wavefront LDS row: every lane writes delta + log_exit,
//     lane q < K takes the first maximum over the SP values of slot q (s ascending) and writes X(q) behind it, and the
//     lanes of slot q + 1 read it back.
// Back-pointers: one byte per (frame, position) — the predecessor state, or kXEntry where the entry won — in rows of
// max_words * SP, and one byte per (frame, slot) — the state that attained X — in rows of max_words, both in the
// workspace.  connected_align_backtrace_kernel, one lane per utterance, walks back and writes the path rows and
// word_start.
//
// OPT (definition tests/_optional_ref.py): transcript slots marked optional may be stepped over.  No two
// neighbours are optional, so a slot has at most two predecessor slots: the X row gets a second leading -inf and a slot
// also reads X of the slot two before it, taken only where strictly greater and recorded as the back-pointer byte
// kAlSkipEntry; the wavefront leaves the slot its path ends in for the back-trace, one byte per utterance behind the
// workspace.  The new paths stand under `if constexpr (OPT)`: the OPT = false instantiations are the kernels as they
// were, and they are what a call without flags launches.
//
// The recursion is float64 adds and compares in the order of the definition: bit for bit the restatement.  No atomics;
// an utterance's outputs are a function of its own frames, its own transcript and the network.  Non-finite values
// propagate, and every index used in the walk is clamped into its row.
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kAlXRow = kWave + 2;    // X row of one wavefront: [0] = -inf (nothing enters slot 0), [q + 1] = X(q)
constexpr int kAlSkipEntry = 254;      // back-pointer byte: the word was entered from the slot two before it

inline int al_check_shape(int32_t W, int32_t S, int32_t max_words) {
  return x_check_chain_shape("alignment", W, S, max_words);
}

template <int RL, int SP, bool OPT>
__global__ __launch_bounds__(kXBlock) void connected_align_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const int32_t *__restrict__ words, const int64_t *__restrict__ word_offsets, int64_t total_words, int32_t max_words,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    double word_penalty, int32_t W, int32_t S, uint8_t *__restrict__ bp, uint8_t *__restrict__ xarg,
    double *__restrict__ score, const uint8_t *__restrict__ optional, uint8_t *__restrict__ end_slot) {
  constexpr int PP = kWave * RL;  // positions the lanes hold (P <= max_words * SP <= PP)
  // tab[w][dd][j] = log_trans[w][i][j] with i = (j - dd) mod SP; then per wavefront cbuf[PP], xbuf[kAlXRow]
  extern __shared__ double smem[];
  double *tab = smem;
  const int n_tab = W * SP * SP;
  for (int n = threadIdx.x; n < n_tab; n += kXBlock) {
    const int w = n / (SP * SP), rem = n - w * (SP * SP);
    const int dd = rem / SP, j = rem - dd * SP;
    const int i = j >= dd ? j - dd : j - dd + SP;
    tab[n] = (i < S && j < S) ? log_trans[(static_cast<int64_t>(w) * S + i) * S + j] : neg_inf();
  }
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cbuf = smem + n_tab + wave * (PP + kAlXRow);
  double *xbuf = cbuf + PP;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXWaves + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  const int64_t T = end - beg;
  int64_t wbeg = word_offsets[u], wend = word_offsets[u + 1];
  if (wbeg < 0 || wend < wbeg || wend > total_words) wend = wbeg = 0;
  const int64_t K64 = wend - wbeg;
  bool path = T > 0 && K64 > 0 && K64 <= max_words;  // (max_words <= 64: a slot per lane in the X step)
  const int K = path ? static_cast<int>(K64) : 0;
  {  // a word outside the vocabulary: no path, and nothing of it is used as an index
    const int w = lane < K ? words[wbeg + lane] : 0;
    if (__ballot(w < 0 || w >= W)) path = false;
  }
  [[maybe_unused]] uint64_t om = 0;  // OPT: bit q = slot q is optional
  if constexpr (OPT) {  // a flag that is not 0 or 1, two optional neighbours, no mandatory slot: no path
    const int o = lane < K ? optional[wbeg + lane] : 0;
    om = __ballot(o == 1);
    const uint64_t all = K >= kWave ? ~0ull : (1ull << K) - 1;
    if (__ballot(o > 1) || (om & (om >> 1)) || om == all) path = false;
  }
  if (!path) {
    if (lane == 0) score[u] = neg_inf();
    return;
  }
  const int P = K * SP;
  const int R = W * SP;
  const int MP = max_words * SP;

  // the distances d = j - i in -(SP - 1) .. SP - 1 at which some transition of the vocabulary is finite (bit
  // d + SP - 1): every wavefront reads the whole table, so the mask is the same in all four
  uint64_t dmask = 0;
  for (int n = lane; n < n_tab; n += kWave) {
    const int rem = n % (SP * SP);
    const int dd = rem / SP, j = rem - dd * SP;
    const int d = j >= dd ? dd : dd - SP;
    if (!(tab[n] == neg_inf())) dmask |= 1ull << (d + SP - 1);
  }
  {
    unsigned lo = static_cast<unsigned>(dmask), hi = static_cast<unsigned>(dmask >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo |= __shfl_xor(lo, o, kWave);
      hi |= __shfl_xor(hi, o, kWave);
    }
    dmask = (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(hi)) << 32) | __builtin_amdgcn_readfirstlane(lo);
  }

  double ls[RL], lx[RL], delta[RL], bn[RL];
  int sk[RL], qk[RL], col[RL], tb[RL];
  bool ok[RL];
  [[maybe_unused]] bool far[RL], first[RL];  // OPT: the slot may be entered from slot q - 2; the path may start in it
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const int p = k * kWave + lane;
    const int q = p / SP, s = p - q * SP;
    ok[k] = p < P;
    const int w = ok[k] ? words[wbeg + q] : 0;  // (checked above: 0 .. W - 1)
    sk[k] = s;
    qk[k] = ok[k] ? q : 0;
    if constexpr (OPT) {
      far[k] = ok[k] && q >= 2 && ((om >> (q - 1)) & 1ull);
      first[k] = qk[k] == 0 || (qk[k] == 1 && (om & 1ull));  // (qk = 1 only where K > 1)
    }
    col[k] = w * SP + s;
    tb[k] = w * (SP * SP) + s;
    const bool real = ok[k] && s < S;
    ls[k] = real ? log_start[w * S + s] : neg_inf();
    lx[k] = real ? log_exit[w * S + s] : neg_inf();
    delta[k] = neg_inf();
  }

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[col[k]] : neg_inf();
  if (lane == 0) xbuf[0] = neg_inf();
  if constexpr (OPT)  // two leading -inf: [q + 2] = X(q), slot q reads [q + 1] (near) and [q] (far)
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
    int back[RL];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        v[k] = ls[k];
        back[k] = kXEntry;
      }
    } else {
      double xe[RL];  // X_{t-1} of the slot before the lane's own (-inf in front of slot 0)
      [[maybe_unused]] bool skip[RL];  // OPT: ... of the slot two before it, where that is strictly greater
      if constexpr (OPT) {
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const double near = xbuf[qk[k] + 1], over = xbuf[qk[k]];
          skip[k] = far[k] && over > near;
          xe[k] = skip[k] ? over : near;
        }
      } else {
#pragma unroll
        for (int k = 0; k < RL; ++k) xe[k] = xbuf[qk[k]];
      }
      double best[RL];
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        best[k] = neg_inf();
        back[k] = 0;
      }
      // predecessors i ascending = distances descending; the first maximum stays (strict compare)
#pragma unroll 1
      for (int d = SP - 1; d > -SP; --d) {
        if (!((dmask >> (d + SP - 1)) & 1ull)) continue;  // (uniform)
        // position p - d: lane (lane - d) & 63 of register k, of k - 1 where lane < d, of k + 1 where lane - d >= 64
        const int off = lane - d;
        const int src = off & (kWave - 1);
        const int drow = (d >= 0 ? d : d + SP) * SP;
        double rot[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) rot[k] = __shfl(delta[k], src, kWave);
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
          const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
          const double prev = off < 0 ? below : (off >= kWave ? above : rot[k]);
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double lt = tab[tb[k] + drow];
          const double c = prev + (in ? lt : neg_inf());
          const bool take = c > best[k];
          best[k] = take ? c : best[k];
          back[k] = take ? i : back[k];
        }
      }
#pragma unroll
      for (int k = 0; k < RL; ++k) {
        const double entry = (xe[k] + word_penalty) + ls[k];
        const bool take = entry > best[k];
        v[k] = take ? entry : best[k];
        if constexpr (OPT)
          back[k] = take ? (skip[k] ? kAlSkipEntry : kXEntry) : back[k];
        else
          back[k] = take ? kXEntry : back[k];
      }
    }
    uint8_t *__restrict__ bprow = bp + (beg + t) * MP;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      if constexpr (OPT)
        delta[k] = (t == 0 && !first[k]) ? neg_inf() : v[k] + b[k];
      else
        delta[k] = (t == 0 && qk[k] > 0) ? neg_inf() : v[k] + b[k];
      if (ok[k]) {
        bprow[k * kWave + lane] = static_cast<uint8_t>(back[k]);
        cbuf[k * kWave + lane] = delta[k] + lx[k];
      }
    }
    wave_lds_sync();
    if (lane < K) {  // the first maximum over the slot's states, s ascending
      int xs;
      xv = x_first_max<SP>(cbuf + lane * SP, &xs);
      xbuf[lane + (OPT ? 2 : 1)] = xv;
      xarg[(beg + t) * max_words + lane] = static_cast<uint8_t>(xs);
    }
    wave_lds_sync();
  }
  if constexpr (OPT) {  // the path may end in slot K - 2 where the last slot is optional: strictly greater only
    const double before = __shfl(xv, (lane - 1) & (kWave - 1), kWave);
    if (lane == K - 1) {
      const bool early = K >= 2 && ((om >> (K - 1)) & 1ull) && before > xv;
      score[u] = early ? before : xv;
      end_slot[u] = static_cast<uint8_t>(early ? K - 2 : K - 1);
    }
  } else {
    if (lane == K - 1) score[u] = xv;
  }
}

// one lane per utterance walks back from the last slot's best exit at the last frame (OPT: from the slot the
// wavefront left in end_slot, two slots back over a skip entry; a slot stepped over keeps word_start = -1)
template <bool OPT>
__global__ __launch_bounds__(kXBlock) void connected_align_backtrace_kernel(
    const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames, const int32_t *__restrict__ words,
    const int64_t *__restrict__ word_offsets, int64_t total_words, int32_t max_words, int32_t SP,
    const uint8_t *__restrict__ bp, const uint8_t *__restrict__ xarg, const double *__restrict__ score,
    int32_t *__restrict__ path_word, int32_t *__restrict__ path_state, uint8_t *__restrict__ path_entry,
    int32_t *__restrict__ word_start, const uint8_t *__restrict__ end_slot) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x;
  if (u >= n_utts) return;
  const XUtt ut = x_utt(offsets, total_frames, word_offsets, total_words, max_words, u);
  const int64_t beg = ut.beg, T = ut.T, wbeg = ut.wbeg;
  if (word_start)  // (every word of the transcript, laid out or not)
    for (int64_t k = 0; k < ut.n_words; ++k) word_start[wbeg + k] = -1;
  // (a finite score was written only for 0 < K <= max_words, T > 0 and words inside the vocabulary)
  if (!finite_f64(score[u]) || !ut.path) {
    x_no_path(beg, T, path_word, path_state, path_entry);
    return;
  }
  const int K = ut.K;
  const int64_t MP = static_cast<int64_t>(max_words) * SP;
  int q = K - 1;
  if constexpr (OPT) q = end_slot[u] < K ? end_slot[u] : K - 1;
  int s = xarg[(beg + T - 1) * max_words + q];
  s = s < SP ? s : 0;
  for (int64_t t = T - 1; t >= 0; --t) {
    if (path_word) path_word[beg + t] = words[wbeg + q];
    if (path_state) path_state[beg + t] = s;
    const int b = bp[(beg + t) * MP + q * SP + s];
    const bool entry = t == 0 || b == kXEntry || (OPT && b == kAlSkipEntry);
    if (path_entry) path_entry[beg + t] = entry ? 1 : 0;
    if (entry) {
      if (word_start) word_start[wbeg + q] = static_cast<int32_t>(t);
      if (t > 0) {
        if constexpr (OPT) q -= b == kAlSkipEntry ? 1 : 0;
        q = q > 0 ? q - 1 : 0;  // (a finite score enters slot 0 at frame 0 only; keep the walk inside the row)
        s = xarg[(beg + t - 1) * max_words + q];
        s = s < SP ? s : 0;
      }
    } else {
      s = b < SP ? b : 0;
    }
  }
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_align_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t max_words,
                                                    int32_t S, size_t *bytes) {
  SAPR_REQUIRE(bytes && total_frames >= 0 && n_utts >= 0 && max_words > 0 && S > 0,
               "bad sizes (total_frames=%lld n_utts=%lld max_words=%d S=%d)", (long long)total_frames,
               (long long)n_utts, max_words, S);
  if (int rc = al_check_shape(1, S, max_words)) return rc;
  const size_t MP = static_cast<size_t>(max_words) * sp_of(S);
  // back-pointers [total_frames][max_words * SP] bytes, then the exit state of every (frame, slot), each padded to 16
  *bytes = x_align16(static_cast<size_t>(total_frames) * MP) +
           x_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(max_words));
  return 0;
}

extern "C" int sapr_connected_align_opt_workspace_bytes(int64_t total_frames, int64_t n_utts, int32_t max_words,
                                                        int32_t S, size_t *bytes) {
  if (int rc = sapr_connected_align_workspace_bytes(total_frames, n_utts, max_words, S, bytes)) return rc;
  *bytes += x_align16(static_cast<size_t>(n_utts));  // the slot every utterance's path ends in, one byte each
  return 0;
}

extern "C" int sapr_connected_align_opt(const double *logb, const int64_t *offsets, int64_t n_utts,
                                        int64_t total_frames, const int32_t *words, const int64_t *word_offsets,
                                        const uint8_t *optional, int64_t total_words, int32_t max_words,
                                        const double *log_start, const double *log_trans, const double *log_exit,
                                        double word_penalty, int32_t W, int32_t S, void *workspace,
                                        size_t workspace_bytes, double *score, int32_t *path_word, int32_t *path_state,
                                        uint8_t *path_entry, int32_t *word_start, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && total_words >= 0 && max_words > 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld total_words=%lld max_words=%d W=%d S=%d)", (long long)n_utts,
               (long long)total_frames, (long long)total_words, max_words, W, S);
  if (int rc = al_check_shape(W, S, max_words)) return rc;
  size_t need = 0, base = 0;
  if (int rc = sapr_connected_align_workspace_bytes(total_frames, n_utts, max_words, S, &base)) return rc;
  need = base + (optional ? x_align16(static_cast<size_t>(n_utts)) : 0);
  SAPR_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "workspace too small: %zu < %zu", workspace_bytes,
               need);
  const int64_t blocks = (n_utts + kXWaves - 1) / kXWaves;
  SAPR_REQUIRE(blocks <= 0x7fffffffLL, "grid too large (%lld blocks)", (long long)blocks);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && word_offsets && log_start && log_trans && log_exit && score && (total_frames == 0 || logb) &&
                   (total_words == 0 || words),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  uint8_t *bp = static_cast<uint8_t *>(workspace);
  uint8_t *xarg = bp + x_align16(static_cast<size_t>(total_frames) * static_cast<size_t>(max_words) * SP);
  uint8_t *end_slot = optional ? bp + base : nullptr;
  hipStream_t st = as_stream(stream);
  if (int rc = x_dispatch(SP, max_words * SP, [&](auto rl, auto sp) {
        constexpr int RL = decltype(rl)::value, SPc = decltype(sp)::value;
        const size_t lds =
            (static_cast<size_t>(W) * SPc * SPc + static_cast<size_t>(kXWaves) * (kWave * RL + kAlXRow)) * sizeof(double);
        const auto launch = [&](auto kern) {
          return x_launch(kern, blocks, kXBlock, lds, st, logb, offsets, n_utts, total_frames, words, word_offsets,
                          total_words, max_words, log_start, log_trans, log_exit, word_penalty, W, S, bp, xarg, score,
                          optional, end_slot);
        };
        return optional ? launch(connected_align_kernel<RL, SPc, true>) : launch(connected_align_kernel<RL, SPc, false>);
      }))
    return rc;
  if (path_word || path_state || path_entry || word_start) {
    const auto trace = [&](auto kern) {
      return x_launch(kern, (n_utts + kXBlock - 1) / kXBlock, kXBlock, 0, st, offsets, n_utts, total_frames, words,
                      word_offsets, total_words, max_words, SP, bp, xarg, score, path_word, path_state, path_entry,
                      word_start, static_cast<const uint8_t *>(end_slot));
    };
    return optional ? trace(connected_align_backtrace_kernel<true>) : trace(connected_align_backtrace_kernel<false>);
  }
  return 0;
}

extern "C" int sapr_connected_align(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                    const int32_t *words, const int64_t *word_offsets, int64_t total_words,
                                    int32_t max_words, const double *log_start, const double *log_trans,
                                    const double *log_exit, double word_penalty, int32_t W, int32_t S, void *workspace,
                                    size_t workspace_bytes, double *score, int32_t *path_word, int32_t *path_state,
                                    uint8_t *path_entry, int32_t *word_start, void *stream) {
  return sapr_connected_align_opt(logb, offsets, n_utts, total_frames, words, word_offsets, nullptr, total_words,
                                  max_words, log_start, log_trans, log_exit, word_penalty, W, S, workspace,
                                  workspace_bytes, score, path_word, path_state, path_entry, word_start, stream);
}
