// Decode with the reference's from-scratch HMM: Viterbi over the first Tq frames (assignment2/custom_hmm.py:462-514)
// and the recogniser's choice among the word models (decoder.py:35-49).  CPU restatement: oracle/custom_hmm_oracle.py.
//
//   custom_decode_lr_kernel<10 | 18>   the trellis in registers: S in {10, 18} unless SAPR_CUSTOM_DECODE_GENERIC=1
//   custom_decode_kernel               run-time S: every other shape, and the tests' reference for the two above
//   custom_best_word_kernel            first strict maximum over the models, when the caller asks for it
// The emission rows come from sapr_custom_emission_exact (custom_emission.hip), called through its C declaration.
#include <cstdlib>
#include <type_traits>

#include "sapr_common.h"

namespace sapr {
namespace {

#include "custom_np.h"

// Viterbi of custom_hmm.py:462-514 for every (utterance, model) over the first Tq frames (Tq =
// features.shape[0] = D, the reference's quirk), strict '>' from -inf.  Erows[(u*W+w)*Tq + t][S] comes from
// custom_emission_exact_kernel, so V holds the reference's bits: np.log(A) is evaluated on the host and the
// trellis only adds and compares.  scores[u][w]; paths[u][w][Tq].
__global__ __launch_bounds__(kBlock) void custom_decode_kernel(
    const double *__restrict__ Erows, int64_t n_utts, int W, int S, int num_states, int Tq, CustomPack P,
    double *__restrict__ scores, int32_t *__restrict__ paths) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x;
  if (idx >= n_utts * W) return;
  const int w = static_cast<int>(idx % W);
  const double *E = Erows + idx * static_cast<int64_t>(Tq) * S;
  const double *lA = P.logA + static_cast<int64_t>(w) * S * S;

  double V[kMaxS], Vn[kMaxS];
  int32_t *bp = paths + idx * static_cast<int64_t>(Tq);
  // back-pointers: Tq x S small ints in a local array (Tq <= kMaxD, S <= kMaxS)
  unsigned char back[kMaxD * kMaxS];
  for (int s = 0; s < S; ++s) V[s] = neg_inf();
  for (int i = 0; i < Tq * S; ++i) back[i] = 0;
  V[0] = 0.0;
  V[1] = lA[0 * S + 1] + E[1];
  for (int t = 1; t < Tq; ++t) {
    for (int s = 0; s < S; ++s) Vn[s] = neg_inf();
    for (int j = 1; j < S; ++j) {
      int cand[2], nc = 0;
      if (j == 1) {
        cand[nc++] = 1;
        if (t == 1) cand[nc++] = 0;
      } else if (j == S - 1) {
        if (t < num_states) continue;
        cand[nc++] = j - 1;
        cand[nc++] = j;
      } else {
        cand[nc++] = j - 1;
        cand[nc++] = j;
      }
      double best = neg_inf();
      int arg = -1;
      for (int c = 0; c < nc; ++c) {
        const double sc = V[cand[c]] + lA[cand[c] * S + j];
        if (sc > best) {
          best = sc;
          arg = cand[c];
        }
      }
      if (arg >= 0) {
        Vn[j] = (j != S - 1) ? best + E[static_cast<int64_t>(t) * S + j] : best;
        back[t * S + j] = static_cast<unsigned char>(arg);
      }
    }
    for (int s = 0; s < S; ++s) V[s] = Vn[s];
  }
  scores[idx] = V[S - 1];
  int cur = S - 1;
  for (int t = Tq - 1; t >= 0; --t) {
    bp[t] = cur;
    cur = back[t * S + cur];
  }
}

// The same trellis for the left-to-right models of this vocabulary with S as a template parameter (10, 18): scores,
// transition terms and the frame's emission row live in registers (the kernel above indexes V[] / back[] with run-time
// values: scratch, and its loads sit inside the dependent chain), the next frame's row is loaded under the current
// frame's arithmetic, the back-pointers of a frame are one 64-bit word (2 bits per state: 0 = unset -> state 0 as in
// the byte array above, 1 = from j - 1, 2 = stay).  Same comparisons in the same order.
template <int S>
__global__ __launch_bounds__(kBlock) void custom_decode_lr_kernel(
    const double *__restrict__ Erows, int64_t n_utts, int W, int num_states, int Tq, CustomPack P,
    double *__restrict__ scores, int32_t *__restrict__ paths) {
  const int64_t idx = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x;
  if (idx >= n_utts * W) return;
  const int w = static_cast<int>(idx % W);
  const double *E = Erows + idx * static_cast<int64_t>(Tq) * S;
  const double *lA = P.logA + static_cast<int64_t>(w) * S * S;
  double a_in[S], a_st[S], V[S];
#pragma unroll
  for (int j = 1; j < S; ++j) {
    a_in[j] = lA[(j - 1) * S + j];
    a_st[j] = lA[j * S + j];
  }
#pragma unroll
  for (int s = 0; s < S; ++s) V[s] = neg_inf();
  V[0] = 0.0;
  V[1] = a_in[1] + E[1];
  unsigned long long back[kMaxD];
  back[0] = 0;
  double e_next[S - 2];
#pragma unroll
  for (int i = 0; i < S - 2; ++i) e_next[i] = Tq > 1 ? E[S + 1 + i] : 0.0;
  for (int t = 1; t < Tq; ++t) {
    double e[S - 2], Vn[S];
#pragma unroll
    for (int i = 0; i < S - 2; ++i) e[i] = e_next[i];
    if (t + 1 < Tq) {
#pragma unroll
      for (int i = 0; i < S - 2; ++i) e_next[i] = E[static_cast<int64_t>(t + 1) * S + 1 + i];
    }
    unsigned long long bits = 0;
    Vn[0] = neg_inf();
    {  // j == 1: stay, then (first step only) the entry state
      double best = neg_inf();
      unsigned code = 0;
      const double s_stay = V[1] + a_st[1];
      if (s_stay > best) {
        best = s_stay;
        code = 2;
      }
      if (t == 1) {
        const double s_in = V[0] + a_in[1];
        if (s_in > best) {
          best = s_in;
          code = 1;
        }
      }
      Vn[1] = code ? best + e[0] : neg_inf();
      bits |= static_cast<unsigned long long>(code) << 2;
    }
#pragma unroll
    for (int j = 2; j < S - 1; ++j) {
      double best = neg_inf();
      unsigned code = 0;
      const double s_in = V[j - 1] + a_in[j], s_stay = V[j] + a_st[j];
      if (s_in > best) {
        best = s_in;
        code = 1;
      }
      if (s_stay > best) {
        best = s_stay;
        code = 2;
      }
      Vn[j] = code ? best + e[j - 1] : neg_inf();
      bits |= static_cast<unsigned long long>(code) << (2 * j);
    }
    Vn[S - 1] = neg_inf();
    if (t >= num_states) {  // the exit state: no emission term
      double best = neg_inf();
      unsigned code = 0;
      const double s_in = V[S - 2] + a_in[S - 1], s_stay = V[S - 1] + a_st[S - 1];
      if (s_in > best) {
        best = s_in;
        code = 1;
      }
      if (s_stay > best) {
        best = s_stay;
        code = 2;
      }
      if (code) Vn[S - 1] = best;
      bits |= static_cast<unsigned long long>(code) << (2 * (S - 1));
    }
    back[t] = bits;
#pragma unroll
    for (int s = 0; s < S; ++s) V[s] = Vn[s];
  }
  scores[idx] = V[S - 1];
  int32_t *bp = paths + idx * static_cast<int64_t>(Tq);
  int cur = S - 1;
  for (int t = Tq - 1; t >= 0; --t) {
    bp[t] = cur;
    const unsigned code = static_cast<unsigned>(back[t] >> (2 * cur)) & 3u;
    cur = code == 2 ? cur : code == 1 ? cur - 1 : 0;
  }
}

// decoder.py:35-49 over the custom models: first strict maximum in model order starting from -inf
// (a NaN score never wins; no finite or +inf score -> word -1, score -inf, path untouched).
__global__ void custom_best_word_kernel(const double *__restrict__ scores, const int32_t *__restrict__ paths,
                                        int64_t n_utts, int W, int Tq, int32_t *__restrict__ best_word,
                                        double *__restrict__ best_score, int32_t *__restrict__ best_path) {
  const int64_t u = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (u >= n_utts) return;
  double best = neg_inf();
  int bw = -1;
  for (int w = 0; w < W; ++w) {
    const double sc = scores[u * W + w];
    if (sc > best) {
      best = sc;
      bw = w;
    }
  }
  best_word[u] = bw;
  best_score[u] = best;
  if (bw >= 0)
    for (int t = 0; t < Tq; ++t) best_path[u * Tq + t] = paths[(u * W + bw) * static_cast<int64_t>(Tq) + t];
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_custom_decode(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t W,
                                  int32_t D, int32_t S, int32_t num_states, int32_t Tq, const double *means,
                                  const double *inv, const double *cterm, const double *A, const double *logA,
                                  double *e_rows, double *scores, int32_t *paths, int32_t *best_word,
                                  double *best_score, int32_t *best_path, void *stream) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0 && W > 0 && Tq > 0 && Tq <= kMaxD, "bad sizes (Tq <= %d)", kMaxD);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(feats && offsets && means && inv && cterm && A && logA && e_rows && scores && paths,
               "NULL pointer argument");
  SAPR_REQUIRE((best_word == nullptr) == (best_score == nullptr) && (best_word == nullptr) == (best_path == nullptr),
               "best_word / best_score / best_path go together");
  // every utterance must hold at least Tq frames (the reference raises IndexError otherwise,
  // custom_hmm.py:500): the host mirror checks before the launch
  if (int rc = sapr_custom_emission_exact(feats, offsets, n_utts, W, D, S, Tq, Tq, means, inv, cterm, e_rows, stream))
    return rc;
  CustomPack P{means, inv, cterm, A, logA};
  const int64_t n = n_utts * W;
  hipStream_t st = as_stream(stream);
  const dim3 dgrid(static_cast<unsigned>((n + kBlock - 1) / kBlock));
  static const bool generic_trellis = [] {
    const char *e = std::getenv("SAPR_CUSTOM_DECODE_GENERIC");
    return e && e[0] == '1';
  }();
  if (S == 10 && !generic_trellis)
    SAPR_LAUNCH(custom_decode_lr_kernel<10>, dgrid, dim3(kBlock), 0, st, e_rows, n_utts, W, num_states, Tq, P, scores, paths);
  else if (S == 18 && !generic_trellis)
    SAPR_LAUNCH(custom_decode_lr_kernel<18>, dgrid, dim3(kBlock), 0, st, e_rows, n_utts, W, num_states, Tq, P, scores, paths);
  else
    SAPR_LAUNCH(custom_decode_kernel, dgrid, dim3(kBlock), 0, st, e_rows, n_utts, W, S, num_states, Tq, P, scores, paths);
  if (best_word)
    SAPR_LAUNCH(custom_best_word_kernel, dim3(static_cast<unsigned>((n_utts + 255) / 256)), dim3(256), 0, st, scores,
                paths, n_utts, W, Tq, best_word, best_score, best_path);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
