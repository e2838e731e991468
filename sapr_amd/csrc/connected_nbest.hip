// Connected-word N-best on gfx950: the n_best <= 8 best DISTINCT word strings of every utterance with their Viterbi
// scores, in one recursion over the word loop under a word-pair language model.  CPU restatement, which
// is the definition: tests/_nbest_ref.py.  The input logb[total_frames][R = W * SP] is what the three emission stages
// of connected.hip write; this unit knows nothing about the emission family.
//
// A hypothesis is (score: double, code: uint64): code is the word string so far as a base-(W + 1) number, the current
// word included, so that two paths carry the same string iff their codes are equal.  Every place of the recursion
// holds a LIST of at most n_best hypotheses with distinct codes, ordered by score descending, then code ascending; an
// empty slot is (-inf, 0).  merge_n of the definition is a function of the candidates' values, so a list may be
// built by inserting the candidates one at a time in any order (nb_insert): the same bytes.
//
// connected_nbest_kernel<RL, SP, NB>: the lane layout of connected_lanes.h over the flat states exactly as
// connected_bigram_kernel uses it — one wavefront per utterance, the transition table by source, lm transposed in LDS,
// the distance mask — with NB in {2, 4, 8} slots per list, n_best <= NB of them in use (uniform; the rest stay empty).
//   * within a word: per live distance the NB scores and codes of the neighbour are rotated (a code is two
//     ds_bpermute's), tab is added and the candidate is inserted into the lane's new list with dedupe on the code;
//   * the coupling goes through per-wavefront LDS rows of (score, code) between wave_lds_sync's: every lane writes
//     its list + log_exit to cbuf; lane v < W merges the lists of word v's states into X(v) (dedupe: two states may
//     carry one string) over the states at which some word can be left (the exit mask, uniform: one state per word
//     under exit_states = "last"); lane w < W merges X(v) + lm[v][w] over v with the word appended to the code into
//     N(w) — a string of cap(W) words cannot grow: overflow; every state lane then reads back the N of its own word
//     and inserts it + log_start beside the within-word candidates.
// No workspace, no back-pointers, no atomics: an utterance's outputs are a function of its own frames and the tables
// alone.  A NaN never enters a list (no compare with it is true), so it drops hypotheses of its utterance only.
// Boundaries come from forced alignment of a returned string (connected_align.hip).
#include "sapr_common.h"

namespace sapr {
namespace {

#include "lse_ops.h"
#include "gmm_ops.h"
#include "connected_lanes.h"

constexpr int kNbMax = 8;  // strings per utterance

// LDS in 8-byte words: shared tab[SP][64 RL], lmt[W][W | 1], lm_end[W]; per wavefront cbuf (scores [NB][64 RL], then
// codes), xbuf and nbuf (scores [NB][64], then codes)
constexpr size_t nb_shared_words(int W, int SP, int RL) {
  return static_cast<size_t>(SP) * kWave * RL + static_cast<size_t>(W) * x_lm_stride(W) + W;
}
constexpr size_t nb_wave_words(int RL, int NB) {
  return static_cast<size_t>(2) * NB * kWave * RL + static_cast<size_t>(4) * NB * kWave;
}

// the 64-bit integer twin of x_rotate: rot[k] = the code of item r - shift, 0 where r - shift leaves 0 .. 64 RL - 1
template <int RL>
__device__ __forceinline__ void nb_rotate_code(const uint64_t (&val)[RL], int lane, int shift, uint64_t (&out)[RL]) {
  const int off = lane - shift;
  const int src = off & (kWave - 1);
  uint64_t rot[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const unsigned lo = __shfl(static_cast<unsigned>(val[k]), src, kWave);
    const unsigned hi = __shfl(static_cast<unsigned>(val[k] >> 32), src, kWave);
    rot[k] = (static_cast<uint64_t>(hi) << 32) | lo;
  }
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const uint64_t below = k > 0 ? rot[k > 0 ? k - 1 : 0] : 0;
    const uint64_t above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : 0;
    out[k] = off < 0 ? below : (off >= kWave ? above : rot[k]);
  }
}

// One candidate (cs, cc) into a list of distinct codes ordered by score descending, then code ascending, of which the
// first n slots are in use: a candidate that is not > -inf (or NaN) goes before nothing; where the list holds the
// candidate's code already, the better of the two stays; otherwise the candidate takes its place, what follows moves
// down one slot and the last falls off.  One pass: `carry` is the candidate until it has taken a slot, then the
// displaced entry on its way down; it ends at the slot that held the candidate's own code (own).
template <int NB>
__device__ __forceinline__ void nb_insert(double (&ls)[NB], uint64_t (&lc)[NB], double cs, uint64_t cc, int n) {
  uint64_t own = cc;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const double os = ls[i];
    const uint64_t oc = lc[i];
    const bool better = cs > os || (cs == os && cc < oc);
    const bool dup = oc == own;  // (own == 0: a dead candidate or a finished one; it matches empty slots, harmlessly)
    const bool take = better && i < n;
    ls[i] = take ? cs : os;
    lc[i] = take ? cc : oc;
    cs = dup ? neg_inf() : (take ? os : cs);
    cc = dup ? 0 : (take ? oc : cc);
    own = dup ? 0 : own;
  }
}

template <int NB>
__device__ __forceinline__ void nb_clear(double (&ls)[NB], uint64_t (&lc)[NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    ls[i] = neg_inf();
    lc[i] = 0;
  }
}

template <int RL, int SP, int NB>
__global__ __launch_bounds__(kXBlock) void connected_nbest_kernel(
    const double *__restrict__ logb, const int64_t *__restrict__ offsets, int64_t n_utts, int64_t total_frames,
    const double *__restrict__ log_start, const double *__restrict__ log_trans, const double *__restrict__ log_exit,
    const double *__restrict__ lm, const double *__restrict__ lm_start, const double *__restrict__ lm_end, int32_t W,
    int32_t S, int32_t n_best, uint64_t limit, double *__restrict__ score, uint64_t *__restrict__ code,
    int32_t *__restrict__ n_found, uint8_t *__restrict__ overflow) {
  constexpr int RP = kWave * RL;  // flat states the lanes hold (R <= RP)
  extern __shared__ double smem[];
  double *tab = smem;             // [SP][RP] by source
  const int R = W * SP;
  const int LS = x_lm_stride(W);
  double *lmt = tab + SP * RP;    // [W][LS]: lmt[w][v] = lm[v][w]
  double *lme = lmt + W * LS;     // [W]
  const int nthreads = blockDim.x;
  x_load_by_source(tab, log_trans, W, S, SP, RP, nthreads);
  x_load_lm(lmt, lme, lm, lm_end, W, true, nthreads);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  double *cs = lme + W + wave * nb_wave_words(RL, NB);          // [NB][RP]: the lists + log_exit, rank-major
  uint64_t *cc = reinterpret_cast<uint64_t *>(cs + NB * RP);    // [NB][RP]
  double *xs = reinterpret_cast<double *>(cc + NB * RP);        // [NB][64]: X(v)
  uint64_t *xc = reinterpret_cast<uint64_t *>(xs + NB * kWave);
  double *ns = reinterpret_cast<double *>(xc + NB * kWave);     // [NB][64]: N(w)
  uint64_t *nc = reinterpret_cast<uint64_t *>(ns + NB * kWave);
  const int64_t u = static_cast<int64_t>(blockIdx.x) * (nthreads / kWave) + wave;
  if (u >= n_utts) return;  // (after the only barrier; a whole wavefront leaves)
  const XFrames fr = x_frames(offsets, total_frames, u);
  const int64_t beg = fr.beg, T = fr.T;
  const uint64_t B = static_cast<uint64_t>(W) + 1;

  double ls[RL], lx[RL], bn[RL];
  double hs[RL][NB];    // the lane's lists: cell_t(w, s) of its RL flat states
  uint64_t hc[RL][NB];
  int sk[RL], wk[RL];
  bool ok[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const XState x = x_flat_state(k * kWave + lane, R, SP, S, log_start, log_exit);
    ok[k] = x.ok;
    sk[k] = x.s;
    wk[k] = x.w;
    ls[k] = x.ls;
    lx[k] = x.lx;
    nb_clear<NB>(hs[k], hc[k]);
  }
  const uint64_t dmask = x_mask_by_source<RL>(tab, sk, lane, SP);
  unsigned xmask = 0;  // bit s: some word can be left from state s
#pragma unroll 1
  for (int s = 0; s < SP; ++s) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < RL; ++k) any |= sk[k] == s && !(lx[k] == neg_inf());
    if (__ballot(any)) xmask |= 1u << s;
  }
  xmask = __builtin_amdgcn_readfirstlane(xmask);
  bool ovf = false;

  const double *__restrict__ brow = logb + beg * R;
#pragma unroll
  for (int k = 0; k < RL; ++k) bn[k] = (ok[k] && T > 0) ? brow[k * kWave + lane] : neg_inf();

  for (int64_t t = 0; t < T; ++t) {
    double b[RL];
#pragma unroll
    for (int k = 0; k < RL; ++k) b[k] = bn[k];
    {  // the next frame's row in flight under this frame's chain
      const int64_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
      for (int k = 0; k < RL; ++k) bn[k] = ok[k] ? brow[tn * R + k * kWave + lane] : neg_inf();
    }
    double qs[RL][NB];  // the new lists
    uint64_t qc[RL][NB];
#pragma unroll
    for (int k = 0; k < RL; ++k) nb_clear<NB>(qs[k], qc[k]);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < RL; ++k)
        nb_insert<NB>(qs[k], qc[k], lm_start[wk[k]] + ls[k], static_cast<uint64_t>(wk[k]) + 1, n_best);
    } else {
#pragma unroll 1
      for (int d = SP - 1; d > -SP; --d) {
        if (!x_live(dmask, d, SP)) continue;  // (uniform)
        double lt[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) {
          const int i = sk[k] - d;
          const bool in = i >= 0 && i < SP;  // (outside the word: no such predecessor)
          const double v = tab[(in ? i : 0) * RP + k * kWave + lane];
          lt[k] = in ? v : neg_inf();
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          if (n >= n_best) break;  // (uniform)
          double col[RL], rs[RL];
          uint64_t ccol[RL], rc[RL];
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            col[k] = hs[k][n];
            ccol[k] = hc[k][n];
          }
          x_rotate<RL>(col, lane, d, [&rs](int k, double prev) { rs[k] = prev; });
          nb_rotate_code<RL>(ccol, lane, d, rc);
#pragma unroll
          for (int k = 0; k < RL; ++k) nb_insert<NB>(qs[k], qc[k], rs[k] + lt[k], rc[k], n_best);
        }
      }
#pragma unroll 1
      for (int n = 0; n < n_best; ++n) {  // the entry: N_{t-1} of the lane's words + log_start
#pragma unroll
        for (int k = 0; k < RL; ++k)
          nb_insert<NB>(qs[k], qc[k], ns[n * kWave + wk[k]] + ls[k], nc[n * kWave + wk[k]], n_best);
      }
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        hs[k][n] = qs[k][n] + b[k];  // (the cell: as it is after + b, no re-sort and no drop)
        hc[k][n] = qc[k][n];
        if (ok[k] && n < n_best) {
          cs[n * RP + k * kWave + lane] = hs[k][n] + lx[k];
          cc[n * RP + k * kWave + lane] = hc[k][n];
        }
      }
    }
    wave_lds_sync();
    if (lane < W) {  // X(v): the lists of the word's states merged, two states may carry one string
      double ms[NB];
      uint64_t mc[NB];
      nb_clear<NB>(ms, mc);
#pragma unroll 1
      for (int s = 0; s < SP; ++s) {
        if (!((xmask >> s) & 1u)) continue;  // (uniform)
#pragma unroll 1
        for (int n = 0; n < n_best; ++n)
          nb_insert<NB>(ms, mc, cs[n * RP + lane * SP + s], cc[n * RP + lane * SP + s], n_best);
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        xs[n * kWave + lane] = ms[n];
        xc[n * kWave + lane] = mc[n];
      }
    }
    wave_lds_sync();
    if (t + 1 < T) {  // (uniform) N(w): the predecessor words merged, the word appended; codes differ by construction
      if (lane < W) {
        double ms[NB];
        uint64_t mc[NB];
        nb_clear<NB>(ms, mc);
        const uint64_t own = static_cast<uint64_t>(lane) + 1;
#pragma unroll 1
        for (int v = 0; v < W; ++v) {
          const double l = lmt[lane * LS + v];
#pragma unroll 1
          for (int n = 0; n < n_best; ++n) {
            const double c = xs[n * kWave + v] + l;
            const uint64_t pc = xc[n * kWave + v];
            const bool fits = pc < limit;
            ovf |= c > neg_inf() && !fits;
            nb_insert<NB>(ms, mc, fits ? c : neg_inf(), (fits ? pc : 0) * B + own, n_best);
          }
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          ns[n * kWave + lane] = ms[n];
          nc[n * kWave + lane] = mc[n];
        }
      }
      wave_lds_sync();
    }
  }
  const bool any_ovf = __ballot(ovf) != 0;
  if (lane == 0) {  // the result: X_{T-1}(v) + lm_end[v] merged over the words
    double ms[NB];
    uint64_t mc[NB];
    nb_clear<NB>(ms, mc);
    if (T > 0) {
#pragma unroll 1
      for (int v = 0; v < W; ++v) {
#pragma unroll 1
        for (int n = 0; n < n_best; ++n) nb_insert<NB>(ms, mc, xs[n * kWave + v] + lme[v], xc[n * kWave + v], n_best);
      }
    }
    int found = 0;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if (n < n_best) {
        score[u * n_best + n] = ms[n];
        code[u * n_best + n] = mc[n];
        found += mc[n] != 0;
      }
    }
    if (n_found) n_found[u] = found;
    if (overflow) overflow[u] = any_ovf ? 1 : 0;
  }
}

struct NbArgs {
  const double *logb;
  const int64_t *offsets;
  int64_t n_utts, total_frames;
  const double *log_start, *log_trans, *log_exit, *lm, *lm_start, *lm_end;
  int32_t W, S, n_best;
  uint64_t limit;
  double *score;
  uint64_t *code;
  int32_t *n_found;
  uint8_t *overflow;
};

template <int RL, int SP, int NB>
int launch_nbest(const NbArgs &a, hipStream_t stream) {
  size_t lds = 0;
  const int waves = x_waves(nb_shared_words(a.W, SP, RL) * sizeof(double), nb_wave_words(RL, NB) * sizeof(double), &lds);
  if (lds > static_cast<size_t>(kXLdsMax))
    return fail(SAPR_ERR_UNSUPPORTED, "the N-best kernel needs %zu bytes of LDS, the device offers %d", lds, kXLdsMax);
  const int64_t blocks = (a.n_utts + waves - 1) / waves;
  return x_launch(connected_nbest_kernel<RL, SP, NB>, blocks, waves * kWave, lds, stream, a.logb, a.offsets, a.n_utts,
                  a.total_frames, a.log_start, a.log_trans, a.log_exit, a.lm, a.lm_start, a.lm_end, a.W, a.S, a.n_best,
                  a.limit, a.score, a.code, a.n_found, a.overflow);
}

template <int RL, int SP>
int launch_nbest_nb(const NbArgs &a, hipStream_t stream) {
  if (a.n_best <= 2) return launch_nbest<RL, SP, 2>(a, stream);  // (n_best = 1 runs in two slots)
  if (a.n_best <= 4) return launch_nbest<RL, SP, 4>(a, stream);
  return launch_nbest<RL, SP, 8>(a, stream);
}

// cap(W): the largest K with (W + 1)^K <= 2^64; *limit = (W + 1)^(K - 1), the codes from which no word can be appended
inline int nb_capacity(int32_t W, uint64_t *limit) {
  const unsigned __int128 top = static_cast<unsigned __int128>(1) << 64;
  const unsigned __int128 B = static_cast<unsigned __int128>(W) + 1;
  unsigned __int128 p = 1;
  int K = 0;
  uint64_t last = 1;
  while (p * B <= top) {
    last = static_cast<uint64_t>(p);
    p *= B;
    ++K;
  }
  *limit = last;
  return K;
}

}  // namespace
}  // namespace sapr

using namespace sapr;

extern "C" int sapr_connected_nbest_capacity(int32_t W, int32_t *max_words) {
  SAPR_REQUIRE(W > 0 && max_words, "bad sizes (W=%d) or NULL max_words", W);
  uint64_t limit = 0;
  *max_words = nb_capacity(W, &limit);
  return 0;
}

extern "C" int sapr_connected_nbest(const double *logb, const int64_t *offsets, int64_t n_utts, int64_t total_frames,
                                    const double *log_start, const double *log_trans, const double *log_exit,
                                    const double *lm, const double *lm_start, const double *lm_end, int32_t W,
                                    int32_t S, int32_t n_best, double *score, uint64_t *code, int32_t *n_found,
                                    uint8_t *overflow, void *stream) {
  SAPR_REQUIRE(n_utts >= 0 && total_frames >= 0 && W > 0 && S > 0,
               "bad sizes (n_utts=%lld total_frames=%lld W=%d S=%d)", (long long)n_utts, (long long)total_frames, W, S);
  if (int rc = x_check_shape(W, S)) return rc;
  if (n_best < 1 || n_best > kNbMax)
    return fail(SAPR_ERR_UNSUPPORTED, "the N-best kernel serves n_best in 1..%d; got %d", kNbMax, n_best);
  SAPR_REQUIRE(lm && lm_start && lm_end, "NULL language model (lm, lm_start, lm_end)");
  SAPR_REQUIRE(n_utts <= 0x7fffffffLL, "grid too large (%lld utterances)", (long long)n_utts);
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(offsets && log_start && log_trans && log_exit && score && code && (total_frames == 0 || logb),
               "NULL pointer argument");
  const int32_t SP = sp_of(S);
  const int32_t R = W * SP;
  NbArgs a{logb, offsets,  n_utts, total_frames, log_start, log_trans, log_exit, lm,       lm_start,
           lm_end, W,      S,      n_best,       0,         score,     code,     n_found,  overflow};
  nb_capacity(W, &a.limit);
  hipStream_t st = as_stream(stream);
  return x_dispatch(SP, R, [&](auto rl, auto sp) {
    return launch_nbest_nb<decltype(rl)::value, decltype(sp)::value>(a, st);
  });
}
