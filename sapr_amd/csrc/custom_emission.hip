// The from-scratch HMM's emission log-densities (assignment2/custom_hmm.py:146-174) in the reference's own evaluation
// order, bit for bit: what decode and the per-method API read.  CPU restatement: oracle/custom_hmm_oracle.py.
//
//   custom_emission_bcast_kernel<13 | 39>   one row per lane, the differences shared over the 16 lanes of a DPP row
//   custom_emission_exact_kernel            one row per thread, run-time width: every other D, and both of the
//                                           above widths under SAPR_CUSTOM_EMISSION_ROWS1=1 (the tests' reference)
// sapr_custom_emission_exact picks by D and that switch; both kernels write the same bits.
#include <cstdlib>
#include <type_traits>

#include "sapr_common.h"

namespace sapr {
namespace {

#include "custom_np.h"

// ---- evaluation-order-faithful emission ---------------------------------------------------------------
// custom_hmm.py:168-172 evaluates  np.sum(diff.T @ inv_cov @ diff, axis=1):  two BLAS products and a numpy
// row sum.  On the build the golden vectors were taken from (numpy 2.2 / OpenBLAS 0.3.29 SkylakeX) every
// element of both products is ONE fused-multiply-add chain over the contraction index in increasing order,
// starting from 0 — checked bit for bit against the reference's emission matrices in
// tests/test_oracle_custom.py — and np.sum over the contiguous rows of the (T,T) Gram matrix is numpy's
// pair-wise sum.  This kernel performs exactly those operations:
//     M1[t][c] = fma-chain_k diff[k][t] * inv[k][c]          (diff.T @ inv_cov)
//     G[t][s]  = fma-chain_k M1[t][k]  * diff[k][s]          ((...) @ diff)
//     E[t][j]  = -0.5 * ((D log 2pi + logdet) + pairwise_s G[t][s])
// so that decisions that hang on the last bit (flat-start ties in decode) come out as in the reference.
// One thread owns one row (model w, state j, frame t); a workgroup owns one utterance, so the feature
// addresses inside the s / k loops are wavefront-uniform.  Cost O(rows * T * D) per state: decode needs the
// first Tq = D rows only (custom_hmm.py:466), the per-method API all T.
// A leaf of the pair-wise sum holds at most 128 frames; the workgroup stages them in LDS as float64
// (numpy promotes the float32 features before the subtraction) and every thread walks them in lockstep.
constexpr int kLeaf = 128;

struct ExactRow {
  double mu[kMaxD], m1[kMaxD];
  int D;

  // G[t][s0 .. s0+N) of the staged frames (xd[k][kLeaf], feature k of frame s at xd[k * kLeaf + s]): N
  // independent chains, each a fused-multiply-add chain over k in increasing order
  template <int N>
  __device__ __forceinline__ void gram(const double *xd, int s0, double (&g)[N]) const {
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxD; ++k)
      if (k < D) {
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = fma(m1[k], xd[k * kLeaf + s0 + j] - mu[k], g[j]);
      }
  }
  // numpy DOUBLE_pairwise_sum over the n <= 128 staged frames
  __device__ __forceinline__ double leaf(const double *xd, int n) const {
    double g[8];
    if (n < 8) {
      double res = 0.0;
      for (int i = 0; i < n; ++i) {
        double g1[1];
        gram<1>(xd, i, g1);
        res += g1[0];
      }
      return res;
    }
    double r[8];
    gram<8>(xd, 0, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = g[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
      gram<8>(xd, i, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += g[j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    if (i < n) {
      // the n % 8 trailing frames as one more block of eight: the columns behind frame n - 1 hold whatever the
      // previous leaf left there (the array has kLeaf columns and i + 8 <= kLeaf), their chains are discarded
      gram<8>(xd, i, g);
#pragma unroll
      for (int j = 0; j < 7; ++j)
        if (i + j < n) res += g[j];
    }
    return res;
  }
};

// grid.x = utterance, grid.y = chunk of 256 rows.
// n_rows > 0: E[((u * W + w) * n_rows + t) * S + j] for t < n_rows (decode: n_rows = Tq <= T);
// n_rows == 0: every frame, E[(offsets[u] + t) * S + j] (W must be 1: the per-method API).
__global__ __launch_bounds__(256, 2) void custom_emission_exact_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, int W, int D, int S, int n_rows,
    CustomPack P, double *__restrict__ E) {
  extern __shared__ double xd[];  // [D][kLeaf]: feature k of the leaf's frame s at xd[k * kLeaf + s]
  const int64_t u = blockIdx.x;
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  const int rows = n_rows ? n_rows : T;
  const int n_emit = S - 2;
  const int tasks = W * n_emit * rows;
  if (static_cast<int64_t>(blockIdx.y) * 256 >= tasks) return;  // whole workgroup: no barrier is skipped
  const float *xu = feats + beg * D;
  const int task = blockIdx.y * 256 + threadIdx.x;
  const bool live = task < tasks;
  const int t = live ? task % rows : 0;
  const int wj = live ? task / rows : 0;
  const int j = 1 + wj % n_emit, w = wj / n_emit;
  // decode asks for the first n_rows = D rows of every utterance (custom_hmm.py:466); an utterance SHORTER than that
  // (the Python mirror raises the reference's IndexError first, a C-ABI caller may not) must not read its neighbour's
  // frames: rows t >= T re-read a valid frame and are written as -inf
  const bool inside = t < T;
  const int tr = inside ? t : (T > 0 ? T - 1 : 0);
  ExactRow R;
  R.D = D;
  {
    const double *mu = P.means + (static_cast<int64_t>(w) * S + j) * D;
    const double *iv = P.inv + (static_cast<int64_t>(w) * S + j) * D * D;
    double drow[kMaxD];
#pragma unroll
    for (int k = 0; k < kMaxD; ++k)
      if (k < D) {
        R.mu[k] = mu[k];
        drow[k] = (T > 0 ? static_cast<double>(xu[static_cast<int64_t>(tr) * D + k]) : 0.0) - R.mu[k];
      }
#pragma unroll
    for (int c = 0; c < kMaxD; ++c)
      if (c < D) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kMaxD; ++k)
          if (k < D) acc = fma(drow[k], iv[k * D + c], acc);
        R.m1[c] = acc;
      }
  }
  // numpy's recursive halving above 128 terms as an explicit post-order walk; T is the same for every
  // thread of the workgroup, so the walk (and its barriers) is uniform.  (bcast_rows_walk below is the same walk:
  // shared as one template over the leaf, the register allocation of both kernels moved — DESIGN 4.4.)
  constexpr int kDepth = 24;
  int st_s[kDepth], st_n[kDepth], st_ph[kDepth];
  double val[kDepth];
  int top = 1, vtop = 0;
  st_s[0] = 0;
  st_n[0] = T;
  st_ph[0] = 0;
  while (top > 0) {
    const int i = top - 1;
    if (st_n[i] <= kLeaf) {
      const int n = st_n[i];
      const float *src = xu + static_cast<int64_t>(st_s[i]) * D;
      __syncthreads();  // the previous leaf has been consumed
      for (int e = threadIdx.x; e < n * D; e += 256) {
        const int k = e / n, fs = e - k * n;
        xd[k * kLeaf + fs] = static_cast<double>(src[fs * D + k]);
      }
      __syncthreads();
      val[vtop++] = R.leaf(xd, n);
      --top;
      continue;
    }
    int n2 = st_n[i] / 2;
    n2 -= n2 % 8;
    if (st_ph[i] == 0) {
      st_ph[i] = 1;
      st_s[top] = st_s[i];
      st_n[top] = n2;
      st_ph[top] = 0;
      ++top;
    } else if (st_ph[i] == 1) {
      st_ph[i] = 2;
      st_s[top] = st_s[i] + n2;
      st_n[top] = st_n[i] - n2;
      st_ph[top] = 0;
      ++top;
    } else {
      val[vtop - 2] = val[vtop - 2] + val[vtop - 1];
      --vtop;
      --top;
    }
  }
  if (!live) return;
  const double e = inside ? -0.5 * (P.cterm[static_cast<int64_t>(w) * S + j] + val[0]) : neg_inf();
  double *row = n_rows ? E + ((u * W + w) * static_cast<int64_t>(n_rows) + t) * S : E + (beg + t) * S;
  row[j] = e;
  if (j == 1) {  // the non-emitting columns of this row
    row[0] = neg_inf();
    row[S - 1] = neg_inf();
  }
}

// ---- the same rows, one per lane, differences shared across the 16 lanes of a DPP row (13 dimensions) ------------
// The difference x[k][s] - mu[k] belongs to the (word, state), not to the row: with the 13 (decode) or 16 (all-frames
// mode) rows of one (word, state) on the 16 lanes of a DPP row, lane k computes the eight differences of dimension k
// for a numpy block ONCE and every lane takes them as the broadcast operand of its multiply-add
//     v_fmac_f64_dpp g[f], d[f] row_newbcast:k, m1[k]        (full rate on this chip: scripts/ubench/mix_rate)
// — per row and block 104 multiply-adds + 8 subtractions + 8 running-sum additions (two rows per thread: 164) and 8
// LDS reads (130).  a * b + c is the same fused operation whichever factor comes first, the chains run over k in
// increasing order from 0: the bits are those of ExactRow.  M1 shares the inverse covariance the same way (lane c loads
// inv[k][c], 13 loads per lane instead of 169).
constexpr int kRowStride = kLeaf + 1;  // staged frames xd[k][kRowStride]: dimension k + 1 starts two banks further

template <int L>
__device__ __forceinline__ void fmac8_bcast(double (&g)[8], const double (&d)[8], double m) {
  // s_nop: a DPP operand written by the preceding VALU instruction needs two wait states
  asm volatile(
      "s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %8, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %9, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %2, %10, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %3, %11, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %4, %12, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %5, %13, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %6, %14, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %7, %15, %16 row_newbcast:%17 row_mask:0xf bank_mask:0xf"
      : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(g[4]), "+v"(g[5]), "+v"(g[6]), "+v"(g[7])
      : "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]), "v"(d[4]), "v"(d[5]), "v"(d[6]), "v"(d[7]), "v"(m), "n"(L));
}
// acc += (src of lane L of the row) * m
template <int L>
__device__ __forceinline__ void fmac_bcast(double &acc, double src, double m) {
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(m), "n"(L));
}
template <int L>
__device__ __forceinline__ double mov_bcast(double src) {
  double r;
  asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(src), "n"(L));
  return r;
}

// D = 13: the 13 dimensions on lanes 0..12 of the row.  D = 39: lane l computes dimensions l, l + 16 and l + 32 (three
// difference arrays; dimension k is read from lane k % 16, array k / 16), 16 of the 39 rows per DPP row.
template <int DD>
struct ExactRowBcast {
  static constexpr int kD = DD;
  static constexpr int kNL = (DD + 15) / 16;  // dimensions per lane
  double m1[kD];
  double mu_own[kNL];  // mean of dimension min((lane & 15) + 16 q, D - 1) of this row's (word, state)
  int x_own[kNL];      // index of that dimension's staged frames: dimension * kRowStride

  template <int K>
  __device__ __forceinline__ void chain(double (&g)[8], const double (&d)[kNL][8]) const {
    fmac8_bcast<K % 16>(g, d[K / 16], m1[K]);
    if constexpr (K + 1 < kD) chain<K + 1>(g, d);
  }
  // G[t][s0 .. s0 + 8) of the staged frames
  __device__ __forceinline__ void block(const double *xd, int s0, double (&g)[8]) const {
    double d[kNL][8];
#pragma unroll
    for (int q = 0; q < kNL; ++q) {
#pragma unroll
      for (int f = 0; f < 8; ++f) d[q][f] = xd[x_own[q] + s0 + f] - mu_own[q];
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) g[f] = 0.0;
    chain<0>(g, d);
  }
  template <int K>
  __device__ __forceinline__ void chain1(double &g, const double *xd, int i) const {
    const double mu_k = mov_bcast<K % 16>(mu_own[K / 16]);
    g = fma(m1[K], xd[K * kRowStride + i] - mu_k, g);
    if constexpr (K + 1 < kD) chain1<K + 1>(g, xd, i);
  }
  // numpy DOUBLE_pairwise_sum over the n <= 128 staged frames
  __device__ __forceinline__ double leaf(const double *xd, int n) const {
    if (n < 8) {
      double res = 0.0;
      for (int i = 0; i < n; ++i) {
        double g = 0.0;
        chain1<0>(g, xd, i);
        res += g;
      }
      return res;
    }
    double r[8], g[8];
    block(xd, 0, r);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
      block(xd, i, g);
#pragma unroll
      for (int f = 0; f < 8; ++f) r[f] += g[f];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    if (i < n) {
      // the n % 8 trailing frames as one more block of eight: the columns behind frame n - 1 hold whatever was
      // staged there before (a row has kRowStride columns and i + 8 <= kLeaf), their chains are discarded
      block(xd, i, g);
#pragma unroll
      for (int f = 0; f < 7; ++f)
        if (i + f < n) res += g[f];
    }
    return res;
  }
  // M1[c] += da * inv[k][c] for every column c: lane c % 16 of the row holds inv[k][c] in iv_k[c / 16]
  template <int C>
  __device__ __forceinline__ void m1_row(const double (&iv_k)[kNL], double da) {
    fmac_bcast<C % 16>(m1[C], iv_k[C / 16], da);
    if constexpr (C + 1 < kD) m1_row<C + 1>(iv_k, da);
  }
};

template <int DD>
__device__ __forceinline__ void bcast_stage_leaf(double *xd, const float *src, int n) {
  for (int fs = threadIdx.x; fs < n; fs += blockDim.x) {
#pragma unroll
    for (int k = 0; k < DD; ++k) xd[k * kRowStride + fs] = static_cast<double>(src[fs * DD + k]);
  }
}

// numpy's recursive halving above 128 terms as an explicit post-order walk, every leaf staged in turn; T is the same
// for every thread of the workgroup, so the walk (and its barriers) is uniform.  (Its own function: inlined, its
// scratch arrays and the second copy of the leaf cost the one-leaf path its registers.)
template <int DD>
__device__ __noinline__ double bcast_rows_walk(const ExactRowBcast<DD> &R, double *xd, const float *xu, int T) {
  constexpr int kDepth = 24;
  int st_s[kDepth], st_n[kDepth], st_ph[kDepth];
  double val[kDepth];
  int top = 1, vtop = 0;
  st_s[0] = 0;
  st_n[0] = T;
  st_ph[0] = 0;
  while (top > 0) {
    const int i = top - 1;
    if (st_n[i] <= kLeaf) {
      __syncthreads();  // the previous leaf has been consumed
      bcast_stage_leaf<DD>(xd, xu + static_cast<int64_t>(st_s[i]) * DD, st_n[i]);
      __syncthreads();
      val[vtop++] = R.leaf(xd, st_n[i]);
      --top;
      continue;
    }
    int n2 = st_n[i] / 2;
    n2 -= n2 % 8;
    if (st_ph[i] == 0) {
      st_ph[i] = 1;
      st_s[top] = st_s[i];
      st_n[top] = n2;
      st_ph[top] = 0;
      ++top;
    } else if (st_ph[i] == 1) {
      st_ph[i] = 2;
      st_s[top] = st_s[i] + n2;
      st_n[top] = st_n[i] - n2;
      st_ph[top] = 0;
      ++top;
    } else {
      val[vtop - 2] = val[vtop - 2] + val[vtop - 1];
      --vtop;
      --top;
    }
  }
  return val[0];
}

// One workgroup per utterance.  A group = the 16 lanes of a DPP row = rows 16 q .. 16 q + 15 of one (word w, state j):
// group (w * n_emit + j - 1) * ceil(rows / 16) + q; the workgroup walks the groups blockDim / 16 at a time.  An
// utterance of at most kLeaf frames (one leaf) is staged once for all of them.  Outputs as custom_emission_exact_kernel.
// Every lane stays active through the arithmetic (a broadcast reads its source lane whatever that lane's own row is
// worth): lanes without a row work on a clamped copy and do not store.
// 13 dimensions: 128 threads, four wavefronts per SIMD; 39: 256 threads (40 KB of staged frames), two per SIMD.
template <int DD>
__global__ __launch_bounds__(DD > 16 ? 256 : 128, DD > 16 ? 2 : 4) void custom_emission_bcast_kernel(
    const float *__restrict__ feats, const int64_t *__restrict__ offsets, int W, int S, int n_rows, CustomPack P,
    double *__restrict__ E) {
  using Row = ExactRowBcast<DD>;
  constexpr int Dn = DD, NL = Row::kNL;
  __shared__ double xd[Dn * kRowStride];
  const int64_t u = blockIdx.x;
  const int64_t beg = offsets[u];
  const int T = static_cast<int>(offsets[u + 1] - beg);
  const int rows = n_rows ? n_rows : T;
  const int rgs = (rows + 15) / 16;
  const int n_emit = S - 2;
  const int n_groups = W * n_emit * rgs;
  const float *xu = feats + beg * Dn;
  const bool single = T <= kLeaf;
  if (single) {
    bcast_stage_leaf<DD>(xd, xu, T);
    __syncthreads();
  }
  const int l16 = threadIdx.x & 15;
  const int groups_per_pass = static_cast<int>(blockDim.x) / 16;
  for (int base = 0; base < n_groups; base += groups_per_pass) {
    const int gi = base + (threadIdx.x >> 4);
    const bool live_g = gi < n_groups;
    const int gc = live_g ? gi : n_groups - 1;
    const int pr = gc / rgs, t = (gc - pr * rgs) * 16 + l16;
    const int j = 1 + pr % n_emit, w = pr / n_emit;
    const bool live = live_g && t < rows;
    // rows t >= T (an utterance shorter than the n_rows decode asks for) re-read a valid frame and are written as -inf
    const bool inside = t < T;
    const int tr = inside ? t : (T > 0 ? T - 1 : 0);
    Row R;
    const double *mu_g = P.means + (static_cast<int64_t>(w) * S + j) * Dn;
    const double *iv = P.inv + (static_cast<int64_t>(w) * S + j) * Dn * Dn;
    int lk[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      lk[q] = min(l16 + 16 * q, Dn - 1);
      R.mu_own[q] = mu_g[lk[q]];
      R.x_own[q] = lk[q] * kRowStride;
    }
#pragma unroll
    for (int c = 0; c < Dn; ++c) R.m1[c] = 0.0;
    // M1[c] = chain_k (x[tr][k] - mu[k]) inv[k][c]: row k of the inverse covariance sits on the lanes of the DPP row
    if constexpr (Dn <= 16) {
      double ivk[Dn], x[Dn];
#pragma unroll
      for (int k = 0; k < Dn; ++k) {
        ivk[k] = iv[k * Dn + lk[0]];
        x[k] = T <= 0 ? 0.0 : single ? xd[k * kRowStride + tr] : static_cast<double>(xu[static_cast<int64_t>(tr) * Dn + k]);
      }
      static_for_c<0, Dn>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const double da = x[k] - mov_bcast<k>(R.mu_own[0]);
        const double row[1] = {ivk[k]};
        R.template m1_row<0>(row, da);
      });
    } else {
      // (rolled: 39 x 3 loads would not stay in registers; the next row is in flight while this one is consumed)
      double row[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) row[q] = iv[lk[q]];
#pragma unroll 1
      for (int k = 0; k < Dn; ++k) {
        double nrow[NL];
        const double *nx = iv + min(k + 1, Dn - 1) * Dn;
#pragma unroll
        for (int q = 0; q < NL; ++q) nrow[q] = nx[lk[q]];
        const double xk = T <= 0 ? 0.0 : single ? xd[k * kRowStride + tr] : static_cast<double>(xu[static_cast<int64_t>(tr) * Dn + k]);
        const double da = xk - mu_g[k];
        R.template m1_row<0>(row, da);
#pragma unroll
        for (int q = 0; q < NL; ++q) row[q] = nrow[q];
      }
    }
    double res;
    if (single) {
      res = R.leaf(xd, T);
    } else {
      const Row Rc = R;
      res = bcast_rows_walk<DD>(Rc, xd, xu, T);
    }
    if (live) {
      const double e = inside ? -0.5 * (P.cterm[static_cast<int64_t>(w) * S + j] + res) : neg_inf();
      double *row = n_rows ? E + ((u * W + w) * static_cast<int64_t>(n_rows) + t) * S : E + (beg + t) * S;
      row[j] = e;
      if (j == 1) {  // the non-emitting columns of this row
        row[0] = neg_inf();
        row[S - 1] = neg_inf();
      }
    }
  }
}

}  // namespace
}  // namespace sapr

using namespace sapr;

static void launch_emission_exact(hipStream_t st, const float *feats, const int64_t *offsets, int64_t n_utts, int W,
                                  int D, int S, int n_rows, int max_T, const CustomPack &P, double *E) {
  // grid.y covers the longest possible row list; workgroups past an utterance's own list exit at once
  const int64_t max_rows = n_rows ? n_rows : max_T;
  const int64_t chunks = (static_cast<int64_t>(W) * (S - 2) * max_rows + 255) / 256;
  SAPR_LAUNCH(custom_emission_exact_kernel, dim3(static_cast<unsigned>(n_utts), static_cast<unsigned>(chunks)),
              dim3(256), kLeaf * D * sizeof(double), st, feats, offsets, W, D, S, n_rows, P, E);
}

extern "C" int sapr_custom_emission_exact(const float *feats, const int64_t *offsets, int64_t n_utts, int32_t W,
                                          int32_t D, int32_t S, int32_t n_rows, int32_t max_T,
                                          const double *means, const double *inv, const double *cterm, double *E,
                                          void *stream) {
  if (int rc = check_dims(S, D)) return rc;
  SAPR_REQUIRE(n_utts >= 0 && W > 0 && n_rows >= 0 && max_T >= 0, "bad sizes");
  SAPR_REQUIRE(static_cast<int64_t>(W) * (S - 2) * (n_rows ? n_rows : max_T) <= 65535 * int64_t{256},
               "too many emission rows per utterance for one launch");
  SAPR_REQUIRE(n_rows > 0 || W == 1, "all-frames mode (n_rows == 0) takes one model");
  SAPR_REQUIRE(n_utts < (int64_t{1} << 31), "too many utterances for one launch");
  if (n_utts == 0) return 0;
  SAPR_REQUIRE(feats && offsets && means && inv && cterm && E, "NULL pointer argument");
  CustomPack P{means, inv, cterm, nullptr, nullptr};
  hipStream_t st = as_stream(stream);
  static const bool rows1 = [] {
    const char *e = std::getenv("SAPR_CUSTOM_EMISSION_ROWS1");
    return e && e[0] == '1';
  }();
  if ((D == 13 || D == 39) && !rows1) {
    // one row per lane, differences broadcast over the DPP row (custom_emission_bcast_kernel);
    // SAPR_CUSTOM_EMISSION_ROWS1=1 keeps the one-thread-per-row kernel
    if (D == 13)
      SAPR_LAUNCH(custom_emission_bcast_kernel<13>, dim3(static_cast<unsigned>(n_utts)), dim3(128), 0, st, feats,
                  offsets, W, S, n_rows, P, E);
    else
      SAPR_LAUNCH(custom_emission_bcast_kernel<39>, dim3(static_cast<unsigned>(n_utts)), dim3(256), 0, st, feats,
                  offsets, W, S, n_rows, P, E);
  } else {
    launch_emission_exact(st, feats, offsets, n_utts, W, D, S, n_rows, max_T, P, E);
  }
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
