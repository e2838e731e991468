// The lane layout behind the connected-word trellis units (connected.hip, connected_align.hip, connected_embed.hip,
// connected_bigram.hip, connected_loop_fb.hip, connected_levels.hip, connected_nbest.hip, connected_lattice.hip; DESIGN
// 4.3o).  Like lse_ops.h and gmm_ops.h this header is included INSIDE the unit's `namespace sapr { namespace {`, after
// both of them.  connected_loop_stats.hip has no recursion; it takes the constants and the host helpers
// from here.
//
// The mapping every recursion kernel of these units uses:
//   * One wavefront serves one utterance; a workgroup holds up to four of them, which share the tables in LDS.  The
//     frame loop has no workgroup barrier: the only __syncthreads() follows the table load.
//   * The utterance's trellis column lies along the lanes, RL in {1, 2, 4} items per lane: item r = k * 64 + lane sits
//     in register k of its lane.  An item is a flat state of the vocabulary, r = w * SP + s (x_flat_state: the word
//     loop and everything built on it), or a position of the transcript's word chain, p = q * SP + s with slot q
//     holding word words[q] (alignment and embedded Baum-Welch, whose kernels lay it out themselves).  A row of R or P values is RL
//     coalesced reads, and the next frame's row is in flight under the current frame's chain.
//   * The within-word neighbour at distance d = j - i of item r is item r - d (a predecessor, forward) or r + d (a
//     successor, backward): lane (lane -/+ d) & 63 of register k, or of k -/+ 1 where the lane index leaves 0..63
//     (x_rotate, one ds_bpermute per register).  d runs over -(SP - 1) .. SP - 1 — a dense model also steps back — but
//     only at the distances at which some transition of the vocabulary is finite (the distance mask, wavefront-uniform:
//     a bidiagonal vocabulary costs two candidates per state, a dense one 2 SP - 1).
//   * The transition table lies in LDS in one of three layouts (the header holds the loader and the distance mask of
//     the first and, for the embedded kernels, of the third; the other kernels keep their own):
//       by source     tab[i][r]                 = log_trans[w][i][s]   the Viterbi recursions over flat states
//       by diagonal   tab[(j - i) mod SP][r]    (r the flat state of j) forward reads it at r, backward at r + d
//       by word       tab[w][(j - i) mod SP][j] the chain units: every lane indexes it through its own word
//   * The coupling between words goes through per-wavefront LDS rows between wave_lds_sync's: every lane writes its
//     value to cbuf[r], lane q < n reduces the SP values of segment q (a word, or a slot of the chain) — the first
//     maximum (x_first_max) or the log-sum-exp (x_segment_lse) — and, under a word-pair language model, lane w reduces
//     the W values xbuf[v] + lm[v][w] (x_first_max_pair over a row of the transposed lm, rows of W | 1 doubles so that
//     W lanes read W different banks while xbuf[v] is a broadcast; pair_lse is the same step in the sum semiring).
// Which recursion step sits behind the rotation — max or lse2, what is stored, which workspace rows — is the unit's.

// ---- constants and host helpers ----------------------------------------------------------------------------------
constexpr int kXMaxR = 256;            // flat states, or chain positions, one wavefront holds
constexpr int kXBlock = 256;           // at most 4 wavefronts per workgroup
constexpr int kXWaves = kXBlock / kWave;
constexpr int kXEntry = 255;           // back-pointer byte: the word was entered at this frame
constexpr int kXLdsMax = 160 * 1024;   // LDS of one gfx950 compute unit

inline size_t x_align16(size_t x) { return (x + 15) / 16 * 16; }

constexpr int x_lm_stride(int W) { return W | 1; }  // doubles per row of lm in LDS

inline int x_check_shape(int32_t W, int32_t S) {
  if (S > kMaxS || static_cast<int64_t>(W) * sp_of(S) > kXMaxR)
    return fail(SAPR_ERR_UNSUPPORTED, "the connected-word kernels serve S in 1..%d and W * SP <= %d; got W=%d S=%d",
                kMaxS, kXMaxR, W, S);
  return 0;
}

// the chain units: the vocabulary's table and the chain's positions both fit one wavefront; what = "alignment", ...
inline int x_check_chain_shape(const char *what, int32_t W, int32_t S, int32_t max_words) {
  if (S > kMaxS || static_cast<int64_t>(W) * sp_of(S) > kXMaxR || static_cast<int64_t>(max_words) * sp_of(S) > kXMaxR)
    return fail(SAPR_ERR_UNSUPPORTED,
                "the %s kernels serve S in 1..%d, W * SP <= %d and max_words * SP <= %d; got W=%d S=%d max_words=%d "
                "(SP=%d)",
                what, kMaxS, kXMaxR, kXMaxR, W, S, max_words, sp_of(S));
  return 0;
}

// as many wavefronts per workgroup as the LDS holds next to the shared tables, at most four; *lds: the bytes to ask for
// (above kXLdsMax where not even one wavefront fits: the caller reports it)
inline int x_waves(size_t shared_bytes, size_t per_wave_bytes, size_t *lds) {
  int waves = kXWaves;
  while (waves > 1 && shared_bytes + waves * per_wave_bytes > static_cast<size_t>(kXLdsMax)) --waves;
  *lds = shared_bytes + waves * per_wave_bytes;
  return waves;
}

// launch with `lds` bytes of dynamic LDS.  Above 64 KB the attribute is raised first — per launch, not once: it
// belongs to the current device's copy of the kernel.
template <typename Kern, typename... Args>
int x_launch(Kern kern, int64_t blocks, int threads, size_t lds, hipStream_t stream, Args... args) {
  if (lds > 64 * 1024)
    SAPR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)));
  SAPR_LAUNCH(kern, dim3(static_cast<unsigned>(blocks)), dim3(static_cast<unsigned>(threads)), lds, stream, args...);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}

// f(integral_constant<int, RL>, integral_constant<int, SP>) for the unit's instantiation: SP in {4, 10, 18} as
// sp_of gives it, RL in {1, 2, 4} from the items (flat states or chain positions) a wavefront has to hold
template <typename F>
int x_dispatch(int SP, int items, F &&f) {
  const auto by_items = [&](auto sp) {
    if (items <= kWave) return f(std::integral_constant<int, 1>{}, sp);
    if (items <= 2 * kWave) return f(std::integral_constant<int, 2>{}, sp);
    return f(std::integral_constant<int, 4>{}, sp);
  };
  if (SP == 4) return by_items(std::integral_constant<int, 4>{});
  if (SP == 10) return by_items(std::integral_constant<int, 10>{});
  return by_items(std::integral_constant<int, 18>{});
}

// ---- device primitives ----------------------------------------------------------------------------------------------
// between the lanes of ONE wavefront: what the lanes wrote to LDS before is what they read after.  The hardware
// completes a wavefront's LDS operations in order; the fences keep the compiler from moving or caching across it.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool finite_f64(double v) { return v - v == 0.0; }

__device__ __forceinline__ uint64_t x_uniform64(uint64_t v) {  // the first lane's value, in scalar registers
  return (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32))) << 32) |
         __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
}

// the frames of utterance u; offsets that leave the batch are served as empty
struct XFrames {
  int64_t beg, T;
};

__device__ __forceinline__ XFrames x_frames(const int64_t *__restrict__ offsets, int64_t total_frames, int64_t u) {
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;
  return XFrames{beg, end - beg};
}

// the frames and the transcript of utterance u, and whether the chain can be laid out at all (the score or the
// likelihood decides the rest)
struct XUtt {
  int64_t beg, T, wbeg, n_words;  // n_words: the transcript's length, whether it can be laid out or not
  int K;                          // ... and the chain's slots: n_words where there is a path, else 0
  bool path;
};

__device__ __forceinline__ XUtt x_utt(const int64_t *__restrict__ offsets, int64_t total_frames,
                                      const int64_t *__restrict__ word_offsets, int64_t total_words,
                                      int32_t max_words, int64_t u) {
  XUtt r;
  int64_t beg = offsets[u], end = offsets[u + 1];
  if (beg < 0 || end < beg || end > total_frames) end = beg = 0;  // offsets that leave the batch: served as empty
  int64_t wbeg = word_offsets[u], wend = word_offsets[u + 1];
  if (wbeg < 0 || wend < wbeg || wend > total_words) wend = wbeg = 0;
  const int64_t K64 = wend - wbeg;
  r.beg = beg;
  r.T = end - beg;
  r.wbeg = wbeg;
  r.n_words = K64;
  r.path = r.T > 0 && K64 > 0 && K64 <= max_words;  // (max_words <= 64: a slot per lane in the coupling step)
  r.K = r.path ? static_cast<int>(K64) : 0;
  return r;
}

// flat state r = k * 64 + lane = w * SP + s, the item in register k of its lane.  ok: r < R; w is 0 for a lane without
// a state (a row of W values indexed by it is not left); real: not a padding state either; ls, lx: the state's
// log_start and log_exit, -inf unless real.  One call per register: the kernels keep ok[RL], sk[RL], ... of their own.
struct XState {
  bool ok, real;
  int s, w;
  double ls, lx;
};

__device__ __forceinline__ XState x_flat_state(int r, int R, int SP, int S, const double *__restrict__ log_start,
                                               const double *__restrict__ log_exit) {
  XState x;
  const int w = r / SP;  // (<= 255 / SP <= 63)
  x.s = r - w * SP;
  x.ok = r < R;
  x.w = x.ok ? w : 0;
  x.real = x.ok && x.s < S;
  x.ls = x.real ? log_start[w * S + x.s] : neg_inf();
  x.lx = x.real ? log_exit[w * S + x.s] : neg_inf();
  return x;
}

// use(k, value of item r - shift) for the lane's RL items r = k * 64 + lane, -inf where r - shift leaves
// 0 .. 64 RL - 1: lane (lane - shift) & 63 of register k, of k - 1 where lane < shift, of k + 1 where
// lane - shift >= 64.  The forward recursions pass shift = d (the predecessor), the backward ones shift = -d (the
// successor); |shift| < 64.  The callback captures what it reads by value and only the arrays it writes by reference,
// [=, &best, &back].
template <int RL, typename F>
__device__ __forceinline__ void x_rotate(const double (&val)[RL], int lane, int shift, F &&use) {
  const int off = lane - shift;
  const int src = off & (kWave - 1);
  double rot[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) rot[k] = __shfl(val[k], src, kWave);
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
    const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
    use(k, off < 0 ? below : (off >= kWave ? above : rot[k]));
  }
}

// x_rotate with an int32 beside every value (the lattice's start frame, which moves with delta): use(k, value, tag) of
// item r - shift; -inf and -1 where r - shift leaves 0 .. 64 RL - 1.  A second ds_bpermute per register.
template <int RL, typename F>
__device__ __forceinline__ void x_rotate_tagged(const double (&val)[RL], const int (&tag)[RL], int lane, int shift,
                                                F &&use) {
  const int off = lane - shift;
  const int src = off & (kWave - 1);
  double rot[RL];
  int rtag[RL];
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    rot[k] = __shfl(val[k], src, kWave);
    rtag[k] = __shfl(tag[k], src, kWave);
  }
#pragma unroll
  for (int k = 0; k < RL; ++k) {
    const double below = k > 0 ? rot[k > 0 ? k - 1 : 0] : neg_inf();
    const double above = k + 1 < RL ? rot[k + 1 < RL ? k + 1 : k] : neg_inf();
    const int tbelow = k > 0 ? rtag[k > 0 ? k - 1 : 0] : -1;
    const int tabove = k + 1 < RL ? rtag[k + 1 < RL ? k + 1 : k] : -1;
    use(k, off < 0 ? below : (off >= kWave ? above : rot[k]), off < 0 ? tbelow : (off >= kWave ? tabove : rtag[k]));
  }
}

// bit d + SP - 1 of a distance mask: some transition of the vocabulary at distance d = j - i is finite
__device__ __forceinline__ bool x_live(uint64_t dmask, int d, int SP) { return (dmask >> (d + SP - 1)) & 1ull; }

// ---- the table by source: tab[i][r] = log_trans[w][i][s], the transition INTO flat state r = w * SP + s from i ------
// (threads 0 .. nthreads - 1 of the workgroup; the caller's barrier follows)
__device__ __forceinline__ void x_load_by_source(double *tab, const double *__restrict__ log_trans, int W, int S,
                                                 int SP, int RP, int nthreads) {
  const int R = W * SP;
  for (int n = threadIdx.x; n < SP * RP; n += nthreads) {
    const int i = n / RP, r = n - i * RP;
    const int w = r / SP, s = r - w * SP;
    double v = neg_inf();
    if (r < R && s < S && i < S) v = log_trans[(static_cast<int64_t>(w) * S + i) * S + s];
    tab[n] = v;
  }
}

template <int RL>
__device__ __forceinline__ uint64_t x_mask_by_source(const double *tab, const int (&sk)[RL], int lane, int SP) {
  constexpr int RP = kWave * RL;
  uint64_t dmask = 0;
#pragma unroll 1
  for (int d = 1 - SP; d < SP; ++d) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
      const int i = sk[k] - d;
      const bool in = i >= 0 && i < SP;
      any |= in && !(tab[(in ? i : 0) * RP + k * kWave + lane] == neg_inf());
    }
    if (__ballot(any)) dmask |= 1ull << (d + SP - 1);
  }
  return x_uniform64(dmask);
}

// ---- the table by word: tab[w][dd][j] = log_trans[w][i][j] with i = (j - dd) mod SP; at one distance the SP lanes of
// a slot read SP consecutive doubles (all threads of the workgroup; followed by a barrier) ---------------------------
template <int SP>
__device__ __forceinline__ void x_load_by_word(double *tab, const double *__restrict__ log_trans, int W, int S) {
  const int n_tab = W * SP * SP;
  for (int n = threadIdx.x; n < n_tab; n += blockDim.x) {
    const int w = n / (SP * SP), rem = n - w * (SP * SP);
    const int dd = rem / SP, j = rem - dd * SP;
    const int i = j >= dd ? j - dd : j - dd + SP;
    tab[n] = (i < S && j < S) ? log_trans[(static_cast<int64_t>(w) * S + i) * S + j] : neg_inf();
  }
  __syncthreads();
}

// every wavefront reads the whole table, so the mask is the same in all of a workgroup's; *nan as above
template <int SP>
__device__ __forceinline__ uint64_t x_mask_by_word(const double *tab, int n_tab, int lane, bool *nan) {
  uint64_t dmask = 0;
  unsigned bad = 0;
  for (int n = lane; n < n_tab; n += kWave) {
    const int rem = n % (SP * SP);
    const int dd = rem / SP, j = rem - dd * SP;
    const int d = j >= dd ? dd : dd - SP;
    const double v = tab[n];
    if (!(v == neg_inf())) dmask |= 1ull << (d + SP - 1);
    if (v != v) bad = 1;
  }
  unsigned lo = static_cast<unsigned>(dmask), hi = static_cast<unsigned>(dmask >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo |= __shfl_xor(lo, o, kWave);
    hi |= __shfl_xor(hi, o, kWave);
    bad |= __shfl_xor(bad, o, kWave);
  }
  *nan = __builtin_amdgcn_readfirstlane(bad) != 0;
  return (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(hi)) << 32) | __builtin_amdgcn_readfirstlane(lo);
}

// ---- the language model: lmx[a][b] = lm[a][b], or lm[b][a] where transposed, in rows of W | 1 doubles; lme = lm_end
// (threads 0 .. nthreads - 1 of the workgroup; the caller's barrier follows)
__device__ __forceinline__ void x_load_lm(double *lmx, double *lme, const double *__restrict__ lm,
                                          const double *__restrict__ lm_end, int W, bool transposed, int nthreads) {
  const int LS = x_lm_stride(W);
  for (int n = threadIdx.x; n < W * W; n += nthreads) {  // (coalesced read of lm[a][b]; transposed: strided write)
    const int a = n / W, b = n - a * W;
    lmx[transposed ? b * LS + a : a * LS + b] = lm[n];
  }
  for (int n = threadIdx.x; n < W; n += nthreads) lme[n] = lm_end[n];
}

// ---- the coupling steps ---------------------------------------------------------------------------------------------
// the first maximum over the SP values seg[0 .. SP - 1] of one segment (a row of LDS), s ascending (strict compares);
// *arg: its place.  The values are read before the first compare: one LDS latency per call, not SP of them.
template <int SP>
__device__ __forceinline__ double x_first_max(const double *seg, int *arg) {
  double c[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) c[s] = seg[s];
  double xv = c[0];
  int xs = 0;
#pragma unroll
  for (int s = 1; s < SP; ++s) {
    const bool take = c[s] > xv;
    xv = take ? c[s] : xv;
    xs = take ? s : xs;
  }
  *arg = xs;
  return xv;
}

// the first maximum over p = 0 .. W - 1 of x[p] + row[p], p ascending (strict compares); *arg: its place
__device__ __forceinline__ double x_first_max_pair(const double *x, const double *row, int W, int *arg) {
  double nv = x[0] + row[0];
  int nw = 0;
#pragma unroll 4
  for (int p = 1; p < W; ++p) {
    const double c = x[p] + row[p];
    const bool take = c > nv;
    nv = take ? c : nv;
    nw = take ? p : nw;
  }
  *arg = nw;
  return nv;
}

// The segmented log-sum-exp: val[k] is the term of the lane's item in register k (in[k]: the item exists, seg[k]: its
// segment — the word of a flat state, the slot of a chain position); lane q < n returns the log-sum-exp over the SP
// terms of segment q — the operations of lse_all<SP> over them in its order (the first maximum by strict compares, the
// exponentials added s ascending, log(sum) + max; an infinite maximum is the result), but with the SP exponentials of
// a segment evaluated by the SP lanes that hold its items instead of by lane q alone: lse_all on n lanes costs the
// whole wavefront SP exponentials per frame, this costs RL.  Three hand-overs through the wavefront's own LDS rows
// cbuf[64 RL] and mbuf[64]; the caller synchronises before it writes cbuf again.
template <int RL, int SP>
__device__ __forceinline__ double x_segment_lse(double *cbuf, double *mbuf, const double (&val)[RL],
                                                const bool (&in)[RL], const int (&seg)[RL], int lane, int n) {
#pragma unroll
  for (int k = 0; k < RL; ++k)
    if (in[k]) cbuf[k * kWave + lane] = val[k];
  wave_lds_sync();
  double m = neg_inf();
  if (lane < n) {
    m = cbuf[lane * SP];
#pragma unroll
    for (int s = 1; s < SP; ++s) {
      const double v = cbuf[lane * SP + s];
      m = v > m ? v : m;
    }
    mbuf[lane] = m;
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < RL; ++k)
    if (in[k]) cbuf[k * kWave + lane] = exp_unit(val[k] - mbuf[seg[k]]);  // (an infinite maximum: selected away below)
  wave_lds_sync();
  double r = m;
  if (lane < n) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < SP; ++s) acc += cbuf[lane * SP + s];
    r = isinf(m) ? m : log(acc) + m;
  }
  return r;
}

// The W x W log-sum-exp against a table in LDS (the word loop's forward-backward and the lattice posteriors): lane
// q < W returns lse_p (mat[q][p] + xbuf[p]), p ascending, in the three steps connected_loop_fb.hip writes out — the
// row maxima, the W * W exponentials spread over the 64 lanes into ebuf[W][W | 1], the row sums.  xbuf[64] is
// synchronised by the caller; mbuf[64] and ebuf are free again when this returns.
__device__ __forceinline__ double pair_lse(const double *mat, const double *xbuf, double *mbuf, double *ebuf, int lane,
                                           int W, int LS) {
  double m = neg_inf();
  if (lane < W) {
    const double *__restrict__ row = mat + lane * LS;
    m = row[0] + xbuf[0];
#pragma unroll 4
    for (int p = 1; p < W; ++p) {
      const double c = row[p] + xbuf[p];
      m = c > m ? c : m;
    }
    mbuf[lane] = m;
  }
  wave_lds_sync();
  {
    const int q64 = kWave / W, r64 = kWave - q64 * W;  // item n + 64 from item n without a division
    int q = lane / W, p = lane - q * W;
    for (int n = lane; n < W * W; n += kWave) {
      ebuf[q * LS + p] = exp_unit((mat[q * LS + p] + xbuf[p]) - mbuf[q]);  // (an infinite maximum: selected away)
      p += r64;
      q += q64;
      if (p >= W) {
        p -= W;
        ++q;
      }
    }
  }
  wave_lds_sync();
  double r = m;
  if (lane < W) {
    const double *__restrict__ e = ebuf + lane * LS;
    double acc = 0.0;
#pragma unroll 4
    for (int p = 0; p < W; ++p) acc += e[p];
    r = isinf(m) ? m : log(acc) + m;
  }
  return r;
}

// ---- the back-trace kernels -----------------------------------------------------------------------------------------
// a non-finite score has no path: the rows of an utterance without one
__device__ __forceinline__ void x_no_path(int64_t beg, int64_t T, int32_t *__restrict__ path_word,
                                          int32_t *__restrict__ path_state, uint8_t *__restrict__ path_entry) {
  for (int64_t t = 0; t < T; ++t) {
    if (path_word) path_word[beg + t] = -1;
    if (path_state) path_state[beg + t] = -1;
    if (path_entry) path_entry[beg + t] = 0;
  }
}
