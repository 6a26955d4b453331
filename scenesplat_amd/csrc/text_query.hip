// Text queries on scene features (gfx950): the device side of DESIGN.md 8t.  X is (N, D), fp32 / fp16 / bf16, rows contiguous; T_hat is
// (Q, D) fp32, the unit text embeddings (normalised on the host in fp64).
//
//   ss_query_scores   scores[q][r] = (x[r] . t_hat[q]) / max(|x[r]|, 1e-12), -inf for a dead row; stats (Q, 3) f64 = {L, sum s, sum s^2}
//   ss_query_select   per query: the rows with s >= tau, cut to the m best (descending score, the lower row first), as a bitmap
//   ss_query_best     per row: the selecting query of highest score
//
// The score pass reads every row once whatever Q is.  A wave owns 32 rows and all 32 query slots: v_mfma_f32_32x32x2_f32 with A = T_hat
// (i = query) and B = X (j = row), so lane (j, kk) feeds the MFMA straight from ITS OWN row of X -- the lanes of half kk take the
// columns [64 it + 32 kk, + 32) of iteration `it` (the order of the k index is free as long as A and B agree), 8 wide loads per lane
// and iteration, the loads of the next iteration in flight under the 32 MFMAs of this one.  T_hat sits in LDS as [d][32]: the 32 lanes
// of one ds_read_b32 group read 32 consecutive floats.  The MFMA is a k-ordered fmaf chain per (query, row), so a score's summation
// order is fixed; |x|^2 is a per-lane fmaf chain over the lane's columns plus one add of the two halves.
//
// Nothing here uses a float atomic.  The statistics are per-lane fp64 sums over the rows a workgroup takes, reduced over the wave by
// a fixed shuffle tree and over the waves and the workgroups in index order.  The select passes count with integer atomics only.
#include "common.h"
#include "feat_in.h"
#include <type_traits>

#define F32MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define QS_THREADS 512
#define QS_WAVES (QS_THREADS / 64)
#define QS_MAX_GRID 512                     // two row blocks in flight per CU's worth of workgroups; the partials' count
#define QS_QP SS_QUERY_MAX_QUERIES          // query slots of the MFMA tile
#define QS_COLS 64                          // columns per iteration: 32 per lane half

static_assert(SS_QUERY_ROWS == QS_WAVES * 32 && QS_QP == 32 && SS_QUERY_MAX_DIM % QS_COLS == 0, "tile shape");

template <int DT, bool VEC>
__global__ void __launch_bounds__(QS_THREADS)
k_query_scores(const void* __restrict__ x_, const float* __restrict__ t_hat, const uint8_t* __restrict__ valid, float* __restrict__ scores,
               double* __restrict__ part, int64_t n, int D, int Q, int Dp, int nblocks) {
  typedef typename PcaIn<DT>::T T;
  const T* __restrict__ x = static_cast<const T*>(x_);
  extern __shared__ __attribute__((aligned(16))) float tq[];           // [Dp][32]: t_hat[q][d] at d * 32 + q, zeros beyond Q and D
  __shared__ double red[QS_WAVES][QS_QP][2];
  __shared__ int red_cnt[QS_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, kk = lane >> 5;
  for (int idx = tid; idx < Dp * QS_QP; idx += QS_THREADS) {
    const int q = idx / Dp, d = idx - q * Dp;                           // d fastest: the global reads are contiguous
    tq[d * QS_QP + q] = (q < Q && d < D) ? t_hat[(int64_t)q * D + d] : 0.f;
  }
  __syncthreads();
  typedef typename std::conditional<VEC, typename PcaIn<DT>::Raw, float4>::type Staged;
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  const int nit = Dp / QS_COLS;
  double dsum[16], dsq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dsum[r] = 0.0; dsq[r] = 0.0; }
  int cnt = 0;
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t row0 = (int64_t)blk * SS_QUERY_ROWS + wave * 32;
    if (row0 >= n) continue;                                            // wave-uniform
    const int64_t row = row0 + j;
    const T* __restrict__ p = x + (row < n ? row : n - 1) * D;
    auto fetch = [&](int it, Staged (&st)[8]) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = it * QS_COLS + kk * 32 + 4 * u;
        if constexpr (VEC) st[u] = PcaIn<DT>::raw(p + (c < D ? c : 0));
        else st[u] = pca_load4<DT, false>(x, row, n - 1, c, D, zero4);
      }
    };
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float nsq = 0.f;
    auto compute = [&](int it, const Staged (&st)[8]) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = it * QS_COLS + kk * 32 + 4 * u;
        float4 v;
        if constexpr (VEC) {
          v = PcaIn<DT>::unpack(st[u]);
          if (c >= D) v = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          v = st[u];
        }
        const float* tp = tq + c * QS_QP + j;
        acc = F32MFMA(tp[0], v.x, acc); acc = F32MFMA(tp[QS_QP], v.y, acc);
        acc = F32MFMA(tp[2 * QS_QP], v.z, acc); acc = F32MFMA(tp[3 * QS_QP], v.w, acc);
        nsq = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, nsq))));
      }
    };
    if constexpr (VEC) {
      Staged s0[8], s1[8];
      fetch(0, s0);
      for (int it = 0; it < nit; it += 2) {
        if (it + 1 < nit) fetch(it + 1, s1);
        compute(it, s0);
        if (it + 1 >= nit) break;
        if (it + 2 < nit) fetch(it + 2, s0);
        compute(it + 1, s1);
      }
    } else {                                                            // element loads (the rare form): one iteration at a time
      Staged s0[8];
      for (int it = 0; it < nit; ++it) { fetch(it, s0); compute(it, s0); }
    }
    // lane (j, kk), register r: query (r & 3) + 8 (r >> 2) + 4 kk of row j
    const float nrm = sqrtf(nsq + __shfl_xor(nsq, 32, 64));            // (IEEE square root and division: the compiler default)
    const float den = fmaxf(nrm, 1e-12f);
    float s[16];
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (r & 3) + 8 * (r >> 2) + 4 * kk;
      s[r] = acc[r] / den;
      if (q < Q && !(fabsf(s[r]) < INFINITY)) bad = 1;                  // (false for NaN too)
    }
    bad |= __shfl_xor(bad, 32, 64);
    const bool live = row < n && !bad && nrm != 0.f && (!valid || valid[row < n ? row : n - 1] != 0);
    if (row < n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = (r & 3) + 8 * (r >> 2) + 4 * kk;
        if (q < Q) {
          const float v = s[r] == 0.f ? 0.f : s[r];                     // -0.0 is written as +0.0
          scores[(int64_t)q * n + row] = live ? v : -INFINITY;
          if (live) { const double dv = (double)v; dsum[r] += dv; dsq[r] += dv * dv; }
        }
      }
    }
    if (live && kk == 0) ++cnt;
  }
  // over the 32 rows' lanes by a fixed tree, then the waves in order
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { dsum[r] += __shfl_xor(dsum[r], o, 64); dsq[r] += __shfl_xor(dsq[r], o, 64); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (j == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (r & 3) + 8 * (r >> 2) + 4 * kk;
      red[wave][q][0] = dsum[r]; red[wave][q][1] = dsq[r];
    }
  }
  if (lane == 0) red_cnt[wave] = cnt;
  __syncthreads();
  if (tid < Q) {
    double a = 0.0, b = 0.0; int c = 0;
    for (int w = 0; w < QS_WAVES; ++w) { a += red[w][tid][0]; b += red[w][tid][1]; c += red_cnt[w]; }
    double* o = part + ((int64_t)blockIdx.x * QS_QP + tid) * 3;
    o[0] = (double)c; o[1] = a; o[2] = b;
  }
}

__global__ void __launch_bounds__(64) k_query_stats_finish(const double* __restrict__ part, double* __restrict__ stats, int Q, int grid) {
  const int q = threadIdx.x;
  if (q >= Q) return;
  double l = 0.0, a = 0.0, b = 0.0;
  for (int g = 0; g < grid; ++g) {
    const double* p = part + ((int64_t)g * QS_QP + q) * 3;
    l += p[0]; a += p[1]; b += p[2];
  }
  stats[q * 3 + 0] = l; stats[q * 3 + 1] = a; stats[q * 3 + 2] = b;
}

static bool query_shape_ok(int64_t N, int Q) { return N >= 1 && N < (1LL << 31) && Q >= 1 && Q <= SS_QUERY_MAX_QUERIES; }
static int query_scores_grid(int64_t N) {
  const int nblocks = ss_div_up(N, SS_QUERY_ROWS);
  return nblocks < QS_MAX_GRID ? nblocks : QS_MAX_GRID;
}

extern "C" size_t ss_query_scores_workspace_bytes(int64_t N, int Q) {
  if (!query_shape_ok(N, Q)) return 0;
  return (size_t)query_scores_grid(N) * QS_QP * 3 * sizeof(double);
}

template <int DT, bool VEC>
static int query_scores_launch(const void* x, int64_t N, int D, const float* t_hat, int Q, const uint8_t* valid, float* scores, double* part,
                               int grid, hipStream_t stream) {
  const int Dp = ss_div_up(D, QS_COLS) * QS_COLS, nblocks = ss_div_up(N, SS_QUERY_ROWS);
  const size_t lds = (size_t)Dp * QS_QP * sizeof(float);
  // above 64 KB of dynamic LDS the runtime wants to be told
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_query_scores<DT, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return SS_ERR_LAUNCH;
  SS_LAUNCH((k_query_scores<DT, VEC>), dim3(grid), dim3(QS_THREADS), lds, stream, x, t_hat, valid, scores, part, N, D, Q, Dp, nblocks);
  return SS_OK;
}

extern "C" int ss_query_scores(const void* x, int dtype, int64_t N, int D, const float* t_hat, int Q, const uint8_t* valid, float* scores,
                               double* stats, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!x || !t_hat || !scores || !stats || !query_shape_ok(N, Q) || D < 1 || D > SS_QUERY_MAX_DIM) return SS_ERR_ARG;
  if (dtype != SS_DTYPE_F32 && dtype != SS_DTYPE_BF16 && dtype != SS_DTYPE_F16) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_query_scores_workspace_bytes(N, Q)) return SS_ERR_WORKSPACE;
  double* part = static_cast<double*>(workspace);
  const int grid = query_scores_grid(N);
  const bool vec = pca_vec_ok(x, dtype, D);
  int rc;
#define QUERY_SCORES_GO(DT)                                                                                             \
  rc = vec ? query_scores_launch<DT, true>(x, N, D, t_hat, Q, valid, scores, part, grid, stream)                        \
           : query_scores_launch<DT, false>(x, N, D, t_hat, Q, valid, scores, part, grid, stream)
  if (dtype == SS_DTYPE_F32) QUERY_SCORES_GO(SS_DTYPE_F32);
  else if (dtype == SS_DTYPE_BF16) QUERY_SCORES_GO(SS_DTYPE_BF16);
  else QUERY_SCORES_GO(SS_DTYPE_F16);
#undef QUERY_SCORES_GO
  if (rc != SS_OK) return rc;
  SS_LAUNCH(k_query_stats_finish, dim3(1), dim3(64), 0, stream, (const double*)part, stats, Q, grid);
  return SS_OK;
}

// ---- selection --------------------------------------------------------------------------------------------------------------------
// A candidate of query q is a live row (s > -inf) with s >= tau[q].  With a cap m >= 0 the min(m, C) best of the C candidates are found
// by a most-significant-digit radix select on an order-preserving uint32 key (four passes of 8 bits: a histogram of the candidates that
// match the prefix so far, then one thread walks the 256 bins from the top), which ends with the pivot key K and the number t of rows
// equal to K that are kept.  The rows equal to K are ranked in row order: a count per segment of SS_QUERY_SELECT_ROWS rows (a wave's
// share), an exclusive scan over the segments, and a ballot prefix inside the segment -- the lower row wins.
#define QL_THREADS 256
#define QL_WAVES (QL_THREADS / 64)
#define QL_STATE 8                          // words per query: C, need, m_eff, prefix / K, remaining / t, take_all
struct QlArgs { float tau[SS_QUERY_MAX_QUERIES]; int32_t m[SS_QUERY_MAX_QUERIES]; };

static_assert(SS_QUERY_SELECT_ROWS % 64 == 0, "a segment is whole ballots");

// larger score <=> larger key; -0.0 and +0.0 share a key
__device__ __forceinline__ uint32_t ql_key(float s) {
  const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ql_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool ql_candidate(float s, float tau) { return s > -INFINITY && s >= tau; }

__global__ void __launch_bounds__(QL_THREADS) k_ql_clear(uint32_t* __restrict__ words, int n) {
  for (int i = blockIdx.x * QL_THREADS + threadIdx.x; i < n; i += gridDim.x * QL_THREADS) words[i] = 0u;
}

// grid (ceil(nseg / 4), Q): a wave per segment
template <int PASS>
__global__ void __launch_bounds__(QL_THREADS)
k_ql_hist(const float* __restrict__ scores, int64_t n, QlArgs args, const uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
  const int q = blockIdx.y;
  if (PASS > 0 && state[q * QL_STATE + 1] == 0u) return;               // uniform over the workgroup
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const float tau = args.tau[q];
  const uint32_t prefix = PASS > 0 ? state[q * QL_STATE + 3] : 0u;
  const int64_t beg = ((int64_t)blockIdx.x * QL_WAVES + (threadIdx.x >> 6)) * SS_QUERY_SELECT_ROWS;
  const int64_t end = beg + SS_QUERY_SELECT_ROWS < n ? beg + SS_QUERY_SELECT_ROWS : n;
  const float* __restrict__ sc = scores + (int64_t)q * n;
  for (int64_t r = beg + (threadIdx.x & 63); r < end; r += 64) {
    const float s = sc[r];
    if (!ql_candidate(s, tau)) continue;
    const uint32_t key = ql_key(s);
    if (PASS > 0 && ((key ^ prefix) >> (32 - 8 * (PASS > 0 ? PASS : 1))) != 0u) continue;
    atomicAdd(&h[(key >> (24 - 8 * PASS)) & 255u], 1u);
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(&hist[(q * 4 + PASS) * 256 + threadIdx.x], c);
}

// one workgroup, thread q: the pivot digit of this pass; after the last pass counts and tau_out
template <int PASS>
__global__ void __launch_bounds__(64)
k_ql_pick(QlArgs args, int Q, uint32_t* __restrict__ state, const uint32_t* __restrict__ hist, float* __restrict__ tau_out,
          int32_t* __restrict__ counts) {
  const int q = threadIdx.x;
  if (q >= Q) return;
  uint32_t* st = state + q * QL_STATE;
  const uint32_t* h = hist + (q * 4 + PASS) * 256;
  if (PASS == 0) {
    uint32_t C = 0;
    for (int b = 0; b < 256; ++b) C += h[b];
    const int32_t m = args.m[q];
    const uint32_t m_eff = m < 0 ? C : ((uint32_t)m < C ? (uint32_t)m : C);
    st[0] = C; st[1] = (m >= 0 && m_eff > 0u) ? 1u : 0u; st[2] = m_eff; st[3] = 0u; st[4] = m_eff; st[5] = m < 0 ? 1u : 0u;
  }
  if (st[1]) {
    const uint32_t rem = st[4];
    uint32_t cum = 0;
    int b = 255;
    while (b > 0 && cum + h[b] < rem) { cum += h[b]; --b; }
    st[3] |= (uint32_t)b << (24 - 8 * PASS);
    st[4] = rem - cum;
  }
  if (PASS == 3) {
    const int32_t m = args.m[q];
    const float tau = args.tau[q];
    counts[q] = (int32_t)st[2];
    // the cap binds, or there is no threshold: the score of the last row kept
    const bool last = m >= 0 && ((uint32_t)m < st[0] || tau == -INFINITY);
    tau_out[q] = last ? (st[2] > 0u ? ql_unkey(st[3]) : INFINITY) : tau;
  }
}

__global__ void __launch_bounds__(QL_THREADS)
k_ql_eq_count(const float* __restrict__ scores, int64_t n, QlArgs args, const uint32_t* __restrict__ state, int nseg,
              uint32_t* __restrict__ seg_count) {
  const int q = blockIdx.y;
  if (state[q * QL_STATE + 1] == 0u) return;
  const int seg = blockIdx.x * QL_WAVES + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const float tau = args.tau[q];
  const uint32_t K = state[q * QL_STATE + 3];
  const int64_t beg = (int64_t)seg * SS_QUERY_SELECT_ROWS, end = beg + SS_QUERY_SELECT_ROWS < n ? beg + SS_QUERY_SELECT_ROWS : n;
  const float* __restrict__ sc = scores + (int64_t)q * n;
  uint32_t c = 0;
  for (int64_t r0 = beg; r0 < end; r0 += 64) {
    const int64_t r = r0 + (threadIdx.x & 63);
    const float s = r < end ? sc[r] : -INFINITY;
    c += (uint32_t)__popcll(__ballot(ql_candidate(s, tau) && ql_key(s) == K));
  }
  if ((threadIdx.x & 63) == 0) seg_count[(int64_t)q * nseg + seg] = c;
}

// grid Q: seg_count -> its exclusive running sum, in place, pieces of 256 with a carry
__global__ void __launch_bounds__(QL_THREADS)
k_ql_eq_scan(const uint32_t* __restrict__ state, int nseg, uint32_t* __restrict__ seg_count) {
  const int q = blockIdx.x;
  if (state[q * QL_STATE + 1] == 0u) return;
  __shared__ uint32_t wave_sum[QL_WAVES];
  uint32_t* v = seg_count + (int64_t)q * nseg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < nseg; base += QL_THREADS) {
    const int i = base + threadIdx.x;
    const uint32_t x = i < nseg ? v[i] : 0u;
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    __syncthreads();                                                    // the previous piece's reads of wave_sum are over
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < QL_WAVES; ++w) { const uint32_t s = wave_sum[w]; if (w < wave) before += s; total += s; }
    if (i < nseg) v[i] = carry + before + inc - x;
    carry += total;
  }
}

// every word of the (Q, words) bitmap is written; bits of rows >= n are 0
__global__ void __launch_bounds__(QL_THREADS)
k_ql_emit(const float* __restrict__ scores, int64_t n, QlArgs args, const uint32_t* __restrict__ state, int nseg,
          const uint32_t* __restrict__ seg_base, int64_t words, uint32_t* __restrict__ bitmap) {
  const int q = blockIdx.y;
  const int seg = blockIdx.x * QL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seg >= nseg) return;
  const uint32_t* st = state + q * QL_STATE;
  const bool need = st[1] != 0u, take_all = st[5] != 0u;
  const uint32_t K = st[3], t = st[4];
  const float tau = args.tau[q];
  const int64_t beg = (int64_t)seg * SS_QUERY_SELECT_ROWS, end = beg + SS_QUERY_SELECT_ROWS < n ? beg + SS_QUERY_SELECT_ROWS : n;
  const float* __restrict__ sc = scores + (int64_t)q * n;
  uint32_t* __restrict__ bm = bitmap + (int64_t)q * words;
  uint32_t rank0 = need ? seg_base[(int64_t)q * nseg + seg] : 0u;
  for (int64_t r0 = beg; r0 < end; r0 += 64) {
    const int64_t r = r0 + lane;
    const float s = r < end ? sc[r] : -INFINITY;
    const bool cand = ql_candidate(s, tau);
    bool take = cand && take_all;
    if (need) {
      const uint32_t key = ql_key(s);
      const bool eq = cand && key == K;
      const unsigned long long eqm = __ballot(eq);
      const uint32_t rank = rank0 + (uint32_t)__popcll(eqm & ((1ull << lane) - 1ull));
      take = cand && (key > K || (eq && rank < t));
      rank0 += (uint32_t)__popcll(eqm);
    }
    const unsigned long long mask = __ballot(take);
    const int64_t w0 = r0 >> 5;
    if (lane == 0) bm[w0] = (uint32_t)mask;
    if (lane == 1 && w0 + 1 < words) bm[w0 + 1] = (uint32_t)(mask >> 32);
  }
}

static int ql_segments(int64_t N) { return ss_div_up(N, SS_QUERY_SELECT_ROWS); }
static size_t ql_words(int64_t N, int Q) { return (size_t)Q * QL_STATE + (size_t)Q * 4 * 256 + (size_t)Q * ql_segments(N); }

extern "C" size_t ss_query_select_workspace_bytes(int64_t N, int Q) {
  if (!query_shape_ok(N, Q)) return 0;
  return ql_words(N, Q) * sizeof(uint32_t);
}

extern "C" int ss_query_select(const float* scores, int64_t N, int Q, const float* h_tau, const int32_t* h_m, uint32_t* bitmap,
                               float* tau_out, int32_t* counts, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!scores || !h_tau || !h_m || !bitmap || !tau_out || !counts || !query_shape_ok(N, Q)) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_query_select_workspace_bytes(N, Q)) return SS_ERR_WORKSPACE;
  QlArgs args;
  for (int q = 0; q < SS_QUERY_MAX_QUERIES; ++q) { args.tau[q] = q < Q ? h_tau[q] : INFINITY; args.m[q] = q < Q ? h_m[q] : 0; }
  uint32_t* state = static_cast<uint32_t*>(workspace);
  uint32_t* hist = state + Q * QL_STATE;
  uint32_t* seg = hist + Q * 4 * 256;
  const int nseg = ql_segments(N);
  const int64_t words = (N + 31) / 32;
  const int head = Q * QL_STATE + Q * 4 * 256;                          // (the segment counts are written before they are read)
  dim3 g(ss_div_up(nseg, QL_WAVES), Q), b(QL_THREADS);
  SS_LAUNCH(k_ql_clear, dim3(ss_div_up(head, QL_THREADS)), b, 0, stream, state, head);
  SS_LAUNCH(k_ql_hist<0>, g, b, 0, stream, scores, N, args, (const uint32_t*)state, hist);
  SS_LAUNCH(k_ql_pick<0>, dim3(1), dim3(64), 0, stream, args, Q, state, (const uint32_t*)hist, tau_out, counts);
  SS_LAUNCH(k_ql_hist<1>, g, b, 0, stream, scores, N, args, (const uint32_t*)state, hist);
  SS_LAUNCH(k_ql_pick<1>, dim3(1), dim3(64), 0, stream, args, Q, state, (const uint32_t*)hist, tau_out, counts);
  SS_LAUNCH(k_ql_hist<2>, g, b, 0, stream, scores, N, args, (const uint32_t*)state, hist);
  SS_LAUNCH(k_ql_pick<2>, dim3(1), dim3(64), 0, stream, args, Q, state, (const uint32_t*)hist, tau_out, counts);
  SS_LAUNCH(k_ql_hist<3>, g, b, 0, stream, scores, N, args, (const uint32_t*)state, hist);
  SS_LAUNCH(k_ql_pick<3>, dim3(1), dim3(64), 0, stream, args, Q, state, (const uint32_t*)hist, tau_out, counts);
  SS_LAUNCH(k_ql_eq_count, g, b, 0, stream, scores, N, args, (const uint32_t*)state, nseg, seg);
  SS_LAUNCH(k_ql_eq_scan, dim3(Q), b, 0, stream, (const uint32_t*)state, nseg, seg);
  SS_LAUNCH(k_ql_emit, g, b, 0, stream, scores, N, args, (const uint32_t*)state, nseg, (const uint32_t*)seg, words, bitmap);
  return SS_OK;
}

// best[r] = among the queries whose bitmap holds row r the one of highest score (the lowest q among equals), or -1
__global__ void __launch_bounds__(256)
k_query_best(const float* __restrict__ scores, const uint32_t* __restrict__ bitmap, int64_t n, int Q, int64_t words, int32_t* __restrict__ best) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int bq = -1;
  float bs = -INFINITY;
  for (int q = 0; q < Q; ++q) {
    if (!((bitmap[(int64_t)q * words + (r >> 5)] >> (r & 31)) & 1u)) continue;
    const float s = scores[(int64_t)q * n + r];
    if (bq < 0 || s > bs) { bq = q; bs = s; }
  }
  best[r] = bq;
}

extern "C" int ss_query_best(const float* scores, const uint32_t* bitmap, int64_t N, int Q, int32_t* best, hipStream_t stream) {
  if (!scores || !bitmap || !best || !query_shape_ok(N, Q)) return SS_ERR_ARG;
  SS_LAUNCH(k_query_best, dim3(ss_div_up(N, 256)), dim3(256), 0, stream, scores, bitmap, N, Q, (N + 31) / 32, best);
  return SS_OK;
}
