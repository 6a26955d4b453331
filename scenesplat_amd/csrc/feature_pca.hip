// PCA colours of a feature matrix (gfx950): the device side of DESIGN.md 8r.  X is (N, D), tall and skinny (a million rows of 768
// language features), fp32 / fp16 / bf16, rows contiguous.
//
//   ss_pca_col_sums   sums[d]  = sum_r ((double)x[r][d] - (double)shift[d])                        one read of X, fp64, fixed order
//   ss_pca_gram       G        = (X - shift)^T (X - shift), (D, D) fp64, both triangles             fp32 MFMA, split over the rows
//   ss_pca_project    y[r][c]  = sum_d (x[r][d] - shift[d]) comp[c][d] - off[c], + min / max of y   one read of X
//   ss_pca_colors     colours  = clip((y - min) / range, 0, 1) laid out as RGB                      elementwise
//
// Nothing here uses a float atomic: every sum that crosses a workgroup goes through a partial that one workgroup owns and a second
// kernel that adds the partials in index order, so two runs give the same bits.
//
// The Gram matrix.  The reduction runs over the ROWS, so the operand maps of v_mfma_f32_32x32x2_f32 (lane l supplies A[i = l & 31]
// [k = l >> 5] and B[k = l >> 5][j = l & 31]; csrc/subm_f32.hip) take both operands straight from a [row][column] LDS image of X: A is
// the column tile ti, B the column tile tj, k the row.  A workgroup owns one pair (ti <= tj) of 128-column tiles and one share of the
// rows; its four waves hold 2 x 2 accumulator tiles of 32 x 32 each (128 x 128 in all).  The MFMA is bit for bit a k-ordered fmaf chain,
// and a chain is cut after SS_PCA_GRAM_CHAIN rows: the fp32 accumulators are added into fp64 registers and cleared, so the fp32 error
// of an entry is that of a chain of SS_PCA_GRAM_CHAIN terms whatever N is.  The shares' fp64 partials are summed in share order by
// k_pca_gram_combine, which also mirrors the tiles above the diagonal into the lower triangle (a diagonal tile is computed whole: the
// products commute, so its two halves already agree bit for bit).
#include "common.h"
#include "feat_in.h"
#include <type_traits>

#define F32MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define PG_TILE 128                         // columns per tile
#define PG_ROWS SS_PCA_GRAM_ROWS            // rows per LDS image
#define PG_LD (PG_TILE + 32)                // floats per LDS row: the two lane halves of an operand read (rows k, k + 1) fall on different banks
#define PG_TARGET_WORKGROUPS 512            // two per CU

static_assert(PG_ROWS == 32 && SS_PCA_GRAM_CHAIN % PG_ROWS == 0 && SS_PCA_GRAM_SHARE_MIN % SS_PCA_GRAM_CHAIN == 0, "row quanta");
static_assert(SS_PCA_MAX_DIM % 4 == 0, "the staged components are read as float4");

// ---- column sums ------------------------------------------------------------------------------------------------------------------
// grid (ceil(D / 64), shares): 64 columns x 4 row lanes per workgroup; part (shares, D) fp64
template <int DT>
__global__ void __launch_bounds__(256)
k_pca_col_sums(const void* __restrict__ x_, const float* __restrict__ shift, double* __restrict__ part, int64_t n, int D,
               int64_t share_rows) {
  typedef typename PcaIn<DT>::T T;
  const T* __restrict__ x = static_cast<const T*>(x_);
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int64_t beg = (int64_t)blockIdx.y * share_rows, end = min(n, beg + share_rows);
  double s = 0.0;
  if (c < D) {
    const double sh = shift ? (double)shift[c] : 0.0;
#pragma unroll 4
    for (int64_t r = beg + rg; r < end; r += 4) s += (double)PcaIn<DT>::one(x + r * D + c) - sh;
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && c < D) part[(int64_t)blockIdx.y * D + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

__global__ void __launch_bounds__(256) k_pca_col_sums_finish(const double* __restrict__ part, double* __restrict__ sums, int D, int shares) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int k = 0; k < shares; ++k) s += part[(int64_t)k * D + c];
  sums[c] = s;
}

static void pca_col_sums_plan(int64_t N, int64_t* share_rows, int* shares) {
  const int64_t want = ss_div_up(N, 1024) < 1024 ? ss_div_up(N, 1024) : 1024;
  *share_rows = (N + want - 1) / want;
  *shares = (int)((N + *share_rows - 1) / *share_rows);
}

extern "C" size_t ss_pca_col_sums_workspace_bytes(int64_t N, int D) {
  if (N < 1 || N >= (1LL << 31) || D < 1 || D > SS_PCA_MAX_DIM) return 0;
  int64_t share_rows; int shares;
  pca_col_sums_plan(N, &share_rows, &shares);
  return (size_t)shares * D * sizeof(double);
}

extern "C" int ss_pca_col_sums(const void* x, int dtype, int64_t N, int D, const float* shift, double* sums, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  if (!x || !sums || N < 1 || N >= (1LL << 31) || D < 1 || D > SS_PCA_MAX_DIM) return SS_ERR_ARG;
  if (dtype != SS_DTYPE_F32 && dtype != SS_DTYPE_BF16 && dtype != SS_DTYPE_F16) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_pca_col_sums_workspace_bytes(N, D)) return SS_ERR_WORKSPACE;
  int64_t share_rows; int shares;
  pca_col_sums_plan(N, &share_rows, &shares);
  double* part = static_cast<double*>(workspace);
  dim3 g(ss_div_up(D, 64), shares), b(256);
  if (dtype == SS_DTYPE_F32) SS_LAUNCH((k_pca_col_sums<SS_DTYPE_F32>), g, b, 0, stream, x, shift, part, N, D, share_rows);
  else if (dtype == SS_DTYPE_BF16) SS_LAUNCH((k_pca_col_sums<SS_DTYPE_BF16>), g, b, 0, stream, x, shift, part, N, D, share_rows);
  else SS_LAUNCH((k_pca_col_sums<SS_DTYPE_F16>), g, b, 0, stream, x, shift, part, N, D, share_rows);
  SS_LAUNCH(k_pca_col_sums_finish, dim3(ss_div_up(D, 256)), b, 0, stream, part, sums, D, shares);
  return SS_OK;
}

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------------
// logical workgroup wg = share * npairs + pair; part
// (shares, npairs, 128, 128) fp64, every element written
template <int DT, bool VEC>
__global__ void __launch_bounds__(256)
k_pca_gram(const void* __restrict__ x_, const float* __restrict__ shift, double* __restrict__ part, int64_t n, int D, int ntiles,
           int npairs, int64_t share_rows) {
  typedef typename PcaIn<DT>::T T;
  const T* __restrict__ x = static_cast<const T*>(x_);
  __shared__ __attribute__((aligned(16))) float As[PG_ROWS * PG_LD];
  __shared__ __attribute__((aligned(16))) float Bs[PG_ROWS * PG_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, kk = lane >> 5;
  // The hardware deals consecutive workgroups round the 8 XCDs; workgroup w = the j-th of XCD w % 8 takes a logical index such that
  // each XCD gets a contiguous run of them: the pairs of one share read the same rows and then meet in one L2 (any bijection is
  // correct; this one only decides which cache sees the reuse)
  const int total = gridDim.x, xcd = blockIdx.x & 7;
  const int wg = xcd * (total >> 3) + min(xcd, total & 7) + (blockIdx.x >> 3);
  const int pair = wg % npairs, share = wg / npairs;
  int ti = 0, rem = pair;                                             // the upper triangle row by row
  while (rem >= ntiles - ti) { rem -= ntiles - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int64_t r_beg = (int64_t)share * share_rows, r_end = min(n, r_beg + share_rows);
  // staging: a thread takes four columns (cg) of the rows r0, r0 + 8, r0 + 16, r0 + 24 of an image: a row is one 512-byte run per wave half
  const int cg = (tid & 31) * 4, r0 = tid >> 5;
  const int ca = ti * PG_TILE + cg, cb = tj * PG_TILE + cg;
  float sa[4], sb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sa[e] = (shift && ca + e < D) ? shift[ca + e] : 0.f;
    sb[e] = (shift && cb + e < D) ? shift[cb + e] : 0.f;
  }
  // VEC: a fetch only LOADS (raw words from a clamped address); the conversion, the shift and the zeros of missing rows / columns wait
  // until the image is written to LDS, so nothing between the loads and the MFMAs they fly under needs their data.  Otherwise
  // (scalar loads, the rare form): finished values at once.
  typedef typename std::conditional<VEC, typename PcaIn<DT>::Raw, float4>::type Staged;
  auto fetch = [&](int64_t rt, Staged (&ra)[4], Staged (&rb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = rt + r0 + 8 * q;
      if constexpr (VEC) {
        const T* p = x + (row < r_end ? row : r_end - 1) * D;
        ra[q] = PcaIn<DT>::raw(p + (ca < D ? ca : 0));
        if (!diag) rb[q] = PcaIn<DT>::raw(p + (cb < D ? cb : 0));
      } else {
        ra[q] = pca_load4<DT, false>(x, row, r_end - 1, ca, D, sa);
        if (!diag) rb[q] = pca_load4<DT, false>(x, row, r_end - 1, cb, D, sb);
      }
    }
  };
  auto finished = [&](const Staged& raw, bool ok, const float (&sh)[4]) -> float4 {
    if constexpr (VEC) {
      float4 v = PcaIn<DT>::unpack(raw);
      v.x = ok ? v.x - sh[0] : 0.f; v.y = ok ? v.y - sh[1] : 0.f; v.z = ok ? v.z - sh[2] : 0.f; v.w = ok ? v.w - sh[3] : 0.f;
      return v;
    } else {
      return raw;
    }
  };
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
  f32x16_t acc00, acc01, acc10, acc11;
  double d00[16], d01[16], d10[16], d11[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc00[r] = 0.f; acc01[r] = 0.f; acc10[r] = 0.f; acc11[r] = 0.f;
    d00[r] = 0.0; d01[r] = 0.0; d10[r] = 0.0; d11[r] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      d00[r] += (double)acc00[r]; d01[r] += (double)acc01[r]; d10[r] += (double)acc10[r]; d11[r] += (double)acc11[r];
      acc00[r] = 0.f; acc01[r] = 0.f; acc10[r] = 0.f; acc11[r] = 0.f;
    }
  };
  const float* const Bp = diag ? As : Bs;
  int chain_rows = 0;
  // one image: registers -> LDS, the loads of the image after the next into the registers just freed (two images of loads fly under
  // one image of MFMAs), 16 k-pairs x 4 MFMAs per wave
  auto image = [&](int64_t rt, Staged (&ra)[4], Staged (&rb)[4]) {
    __syncthreads();                                                  // the previous image has been read
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool row_ok = rt + r0 + 8 * q < r_end;
      *reinterpret_cast<float4*>(As + (r0 + 8 * q) * PG_LD + cg) = finished(ra[q], row_ok && ca < D, sa);
      if (!diag) *reinterpret_cast<float4*>(Bs + (r0 + 8 * q) * PG_LD + cg) = finished(rb[q], row_ok && cb < D, sb);
    }
    __syncthreads();
    if (rt + 2 * PG_ROWS < r_end) fetch(rt + 2 * PG_ROWS, ra, rb);
#pragma unroll
    for (int u = 0; u < PG_ROWS / 2; ++u) {
      const int k = (2 * u + kk) * PG_LD;
      const float a0 = As[k + wi + i], a1 = As[k + wi + 32 + i];
      const float b0 = Bp[k + wj + i], b1 = Bp[k + wj + 32 + i];
      acc00 = F32MFMA(a0, b0, acc00); acc01 = F32MFMA(a0, b1, acc01);
      acc10 = F32MFMA(a1, b0, acc10); acc11 = F32MFMA(a1, b1, acc11);
    }
    chain_rows += PG_ROWS;
    if (chain_rows == SS_PCA_GRAM_CHAIN) { flush(); chain_rows = 0; }
  };
  Staged ra0[4], rb0[4], ra1[4], rb1[4];
  if (r_beg < r_end) fetch(r_beg, ra0, rb0);
  if (r_beg + PG_ROWS < r_end) fetch(r_beg + PG_ROWS, ra1, rb1);
  for (int64_t rt = r_beg; rt < r_end; rt += 2 * PG_ROWS) {
    image(rt, ra0, rb0);
    if (rt + PG_ROWS >= r_end) break;
    image(rt + PG_ROWS, ra1, rb1);
  }
  if (chain_rows) flush();
  // D: column (lane & 31) = column of tile tj, register r of half kk = column (r & 3) + 8 (r >> 2) + 4 kk of tile ti
  double* const out = part + (int64_t)wg * (PG_TILE * PG_TILE);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
    out[(wi + row) * PG_TILE + wj + i] = d00[r];
    out[(wi + row) * PG_TILE + wj + 32 + i] = d01[r];
    out[(wi + 32 + row) * PG_TILE + wj + i] = d10[r];
    out[(wi + 32 + row) * PG_TILE + wj + 32 + i] = d11[r];
  }
}

// grid npairs * 64: one thread per element of a tile pair; the shares in index order; both triangles of G
__global__ void __launch_bounds__(256)
k_pca_gram_combine(const double* __restrict__ part, double* __restrict__ G, int D, int ntiles, int npairs, int shares) {
  const int pair = blockIdx.x >> 6, e = (blockIdx.x & 63) * 256 + threadIdx.x;
  int ti = 0, rem = pair;
  while (rem >= ntiles - ti) { rem -= ntiles - ti; ++ti; }
  const int tj = ti + rem;
  const int gr = ti * PG_TILE + (e >> 7), gc = tj * PG_TILE + (e & 127);
  if (gr >= D || gc >= D) return;
  double s = 0.0;
  for (int k = 0; k < shares; ++k) s += part[((int64_t)k * npairs + pair) * (PG_TILE * PG_TILE) + e];
  G[(int64_t)gr * D + gc] = s;
  if (ti != tj) G[(int64_t)gc * D + gr] = s;
}

static void pca_gram_plan(int64_t N, int D, int* ntiles, int* npairs, int64_t* share_rows, int* shares) {
  *ntiles = ss_div_up(D, PG_TILE);
  *npairs = *ntiles * (*ntiles + 1) / 2;
  const int max_shares = PG_TARGET_WORKGROUPS / *npairs > 1 ? PG_TARGET_WORKGROUPS / *npairs : 1;
  const int64_t chains = (N + SS_PCA_GRAM_CHAIN - 1) / SS_PCA_GRAM_CHAIN;
  int64_t per = ((chains + max_shares - 1) / max_shares) * SS_PCA_GRAM_CHAIN;
  if (per < SS_PCA_GRAM_SHARE_MIN) per = SS_PCA_GRAM_SHARE_MIN;
  *share_rows = per;
  *shares = (int)((N + per - 1) / per);
}

static bool pca_shape_ok(int64_t N, int D) { return N >= 1 && N < (1LL << 31) && D >= 1 && D <= SS_PCA_MAX_DIM; }

extern "C" int64_t ss_pca_gram_share_rows(int64_t N, int D) {
  if (!pca_shape_ok(N, D)) return 0;
  int ntiles, npairs, shares; int64_t share_rows;
  pca_gram_plan(N, D, &ntiles, &npairs, &share_rows, &shares);
  return share_rows;
}

extern "C" size_t ss_pca_gram_workspace_bytes(int64_t N, int D) {
  if (!pca_shape_ok(N, D)) return 0;
  int ntiles, npairs, shares; int64_t share_rows;
  pca_gram_plan(N, D, &ntiles, &npairs, &share_rows, &shares);
  return (size_t)shares * npairs * PG_TILE * PG_TILE * sizeof(double);
}

extern "C" int ss_pca_gram(const void* x, int dtype, int64_t N, int D, const float* shift, double* gram, void* workspace,
                           size_t workspace_bytes, hipStream_t stream) {
  if (!x || !gram || !pca_shape_ok(N, D)) return SS_ERR_ARG;
  if (dtype != SS_DTYPE_F32 && dtype != SS_DTYPE_BF16 && dtype != SS_DTYPE_F16) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_pca_gram_workspace_bytes(N, D)) return SS_ERR_WORKSPACE;
  int ntiles, npairs, shares; int64_t share_rows;
  pca_gram_plan(N, D, &ntiles, &npairs, &share_rows, &shares);
  double* part = static_cast<double*>(workspace);
  dim3 g(shares * npairs), b(256);
  const bool vec = pca_vec_ok(x, dtype, D);
#define PCA_GRAM_GO(DT)                                                                                                   \
  do {                                                                                                                    \
    if (vec) SS_LAUNCH((k_pca_gram<DT, true>), g, b, 0, stream, x, shift, part, N, D, ntiles, npairs, share_rows);        \
    else SS_LAUNCH((k_pca_gram<DT, false>), g, b, 0, stream, x, shift, part, N, D, ntiles, npairs, share_rows);           \
  } while (0)
  if (dtype == SS_DTYPE_F32) PCA_GRAM_GO(SS_DTYPE_F32);
  else if (dtype == SS_DTYPE_BF16) PCA_GRAM_GO(SS_DTYPE_BF16);
  else PCA_GRAM_GO(SS_DTYPE_F16);
#undef PCA_GRAM_GO
  SS_LAUNCH(k_pca_gram_combine, dim3(npairs * 64), b, 0, stream, part, gram, D, ntiles, npairs, shares);
  return SS_OK;
}

// ---- projection + extremes --------------------------------------------------------------------------------------------------------
// A workgroup takes blocks of SS_PCA_PROJECT_ROWS rows (grid stride), a wave 64 of them, four rows at a time: the lanes stride over
// the columns, each row's K partial dot products are summed over the wave by xor shuffles (a fixed tree), and every lane ends up with
// the value that is written -- so the minima / maxima a lane keeps are those of the written y.  part (grid, 2 K): minima, maxima.
#define PP_MAX_GRID 2048

template <int DT, bool VEC, int K>
__global__ void __launch_bounds__(256)
k_pca_project(const void* __restrict__ x_, const float* __restrict__ shift, const float* __restrict__ comp,
              const float* __restrict__ off, float* __restrict__ y, float* __restrict__ part, int64_t n, int D, int nblocks) {
  typedef typename PcaIn<DT>::T T;
  const T* __restrict__ x = static_cast<const T*>(x_);
  __shared__ __attribute__((aligned(16))) float cs[K + 1][SS_PCA_MAX_DIM];           // the components, then the shift
  __shared__ float ext[4][2 * K];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int d = tid; d < SS_PCA_MAX_DIM; d += 256) {
#pragma unroll
    for (int c = 0; c < K; ++c) cs[c][d] = d < D ? comp[c * D + d] : 0.f;
    cs[K][d] = (shift && d < D) ? shift[d] : 0.f;
  }
  __syncthreads();
  float offv[K], mn[K], mx[K];
#pragma unroll
  for (int c = 0; c < K; ++c) { offv[c] = off ? off[c] : 0.f; mn[c] = INFINITY; mx[c] = -INFINITY; }
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t base = (int64_t)blk * SS_PCA_PROJECT_ROWS + wave * 64;
    for (int g = 0; g < 16; ++g) {
      const int64_t row0 = base + 4 * g;
      if (row0 >= n) break;                                             // wave-uniform
      float acc[4][K];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < K; ++c) acc[q][c] = 0.f;
      if (VEC) {
        for (int d = lane * 4; d < D; d += 256) {
          const float4 s4 = *reinterpret_cast<const float4*>(&cs[K][d]);
          const float s[4] = {s4.x, s4.y, s4.z, s4.w};
          float4 v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = pca_load4<DT, true>(x, row0 + q, n - 1, d, D, s);
#pragma unroll
          for (int c = 0; c < K; ++c) {
            const float4 w = *reinterpret_cast<const float4*>(&cs[c][d]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[q][c] = fmaf(v[q].w, w.w, fmaf(v[q].z, w.z, fmaf(v[q].y, w.y, fmaf(v[q].x, w.x, acc[q][c]))));
          }
        }
      } else {
        for (int d = lane; d < D; d += 64) {
          const float s = cs[K][d];
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float e = PcaIn<DT>::one(x + min(row0 + q, n - 1) * D + d);           // clamped row, then a select (pca_load4)
            v[q] = row0 + q < n ? e - s : 0.f;
          }
#pragma unroll
          for (int c = 0; c < K; ++c) {
            const float w = cs[c][d];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q][c] = fmaf(v[q], w, acc[q][c]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < K; ++c) {
          float t = acc[q][c];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
          t -= offv[c];
          acc[q][c] = t;
          if (row0 + q < n) { mn[c] = fminf(mn[c], t); mx[c] = fmaxf(mx[c], t); }
        }
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (row0 + q < n) {
#pragma unroll
            for (int c = 0; c < K; ++c) y[(row0 + q) * K + c] = acc[q][c];
          }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < K; ++c) { ext[wave][c] = mn[c]; ext[wave][K + c] = mx[c]; }
  }
  __syncthreads();
  if (tid < 2 * K) {
    float v = ext[0][tid];
    for (int w = 1; w < 4; ++w) v = tid < K ? fminf(v, ext[w][tid]) : fmaxf(v, ext[w][tid]);
    part[(int64_t)blockIdx.x * 2 * K + tid] = v;
  }
}

__global__ void __launch_bounds__(64) k_pca_extremes_finish(const float* __restrict__ part, float* __restrict__ extremes, int K, int grid) {
  const int t = threadIdx.x;
  if (t >= 2 * K) return;
  float v = part[t];
  for (int b = 1; b < grid; ++b) v = t < K ? fminf(v, part[b * 2 * K + t]) : fmaxf(v, part[b * 2 * K + t]);
  extremes[t] = v;
}

static int pca_project_grid(int64_t N) {
  const int nblocks = ss_div_up(N, SS_PCA_PROJECT_ROWS);
  return nblocks < PP_MAX_GRID ? nblocks : PP_MAX_GRID;
}

extern "C" size_t ss_pca_project_workspace_bytes(int64_t N) {
  if (N < 1 || N >= (1LL << 31)) return 0;
  return (size_t)pca_project_grid(N) * 6 * sizeof(float);
}

template <int DT, bool VEC>
static int pca_project_launch(const void* x, int64_t N, int D, const float* shift, const float* comp, const float* off, int k, float* y,
                              float* part, int grid, hipStream_t stream) {
  const int nblocks = ss_div_up(N, SS_PCA_PROJECT_ROWS);
  dim3 g(grid), b(256);
  if (k == 1) SS_LAUNCH((k_pca_project<DT, VEC, 1>), g, b, 0, stream, x, shift, comp, off, y, part, N, D, nblocks);
  else if (k == 2) SS_LAUNCH((k_pca_project<DT, VEC, 2>), g, b, 0, stream, x, shift, comp, off, y, part, N, D, nblocks);
  else SS_LAUNCH((k_pca_project<DT, VEC, 3>), g, b, 0, stream, x, shift, comp, off, y, part, N, D, nblocks);
  return SS_OK;
}

extern "C" int ss_pca_project(const void* x, int dtype, int64_t N, int D, const float* shift, const float* comp, const float* off, int k,
                              float* y, float* extremes, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!x || !comp || !y || !extremes || !pca_shape_ok(N, D) || k < 1 || k > 3 || k > D) return SS_ERR_ARG;
  if (dtype != SS_DTYPE_F32 && dtype != SS_DTYPE_BF16 && dtype != SS_DTYPE_F16) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_pca_project_workspace_bytes(N)) return SS_ERR_WORKSPACE;
  float* part = static_cast<float*>(workspace);
  const int grid = pca_project_grid(N);
  const bool vec = pca_vec_ok(x, dtype, D);
  int rc;
#define PCA_PROJECT_GO(DT)                                                                                              \
  rc = vec ? pca_project_launch<DT, true>(x, N, D, shift, comp, off, k, y, part, grid, stream)                          \
           : pca_project_launch<DT, false>(x, N, D, shift, comp, off, k, y, part, grid, stream)
  if (dtype == SS_DTYPE_F32) PCA_PROJECT_GO(SS_DTYPE_F32);
  else if (dtype == SS_DTYPE_BF16) PCA_PROJECT_GO(SS_DTYPE_BF16);
  else PCA_PROJECT_GO(SS_DTYPE_F16);
#undef PCA_PROJECT_GO
  if (rc != SS_OK) return rc;
  SS_LAUNCH(k_pca_extremes_finish, dim3(1), dim3(64), 0, stream, part, extremes, k, grid);
  return SS_OK;
}

// ---- colours ----------------------------------------------------------------------------------------------------------------------
// DESIGN.md 8r step 6 in fp32, each operation rounded on its own (IEEE division): k = 3: P; k = 2: [P0, P1, 0.5]; k = 1: P0 three times
template <int K>
__global__ void __launch_bounds__(256)
k_pca_colors(const float* __restrict__ y, const float* __restrict__ extremes, float* __restrict__ colors, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  float p[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const float mn = extremes[c];
    float range = extremes[K + c] - mn;
    if (range == 0.f) range = 1.f;
    p[c] = fminf(fmaxf((y[r * K + c] - mn) / range, 0.f), 1.f);
  }
  float* o = colors + r * 3;
  if (K == 1) { o[0] = p[0]; o[1] = p[0]; o[2] = p[0]; }
  else if (K == 2) { o[0] = p[0]; o[1] = p[K - 1]; o[2] = 0.5f; }
  else { o[0] = p[0]; o[1] = p[K > 1 ? 1 : 0]; o[2] = p[K - 1]; }
}

extern "C" int ss_pca_colors(const float* y, const float* extremes, int64_t N, int k, float* colors, hipStream_t stream) {
  if (!y || !extremes || !colors || N < 1 || N >= (1LL << 31) || k < 1 || k > 3) return SS_ERR_ARG;
  dim3 g(ss_div_up(N, 256)), b(256);
  if (k == 1) SS_LAUNCH(k_pca_colors<1>, g, b, 0, stream, y, extremes, colors, N);
  else if (k == 2) SS_LAUNCH(k_pca_colors<2>, g, b, 0, stream, y, extremes, colors, N);
  else SS_LAUNCH(k_pca_colors<3>, g, b, 0, stream, y, extremes, colors, N);
  return SS_OK;
}
