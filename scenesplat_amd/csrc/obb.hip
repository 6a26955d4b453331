// The minimal oriented bounding box of a scan and the Gaussians inside it: what Open3D's get_minimal_oriented_bounding_box() and
// get_point_indices_within_bounding_box() do for preprocess_scannet_gs.py / preprocess_scannetpp_gs.py, in the definition of
// DESIGN.md 8q (every edge of every hull triangle is a candidate frame).
//   extremes  one pass over the N points: a workgroup stages a tile of points in LDS, every wave owns groups of four directions
//             (wave-uniform), its lanes walk the tile and keep (value, row) of the largest and smallest projection; one shuffle
//             reduction per (tile, direction), the workgroup's running best in LDS, then a second launch over the workgroups' partials.
//             (value, row) pairs are compared as a whole: equal values go to the lower row, whatever the order of arrival.
//   filter    one lane per point against the F planes of the polytope of those extremes (staged in LDS, read as broadcasts): a row
//             is dropped only when it lies below EVERY plane by more than tol.  A comparison with NaN keeps the row.
//   search    one lane per candidate frame (3 per hull triangle) against the H hull vertices staged in LDS: six running min / max,
//             volume = extent product; then one workgroup picks the least volume (equal: the lowest candidate) by comparing
//             (volume, index) pairs and recomputes that candidate's box.  No atomics anywhere.
//   within    one lane per point against one box (15 doubles as kernel arguments), inclusive, in fp64.
// filter and within write the (1, ceil(n / 32)) bitmap ss_pc_compact_scan / ss_pc_compact (pc_attach.hip) turn into ascending rows.
#include "common.h"
// search and within are stated operation by operation (tests/obb_cases.py restates them in numpy): no product may fuse
// into a sum there.  extremes and filter only select rows, they allow the fused form locally.
#pragma clang fp contract(off)

#define OBB_THREADS 256
#define OBB_MAX_WG 1024                // extremes: workgroups (= partials per direction)
#define OBB_TILE 1024                  // extremes: points of one LDS tile
#define OBB_MAX_DIRS 1024
#define OBB_PLANE_CHUNK 2048           // filter: planes of one LDS chunk (64 KiB)
#define OBB_VERT_CHUNK 1024            // search: hull vertices of one LDS chunk (24 KiB)
#define OBB_NONE 0x7fffffff

// (value, row) a is better than b as a maximum / minimum: the value decides, then the lower row
__device__ __forceinline__ bool obb_more(double av, int ar, double bv, int br) { return av > bv || (av == bv && ar < br); }
__device__ __forceinline__ bool obb_less(double av, int ar, double bv, int br) { return av < bv || (av == bv && ar < br); }

__global__ void __launch_bounds__(OBB_THREADS)
k_obb_extremes(const float* __restrict__ points, int64_t N, const double* __restrict__ dirs, int K, double* __restrict__ part_val,
               int32_t* __restrict__ part_row) {
#pragma clang fp contract(fast)
  __shared__ float tile[OBB_TILE * 3];
  __shared__ double best_val[2][OBB_MAX_DIRS];
  __shared__ int32_t best_row[2][OBB_MAX_DIRS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int d = threadIdx.x; d < K; d += OBB_THREADS) {
    best_val[0][d] = -INFINITY; best_val[1][d] = INFINITY;
    best_row[0][d] = OBB_NONE; best_row[1][d] = OBB_NONE;
  }
  for (int64_t base = (int64_t)blockIdx.x * OBB_TILE; base < N; base += (int64_t)gridDim.x * OBB_TILE) {
    const int cnt = (int)(N - base < OBB_TILE ? N - base : OBB_TILE);
    __syncthreads();                                                   // the previous tile is read (and best_* is initialised)
    for (int i = threadIdx.x; i < cnt * 3; i += OBB_THREADS) tile[i] = points[base * 3 + i];
    __syncthreads();
    for (int g = wave * 4; g < K; g += 4 * (OBB_THREADS / 64)) {        // directions g .. g + 3: wave-uniform
      double dx[4], dy[4], dz[4], mx[4], mn[4];
      int mxr[4], mnr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = g + j < K ? g + j : K - 1;
        dx[j] = dirs[d * 3 + 0]; dy[j] = dirs[d * 3 + 1]; dz[j] = dirs[d * 3 + 2];
        mx[j] = -INFINITY; mn[j] = INFINITY; mxr[j] = OBB_NONE; mnr[j] = OBB_NONE;
      }
      for (int i = lane; i < cnt; i += 64) {                            // ascending rows: a strict comparison keeps the lower row
        const double x = tile[i * 3 + 0], y = tile[i * 3 + 1], z = tile[i * 3 + 2];
        const int row = (int)(base + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double v = x * dx[j] + y * dy[j] + z * dz[j];
          if (v > mx[j]) { mx[j] = v; mxr[j] = row; }
          if (v < mn[j]) { mn[j] = v; mnr[j] = row; }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double ov = __shfl_xor(mx[j], o, 64), uv = __shfl_xor(mn[j], o, 64);
          const int orow = __shfl_xor(mxr[j], o, 64), urow = __shfl_xor(mnr[j], o, 64);
          if (obb_more(ov, orow, mx[j], mxr[j])) { mx[j] = ov; mxr[j] = orow; }
          if (obb_less(uv, urow, mn[j], mnr[j])) { mn[j] = uv; mnr[j] = urow; }
        }
        if (lane == 0 && g + j < K) {                                   // this wave alone ever touches direction g + j of best_*
          const int d = g + j;
          if (obb_more(mx[j], mxr[j], best_val[0][d], best_row[0][d])) { best_val[0][d] = mx[j]; best_row[0][d] = mxr[j]; }
          if (obb_less(mn[j], mnr[j], best_val[1][d], best_row[1][d])) { best_val[1][d] = mn[j]; best_row[1][d] = mnr[j]; }
        }
      }
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < K; d += OBB_THREADS) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      part_val[((int64_t)blockIdx.x * K + d) * 2 + s] = best_val[s][d];
      part_row[((int64_t)blockIdx.x * K + d) * 2 + s] = best_row[s][d];
    }
  }
}

// one wave per direction over the nb partials
__global__ void __launch_bounds__(64)
k_obb_extremes_final(const double* __restrict__ part_val, const int32_t* __restrict__ part_row, int nb, int K, int32_t* __restrict__ rows_max,
                     int32_t* __restrict__ rows_min) {
  const int d = blockIdx.x, lane = threadIdx.x;
  double mx = -INFINITY, mn = INFINITY;
  int mxr = OBB_NONE, mnr = OBB_NONE;
  for (int b = lane; b < nb; b += 64) {
    const int64_t at = ((int64_t)b * K + d) * 2;
    if (obb_more(part_val[at], part_row[at], mx, mxr)) { mx = part_val[at]; mxr = part_row[at]; }
    if (obb_less(part_val[at + 1], part_row[at + 1], mn, mnr)) { mn = part_val[at + 1]; mnr = part_row[at + 1]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(mx, o, 64), uv = __shfl_xor(mn, o, 64);
    const int orow = __shfl_xor(mxr, o, 64), urow = __shfl_xor(mnr, o, 64);
    if (obb_more(ov, orow, mx, mxr)) { mx = ov; mxr = orow; }
    if (obb_less(uv, urow, mn, mnr)) { mn = uv; mnr = urow; }
  }
  if (lane == 0) {
    rows_max[d] = mxr == OBB_NONE ? -1 : mxr;
    rows_min[d] = mnr == OBB_NONE ? -1 : mnr;
  }
}

// the two bitmap words of a wave's 64 rows (rows at or beyond n carry keep = false)
__device__ __forceinline__ void obb_store_bits(bool keep, int64_t row0, int64_t words, uint32_t* __restrict__ bitmap, bool merge) {
  const unsigned long long bits = __ballot(keep);
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0) {
    const int64_t w = (row0 >> 5) + (lane >> 5);                        // row0: the first row of this wave, a multiple of 64
    if (w < words) {
      const uint32_t v = (uint32_t)(bits >> (lane & 32));
      bitmap[w] = merge ? (bitmap[w] | v) : v;
    }
  }
}

__global__ void __launch_bounds__(OBB_THREADS)
k_obb_filter(const float* __restrict__ points, int64_t N, const double* __restrict__ planes, int F, double tol, int64_t words,
             uint32_t* __restrict__ bitmap) {
#pragma clang fp contract(fast)
  __shared__ double pl[OBB_PLANE_CHUNK * 4];
  const int64_t tiles = (N + OBB_THREADS - 1) / OBB_THREADS;
  for (int f0 = 0; f0 < F; f0 += OBB_PLANE_CHUNK) {
    const int fn = F - f0 < OBB_PLANE_CHUNK ? F - f0 : OBB_PLANE_CHUNK;
    __syncthreads();
    for (int i = threadIdx.x; i < fn * 4; i += OBB_THREADS) pl[i] = planes[(int64_t)f0 * 4 + i];
    __syncthreads();
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {           // a tile always meets the same workgroup and lane: `merge` is plain
      const int64_t row = t * OBB_THREADS + threadIdx.x;
      bool keep = false;
      if (row < N) {
        const double x = points[row * 3 + 0], y = points[row * 3 + 1], z = points[row * 3 + 2];
        for (int f = 0; f < fn; ++f) {
          const double s = x * pl[f * 4 + 0] + y * pl[f * 4 + 1] + z * pl[f * 4 + 2] + pl[f * 4 + 3];
          keep |= !(s < -tol);                                           // on or above the plane, within tol of it, or not comparable
        }
      }
      obb_store_bits(keep, t * OBB_THREADS + (threadIdx.x & ~63), words, bitmap, f0 > 0);
    }
  }
}

struct ObbBox { double c[3], r[9], e[3]; };                             // center, R row-major (R[i][k] = component i of axis k), extent

__global__ void __launch_bounds__(OBB_THREADS)
k_obb_within(const float* __restrict__ points, int64_t M, ObbBox box, int64_t words, uint32_t* __restrict__ bitmap) {
  const int64_t tiles = (M + OBB_THREADS - 1) / OBB_THREADS;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t row = t * OBB_THREADS + threadIdx.x;
    bool keep = false;
    if (row < M) {
      const double dx = (double)points[row * 3 + 0] - box.c[0], dy = (double)points[row * 3 + 1] - box.c[1],
                   dz = (double)points[row * 3 + 2] - box.c[2];
      keep = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double q = (dx * box.r[k] + dy * box.r[3 + k]) + dz * box.r[6 + k];
        keep &= fabs(q) <= box.e[k] * 0.5;                               // inclusive; false for NaN
      }
    }
    obb_store_bits(keep, t * OBB_THREADS + (threadIdx.x & ~63), words, bitmap, false);
  }
}

// ---- the search -----------------------------------------------------------------------------------------------------------------------
struct ObbFrame { double a[3], u[3], v[3], w[3]; bool ok; };

__device__ __forceinline__ void obb_unit(double* x) {
  const double n = __dsqrt_rn((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  x[0] = x[0] / n; x[1] = x[1] / n; x[2] = x[2] / n;
}
__device__ __forceinline__ void obb_cross(const double* a, const double* b, double* out) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

// candidate 3 t + k: corners a, b, c of triangle t taken cyclically from corner k; u = unit(b - a), w = unit(u x (c - a)), v = unit(w x u)
__device__ __forceinline__ ObbFrame obb_frame(const double* __restrict__ verts, int H, const int32_t* __restrict__ tris, int cand) {
  ObbFrame f;
  const int t = cand / 3, k = cand - 3 * t;
  const int ia = tris[t * 3 + k], ib = tris[t * 3 + (k + 1) % 3], ic = tris[t * 3 + (k + 2) % 3];
  f.ok = ia >= 0 && ia < H && ib >= 0 && ib < H && ic >= 0 && ic < H;
  if (!f.ok) return f;
  double e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f.a[i] = verts[ia * 3 + i];
    f.u[i] = verts[ib * 3 + i] - f.a[i];
    e[i] = verts[ic * 3 + i] - f.a[i];
  }
  obb_unit(f.u);
  obb_cross(f.u, e, f.w);
  obb_unit(f.w);
  obb_cross(f.w, f.u, f.v);
  obb_unit(f.v);
  // an edge without a length or a triangle without an area has no frame (0 / 0): its volume is NaN, not the -inf of empty extents
  f.ok = isfinite(f.u[0]) && isfinite(f.u[1]) && isfinite(f.u[2]) && isfinite(f.v[0]) && isfinite(f.v[1]) && isfinite(f.v[2]) &&
         isfinite(f.w[0]) && isfinite(f.w[1]) && isfinite(f.w[2]);
  return f;
}

// q = R^T (p - a), folded into lo / hi
__device__ __forceinline__ void obb_project(const ObbFrame& f, double px, double py, double pz, double* lo, double* hi) {
  const double dx = px - f.a[0], dy = py - f.a[1], dz = pz - f.a[2];
  const double q0 = (dx * f.u[0] + dy * f.u[1]) + dz * f.u[2];
  const double q1 = (dx * f.v[0] + dy * f.v[1]) + dz * f.v[2];
  const double q2 = (dx * f.w[0] + dy * f.w[1]) + dz * f.w[2];
  lo[0] = fmin(lo[0], q0); hi[0] = fmax(hi[0], q0);
  lo[1] = fmin(lo[1], q1); hi[1] = fmax(hi[1], q1);
  lo[2] = fmin(lo[2], q2); hi[2] = fmax(hi[2], q2);
}

__global__ void __launch_bounds__(64)
k_obb_volumes(const double* __restrict__ verts, int H, const int32_t* __restrict__ tris, int ncand, double* __restrict__ volumes) {
  __shared__ double vt[OBB_VERT_CHUNK * 3];
  const int cand = blockIdx.x * 64 + threadIdx.x;
  const bool live = cand < ncand;
  ObbFrame f;
  f.ok = false;
  if (live) f = obb_frame(verts, H, tris, cand);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int h0 = 0; h0 < H; h0 += OBB_VERT_CHUNK) {
    const int hn = H - h0 < OBB_VERT_CHUNK ? H - h0 : OBB_VERT_CHUNK;
    __syncthreads();
    for (int i = threadIdx.x; i < hn * 3; i += 64) vt[i] = verts[(int64_t)h0 * 3 + i];
    __syncthreads();
    if (f.ok)
      for (int h = 0; h < hn; ++h) obb_project(f, vt[h * 3 + 0], vt[h * 3 + 1], vt[h * 3 + 2], lo, hi);   // broadcast reads
  }
  if (live) volumes[cand] = f.ok ? ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2]) : (double)NAN;
}

// one workgroup: the least (volume, index) pair (a NaN volume never wins), then the box of that candidate
__global__ void __launch_bounds__(OBB_THREADS)
k_obb_pick(const double* __restrict__ verts, int H, const int32_t* __restrict__ tris, int ncand, const double* __restrict__ volumes,
           int32_t* __restrict__ best_index, double* __restrict__ box) {
  __shared__ double s_val[OBB_THREADS / 64][6];
  __shared__ int s_idx[OBB_THREADS / 64];
  __shared__ int s_best;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double bv = INFINITY;
  int bi = OBB_NONE;
  for (int c = threadIdx.x; c < ncand; c += OBB_THREADS) {
    const double v = volumes[c];
    if (obb_less(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (obb_less(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { s_val[wave][0] = bv; s_idx[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OBB_THREADS / 64; ++w)
      if (obb_less(s_val[w][0], s_idx[w], bv, bi)) { bv = s_val[w][0]; bi = s_idx[w]; }
    s_best = bi;
  }
  __syncthreads();
  const int best = s_best;
  if (best == OBB_NONE) {                                               // no candidate with a comparable volume
    if (threadIdx.x == 0) *best_index = -1;
    if (threadIdx.x < 15) box[threadIdx.x] = 0.0;
    return;
  }
  const ObbFrame f = obb_frame(verts, H, tris, best);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int h = threadIdx.x; h < H; h += OBB_THREADS) obb_project(f, verts[h * 3 + 0], verts[h * 3 + 1], verts[h * 3 + 2], lo, hi);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o, 64));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o, 64));
    }
  }
  __syncthreads();                                                     // s_val[..][0] has been read
  if (lane == 0)
    for (int k = 0; k < 3; ++k) { s_val[wave][k] = lo[k]; s_val[wave][3 + k] = hi[k]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OBB_THREADS / 64; ++w)
      for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], s_val[w][k]); hi[k] = fmax(hi[k], s_val[w][3 + k]); }
    const double m0 = (lo[0] + hi[0]) * 0.5, m1 = (lo[1] + hi[1]) * 0.5, m2 = (lo[2] + hi[2]) * 0.5;
    for (int i = 0; i < 3; ++i) {
      box[i] = f.a[i] + ((f.u[i] * m0 + f.v[i] * m1) + f.w[i] * m2);
      box[3 + i * 3 + 0] = f.u[i]; box[3 + i * 3 + 1] = f.v[i]; box[3 + i * 3 + 2] = f.w[i];
      box[12 + i] = hi[i] - lo[i];
    }
    *best_index = best;
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
static inline int obb_extreme_groups(int64_t N) {
  const int64_t b = (N + OBB_TILE - 1) / OBB_TILE;
  return (int)(b < 1 ? 1 : b > OBB_MAX_WG ? OBB_MAX_WG : b);
}
static inline int obb_grid(int64_t items, int cap) {
  const int64_t b = (items + OBB_THREADS - 1) / OBB_THREADS;
  return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" size_t ss_obb_extremes_workspace_bytes(int64_t N, int K) {
  if (N < 1 || K < 1) return 0;
  return (size_t)obb_extreme_groups(N) * (size_t)K * 2 * (sizeof(double) + sizeof(int32_t));
}

extern "C" int ss_obb_extremes(const float* points, int64_t N, const double* dirs, int K, int32_t* rows_max, int32_t* rows_min,
                               void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (N < 1 || N >= (1ll << 31) || K < 1 || K > OBB_MAX_DIRS || !points || !dirs || !rows_max || !rows_min || !workspace) return SS_ERR_ARG;
  if (workspace_bytes < ss_obb_extremes_workspace_bytes(N, K)) return SS_ERR_WORKSPACE;
  const int nb = obb_extreme_groups(N);
  double* part_val = (double*)workspace;                                // (nb, K, 2) doubles, then (nb, K, 2) rows
  int32_t* part_row = (int32_t*)(part_val + (size_t)nb * K * 2);
  SS_LAUNCH(k_obb_extremes, dim3(nb), dim3(OBB_THREADS), 0, stream, points, N, dirs, K, part_val, part_row);
  SS_LAUNCH(k_obb_extremes_final, dim3(K), dim3(64), 0, stream, (const double*)part_val, (const int32_t*)part_row, nb, K, rows_max, rows_min);
  return SS_OK;
}

extern "C" int ss_obb_filter(const float* points, int64_t N, const double* planes, int F, const double* h_tol, uint32_t* bitmap,
                             hipStream_t stream) {
  if (N < 1 || N >= (1ll << 31) || F < 1 || !points || !planes || !h_tol || !bitmap || !(*h_tol >= 0.0)) return SS_ERR_ARG;
  SS_LAUNCH(k_obb_filter, dim3(obb_grid(N, 2048)), dim3(OBB_THREADS), 0, stream, points, N, planes, F, *h_tol, (N + 31) / 32, bitmap);
  return SS_OK;
}

extern "C" int ss_obb_search(const double* verts, int H, const int32_t* tris, int T, double* volumes, int32_t* best_index, double* box,
                             hipStream_t stream) {
  if (H < 1 || T < 1 || T > (1 << 29) || !verts || !tris || !volumes || !best_index || !box) return SS_ERR_ARG;
  const int ncand = 3 * T;
  SS_LAUNCH(k_obb_volumes, dim3((ncand + 63) / 64), dim3(64), 0, stream, verts, H, tris, ncand, volumes);
  SS_LAUNCH(k_obb_pick, dim3(1), dim3(OBB_THREADS), 0, stream, verts, H, tris, ncand, (const double*)volumes, best_index, box);
  return SS_OK;
}

extern "C" int ss_obb_within(const float* points, int64_t M, const double* h_box, uint32_t* bitmap, hipStream_t stream) {
  if (M < 0 || M >= (1ll << 31) || !h_box) return SS_ERR_ARG;
  if (M == 0) return SS_OK;
  if (!points || !bitmap) return SS_ERR_ARG;
  ObbBox box;
  for (int i = 0; i < 3; ++i) { box.c[i] = h_box[i]; box.e[i] = h_box[12 + i]; }
  for (int i = 0; i < 9; ++i) box.r[i] = h_box[3 + i];
  SS_LAUNCH(k_obb_within, dim3(obb_grid(M, 2048)), dim3(OBB_THREADS), 0, stream, points, M, box, (M + 31) / 32, bitmap);
  return SS_OK;
}
