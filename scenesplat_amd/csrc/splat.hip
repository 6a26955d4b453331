// Headless Gaussian-splat rendering (gfx950): the device side of DESIGN.md 8u.  A scene folder's rows (coord, scale, quat, opacity, colour)
// become an image by the standard EWA splatting steps: project, count (Gaussian, tile) pairs, sort them by (tile, depth), composite.
//
//   ss_splat_project     one lane per Gaussian: cull, 2-D covariance, conic, radius, mean, tile rectangle, tiles_touched
//   ss_splat_offsets     exclusive int64 scan of tiles_touched in two levels (block sums, a one-block finish, the add) + {P, visible}
//   ss_splat_keys        one lane per Gaussian: a key (tile << 32) | bits(depth) and the row per tile of its rectangle
//   ss_splat_ranges      [start, end) of each tile in the sorted keys; the sort's permutation gathers the rows
//   ss_splat_composite   one 256-thread workgroup per 16 x 16 tile, one pixel per lane, the tile's Gaussians through LDS 256 at a time
//
// Every fp32 operation below is rounded on its own, in the order DESIGN.md 8u states (contraction is off), so the projection differs
// from a numpy fp32 statement only where sqrt, division or expf do.  Nothing here uses an atomic; no workgroup waits on another.
// Forward only, nothing tuned: exp2 with a prescaled conic, per-tile load balancing and 32-wide staging are what comes next
// (profiles/splat_render.md).
#include "common.h"
#include <string.h>

#pragma clang fp contract(off)

#define SP_THREADS 256
#define SP_SCAN_ITEMS 8
static_assert(SS_SPLAT_SCAN_ROWS == SP_THREADS * SP_SCAN_ITEMS, "a scan block is 8 rows per lane");
static_assert(SS_SPLAT_TILE * SS_SPLAT_TILE == SP_THREADS && SS_SPLAT_BATCH == SP_THREADS, "a lane per pixel, a staged Gaussian per lane");
static_assert(SS_SPLAT_CAMERA_WORDS >= 21, "camera block");

// the packed camera block (SS_SPLAT_CAMERA_WORDS 32-bit words on the host), as a kernel argument
struct SplatCam {
  float R[9], t[3];
  float fx, fy, cx, cy, near_z, limx, limy;
  int32_t width, height;
  int32_t pad[SS_SPLAT_CAMERA_WORDS - 21];
};
static_assert(sizeof(SplatCam) == SS_SPLAT_CAMERA_WORDS * 4, "camera block");

static bool splat_cam_ok(const void* h_camera, const SplatCam& c) {
  if (c.width < 1 || c.width > SS_SPLAT_MAX_DIM || c.height < 1 || c.height > SS_SPLAT_MAX_DIM) return false;
  float f[19];                                                          // the block's float words
  memcpy(f, h_camera, sizeof(f));
  for (int i = 0; i < 19; ++i)
    if (!(fabsf(f[i]) < INFINITY)) return false;
  return c.fx > 0.f && c.fy > 0.f && c.near_z > 0.f && c.limx > 0.f && c.limy > 0.f;
}
static bool splat_n_ok(int64_t N) { return N >= 1 && N < (1LL << 31); }
static int splat_tiles_x(const SplatCam& c) { return (c.width + SS_SPLAT_TILE - 1) / SS_SPLAT_TILE; }
static int splat_tiles_y(const SplatCam& c) { return (c.height + SS_SPLAT_TILE - 1) / SS_SPLAT_TILE; }

__device__ __forceinline__ bool sp_finite(float v) { return fabsf(v) < INFINITY; }   // false for NaN too

// ---- projection -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
k_splat_project(const float* __restrict__ coord, const float* __restrict__ scale, const float* __restrict__ quat,
                const float* __restrict__ opacity, const float* __restrict__ color, int64_t n, SplatCam cam, int mode, float scale_modifier,
                float point_size, int tiles_x, int tiles_y, float2* __restrict__ mean2d, float4* __restrict__ conic_opacity,
                float* __restrict__ depth, int4* __restrict__ rect, int32_t* __restrict__ radius, int32_t* __restrict__ tiles_touched) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n) return;
  float2 m2 = make_float2(0.f, 0.f);
  float4 co = make_float4(0.f, 0.f, 0.f, 0.f);
  float z_out = 0.f;
  int4 rc = make_int4(0, 0, 0, 0);
  int rad = 0, touched = 0;
  do {
    const float px = coord[3 * g], py = coord[3 * g + 1], pz = coord[3 * g + 2];
    const float s0 = scale[3 * g], s1 = scale[3 * g + 1], s2 = scale[3 * g + 2];
    const float qw = quat[4 * g], qx = quat[4 * g + 1], qy = quat[4 * g + 2], qz = quat[4 * g + 3];
    float o = opacity[g];
    const float c0 = color[3 * g], c1 = color[3 * g + 1], c2 = color[3 * g + 2];
    // 1. cull
    if (!(sp_finite(px) && sp_finite(py) && sp_finite(pz) && sp_finite(s0) && sp_finite(s1) && sp_finite(s2) && sp_finite(qw) &&
          sp_finite(qx) && sp_finite(qy) && sp_finite(qz) && sp_finite(o) && sp_finite(c0) && sp_finite(c1) && sp_finite(c2)))
      break;
    const float qn = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    if (!(qn > 0.f)) break;
    const float* R = cam.R;
    const float x = ((R[0] * px + R[1] * py) + R[2] * pz) + cam.t[0];
    const float y = ((R[3] * px + R[4] * py) + R[5] * pz) + cam.t[1];
    const float z = ((R[6] * px + R[7] * py) + R[8] * pz) + cam.t[2];
    if (!(z > cam.near_z)) break;
    const float xz = x / z, yz = y / z;
    float a, b, c;
    if (mode == SS_SPLAT_MODE_POINTCLOUD) {
      const float k = point_size / 3.0f;
      a = k * k; b = 0.f; c = a; o = 1.f;
    } else {
      // 2. W = R Rot(q / |q|), B = W diag(s): the 3-D covariance in camera axes is B B^T
      const float w_ = qw / qn, x_ = qx / qn, y_ = qy / qn, z_ = qz / qn;
      const float r00 = 1.f - 2.f * (y_ * y_ + z_ * z_), r01 = 2.f * (x_ * y_ - w_ * z_), r02 = 2.f * (x_ * z_ + w_ * y_);
      const float r10 = 2.f * (x_ * y_ + w_ * z_), r11 = 1.f - 2.f * (x_ * x_ + z_ * z_), r12 = 2.f * (y_ * z_ - w_ * x_);
      const float r20 = 2.f * (x_ * z_ - w_ * y_), r21 = 2.f * (y_ * z_ + w_ * x_), r22 = 1.f - 2.f * (x_ * x_ + y_ * y_);
      const float e0 = s0 * scale_modifier, e1 = s1 * scale_modifier, e2 = s2 * scale_modifier;
      float B[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        B[i][0] = ((R[3 * i] * r00 + R[3 * i + 1] * r10) + R[3 * i + 2] * r20) * e0;
        B[i][1] = ((R[3 * i] * r01 + R[3 * i + 1] * r11) + R[3 * i + 2] * r21) * e1;
        B[i][2] = ((R[3 * i] * r02 + R[3 * i + 1] * r12) + R[3 * i + 2] * r22) * e2;
      }
      // 3. A = J B with the clamped x/z, y/z; Sigma' = A A^T + 0.3 I
      const float tx = fminf(cam.limx, fmaxf(-cam.limx, xz)), ty = fminf(cam.limy, fmaxf(-cam.limy, yz));
      const float j00 = cam.fx / z, j02 = -(j00 * tx), j11 = cam.fy / z, j12 = -(j11 * ty);
      const float a0 = j00 * B[0][0] + j02 * B[2][0], a1 = j00 * B[0][1] + j02 * B[2][1], a2 = j00 * B[0][2] + j02 * B[2][2];
      const float b0 = j11 * B[1][0] + j12 * B[2][0], b1 = j11 * B[1][1] + j12 * B[2][1], b2 = j11 * B[1][2] + j12 * B[2][2];
      a = ((a0 * a0 + a1 * a1) + a2 * a2) + 0.3f;
      b = (a0 * b0 + a1 * b1) + a2 * b2;
      c = ((b0 * b0 + b1 * b1) + b2 * b2) + 0.3f;
    }
    const float det = a * c - b * b;
    if (!(det > 0.f)) break;
    // 4. conic, radius, mean
    const float inv = 1.f / det;
    const float ca = c * inv, cb = -(b * inv), cc = a * inv;
    const float mid = 0.5f * (a + c);
    const float lambda = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float r = ceilf(3.f * sqrtf(lambda));
    const float mx = cam.fx * xz + cam.cx, my = cam.fy * yz + cam.cy;
    if (!(sp_finite(mx) && sp_finite(my) && sp_finite(r) && sp_finite(ca) && sp_finite(cb) && sp_finite(cc))) break;
    // 5. tile rectangle, clamped as floats (a radius may exceed any integer)
    const float fx0 = fminf(fmaxf(floorf((mx - r) / 16.f), 0.f), (float)tiles_x);
    const float fy0 = fminf(fmaxf(floorf((my - r) / 16.f), 0.f), (float)tiles_y);
    const float fx1 = fminf(fmaxf(floorf(((mx + r) + 15.f) / 16.f), 0.f), (float)tiles_x);
    const float fy1 = fminf(fmaxf(floorf(((my + r) + 15.f) / 16.f), 0.f), (float)tiles_y);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = (int)fx1, y1 = (int)fy1;
    if (x1 <= x0 || y1 <= y0) break;
    m2 = make_float2(mx, my);
    co = make_float4(ca, cb, cc, o);
    z_out = z;
    rc = make_int4(x0, y0, x1, y1);
    rad = (int)fminf(r, 1073741824.f);
    touched = (x1 - x0) * (y1 - y0);
  } while (0);
  mean2d[g] = m2;
  conic_opacity[g] = co;
  depth[g] = z_out;
  rect[g] = rc;
  if (radius) radius[g] = rad;
  tiles_touched[g] = touched;
}

extern "C" int ss_splat_project(const float* coord, const float* scale, const float* quat, const float* opacity, const float* color,
                                int64_t N, const void* h_camera, int mode, float scale_modifier, float point_size, float* mean2d,
                                float* conic_opacity, float* depth, int32_t* rect, int32_t* radius, int32_t* tiles_touched,
                                hipStream_t stream) {
  if (!coord || !scale || !quat || !opacity || !color || !h_camera || !mean2d || !conic_opacity || !depth || !rect || !tiles_touched ||
      !splat_n_ok(N))
    return SS_ERR_ARG;
  if (mode != SS_SPLAT_MODE_GAUSSIANS && mode != SS_SPLAT_MODE_POINTCLOUD) return SS_ERR_ARG;
  if (!(fabsf(scale_modifier) < INFINITY) || !(point_size > 0.f) || !(point_size < INFINITY)) return SS_ERR_ARG;
  SplatCam cam;
  memcpy(&cam, h_camera, sizeof(cam));
  if (!splat_cam_ok(h_camera, cam)) return SS_ERR_ARG;
  SS_LAUNCH(k_splat_project, dim3(ss_div_up(N, SP_THREADS)), dim3(SP_THREADS), 0, stream, coord, scale, quat, opacity, color, N, cam, mode,
            scale_modifier, point_size, splat_tiles_x(cam), splat_tiles_y(cam), reinterpret_cast<float2*>(mean2d),
            reinterpret_cast<float4*>(conic_opacity), depth, reinterpret_cast<int4*>(rect), radius, tiles_touched);
  return SS_OK;
}

// ---- pair offsets -----------------------------------------------------------------------------------------------------------------
// A block of SS_SPLAT_SCAN_ROWS rows sums below 2^31 (a row touches at most 2^16 tiles), so the work inside a block is 32-bit.
__device__ __forceinline__ uint32_t sp_block_exclusive(uint32_t v, uint32_t* wave_sum /*[4]*/, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
  __syncthreads();                                                      // an earlier call's reads of wave_sum are over
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < SP_THREADS / 64; ++w) { const uint32_t s = wave_sum[w]; if (w < wave) before += s; all += s; }
  *total = all;
  return before + inc - v;
}

__global__ void __launch_bounds__(SP_THREADS)
k_splat_block_sums(const int32_t* __restrict__ touched, int64_t n, int64_t* __restrict__ sums, int64_t* __restrict__ visible) {
  __shared__ uint32_t ws[SP_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * SS_SPLAT_SCAN_ROWS;
  uint32_t s = 0, c = 0;
#pragma unroll
  for (int k = 0; k < SP_SCAN_ITEMS; ++k) {
    const int64_t i = base + k * SP_THREADS + threadIdx.x;
    const int32_t v = i < n ? touched[i] : 0;
    if (v > 0) { s += (uint32_t)v; ++c; }
  }
  uint32_t ts, tc;
  sp_block_exclusive(s, ws, &ts);
  sp_block_exclusive(c, ws, &tc);
  if (threadIdx.x == 0) { sums[blockIdx.x] = (int64_t)ts; visible[blockIdx.x] = (int64_t)tc; }
}

// one workgroup: sums -> their exclusive running sum in place, pieces of 256 with a carry; totals = {P, visible rows}
__global__ void __launch_bounds__(SP_THREADS)
k_splat_scan_sums(int64_t* __restrict__ sums, const int64_t* __restrict__ visible, int nblocks, int64_t* __restrict__ totals) {
  __shared__ int64_t sh[SP_THREADS];
  __shared__ int64_t shv[SP_THREADS];
  int64_t carry = 0, vis = 0;
  for (int base = 0; base < nblocks; base += SP_THREADS) {
    const int i = base + threadIdx.x;
    const int64_t x = i < nblocks ? sums[i] : 0;
    __syncthreads();
    sh[threadIdx.x] = x;
    shv[threadIdx.x] = i < nblocks ? visible[i] : 0;
    __syncthreads();
    int64_t before = 0, all = 0, allv = 0;
    for (int j = 0; j < SP_THREADS; ++j) { const int64_t s = sh[j]; if (j < (int)threadIdx.x) before += s; all += s; allv += shv[j]; }
    if (i < nblocks) sums[i] = carry + before;
    carry += all; vis += allv;
  }
  if (threadIdx.x == 0) { totals[0] = carry; totals[1] = vis; }
}

__global__ void __launch_bounds__(SP_THREADS)
k_splat_offsets_add(const int32_t* __restrict__ touched, int64_t n, const int64_t* __restrict__ sums, int64_t* __restrict__ offsets) {
  __shared__ uint32_t ws[SP_THREADS / 64];
  const int64_t first = (int64_t)blockIdx.x * SS_SPLAT_SCAN_ROWS + (int64_t)threadIdx.x * SP_SCAN_ITEMS;
  uint32_t v[SP_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < SP_SCAN_ITEMS; ++k) {
    const int32_t t = first + k < n ? touched[first + k] : 0;
    v[k] = t > 0 ? (uint32_t)t : 0u;
    s += v[k];
  }
  uint32_t total;
  uint32_t run = sp_block_exclusive(s, ws, &total);
  const int64_t base = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SP_SCAN_ITEMS; ++k) {
    if (first + k < n) offsets[first + k] = base + (int64_t)run;
    run += v[k];
  }
}

extern "C" size_t ss_splat_offsets_workspace_bytes(int64_t N) {
  if (!splat_n_ok(N)) return 0;
  return (size_t)ss_div_up(N, SS_SPLAT_SCAN_ROWS) * 2 * sizeof(int64_t);
}

extern "C" int ss_splat_offsets(const int32_t* tiles_touched, int64_t N, int64_t* offsets, int64_t* totals, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
  if (!tiles_touched || !offsets || !totals || !splat_n_ok(N)) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_splat_offsets_workspace_bytes(N)) return SS_ERR_WORKSPACE;
  const int nblocks = ss_div_up(N, SS_SPLAT_SCAN_ROWS);
  int64_t* sums = static_cast<int64_t*>(workspace);
  int64_t* visible = sums + nblocks;
  SS_LAUNCH(k_splat_block_sums, dim3(nblocks), dim3(SP_THREADS), 0, stream, tiles_touched, N, sums, visible);
  SS_LAUNCH(k_splat_scan_sums, dim3(1), dim3(SP_THREADS), 0, stream, sums, (const int64_t*)visible, nblocks, totals);
  SS_LAUNCH(k_splat_offsets_add, dim3(nblocks), dim3(SP_THREADS), 0, stream, tiles_touched, N, (const int64_t*)sums, offsets);
  return SS_OK;
}

// ---- keys -------------------------------------------------------------------------------------------------------------------------
// the bits of a positive finite fp32 depth order as integers
__global__ void __launch_bounds__(SP_THREADS)
k_splat_keys(const float* __restrict__ depth, const int4* __restrict__ rect, const int32_t* __restrict__ touched,
             const int64_t* __restrict__ offsets, int64_t n, int64_t P, int tiles_x, int64_t* __restrict__ keys,
             int32_t* __restrict__ rows) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n || touched[g] <= 0) return;
  const int4 rc = rect[g];
  const uint32_t zb = __float_as_uint(depth[g]);
  int64_t off = offsets[g];
  for (int ty = rc.y; ty < rc.w; ++ty)
    for (int tx = rc.x; tx < rc.z; ++tx) {
      if (off < 0 || off >= P) return;                                  // the one guard: no write outside keys / rows
      keys[off] = (int64_t)(((uint64_t)(uint32_t)(ty * tiles_x + tx) << 32) | zb);
      rows[off] = (int32_t)g;
      ++off;
    }
}

extern "C" int ss_splat_keys(const float* depth, const int32_t* rect, const int32_t* tiles_touched, const int64_t* offsets, int64_t N,
                             int64_t P, int tiles_x, int tiles_y, int64_t* keys, int32_t* rows, hipStream_t stream) {
  if (!depth || !rect || !tiles_touched || !offsets || !keys || !rows || !splat_n_ok(N) || P < 1 || P >= (1LL << 31)) return SS_ERR_ARG;
  if (tiles_x < 1 || tiles_y < 1 || tiles_x > SS_SPLAT_MAX_DIM / SS_SPLAT_TILE || tiles_y > SS_SPLAT_MAX_DIM / SS_SPLAT_TILE) return SS_ERR_ARG;
  SS_LAUNCH(k_splat_keys, dim3(ss_div_up(N, SP_THREADS)), dim3(SP_THREADS), 0, stream, depth, reinterpret_cast<const int4*>(rect),
            tiles_touched, offsets, N, P, tiles_x, keys, rows);
  return SS_OK;
}

// ---- tile ranges ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS) k_splat_ranges_clear(int32_t* __restrict__ ranges, int words) {
  const int i = blockIdx.x * SP_THREADS + threadIdx.x;
  if (i < words) ranges[i] = 0;
}

__global__ void __launch_bounds__(SP_THREADS)
k_splat_ranges(const int64_t* __restrict__ sorted_keys, const int32_t* __restrict__ order, const int32_t* __restrict__ rows, int64_t P,
               int num_tiles, int32_t* __restrict__ ranges, int32_t* __restrict__ sorted_rows) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= P) return;
  const int32_t src = order[i];
  sorted_rows[i] = rows[src];
  const uint32_t tile = (uint32_t)((uint64_t)sorted_keys[i] >> 32);
  if (tile >= (uint32_t)num_tiles) return;
  if (i == 0 || (uint32_t)((uint64_t)sorted_keys[i - 1] >> 32) != tile) ranges[2 * tile] = (int32_t)i;
  if (i == P - 1 || (uint32_t)((uint64_t)sorted_keys[i + 1] >> 32) != tile) ranges[2 * tile + 1] = (int32_t)(i + 1);
}

extern "C" int ss_splat_ranges(const int64_t* sorted_keys, const int32_t* order, const int32_t* rows, int64_t P, int num_tiles,
                               int32_t* ranges, int32_t* sorted_rows, hipStream_t stream) {
  const int max_tiles = (SS_SPLAT_MAX_DIM / SS_SPLAT_TILE) * (SS_SPLAT_MAX_DIM / SS_SPLAT_TILE);
  if (!sorted_keys || !order || !rows || !ranges || !sorted_rows || P < 1 || P >= (1LL << 31) || num_tiles < 1 || num_tiles > max_tiles)
    return SS_ERR_ARG;
  SS_LAUNCH(k_splat_ranges_clear, dim3(ss_div_up(2 * num_tiles, SP_THREADS)), dim3(SP_THREADS), 0, stream, ranges, 2 * num_tiles);
  SS_LAUNCH(k_splat_ranges, dim3(ss_div_up(P, SP_THREADS)), dim3(SP_THREADS), 0, stream, sorted_keys, order, rows, P, num_tiles, ranges,
            sorted_rows);
  return SS_OK;
}

// ---- composite --------------------------------------------------------------------------------------------------------------------
struct SplatBg { float c[3]; };

__global__ void __launch_bounds__(SP_THREADS)
k_splat_composite(const float2* __restrict__ mean2d, const float4* __restrict__ conic_opacity, const float* __restrict__ color,
                  const float* __restrict__ depth, const int32_t* __restrict__ ranges, const int32_t* __restrict__ sorted_rows,
                  int width, int height, int tiles_x, SplatBg bg, float* __restrict__ image, float* __restrict__ alpha_out,
                  float* __restrict__ depth_out) {
  // 40 bytes per staged Gaussian
  __shared__ float2 s_mean[SS_SPLAT_BATCH];
  __shared__ float4 s_co[SS_SPLAT_BATCH];
  __shared__ float s_col[SS_SPLAT_BATCH][3];
  __shared__ float s_z[SS_SPLAT_BATCH];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int px_i = (tile % tiles_x) * SS_SPLAT_TILE + (tid & (SS_SPLAT_TILE - 1));
  const int py_i = (tile / tiles_x) * SS_SPLAT_TILE + (tid / SS_SPLAT_TILE);
  const bool inside = px_i < width && py_i < height;
  const float pxf = (float)px_i + 0.5f, pyf = (float)py_i + 0.5f;
  const int64_t start = ranges[2 * tile], end = ranges[2 * tile + 1];
  float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Z = 0.f;
  bool done = !inside;
  for (int64_t b0 = start; b0 < end; b0 += SS_SPLAT_BATCH) {
    // (a barrier too: the reads of the batch before are over)
    if (__syncthreads_and(done ? 1 : 0)) break;
    const int64_t i = b0 + tid;
    if (i < end) {
      const int64_t g = sorted_rows[i];
      s_mean[tid] = mean2d[g];
      s_co[tid] = conic_opacity[g];
      s_col[tid][0] = color[3 * g]; s_col[tid][1] = color[3 * g + 1]; s_col[tid][2] = color[3 * g + 2];
      s_z[tid] = depth[g];
    }
    __syncthreads();
    const int count = (int)(end - b0 < SS_SPLAT_BATCH ? end - b0 : SS_SPLAT_BATCH);
    for (int j = 0; j < count && !done; ++j) {
      const float2 m = s_mean[j];
      const float4 co = s_co[j];
      const float dx = m.x - pxf, dy = m.y - pyf;
      const float power = -0.5f * ((co.x * dx) * dx + (co.z * dy) * dy) - (co.y * dx) * dy;
      if (!(power <= 0.f)) continue;                                    // (NaN too)
      const float a = fminf(0.99f, co.w * expf(power));
      if (a < 1.f / 255.f) continue;
      const float Tn = T * (1.f - a);
      if (Tn < 1e-4f) { done = true; continue; }
      const float w = a * T;
      C0 = C0 + s_col[j][0] * w; C1 = C1 + s_col[j][1] * w; C2 = C2 + s_col[j][2] * w;
      Z = Z + s_z[j] * w;
      T = Tn;
    }
  }
  if (inside) {
    const int64_t p = (int64_t)py_i * width + px_i;
    image[3 * p] = C0 + T * bg.c[0]; image[3 * p + 1] = C1 + T * bg.c[1]; image[3 * p + 2] = C2 + T * bg.c[2];
    alpha_out[p] = 1.f - T;
    depth_out[p] = Z;
  }
}

extern "C" int ss_splat_composite(const float* mean2d, const float* conic_opacity, const float* color, const float* depth,
                                  const int32_t* ranges, const int32_t* sorted_rows, int64_t N, int64_t P, int width, int height,
                                  const float* h_background, float* image, float* alpha, float* depth_out, hipStream_t stream) {
  if (!mean2d || !conic_opacity || !color || !depth || !ranges || !sorted_rows || !h_background || !image || !alpha || !depth_out ||
      !splat_n_ok(N) || P < 1 || P >= (1LL << 31))
    return SS_ERR_ARG;
  if (width < 1 || width > SS_SPLAT_MAX_DIM || height < 1 || height > SS_SPLAT_MAX_DIM) return SS_ERR_ARG;
  SplatBg bg;
  for (int k = 0; k < 3; ++k) {
    bg.c[k] = h_background[k];
    if (!(fabsf(bg.c[k]) < INFINITY)) return SS_ERR_ARG;
  }
  const int tiles_x = (width + SS_SPLAT_TILE - 1) / SS_SPLAT_TILE, tiles_y = (height + SS_SPLAT_TILE - 1) / SS_SPLAT_TILE;
  SS_LAUNCH(k_splat_composite, dim3(tiles_x * tiles_y), dim3(SP_THREADS), 0, stream, reinterpret_cast<const float2*>(mean2d),
            reinterpret_cast<const float4*>(conic_opacity), color, depth, ranges, sorted_rows, width, height, tiles_x, bg, image,
            alpha, depth_out);
  return SS_OK;
}
