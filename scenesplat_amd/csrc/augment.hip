// Per-sample Gaussian augmentations on the device: the head of the training transform list (CenterShift ... ChromaticJitter,
// pointcept/datasets/transform.py:446-816,1120-1178) that every shipped lang-pretrain / semseg-gs config runs in front of GridSample.
// Four HBM-bound one-pass kernels, fp32, in place; the host (pointcept_api/transform.py) draws the random parameters, composes
// the rigid ops into ONE affine + quaternion + reflection and hands them over as kernel arguments, so nothing but the per-point
// arrays is read from memory.  One thread per point, grid-stride, at most AUG_MAX_BLOCKS workgroups.
// Behind them the kernels of the transforms outside the shipped lists (transform.py:423-434, 1035-1100, 1620-1664): the fp64 HSV round
// trip of HueSaturationTranslation, the fp64 moments NormalizeCoord folds into the pending affine, and InstanceParser's per-instance
// boxes and centroids over a sorted CSR (one workgroup per instance).  No float atomics: every result is the same on every run.
#include "common.h"
#include <math.h>

namespace {

constexpr int AUG_BLOCK = 256;
// Workgroup cap, four per CU.  profiles/augment_chain.md compares 256 / 1,024 / 2,048: one wave per SIMD leaves the full pass waiting on
// its own loads, 2,048 partials double the one-wave finish of the box.  SS_EXTRA_HIPCC_FLAGS=-DSS_AUG_MAX_BLOCKS=n builds another cap.
#ifndef SS_AUG_MAX_BLOCKS
#define SS_AUG_MAX_BLOCKS 1024
#endif
constexpr int AUG_MAX_BLOCKS = SS_AUG_MAX_BLOCKS;
constexpr int AUG_WAVES = AUG_BLOCK / 64;

struct Affine { float a[9]; float b[3]; };       // y = A x + b, A row-major
struct Vec3 { float v[3]; };

inline int aug_blocks(int64_t n) {
  const int64_t b = (n + AUG_BLOCK - 1) / AUG_BLOCK;
  return (int)(b < 1 ? 1 : (b > AUG_MAX_BLOCKS ? AUG_MAX_BLOCKS : b));
}

// the ONE form of A x + b both ss_aug_bbox and ss_aug_gaussians evaluate: the box of a pending affine is the box of the flushed coordinates
__device__ __forceinline__ void affine_apply(const Affine& f, float (&p)[3]) {
  const float x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = fmaf(f.a[3 * i + 2], z, fmaf(f.a[3 * i + 1], y, fmaf(f.a[3 * i], x, f.b[i])));
}

__device__ __forceinline__ float wave_reduce_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// three N(0,1) draws of point i: Philox4x32-10 under the 64-bit seed, counter (i, stream), Box-Muller on the four words
__device__ __forceinline__ void normal3(uint64_t seed, int64_t i, uint32_t stream, float (&z)[3]) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), stream, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float k = 1.0f / 16777216.0f;
  const float u0 = (float)((c[0] >> 8) + 1u) * k, u1 = (float)(c[1] >> 8) * k;      // u0, u2 in (0, 1]: log stays finite
  const float u2 = (float)((c[2] >> 8) + 1u) * k, u3 = (float)(c[3] >> 8) * k;
  const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
  float s0, c0;
  sincospif(2.0f * u1, &s0, &c0);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * cospif(2.0f * u3);
}

// ---- bounding box ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_bbox(const float* __restrict__ x, int64_t n, Affine af, int use_affine, float* __restrict__ partials) {
  __shared__ float red[AUG_WAVES][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
    if (use_affine) affine_apply(af, p);
#pragma unroll
    for (int j = 0; j < 3; ++j) { lo[j] = fminf(lo[j], p[j]); hi[j] = fmaxf(hi[j], p[j]); }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float l = wave_reduce_min(lo[j]), h = wave_reduce_max(hi[j]);
    if (lane == 0) { red[wave][j] = l; red[wave][3 + j] = h; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[0][threadIdx.x];
    for (int w = 1; w < AUG_WAVES; ++w) v = threadIdx.x < 3 ? fminf(v, red[w][threadIdx.x]) : fmaxf(v, red[w][threadIdx.x]);
    partials[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

// one wave: lane -> partial rows lane, lane + 64, ...; min and max are exact, so the order of the reduction does not show
__global__ void __launch_bounds__(64)
k_aug_bbox_finish(const float* __restrict__ partials, int nb, float* __restrict__ out6) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float v = j < 3 ? INFINITY : -INFINITY;
    for (int b = threadIdx.x; b < nb; b += 64) v = j < 3 ? fminf(v, partials[b * 6 + j]) : fmaxf(v, partials[b * 6 + j]);
    v = j < 3 ? wave_reduce_min(v) : wave_reduce_max(v);
    if (threadIdx.x == 0) out6[j] = v;
  }
}

// ---- the fused rigid pass -------------------------------------------------------------------------------------------------------
struct GaussParams {
  Affine af;
  float rq[4];        // w x y z
  float smul[3];
  float lin[9];
  int use_affine, use_rq, flip, jitter;
  float sigma, clip;
  uint64_t seed;
};

__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_gaussians(float* __restrict__ coord, float* __restrict__ quat, float* __restrict__ scale, float* __restrict__ normal, int64_t n,
                GaussParams P, const float* __restrict__ noise) {
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    if (coord) {
      float p[3] = {coord[3 * i], coord[3 * i + 1], coord[3 * i + 2]};
      if (P.use_affine) affine_apply(P.af, p);
      if (P.jitter) {
        float z[3];
        if (noise) { z[0] = noise[3 * i]; z[1] = noise[3 * i + 1]; z[2] = noise[3 * i + 2]; }
        else normal3(P.seed, i, 0u, z);
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] += fminf(fmaxf(P.sigma * z[j], -P.clip), P.clip);
      }
      coord[3 * i] = p[0]; coord[3 * i + 1] = p[1]; coord[3 * i + 2] = p[2];
    }
    if (quat) {
      const float4 q4 = reinterpret_cast<const float4*>(quat)[i];
      float w = q4.x, x = q4.y, y = q4.z, z = q4.w;
      const float n2 = w * w + x * x + y * y + z * z;
      if (n2 > 0.0f) {                                   // zero-norm rows (and NaN rows) stay as they are
        const float inv = 1.0f / sqrtf(n2);
        w *= inv; x *= inv; y *= inv; z *= inv;
        if (P.use_rq) {                                  // r (x) q
          const float rw = P.rq[0], rx = P.rq[1], ry = P.rq[2], rz = P.rq[3];
          const float nw = rw * w - rx * x - ry * y - rz * z;
          const float nx = rw * x + rx * w + ry * z - rz * y;
          const float ny = rw * y - rx * z + ry * w + rz * x;
          const float nz = rw * z + rx * y - ry * x + rz * w;
          w = nw; x = nx; y = ny; z = nz;
        }
        if (P.flip) {
          // F R F on the quaternion: a reflection of an axis negates the two OTHER vector components
          if (P.flip & 1) { y = -y; z = -z; }
          if (P.flip & 2) { x = -x; z = -z; }
          // scipy's from_matrix takes the branch arg-max [M00, M11, M22, trace] and leaves that component positive; for a unit
          // quaternion M00 - M11 = 2 (x^2 - y^2), M00 - trace = 2 (x^2 - w^2), ...: the first largest of x^2, y^2, z^2, w^2
          const float c[4] = {x, y, z, w};
          int best = 0;
          float bv = x * x;
#pragma unroll
          for (int j = 1; j < 4; ++j) { const float v = c[j] * c[j]; if (v > bv) { bv = v; best = j; } }
          const float lead = best == 0 ? x : (best == 1 ? y : (best == 2 ? z : w));
          if (lead < 0.0f) { w = -w; x = -x; y = -y; z = -z; }
        }
        reinterpret_cast<float4*>(quat)[i] = make_float4(w, x, y, z);
      }
    }
    if (scale) {
#pragma unroll
      for (int j = 0; j < 3; ++j) scale[3 * i + j] *= P.smul[j];
    }
    if (normal) {
      const float a = normal[3 * i], b = normal[3 * i + 1], c = normal[3 * i + 2];
#pragma unroll
      for (int j = 0; j < 3; ++j) normal[3 * i + j] = fmaf(P.lin[3 * j + 2], c, fmaf(P.lin[3 * j + 1], b, P.lin[3 * j] * a));
    }
  }
}

// ---- elastic distortion ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_elastic(float* __restrict__ coord, int64_t n, const float* __restrict__ noise, int d0, int d1, int d2, Vec3 origin, float gran,
              float magnitude) {
  const int d[3] = {d0, d1, d2};
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    float p[3] = {coord[3 * i], coord[3 * i + 1], coord[3 * i + 2]};
    int c0[3];
    float f[3];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float t = (p[j] - origin.v[j]) / gran;
      inside = inside && t >= 0.0f && t <= (float)(d[j] - 1);       // false for NaN as well
      const int c = min(max((int)floorf(t), 0), d[j] - 2);          // the last node belongs to the last cell (f = 1)
      c0[j] = c; f[j] = t - (float)c;
    }
    if (!inside) continue;                                          // fill value 0: no displacement
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
      const float w = (dx ? f[0] : 1.0f - f[0]) * (dy ? f[1] : 1.0f - f[1]) * (dz ? f[2] : 1.0f - f[2]);
      const float* g = noise + (((int64_t)(c0[0] + dx) * d1 + (c0[1] + dy)) * d2 + (c0[2] + dz)) * 3;
      acc[0] = fmaf(w, g[0], acc[0]); acc[1] = fmaf(w, g[1], acc[1]); acc[2] = fmaf(w, g[2], acc[2]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) coord[3 * i + j] = fmaf(acc[j], magnitude, p[j]);
  }
}

// ---- colour ---------------------------------------------------------------------------------------------------------------------
struct ColorParams {
  float lo[3], cscale[3], tr[3];     // cscale = 255 / (hi - lo)
  int flags, normalize;
  float blend, jitter_scale;        // jitter_scale = std * 255
  uint64_t seed;
};

__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_color(float* __restrict__ color, int64_t n, ColorParams P, const float* __restrict__ noise) {
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    float c[3] = {color[3 * i], color[3 * i + 1], color[3 * i + 2]};
    if (P.flags & 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = (1.0f - P.blend) * c[j] + P.blend * ((c[j] - P.lo[j]) * P.cscale[j]);
    }
    if (P.flags & 2) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = fminf(fmaxf(c[j] + P.tr[j], 0.0f), 255.0f);
    }
    if (P.flags & 4) {
      float z[3];
      if (noise) { z[0] = noise[3 * i]; z[1] = noise[3 * i + 1]; z[2] = noise[3 * i + 2]; }
      else normal3(P.seed, i, 1u, z);
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = fminf(fmaxf(c[j] + z[j] * P.jitter_scale, 0.0f), 255.0f);
    }
    if (P.normalize) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = c[j] / 127.5f - 1.0f;
    }
    color[3 * i] = c[0]; color[3 * i + 1] = c[1]; color[3 * i + 2] = c[2];
  }
}

// ---- GridSample over the point cloud beside the Gaussians -----------------------------------------------------------------------
// One member per occupied cell (pointcept/datasets/transform.py:1245-1253): the first member in sorted order whose label is not
// ignore_index, the first member when the cell has none or there are no labels.  One thread per cell, grid-stride; the thread walks
// its run of `order` and writes one int.  No LDS, no atomics: the pick is exact and the same on every run.
__global__ void __launch_bounds__(AUG_BLOCK)
k_voxel_pick_labelled(const int32_t* __restrict__ order, const int32_t* __restrict__ idx_ptr, int64_t n_cells,
                      const int64_t* __restrict__ label, int64_t ignore_index, int32_t* __restrict__ chosen) {
  for (int64_t c = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * AUG_BLOCK) {
    const int32_t lo = idx_ptr[c], hi = idx_ptr[c + 1];
    int32_t pick = lo < hi ? order[lo] : -1;                        // (a partition has no empty run)
    if (label) {
      for (int32_t j = lo; j < hi; ++j) {
        const int32_t r = order[j];
        if (label[r] != ignore_index) { pick = r; break; }
      }
    }
    chosen[c] = pick;
  }
}

// ---- HueSaturationTranslation ---------------------------------------------------------------------------------------------------
// transform.py:1037-1100 per point, in fp64 and in the reference's operation order: it truncates twice through uint8 (the sector
// i = (h * 6.0).astype("uint8") and the final rgb.astype("uint8")), so a value that an fp32 evaluation or a fused multiply-add
// moves across an integer changes the output by a whole step.  No contraction in here; the divisions are IEEE.
__device__ __forceinline__ double np_mod1(double a) {          // numpy's a % 1.0: fmod, lifted by 1 when negative (may give exactly 1.0)
#pragma clang fp contract(off)
  double r = fmod(a, 1.0);
  if (r < 0.0) r += 1.0;
  return r;
}

__device__ __forceinline__ float to_u8(double v) {             // astype("uint8") on 0..255; outside it (numpy: undefined) saturates, NaN -> 0
  return v >= 255.0 ? 255.0f : (v >= 0.0 ? (float)(int)v : 0.0f);
}

__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_hsv(float* __restrict__ color, int64_t n, double hue_val, double sat_ratio) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    const double r = color[3 * i], g = color[3 * i + 1], b = color[3 * i + 2];
    const double maxc = fmax(r, fmax(g, b)), minc = fmin(r, fmin(g, b));
    const double v = maxc;
    double s = 0.0, rc = 0.0, gc = 0.0, bc = 0.0;
    if (maxc != minc) {
      const double d = maxc - minc;
      s = d / maxc;
      rc = (maxc - r) / d; gc = (maxc - g) / d; bc = (maxc - b) / d;
    }
    double h = r == maxc ? bc - gc : (g == maxc ? (2.0 + rc) - bc : (4.0 + gc) - rc);
    h = np_mod1(h / 6.0);
    h = np_mod1((hue_val + h) + 1.0);
    s = fmin(fmax(sat_ratio * s, 0.0), 1.0);
    const double h6 = h * 6.0;
    const int sector = (int)to_u8(h6);
    const double f = h6 - (double)sector;
    const double p = v * (1.0 - s);
    const double q = v * (1.0 - s * f);
    const double t = v * (1.0 - s * (1.0 - f));
    double o0 = v, o1 = t, o2 = p;                               // sector 0 (and 6: h == 1.0)
    if (s == 0.0) { o0 = v; o1 = v; o2 = v; }
    else switch (sector % 6) {
      case 1: o0 = q; o1 = v; o2 = p; break;
      case 2: o0 = p; o1 = v; o2 = t; break;
      case 3: o0 = p; o1 = q; o2 = v; break;
      case 4: o0 = t; o1 = p; o2 = v; break;
      case 5: o0 = v; o1 = p; o2 = q; break;
      default: break;
    }
    color[3 * i] = to_u8(o0); color[3 * i + 1] = to_u8(o1); color[3 * i + 2] = to_u8(o2);
  }
}

// ---- fp64 moments of A x + b ----------------------------------------------------------------------------------------------------
// NormalizeCoord's two reductions: the sums of the three components (the centroid) and the largest squared norm.  fp64, the
// products and sums uncontracted in the written order, so the maximum is the value numpy gives for the same expression.  Per-block
// partials and a one-wave finish: a fixed tree, the same bits on every run.
struct Affine64 { double a[9]; double b[3]; };

__device__ __forceinline__ double wave_reduce_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_reduce_max64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(AUG_BLOCK)
k_aug_moments(const float* __restrict__ x, int64_t n, Affine64 af, int use_affine, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double red[AUG_WAVES][4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    const double px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
    double p[3] = {px, py, pz};
    if (use_affine) {
#pragma unroll
      for (int j = 0; j < 3; ++j) p[j] = ((af.a[3 * j] * px + af.a[3 * j + 1] * py) + af.a[3 * j + 2] * pz) + af.b[j];
    }
    acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
    acc[3] = fmax(acc[3], (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double r = j < 3 ? wave_reduce_sum64(acc[j]) : wave_reduce_max64(acc[j]);
    if (lane == 0) red[wave][j] = r;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double r = red[0][threadIdx.x];
    for (int w = 1; w < AUG_WAVES; ++w) r = threadIdx.x < 3 ? r + red[w][threadIdx.x] : fmax(r, red[w][threadIdx.x]);
    partials[(int64_t)blockIdx.x * 4 + threadIdx.x] = r;
  }
}

__global__ void __launch_bounds__(64)
k_aug_moments_finish(const double* __restrict__ partials, int nb, double* __restrict__ out4) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double r = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) r = j < 3 ? r + partials[b * 4 + j] : fmax(r, partials[b * 4 + j]);
    r = j < 3 ? wave_reduce_sum64(r) : wave_reduce_max64(r);
    if (threadIdx.x == 0) out4[j] = r;
  }
}

// ---- InstanceParser -------------------------------------------------------------------------------------------------------------
// transform.py:1626-1664 over the CSR of a stable argsort of the instance ids (instance k holds rows order[idx_ptr[k] .. idx_ptr[k+1]),
// ascending).  One workgroup per instance, the whole workgroup striding the run (one instance may hold almost every row): min / max
// are exact, the coordinate sum is fp64 in a fixed order (thread-strided, wave tree, waves in order) and is rounded to fp32 once.
constexpr int INST_MAX_VACANCY = 16;
struct Vacancy { int64_t v[INST_MAX_VACANCY]; int count; };

__global__ void __launch_bounds__(AUG_BLOCK)
k_instance_boxes(const float* __restrict__ coord, const int64_t* __restrict__ segment, const int32_t* __restrict__ order,
                 const int32_t* __restrict__ idx_ptr, int64_t K, Vacancy vac, float* __restrict__ bbox, float* __restrict__ centroid) {
#pragma clang fp contract(off)
  __shared__ float red_lo[AUG_WAVES][3], red_hi[AUG_WAVES][3];
  __shared__ double red_sum[AUG_WAVES][3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
    const int32_t lo_j = idx_ptr[k], hi_j = idx_ptr[k + 1];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double sum[3] = {0.0, 0.0, 0.0};
    for (int32_t j = lo_j + (int32_t)threadIdx.x; j < hi_j; j += AUG_BLOCK) {
      const int64_t r = order[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = coord[3 * r + c];
        lo[c] = fminf(lo[c], p); hi[c] = fmaxf(hi[c], p); sum[c] += (double)p;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float l = wave_reduce_min(lo[c]), h = wave_reduce_max(hi[c]);
      const double s = wave_reduce_sum64(sum[c]);
      if (lane == 0) { red_lo[wave][c] = l; red_hi[wave][c] = h; red_sum[wave][c] = s; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int c = threadIdx.x;
      float l = red_lo[0][c], h = red_hi[0][c];
      double s = red_sum[0][c];
      for (int w = 1; w < AUG_WAVES; ++w) { l = fminf(l, red_lo[w][c]); h = fmaxf(h, red_hi[w][c]); s += red_sum[w][c]; }
      bbox[8 * k + c] = (h + l) / 2.0f;
      bbox[8 * k + 3 + c] = h - l;
      centroid[3 * k + c] = (float)(s / (double)(hi_j - lo_j));
    }
    if (threadIdx.x == 3) {
      const int64_t cls = segment[order[lo_j]];                 // the run's first member: segment[mask_][0] (the sort is stable)
      int below = 0;
      for (int v = 0; v < vac.count; ++v) below += cls > vac.v[v] ? 1 : 0;
      bbox[8 * k + 6] = 0.0f;
      bbox[8 * k + 7] = (float)cls - (float)below;
    }
    __syncthreads();
  }
}

// cluster[row] = the run of the row; runs K and above (the ignored rows' sentinel run) get the ignore value in both outputs
__global__ void __launch_bounds__(AUG_BLOCK)
k_instance_scatter(const int32_t* __restrict__ cluster, int64_t n, int64_t K, const float* __restrict__ centroid, void* __restrict__ instance,
                   int is64, int64_t ignore_index, float* __restrict__ out) {
  const float ign = (float)ignore_index;
  for (int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_BLOCK) {
    const int64_t k = cluster ? cluster[i] : K;
    const bool member = k >= 0 && k < K;
    const int64_t id = member ? k : ignore_index;
    if (is64) static_cast<int64_t*>(instance)[i] = id; else static_cast<int32_t*>(instance)[i] = (int32_t)id;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = member ? centroid[3 * k + c] : ign;
  }
}

}  // namespace

extern "C" int ss_aug_bbox_blocks(int64_t n) { return aug_blocks(n); }

extern "C" int ss_aug_bbox(const float* x, int64_t n, const float* h_affine, float* partials, float* out6, hipStream_t stream) {
  if (n < 1 || !x || !partials || !out6) return SS_ERR_ARG;
  Affine af = {};
  if (h_affine) {
    for (int i = 0; i < 9; ++i) af.a[i] = h_affine[i];
    for (int i = 0; i < 3; ++i) af.b[i] = h_affine[9 + i];
  }
  const int nb = aug_blocks(n);
  SS_LAUNCH(k_aug_bbox, dim3((unsigned)nb), dim3(AUG_BLOCK), 0, stream, x, n, af, h_affine ? 1 : 0, partials);
  SS_LAUNCH(k_aug_bbox_finish, dim3(1), dim3(64), 0, stream, (const float*)partials, nb, out6);
  return SS_OK;
}

extern "C" int ss_aug_gaussians(float* coord, float* quat, float* scale, float* normal, int64_t n, const float* h_affine,
                                const float* h_rquat, int flip, const float* h_scale_mul, const float* h_lin, int jitter,
                                float jitter_sigma, float jitter_clip, const float* noise, uint64_t seed, hipStream_t stream) {
  if (n < 0 || flip < 0 || flip > 3) return SS_ERR_ARG;
  if ((scale && !h_scale_mul) || (normal && !h_lin)) return SS_ERR_ARG;
  if (jitter && !(jitter_clip > 0.0f)) return SS_ERR_ARG;
  if (quat && (reinterpret_cast<uintptr_t>(quat) & 15)) return SS_ERR_ARG;          // rows are read as float4
  if (!h_affine && !jitter) coord = nullptr;                                         // nothing to do on the coordinates
  if (!h_rquat && !flip) quat = nullptr;
  if (n == 0 || (!coord && !quat && !scale && !normal)) return SS_OK;
  GaussParams P = {};
  if (h_affine) {
    for (int i = 0; i < 9; ++i) P.af.a[i] = h_affine[i];
    for (int i = 0; i < 3; ++i) P.af.b[i] = h_affine[9 + i];
  }
  if (h_rquat) for (int i = 0; i < 4; ++i) P.rq[i] = h_rquat[i];
  if (h_scale_mul) for (int i = 0; i < 3; ++i) P.smul[i] = h_scale_mul[i];
  if (h_lin) for (int i = 0; i < 9; ++i) P.lin[i] = h_lin[i];
  P.use_affine = h_affine ? 1 : 0; P.use_rq = h_rquat ? 1 : 0; P.flip = flip; P.jitter = jitter ? 1 : 0;
  P.sigma = jitter_sigma; P.clip = jitter_clip; P.seed = seed;
  SS_LAUNCH(k_aug_gaussians, dim3((unsigned)aug_blocks(n)), dim3(AUG_BLOCK), 0, stream, coord, quat, scale, normal, n, P,
            jitter ? noise : (const float*)nullptr);
  return SS_OK;
}

extern "C" int ss_aug_elastic(float* coord, int64_t n, const float* noise, int d0, int d1, int d2, const float* h_origin,
                              float granularity, float magnitude, hipStream_t stream) {
  if (n < 0 || d0 < 2 || d1 < 2 || d2 < 2 || !h_origin || !(granularity > 0.0f)) return SS_ERR_ARG;
  if ((int64_t)d0 * d1 * d2 * 3 > INT32_MAX) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!coord || !noise) return SS_ERR_ARG;
  Vec3 o = {{h_origin[0], h_origin[1], h_origin[2]}};
  SS_LAUNCH(k_aug_elastic, dim3((unsigned)aug_blocks(n)), dim3(AUG_BLOCK), 0, stream, coord, n, noise, d0, d1, d2, o, granularity,
            magnitude);
  return SS_OK;
}

extern "C" int ss_aug_color(float* color, int64_t n, int flags, const float* h_lo, const float* h_hi, float blend, const float* h_tr,
                            float jitter_std, const float* noise, uint64_t seed, int normalize, hipStream_t stream) {
  if (n < 0 || flags < 0 || flags > 7) return SS_ERR_ARG;
  if (((flags & 1) && (!h_lo || !h_hi)) || ((flags & 2) && !h_tr)) return SS_ERR_ARG;
  if (n == 0 || (!flags && !normalize)) return SS_OK;
  if (!color) return SS_ERR_ARG;
  ColorParams P = {};
  if (flags & 1) for (int i = 0; i < 3; ++i) { P.lo[i] = h_lo[i]; P.cscale[i] = 255.0f / (h_hi[i] - h_lo[i]); }
  if (flags & 2) for (int i = 0; i < 3; ++i) P.tr[i] = h_tr[i];
  P.flags = flags; P.normalize = normalize ? 1 : 0; P.blend = blend; P.jitter_scale = jitter_std * 255.0f; P.seed = seed;
  SS_LAUNCH(k_aug_color, dim3((unsigned)aug_blocks(n)), dim3(AUG_BLOCK), 0, stream, color, n, P,
            (flags & 4) ? noise : (const float*)nullptr);
  return SS_OK;
}

extern "C" int ss_aug_hsv(float* color, int64_t n, const double* h_hue_sat, hipStream_t stream) {
  if (n < 0 || !h_hue_sat) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!color) return SS_ERR_ARG;
  SS_LAUNCH(k_aug_hsv, dim3((unsigned)aug_blocks(n)), dim3(AUG_BLOCK), 0, stream, color, n, h_hue_sat[0], h_hue_sat[1]);
  return SS_OK;
}

extern "C" int ss_aug_moments_blocks(int64_t n) { return aug_blocks(n); }

extern "C" int ss_aug_moments(const float* x, int64_t n, const double* h_affine, double* partials, double* out4, hipStream_t stream) {
  if (n < 1 || !x || !partials || !out4) return SS_ERR_ARG;
  Affine64 af = {};
  if (h_affine) {
    for (int i = 0; i < 9; ++i) af.a[i] = h_affine[i];
    for (int i = 0; i < 3; ++i) af.b[i] = h_affine[9 + i];
  }
  const int nb = aug_blocks(n);
  SS_LAUNCH(k_aug_moments, dim3((unsigned)nb), dim3(AUG_BLOCK), 0, stream, x, n, af, h_affine ? 1 : 0, partials);
  SS_LAUNCH(k_aug_moments_finish, dim3(1), dim3(64), 0, stream, (const double*)partials, nb, out4);
  return SS_OK;
}

extern "C" int ss_instance_boxes(const float* coord, const int64_t* segment, const int32_t* order, const int32_t* idx_ptr, int64_t K,
                                 const int64_t* h_vacancy, int num_vacancy, float* bbox, float* centroid, hipStream_t stream) {
  if (K < 0 || num_vacancy < 0 || num_vacancy > INST_MAX_VACANCY || (num_vacancy && !h_vacancy)) return SS_ERR_ARG;
  if (K == 0) return SS_OK;
  if (!coord || !segment || !order || !idx_ptr || !bbox || !centroid) return SS_ERR_ARG;
  Vacancy vac = {};
  for (int i = 0; i < num_vacancy; ++i) vac.v[i] = h_vacancy[i];
  vac.count = num_vacancy;
  const unsigned grid = (unsigned)(K > AUG_MAX_BLOCKS ? AUG_MAX_BLOCKS : K);
  SS_LAUNCH(k_instance_boxes, dim3(grid), dim3(AUG_BLOCK), 0, stream, coord, segment, order, idx_ptr, K, vac, bbox, centroid);
  return SS_OK;
}

extern "C" int ss_instance_scatter(const int32_t* cluster, int64_t n, int64_t K, const float* centroid, void* instance, int instance_is_i64,
                                   int64_t ignore_index, float* instance_centroid, hipStream_t stream) {
  if (n < 0 || K < 0) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!instance || !instance_centroid || (K > 0 && (!cluster || !centroid))) return SS_ERR_ARG;
  SS_LAUNCH(k_instance_scatter, dim3((unsigned)aug_blocks(n)), dim3(AUG_BLOCK), 0, stream, K > 0 ? cluster : (const int32_t*)nullptr, n, K,
            centroid, instance, instance_is_i64 ? 1 : 0, ignore_index, instance_centroid);
  return SS_OK;
}

extern "C" int ss_voxel_pick_labelled(const int32_t* order, const int32_t* idx_ptr, int64_t n_cells, const int64_t* label,
                                      int64_t ignore_index, int32_t* chosen, hipStream_t stream) {
  if (n_cells < 0) return SS_ERR_ARG;
  if (n_cells == 0) return SS_OK;
  if (!order || !idx_ptr || !chosen) return SS_ERR_ARG;
  SS_LAUNCH(k_voxel_pick_labelled, dim3((unsigned)aug_blocks(n_cells)), dim3(AUG_BLOCK), 0, stream, order, idx_ptr, n_cells, label,
            ignore_index, chosen);
  return SS_OK;
}
