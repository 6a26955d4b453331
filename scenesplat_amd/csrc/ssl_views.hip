// The colour and blur transforms of the self-supervised view generator on the device (pointcept/datasets/transform.py:60-176 GSGaussianBlurVoxelOpc,
// :820-1032 RandomColorGrayScale / RandomColorJitter).  Two families of kernels, fp32 arrays, in place:
//   colour chain   up to 8 (code, factor) steps per point in ONE pass; a contrast step needs the mean gray of the colours as they are when it is
//                  reached, which a reduction pass gets by re-applying the step prefix in registers (per-block partials + a one-wave finish, no
//                  atomics: the same bits on every run) and leaves in device memory for the apply pass.
//   voxel blur     the reference scatters the view into a DENSE grid and runs scipy's separable gaussian_filter over it; here the masked voxels
//                  go into an open-addressing hash and every masked voxel gathers its (2r+1)^3 neighbourhood directly: O(n) memory, no readback.
// One thread per point, grid-stride, at most SSL_MAX_BLOCKS workgroups.
#include "common.h"
#include <math.h>

namespace {

constexpr int SSL_BLOCK = 256;
constexpr int SSL_MAX_BLOCKS = 1024;       // four workgroups per CU, as csrc/augment.hip
constexpr int SSL_WAVES = SSL_BLOCK / 64;

inline int ssl_blocks(int64_t n) {
  const int64_t b = (n + SSL_BLOCK - 1) / SSL_BLOCK;
  return (int)(b < 1 ? 1 : (b > SSL_MAX_BLOCKS ? SSL_MAX_BLOCKS : b));
}

// ---- colour chain ---------------------------------------------------------------------------------------------------------------
constexpr int CHAIN_MAX = 8;
enum { STEP_BRIGHTNESS = 1, STEP_CONTRAST = 2, STEP_SATURATION = 3, STEP_HUE = 4, STEP_GRAY = 5 };

struct Chain {
  int count;
  int code[CHAIN_MAX];
  float f[CHAIN_MAX];
  float omf[CHAIN_MAX];      // 1 - f, rounded once from the fp64 difference as the reference's blend() does
};

__device__ __forceinline__ float gray_of(const float (&c)[3]) { return 0.2989f * c[0] + 0.587f * c[1] + 0.114f * c[2]; }

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.0f), 255.0f); }

// adjust_hue (transform.py:905-979).  The reference's rgb2hsv multiplies by (1 - eqc), an integer array, so everything behind color / 255.0 is
// float64 there; the step is evaluated in fp64 here as well (a few dozen operations per point of an HBM-bound pass).
__device__ __forceinline__ void hue_step(float (&c)[3], float factor) {
  const double r = (double)(c[0] / 255.0f), g = (double)(c[1] / 255.0f), b = (double)(c[2] / 255.0f);
  const double maxc = fmax(r, fmax(g, b)), minc = fmin(r, fmin(g, b));
  const bool eqc = maxc == minc;
  const double cr = maxc - minc;
  const double s = cr / (eqc ? 1.0 : maxc);
  const double div = eqc ? 1.0 : cr;
  const double rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  double h;
  if (maxc == r) h = bc - gc;
  else if (maxc == g) h = 2.0 + rc - bc;
  else h = 4.0 + gc - rc;
  h = h / 6.0 + 1.0;
  h = h - floor(h);
  h = h + (double)factor;
  h = h - floor(h);                                   // numpy's %: the result has the sign of the divisor
  const double h6 = h * 6.0, fl = floor(h6), f = h6 - fl;
  const int i = ((int)fl) % 6;
  const double v = maxc;
  const double p = fmin(fmax(v * (1.0 - s), 0.0), 1.0);
  const double q = fmin(fmax(v * (1.0 - s * f), 0.0), 1.0);
  const double t = fmin(fmax(v * (1.0 - s * (1.0 - f)), 0.0), 1.0);
  const double o0 = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  const double o1 = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  const double o2 = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
  c[0] = (float)(o0 * 255.0); c[1] = (float)(o1 * 255.0); c[2] = (float)(o2 * 255.0);
}

// steps [0, upto) of the chain on one colour; means[k] is the mean gray a contrast step at position k blends against
__device__ __forceinline__ void chain_apply(float (&c)[3], const Chain& ch, int upto, const float* __restrict__ means) {
  for (int k = 0; k < upto; ++k) {
    const int code = ch.code[k];
    const float f = ch.f[k], omf = ch.omf[k];
    if (code == STEP_BRIGHTNESS) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = clip255(f * c[j]);
    } else if (code == STEP_CONTRAST) {
      const float m = omf * means[k];
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = clip255(f * c[j] + m);
    } else if (code == STEP_SATURATION) {
      const float m = omf * gray_of(c);
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = clip255(f * c[j] + m);
    } else if (code == STEP_HUE) {
      hue_step(c, f);
    } else if (code == STEP_GRAY) {
      const float gr = gray_of(c);
      c[0] = gr; c[1] = gr; c[2] = gr;
    }
  }
}

// per-block sum of the gray of the colours as they are in front of step `upto`; color is only read
__global__ void __launch_bounds__(SSL_BLOCK)
k_chain_gray_sum(const float* __restrict__ color, int64_t n, Chain ch, int upto, const float* __restrict__ means, float* __restrict__ partials) {
  __shared__ float red[SSL_WAVES];
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * SSL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSL_BLOCK) {
    float c[3] = {color[3 * i], color[3 * i + 1], color[3 * i + 2]};
    chain_apply(c, ch, upto, means);
    acc += gray_of(c);
  }
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = red[0];
    for (int w = 1; w < SSL_WAVES; ++w) v += red[w];
    partials[blockIdx.x] = v;
  }
}

// one wave: lane -> partials lane, lane + 64, ... in fp64, a fixed butterfly over the lanes, mean -> means[slot]
__global__ void __launch_bounds__(64)
k_chain_gray_finish(const float* __restrict__ partials, int nb, int64_t n, float* __restrict__ means, int slot) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nb; b += 64) v += (double)partials[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (threadIdx.x == 0) means[slot] = (float)(v / (double)n);
}

__global__ void __launch_bounds__(SSL_BLOCK)
k_chain_apply(float* __restrict__ color, int64_t n, Chain ch, const float* __restrict__ means) {
  for (int64_t i = (int64_t)blockIdx.x * SSL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSL_BLOCK) {
    float c[3] = {color[3 * i], color[3 * i + 1], color[3 * i + 2]};
    chain_apply(c, ch, ch.count, means);
    color[3 * i] = c[0]; color[3 * i + 1] = c[1]; color[3 * i + 2] = c[2];
  }
}

// ---- sparse voxel blur ----------------------------------------------------------------------------------------------------------
constexpr int BLUR_MAX_R = 8;                      // sigma < 4.25
constexpr int BLUR_AXIS_BITS = 21;                 // cells per axis the 63-bit voxel key holds
constexpr long long BLUR_EMPTY = -1;

struct BlurWeights { double w[2 * BLUR_MAX_R + 1]; };     // w[d + r], normalised over -r .. r
struct BlurSlot { long long key; long long row; };        // 16 bytes: one load per probe
// the head of the workspace: int32 words 0-5 the box of grid_coord, word 6 the status (!= 0: an axis spans 2^21 cells or more, nothing is blurred)
struct BlurBox { int lo[3]; int hi[3]; int status; int pad; };

// fixed slots of a packed row whatever arrays are present: colour 0-2, opacity 3, scale 4-6, quat 8-11, normal 12-14
constexpr int SLOT_COLOR = 0, SLOT_OPACITY = 3, SLOT_SCALE = 4, SLOT_QUAT = 8, SLOT_NORMAL = 12;

__device__ __forceinline__ uint64_t blur_hash(uint64_t k) {                  // the 64-bit finaliser of MurmurHash3
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}

__global__ void __launch_bounds__(SSL_BLOCK)
k_blur_box(const int32_t* __restrict__ gc, int64_t n, int* __restrict__ partials) {
  __shared__ int red[SSL_WAVES][6];
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (int64_t i = (int64_t)blockIdx.x * SSL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSL_BLOCK) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { const int v = gc[3 * i + j]; lo[j] = min(lo[j], v); hi[j] = max(hi[j], v); }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo[j] = min(lo[j], __shfl_xor(lo[j], o, 64)); hi[j] = max(hi[j], __shfl_xor(hi[j], o, 64)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][j] = lo[j]; red[threadIdx.x >> 6][3 + j] = hi[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    int v = red[0][threadIdx.x];
    for (int w = 1; w < SSL_WAVES; ++w) v = threadIdx.x < 3 ? min(v, red[w][threadIdx.x]) : max(v, red[w][threadIdx.x]);
    partials[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64)
k_blur_box_finish(const int* __restrict__ partials, int nb, BlurBox* __restrict__ box) {
  int ok = 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int l = INT32_MAX, h = INT32_MIN;
    for (int b = threadIdx.x; b < nb; b += 64) { l = min(l, partials[b * 6 + j]); h = max(h, partials[b * 6 + 3 + j]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { l = min(l, __shfl_xor(l, o, 64)); h = max(h, __shfl_xor(h, o, 64)); }
    if ((int64_t)h - (int64_t)l >= ((int64_t)1 << BLUR_AXIS_BITS)) ok = 0;
    if (threadIdx.x == 0) { box->lo[j] = l; box->hi[j] = h; }
  }
  if (threadIdx.x == 0) { box->status = ok ? 0 : 1; box->pad = 0; }
}

// masked rows: their channels into the packed copy the gather reads (the arrays themselves are overwritten in place), their voxel into the hash
template <int NV4>
__global__ void __launch_bounds__(SSL_BLOCK)
k_blur_build(const int32_t* __restrict__ gc, const uint8_t* __restrict__ mask, int64_t n, const float* __restrict__ color,
             const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ quat, const float* __restrict__ normal,
             const BlurBox* __restrict__ box, BlurSlot* __restrict__ table, uint64_t tmask, float* __restrict__ packed) {
  if (box->status) return;
  const int lo0 = box->lo[0], lo1 = box->lo[1], lo2 = box->lo[2];
  for (int64_t i = (int64_t)blockIdx.x * SSL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSL_BLOCK) {
    if (mask && !mask[i]) continue;
    float v[4 * NV4];
#pragma unroll
    for (int j = 0; j < 4 * NV4; ++j) v[j] = 0.0f;
    v[SLOT_COLOR] = color[3 * i]; v[SLOT_COLOR + 1] = color[3 * i + 1]; v[SLOT_COLOR + 2] = color[3 * i + 2];
    if (opacity) v[SLOT_OPACITY] = opacity[i];
    if constexpr (NV4 >= 2) {
      if (scale) { v[SLOT_SCALE] = scale[3 * i]; v[SLOT_SCALE + 1] = scale[3 * i + 1]; v[SLOT_SCALE + 2] = scale[3 * i + 2]; }
    }
    if constexpr (NV4 >= 3) {
      if (quat) { v[SLOT_QUAT] = quat[4 * i]; v[SLOT_QUAT + 1] = quat[4 * i + 1]; v[SLOT_QUAT + 2] = quat[4 * i + 2]; v[SLOT_QUAT + 3] = quat[4 * i + 3]; }
    }
    if constexpr (NV4 >= 4) {
      if (normal) { v[SLOT_NORMAL] = normal[3 * i]; v[SLOT_NORMAL + 1] = normal[3 * i + 1]; v[SLOT_NORMAL + 2] = normal[3 * i + 2]; }
    }
    float4* dst = reinterpret_cast<float4*>(packed) + i * NV4;
#pragma unroll
    for (int j = 0; j < NV4; ++j) dst[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    const long long key = ((long long)(gc[3 * i] - lo0) << (2 * BLUR_AXIS_BITS)) | ((long long)(gc[3 * i + 1] - lo1) << BLUR_AXIS_BITS) |
                          (long long)(gc[3 * i + 2] - lo2);
    uint64_t s = blur_hash((uint64_t)key) & tmask;
    for (uint64_t probe = 0; probe <= tmask; ++probe) {              // the table holds twice the rows: an empty slot is always met
      const long long prev = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&table[s].key), (unsigned long long)BLUR_EMPTY,
                                                  (unsigned long long)key);
      if (prev == BLUR_EMPTY) { table[s].row = i; break; }
      s = (s + 1) & tmask;                                           // another voxel (rows are unique): next slot
    }
  }
}

// scipy's `reflect` (d c b a | a b c d | d c b a): period 2 * size, also when the offset exceeds the axis
__device__ __forceinline__ int blur_reflect(int j, int size) {
  const int p = 2 * size;
  int m = j % p;
  if (m < 0) m += p;
  return m >= size ? p - 1 - m : m;
}

template <int NV4>
__global__ void __launch_bounds__(SSL_BLOCK)
k_blur_gather(const int32_t* __restrict__ gc, const uint8_t* __restrict__ mask, int64_t n, float* __restrict__ color, float* __restrict__ opacity,
              float* __restrict__ scale, float* __restrict__ quat, float* __restrict__ normal, int normalize_quat,
              const BlurBox* __restrict__ box, const BlurSlot* __restrict__ table, uint64_t tmask, const float* __restrict__ packed, int r,
              BlurWeights W) {
  const bool blur = box->status == 0;
  const int lo0 = box->lo[0], lo1 = box->lo[1], lo2 = box->lo[2];
  const int s0 = blur ? box->hi[0] - lo0 + 1 : 1, s1 = blur ? box->hi[1] - lo1 + 1 : 1, s2 = blur ? box->hi[2] - lo2 + 1 : 1;
  for (int64_t i = (int64_t)blockIdx.x * SSL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSL_BLOCK) {
    const bool masked = blur && (!mask || mask[i]);
    float q4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (quat) { q4[0] = quat[4 * i]; q4[1] = quat[4 * i + 1]; q4[2] = quat[4 * i + 2]; q4[3] = quat[4 * i + 3]; }
    if (masked) {
      const int c0 = gc[3 * i] - lo0, c1 = gc[3 * i + 1] - lo1, c2 = gc[3 * i + 2] - lo2;
      double acc[4 * NV4];
#pragma unroll
      for (int j = 0; j < 4 * NV4; ++j) acc[j] = 0.0;
      double wsum = 0.0;
      for (int dx = -r; dx <= r; ++dx) {
        const long long kx = (long long)blur_reflect(c0 + dx, s0) << (2 * BLUR_AXIS_BITS);
        for (int dy = -r; dy <= r; ++dy) {
          const long long kxy = kx | ((long long)blur_reflect(c1 + dy, s1) << BLUR_AXIS_BITS);
          const double wxy = W.w[dx + r] * W.w[dy + r];
          for (int dz = -r; dz <= r; ++dz) {
            const long long key = kxy | (long long)blur_reflect(c2 + dz, s2);
            uint64_t s = blur_hash((uint64_t)key) & tmask;
            long long row = -1;
            for (uint64_t probe = 0; probe <= tmask; ++probe) {
              const BlurSlot e = table[s];
              if (e.key == key) { row = e.row; break; }
              if (e.key == BLUR_EMPTY) break;
              s = (s + 1) & tmask;
            }
            if (row < 0) continue;
            const double w = wxy * W.w[dz + r];
            const float4* src = reinterpret_cast<const float4*>(packed) + row * NV4;
#pragma unroll
            for (int j = 0; j < NV4; ++j) {
              const float4 t = src[j];
              acc[4 * j] = fma(w, (double)t.x, acc[4 * j]); acc[4 * j + 1] = fma(w, (double)t.y, acc[4 * j + 1]);
              acc[4 * j + 2] = fma(w, (double)t.z, acc[4 * j + 2]); acc[4 * j + 3] = fma(w, (double)t.w, acc[4 * j + 3]);
            }
            wsum += w;
          }
        }
      }
      const double inv = 1.0 / (wsum + 1e-7);
      color[3 * i] = (float)(acc[SLOT_COLOR] * inv); color[3 * i + 1] = (float)(acc[SLOT_COLOR + 1] * inv);
      color[3 * i + 2] = (float)(acc[SLOT_COLOR + 2] * inv);
      if (opacity) opacity[i] = (float)(acc[SLOT_OPACITY] * inv);
      if constexpr (NV4 >= 2) {
        if (scale) {
          scale[3 * i] = (float)(acc[SLOT_SCALE] * inv); scale[3 * i + 1] = (float)(acc[SLOT_SCALE + 1] * inv);
          scale[3 * i + 2] = (float)(acc[SLOT_SCALE + 2] * inv);
        }
      }
      if constexpr (NV4 >= 3) {
        if (quat) {
#pragma unroll
          for (int j = 0; j < 4; ++j) q4[j] = (float)(acc[SLOT_QUAT + j] * inv);
        }
      }
      if constexpr (NV4 >= 4) {
        if (normal) {
          normal[3 * i] = (float)(acc[SLOT_NORMAL] * inv); normal[3 * i + 1] = (float)(acc[SLOT_NORMAL + 1] * inv);
          normal[3 * i + 2] = (float)(acc[SLOT_NORMAL + 2] * inv);
        }
      }
    }
    if (quat && (normalize_quat || masked)) {
      if (normalize_quat) {                              // EVERY row, blurred or not (transform.py:166); rows of zero norm stay as they are
        const float nrm = sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
        if (nrm > 0.0f) { q4[0] /= nrm; q4[1] /= nrm; q4[2] /= nrm; q4[3] /= nrm; }
      }
      quat[4 * i] = q4[0]; quat[4 * i + 1] = q4[1]; quat[4 * i + 2] = q4[2]; quat[4 * i + 3] = q4[3];
    }
  }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" int ss_color_chain_blocks(int64_t n) { return ssl_blocks(n); }

extern "C" int ss_color_chain(float* color, int64_t n, int num_steps, const int* h_codes, const float* h_factors, float* partials,
                              float* means, hipStream_t stream) {
  if (n < 0 || num_steps < 0 || num_steps > CHAIN_MAX) return SS_ERR_ARG;
  if (num_steps > 0 && (!h_codes || !h_factors)) return SS_ERR_ARG;
  Chain ch = {};
  ch.count = num_steps;
  bool contrast = false;
  for (int k = 0; k < num_steps; ++k) {
    if (h_codes[k] < STEP_BRIGHTNESS || h_codes[k] > STEP_GRAY) return SS_ERR_ARG;
    if (h_codes[k] == STEP_HUE ? !(h_factors[k] >= -0.5f && h_factors[k] <= 0.5f) : !(h_factors[k] >= 0.0f)) return SS_ERR_ARG;
    ch.code[k] = h_codes[k]; ch.f[k] = h_factors[k]; ch.omf[k] = (float)(1.0 - (double)h_factors[k]);
    contrast = contrast || h_codes[k] == STEP_CONTRAST;
  }
  if (n == 0 || num_steps == 0) return SS_OK;
  if (!color || (contrast && (!partials || !means))) return SS_ERR_ARG;
  const int nb = ssl_blocks(n);
  for (int k = 0; k < num_steps; ++k) {
    if (ch.code[k] != STEP_CONTRAST) continue;
    SS_LAUNCH(k_chain_gray_sum, dim3((unsigned)nb), dim3(SSL_BLOCK), 0, stream, (const float*)color, n, ch, k, (const float*)means, partials);
    SS_LAUNCH(k_chain_gray_finish, dim3(1), dim3(64), 0, stream, (const float*)partials, nb, n, means, k);
  }
  SS_LAUNCH(k_chain_apply, dim3((unsigned)nb), dim3(SSL_BLOCK), 0, stream, color, n, ch, (const float*)means);
  return SS_OK;
}

extern "C" int64_t ss_voxel_blur_table_size(int64_t n) {
  int64_t t = 64;
  while (t < 2 * n) t <<= 1;
  return t;
}

extern "C" size_t ss_voxel_blur_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return 256 + up256((size_t)ssl_blocks(n) * 6 * sizeof(int)) + (size_t)ss_voxel_blur_table_size(n) * sizeof(BlurSlot) + up256((size_t)n * 16 * sizeof(float));
}

extern "C" int ss_voxel_blur(const int32_t* grid_coord, const uint8_t* mask, int64_t n, float* color, float* opacity, float* scale, float* quat,
                             float* normal, int normalize_quat, float sigma, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n < 0 || !(sigma > 0.0f)) return SS_ERR_ARG;
  const int r = (int)(2.0 * (double)sigma + 0.5);
  if (r > BLUR_MAX_R) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!grid_coord || !color || !workspace) return SS_ERR_ARG;
  if (workspace_bytes < ss_voxel_blur_workspace_bytes(n) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return SS_ERR_WORKSPACE;
  BlurWeights W = {};
  double sum = 0.0;
  for (int d = -r; d <= r; ++d) { W.w[d + r] = exp(-0.5 * (double)d * (double)d / ((double)sigma * (double)sigma)); sum += W.w[d + r]; }
  for (int d = 0; d <= 2 * r; ++d) W.w[d] /= sum;
  const int nb = ssl_blocks(n);
  char* ws = static_cast<char*>(workspace);
  BlurBox* box = reinterpret_cast<BlurBox*>(ws);
  int* partials = reinterpret_cast<int*>(ws + 256);
  BlurSlot* table = reinterpret_cast<BlurSlot*>(ws + 256 + up256((size_t)nb * 6 * sizeof(int)));
  const int64_t tsize = ss_voxel_blur_table_size(n);
  float* packed = reinterpret_cast<float*>(reinterpret_cast<char*>(table) + (size_t)tsize * sizeof(BlurSlot));
  const uint64_t tmask = (uint64_t)tsize - 1;
  if (hipMemsetAsync(table, 0xFF, (size_t)tsize * sizeof(BlurSlot), stream) != hipSuccess) return SS_ERR_LAUNCH;
  SS_LAUNCH(k_blur_box, dim3((unsigned)nb), dim3(SSL_BLOCK), 0, stream, grid_coord, n, partials);
  SS_LAUNCH(k_blur_box_finish, dim3(1), dim3(64), 0, stream, (const int*)partials, nb, box);
  const int nv4 = normal ? 4 : quat ? 3 : scale ? 2 : 1;
#define SS_BLUR_LAUNCH(NV4)                                                                                                              \
  do {                                                                                                                                   \
    SS_LAUNCH(k_blur_build<NV4>, dim3((unsigned)nb), dim3(SSL_BLOCK), 0, stream, grid_coord, mask, n, (const float*)color,               \
              (const float*)opacity, (const float*)scale, (const float*)quat, (const float*)normal, (const BlurBox*)box, table, tmask,   \
              packed);                                                                                                                   \
    SS_LAUNCH(k_blur_gather<NV4>, dim3((unsigned)nb), dim3(SSL_BLOCK), 0, stream, grid_coord, mask, n, color, opacity, scale, quat,      \
              normal, normalize_quat, (const BlurBox*)box, (const BlurSlot*)table, tmask, (const float*)packed, r, W);                   \
  } while (0)
  switch (nv4) {
    case 1: SS_BLUR_LAUNCH(1); break;
    case 2: SS_BLUR_LAUNCH(2); break;
    case 3: SS_BLUR_LAUNCH(3); break;
    default: SS_BLUR_LAUNCH(4); break;
  }
#undef SS_BLUR_LAUNCH
  return SS_OK;
}
