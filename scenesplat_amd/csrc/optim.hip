// Optimizer step kernels (HBM-bound): the global gradient norm of clip_grad_norm_ and the AdamW update of ALL parameters of a model,
// every tensor of every parameter group in one launch each.  Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step
// (pointcept/engines/train.py:196-232), which walk the parameter memory about ten times in separate multi-tensor launches and
// build a parameter-sized temporary for the denominator.  Here the gradient is read once for the norm, then p, g, m, v are read
// and p, m, v written once: 32 bytes per parameter for the update.  The clip coefficient never leaves the device.
//
// Grouped launches (grouped.h), one descriptor row per tensor; a workgroup of 256 threads owns OPTG_PER_WG consecutive elements of
// one tensor.  No atomics anywhere: every sum has a fixed order, so results are bitwise reproducible.
#include "grouped.h"

#define OPTG_PER_WG 8192
#define OPTG_FLAG_VEC16 1        // every base pointer of the row is 16-byte aligned: 16-byte lanes; else one element per lane

// sum over the workgroup in a fixed order: lanes by xor-butterfly (every lane ends with the same value), then the 4 waves in order
__device__ __forceinline__ double optg_block_sum(double x, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// ---- sum of squares of all gradients: one fp64 partial per workgroup --------------------------------------------------------
// desc: 3 int64 words per tensor = {g f32 pointer, numel, flags}.  The squares are exact in fp64 and the sum is carried in fp64
// (the kernel stays HBM-bound: one convert + one fma per 4 bytes read), so the norm is good to fp32 rounding for any model size.
__global__ void __launch_bounds__(256)
k_grad_sqnorm_group(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob, double* __restrict__ partials) {
  __shared__ double lds[4];
  const int b = blockIdx.x;
  const int lo = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)lo * 3;
  cgf32* g = reinterpret_cast<cgf32*>(d[0]);
  double acc = 0.0;
  group_span<OPTG_PER_WG, 8>(
      (int64_t)(b - wg_start[lo]) * OPTG_PER_WG, d[1], d[2] & OPTG_FLAG_VEC16,
      [&](int64_t e) {
        const f32x4_t a = ld4(g + e), c = ld4(g + e + 4);
        const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (double)x[k] * (double)x[k];
      },
      [&](int64_t k) { acc += (double)g[k] * (double)g[k]; });
  const double s = optg_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[b] = s;
}

// ---- finish: record = {total_norm, coef}, clip_grad_norm_'s arithmetic (norm_type 2, error_if_nonfinite False) -----------------
// One workgroup; thread t sums partials t, t + 256, ... in order, then the fixed block sum.  coef = clamp(max_norm / (norm + 1e-6),
// max = 1) in fp32 as torch computes it: a NaN norm gives a NaN coefficient, an infinite norm 0 (no fminf: it would drop the NaN).
__global__ void __launch_bounds__(256)
k_grad_norm_finish(const double* __restrict__ partials, int n, float max_norm, float* __restrict__ record) {
  __shared__ double lds[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
  const double s = optg_block_sum(acc, lds);
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(s);
    const float c = max_norm / (total + 1e-6f);
    record[0] = total;
    record[1] = c > 1.0f ? 1.0f : c;
  }
}

// ---- AdamW update of every tensor of every parameter group ------------------------------------------------------------------
// desc: 10 int64 words per tensor = {p, g, m, v (f32 pointers), numel, flags, 8 floats: 1 - lr*wd, 1 - beta1, beta2, 1 - beta2,
// sqrt(1 - beta2^t), eps, lr / (1 - beta1^t), unused}.  The scalars are per tensor: groups differ in lr / wd / beta1 and a
// parameter that skipped steps has its own t.  fp32 arithmetic in the order of torch's single-tensor AdamW (mul_, lerp_, mul_ +
// addcmul_, sqrt / bc2_sqrt + eps, addcdiv_), IEEE sqrt and divide.  g is only read; the clipped gradient g * coef is never stored.
#define OPTG_ADAMW_WORDS 10
struct AdamwScalars { float decay, omb1, beta2, omb2, bc2_sqrt, eps, step_size, coef; };

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamwScalars& s) {
  g = g * s.coef;
  p = p * s.decay;
  m = m + (g - m) * s.omb1;
  v = v * s.beta2 + (s.omb2 * g) * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p - s.step_size * (m / denom);
}

__device__ __forceinline__ void adamw_vec4(f32x4_t& p, const f32x4_t g, f32x4_t& m, f32x4_t& v, const AdamwScalars& s) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = p[k], mk = m[k], vk = v[k];
    adamw_elem(pk, g[k], mk, vk, s);
    p[k] = pk; m[k] = mk; v[k] = vk;
  }
}

__global__ void __launch_bounds__(256)
k_adamw_group(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob, const float* __restrict__ record) {
  const int b = blockIdx.x;
  const int lo = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)lo * OPTG_ADAMW_WORDS;
  gf32* p = reinterpret_cast<gf32*>(d[0]);
  cgf32* g = reinterpret_cast<cgf32*>(d[1]);
  gf32* m = reinterpret_cast<gf32*>(d[2]);
  gf32* v = reinterpret_cast<gf32*>(d[3]);
  float f[8];
  __builtin_memcpy(f, d + 6, sizeof(f));              // the row's last four words hold 8 floats
  AdamwScalars s;
  s.decay = f[0]; s.omb1 = f[1]; s.beta2 = f[2]; s.omb2 = f[3]; s.bc2_sqrt = f[4]; s.eps = f[5]; s.step_size = f[6];
  s.coef = record ? record[1] : 1.0f;
  group_span<OPTG_PER_WG, 8>(
      (int64_t)(b - wg_start[lo]) * OPTG_PER_WG, d[4], d[5] & OPTG_FLAG_VEC16,
      [&](int64_t e) {
        f32x4_t pa = ld4(p + e), pb = ld4(p + e + 4);
        const f32x4_t ga = ld4(g + e), gb = ld4(g + e + 4);
        f32x4_t ma = ld4(m + e), mb = ld4(m + e + 4);
        f32x4_t va = ld4(v + e), vb = ld4(v + e + 4);
        adamw_vec4(pa, ga, ma, va, s); adamw_vec4(pb, gb, mb, vb, s);
        st4(p + e, pa); st4(p + e + 4, pb);
        st4(m + e, ma); st4(m + e + 4, mb);
        st4(v + e, va); st4(v + e + 4, vb);
      },
      [&](int64_t k) {
        float pk = p[k], mk = m[k], vk = v[k];
        adamw_elem(pk, g[k], mk, vk, s);
        p[k] = pk; m[k] = mk; v[k] = vk;
      });
}

extern "C" int ss_optim_group_elems_per_workgroup(void) { return OPTG_PER_WG; }

extern "C" int ss_grad_sqnorm_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, double* partials,
                                    hipStream_t stream) {
  SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups);
  if (!partials) return SS_ERR_ARG;
  SS_LAUNCH(k_grad_sqnorm_group, dim3((unsigned)total_workgroups), dim3(256), 0, stream, desc, wg_start, nprob, partials);
  return SS_OK;
}

extern "C" int ss_grad_norm_finish(const double* partials, int num_partials, float max_norm, float* record, hipStream_t stream) {
  if (num_partials < 0 || !record || (num_partials > 0 && !partials)) return SS_ERR_ARG;
  SS_LAUNCH(k_grad_norm_finish, dim3(1), dim3(256), 0, stream, partials, num_partials, max_norm, record);
  return SS_OK;
}

extern "C" int ss_adamw_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, const float* record,
                              hipStream_t stream) {
  SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups);
  SS_LAUNCH(k_adamw_group, dim3((unsigned)total_workgroups), dim3(256), 0, stream, desc, wg_start, nprob, record);
  return SS_OK;
}
