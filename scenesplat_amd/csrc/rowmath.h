// Row-wise device helpers shared by the norm / GELU kernels (norm.hip) and the fused Block tail (block_tail.hip): the element
// loads / stores, the exact-erf GELU pair and the LayerNorm row formulas (sum, squared deviation, apply, x-hat, input gradient)
// are ONE piece of code: k_add_ln_*, k_ln_add_ln_* and k_block_tail_* all evaluate these functions.
#pragma once
#include "common.h"

__device__ __forceinline__ float4 ln_ld4(const void* p, int dtype, int64_t idx) {
  if (dtype == SS_F32) return *reinterpret_cast<const float4*>((const float*)p + idx);
  uint2 u = *reinterpret_cast<const uint2*>((const unsigned short*)p + idx);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ void ln_st4(void* p, int dtype, int64_t idx, float4 v) {
  if (dtype == SS_F32) { *reinterpret_cast<float4*>((float*)p + idx) = v; return; }
  uint2 u; u.x = pack_bf16x2(v.x, v.y); u.y = pack_bf16x2(v.z, v.w);
  *reinterpret_cast<uint2*>((unsigned short*)p + idx) = u;
}

__device__ __forceinline__ float gelu_f(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_f(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * __expf(-0.5f * z * z);
}
// the backward of the stand-alone GELU (expf, not __expf: the fp32 formula torch evaluates)
__device__ __forceinline__ float dgelu_exact(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * expf(-0.5f * z * z);
}
__device__ __forceinline__ void bf8_unpack(const uint4& u, float (&v)[8]) {
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u); v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
  v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u); v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 bf8_pack(const float (&v)[8]) {
  uint4 o; o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]); o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
  return o;
}

// ---- LayerNorm of one row held four elements per lane ------------------------------------------------------------------------
__device__ __forceinline__ float ln_sum4(const float4& a) { return a.x + a.y + a.z + a.w; }
__device__ __forceinline__ float ln_sqdev4(const float4& a, float mu) {
  const float dx = a.x - mu, dy = a.y - mu, dz = a.z - mu, dw = a.w - mu;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}
// (v - mu) * r * gamma + beta
__device__ __forceinline__ float4 ln_apply4(const float4& v, float mu, float r, const float4& g, const float4& b) {
  return make_float4((v.x - mu) * r * g.x + b.x, (v.y - mu) * r * g.y + b.y, (v.z - mu) * r * g.z + b.z, (v.w - mu) * r * g.w + b.w);
}
__device__ __forceinline__ float4 ln_xhat4(const float4& a, float mu, float r) {
  return make_float4((a.x - mu) * r, (a.y - mu) * r, (a.z - mu) * r, (a.w - mu) * r);
}
// input gradient of a row from xh (normalised input), gy (= g_out * gamma) and the row means c1 = mean(gy), c2 = mean(gy * xh)
__device__ __forceinline__ float4 ln_dx4(const float4& gy, const float4& xh, float c1, float c2, float r) {
  return make_float4(r * (gy.x - c1 - xh.x * c2), r * (gy.y - c1 - xh.y * c2), r * (gy.z - c1 - xh.z * c2), r * (gy.w - c1 - xh.w * c2));
}
// sum over an aligned group of W lanes (W a power of two <= 64), every lane of the group gets the result
template <int W>
__device__ __forceinline__ float lanes_reduce_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
