// Reading a feature matrix (N, D) of fp32 / fp16 / bf16 rows: the element loads the kernels of feature_pca.hip and text_query.hip share.
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>

// ---- element loads: one value, or four consecutive ones with one 16- / 8-byte access ------------------------------------------
template <int DT> struct PcaIn;
template <> struct PcaIn<SS_DTYPE_F32> {
  typedef float T;
  static __device__ __forceinline__ float one(const T* p) { return *p; }
  static __device__ __forceinline__ float4 four(const T* p) { return *reinterpret_cast<const float4*>(p); }
  typedef float4 Raw;                                                  // four values as loaded, before any arithmetic
  static __device__ __forceinline__ Raw raw(const T* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ float4 unpack(Raw v) { return v; }
};
template <> struct PcaIn<SS_DTYPE_BF16> {
  typedef unsigned short T;
  static __device__ __forceinline__ float one(const T* p) { return bf16_to_f32(*p); }
  typedef uint2 Raw;
  static __device__ __forceinline__ Raw raw(const T* p) { return *reinterpret_cast<const uint2*>(p); }
  static __device__ __forceinline__ float4 unpack(Raw v) {
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xffff0000u));
  }
  static __device__ __forceinline__ float4 four(const T* p) { return unpack(raw(p)); }
};
template <> struct PcaIn<SS_DTYPE_F16> {
  typedef __half T;
  static __device__ __forceinline__ float one(const T* p) { return __half2float(*p); }
  typedef uint2 Raw;
  static __device__ __forceinline__ Raw raw(const T* p) { return *reinterpret_cast<const uint2*>(p); }
  static __device__ __forceinline__ float4 unpack(Raw v) {
    const float2 lo = __half22float2(__builtin_bit_cast(__half2, v.x)), hi = __half22float2(__builtin_bit_cast(__half2, v.y));
    return make_float4(lo.x, lo.y, hi.x, hi.y);
  }
  static __device__ __forceinline__ float4 four(const T* p) { return unpack(raw(p)); }
};

// four values of a row from column c on, minus the shift; zeros where the row (row > last_row) or the column does not exist.  The loads
// are UNCONDITIONAL, from a clamped address, and the zeros are selects: the loads of an image are then issued back to back, where an
// exec-masked branch per load made each one wait for its own data.  VEC: D % 4 == 0 and an aligned base, so a group of four is inside
// the row or outside it as a whole.  last_row >= 0.
template <int DT, bool VEC>
__device__ __forceinline__ float4 pca_load4(const typename PcaIn<DT>::T* __restrict__ x, int64_t row, int64_t last_row, int c, int D,
                                            const float (&s)[4]) {
  const bool row_ok = row <= last_row;
  const typename PcaIn<DT>::T* p = x + (row_ok ? row : last_row) * D;
  float4 v;
  if (VEC) {
    const bool ok = row_ok && c < D;
    v = PcaIn<DT>::four(p + (c < D ? c : 0));
    v.x = ok ? v.x - s[0] : 0.f; v.y = ok ? v.y - s[1] : 0.f; v.z = ok ? v.z - s[2] : 0.f; v.w = ok ? v.w - s[3] : 0.f;
  } else {
    const float e0 = PcaIn<DT>::one(p + min(c + 0, D - 1)), e1 = PcaIn<DT>::one(p + min(c + 1, D - 1));
    const float e2 = PcaIn<DT>::one(p + min(c + 2, D - 1)), e3 = PcaIn<DT>::one(p + min(c + 3, D - 1));
    v.x = (row_ok && c + 0 < D) ? e0 - s[0] : 0.f; v.y = (row_ok && c + 1 < D) ? e1 - s[1] : 0.f;
    v.z = (row_ok && c + 2 < D) ? e2 - s[2] : 0.f; v.w = (row_ok && c + 3 < D) ? e3 - s[3] : 0.f;
  }
  return v;
}

// a group of four starts 16-byte (fp32) / 8-byte (16-bit) aligned in every row
static inline bool pca_vec_ok(const void* x, int dtype, int D) {
  return D % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (dtype == SS_DTYPE_F32 ? 16 : 8) == 0;
}
