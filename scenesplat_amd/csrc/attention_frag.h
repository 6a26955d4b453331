// bf16-MFMA fragment helpers shared by the window-attention kernels (attention_mfma.hip, attention_mfma32.hip,
// attention_hm.hip, attention_rpe.hip): operand vector types, the two matrix instructions, 16-byte and transposed LDS reads,
// bf16 packing, cross-lane reductions, the XCD block remap, and the LDS image geometry / K+V tile staging of the 16x16x32
// kernels.  Everything is __device__ __forceinline__; a tuning macro (FA_WAVES) set before the include wins.
#pragma once
#include "common.h"
#include "attention_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf8_t;
typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((ext_vector_type(8))) short s8_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ bf8_t as_bf8(uint4 v) { return __builtin_bit_cast(bf8_t, v); }
__device__ __forceinline__ uint4 ld16(const void* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ bf8_t lds_b128(const char* base, int off) {
  return as_bf8(*reinterpret_cast<const uint4*>(base + off));
}
// transposed read: lane i of each 16-lane group receives column i of a 4-row x 16-col block;
// lane 4q+p supplies the address of (row q, cols 4p..4p+3)
__device__ __forceinline__ s4_t lds_tr(const char* addr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(addr));
}
__device__ __forceinline__ bf8_t cat_tr(s4_t lo, s4_t hi) {
  s8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf8_t, v);
}
// 8 f32 -> bf16x8 operand: elements 0..3 from a, 4..7 from b
__device__ __forceinline__ bf8_t pack8(f32x4_t a, f32x4_t b) {
  uint4 v;
  v.x = pack_bf16x2(a[0], a[1]); v.y = pack_bf16x2(a[2], a[3]);
  v.z = pack_bf16x2(b[0], b[1]); v.w = pack_bf16x2(b[2], b[3]);
  return as_bf8(v);
}
// 8 bf16 (one uint4) times a scalar, rounded back to bf16 (RNE)
__device__ __forceinline__ uint4 scale_bf16x8(uint4 v, float c) {
  uint4 r;
  r.x = pack_bf16x2(__uint_as_float(v.x << 16) * c, __uint_as_float(v.x & 0xffff0000u) * c);
  r.y = pack_bf16x2(__uint_as_float(v.y << 16) * c, __uint_as_float(v.y & 0xffff0000u) * c);
  r.z = pack_bf16x2(__uint_as_float(v.z << 16) * c, __uint_as_float(v.z & 0xffff0000u) * c);
  r.w = pack_bf16x2(__uint_as_float(v.w << 16) * c, __uint_as_float(v.w & 0xffff0000u) * c);
  return r;
}
__device__ __forceinline__ float bf16_round(float x) { return __uint_as_float(pack_bf16x2(x, 0.f) << 16); }
// x ~= hi + lo with both exactly representable in bf16 (relative error ~2^-17): packed {hi, lo}
__device__ __forceinline__ unsigned int bf16_hi_lo(float x) {
  float hi = bf16_round(x);
  return pack_bf16x2(hi, x - hi);
}
__device__ __forceinline__ float xmax4(float v) {   // max over the 4 lane groups (lanes l, l^16, l^32, l^48)
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xsum4(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float swap32(float v) {     // value of lane ^ 32
  unsigned int u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}
__device__ __forceinline__ int xcd_remap(int bid, int nb) {   // bijective: blocks sharing an XCD get adjacent logical ids
  int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7, slot = bid >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// ---- 16x16x32 kernels (attention_mfma.hip, attention_rpe.hip) --------------------------------------------------------
// LDS images: "row" images ([row][DP] bf16, XOR-swizzled 16-B chunks, conflict-free ds_read_b128) and "tr" images
// ([row][D] plain, for the transposed reads)
template <int D> struct ACfg {
  static constexpr int DP = (D <= 32) ? 32 : 64;   // padded contraction width of QK^T / dO V^T
  static constexpr int NKS = DP / 32;              // 32-wide k steps over d
  static constexpr int NDT = D / 16;               // 16-wide d tiles
  static constexpr int CH = D / 8;                 // 16-byte chunks per global row
  static constexpr int CHP = DP / 8;               // 16-byte chunks per padded LDS row
  static constexpr int ROWB = DP * 2;              // bytes per row of a "row" image
  static constexpr int TRB = D * 2;                // bytes per row of a "tr" image
};
template <int D> __device__ __forceinline__ int row_img_off(int row, int chunk) {
  if (ACfg<D>::DP == 64) return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
  return row * 64 + ((chunk ^ ((3 * (row >> 2)) & 3)) << 4);
}

// FA_WAVES waves per workgroup, each owning FA_NT = 2 sixteen-wide tiles (32 queries, or 32 keys in the dK/dV
// kernels): ~100-130 VGPRs per wave so several waves share a SIMD and one wave's softmax VALU work overlaps another's
// MFMAs (a 4-tile / 4-wave variant needed >256 registers and spent half its instructions on v_accvgpr copies: 7.7k
// cycles per 64-key tile against 0.9k of MFMA).
#define FA_NT 2
#ifndef FA_WAVES
#define FA_WAVES 4
#endif
#define FA_THREADS (64 * FA_WAVES)
#define FA_WQ (16 * FA_NT)            // rows (queries / keys) per wave
#define FA_BQ (FA_WQ * FA_WAVES)      // rows per workgroup
#define FA_BK 64
#define FA_IDX_CAP SS_ATTN_MFMA_MAX_WINDOW   // longest window whose gather rows fit the LDS copy (launchers refuse longer ones)

// stage a 64-row K/V tile (window slots r0 .. r0+63, column blocks colofs_a = K and colofs_b = V) into registers.
// gidx_w: the window's gather rows as 16-byte offsets (row * 3C / 8), copied to LDS once per workgroup (FA_IDX_CAP), so the
// address is one shift-add -- a per-step global index load followed by the dependent row load put a full memory round trip
// (s_waitcnt vmcnt(0)) inside every step.  Rows past the window end are clamped to its last row: finite duplicates whose
// scores are masked (K) or multiplied by p = 0 (V), so no zero fill and no divergent branch.
template <int D, int NLD>
__device__ __forceinline__ void tile_load(uint4 (&reg)[NLD], const unsigned short* __restrict__ qkv, const int32_t* gidx_w,
                                          int r0, int L, int colofs_a, int colofs_b, int tid) {
  constexpr int CH = ACfg<D>::CH;
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    int c = i * FA_THREADS + tid;
    int second = c >= 64 * CH;
    int cc = second ? c - 64 * CH : c;
    int r = cc / CH, ch = cc - r * CH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((2 * 64 * CH) % FA_THREADS == 0 || c < 2 * 64 * CH) {
      const uint64_t o16 = (uint32_t)gidx_w[min(r0 + r, L - 1)];
      v = ld16(reinterpret_cast<const char*>(qkv + (second ? colofs_b : colofs_a) + ch * 8) + (o16 << 4));
    }
    reg[i] = v;
  }
}
