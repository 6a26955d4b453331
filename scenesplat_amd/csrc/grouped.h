// Grouped launches: many small problems in ONE launch (the contract of the C entry points is in scenesplat_hip.h).
// desc holds one row of int64 words per problem, wg_start (nprob + 1) the first workgroup of every problem and, last, the launch's
// total.  wg_start is non-decreasing (an empty problem repeats its neighbour's value) and wg_start[0] = 0, so every workgroup b of
// the launch has exactly one owner: the LAST problem p with wg_start[p] <= b.  It works on the problem's piece b - wg_start[p].
#pragma once
#include "common.h"

// the owner of workgroup b by binary search (b is the block index: the search is uniform over the workgroup)
__device__ __forceinline__ int group_owner(const int32_t* __restrict__ wg_start, int nprob, int b) {
  int lo = 0, hi = nprob - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (wg_start[mid] <= b) lo = mid; else hi = mid - 1; }
  return lo;
}

// the guard the entry points share: an empty launch is SS_OK without a launch, a null table SS_ERR_ARG
#define SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups)            \
  do {                                                                      \
    if ((nprob) <= 0 || (total_workgroups) <= 0) return SS_OK;              \
    if (!(desc) || !(wg_start)) return SS_ERR_ARG;                          \
  } while (0)

// tensor pointers come out of the descriptor table as integers: typed as global-address-space pointers they compile to global_load /
// global_store (a plain float* from an integer is a generic pointer: flat_ instructions, which also occupy the LDS counter)
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) const float cgf32;
typedef __attribute__((address_space(1))) f32x4_t gf32x4;
typedef __attribute__((address_space(1))) const f32x4_t cgf32x4;
__device__ __forceinline__ f32x4_t ld4(cgf32* p) { return *reinterpret_cast<cgf32x4*>(p); }
__device__ __forceinline__ f32x4_t ld4(gf32* p) { return *reinterpret_cast<cgf32x4*>(p); }
__device__ __forceinline__ void st4(gf32* p, f32x4_t v) { *reinterpret_cast<gf32x4*>(p) = v; }

// The elementwise kernels: a workgroup of 256 threads owns the PER_WG consecutive elements of one tensor that start at e0.
// vec16 (every base pointer of the row is 16-byte aligned): thread t takes the W elements at e0 + (i * 256 + t) * W, i ascending,
// through body_vec(e); the one thread whose W elements straddle numel walks the tail through body_one(k).  Otherwise one element
// per thread and pass through body_one.  The per-thread element order is part of the results (fixed-order sums).
template <int PER_WG, int W, typename BodyVec, typename BodyOne>
__device__ __forceinline__ void group_span(int64_t e0, int64_t numel, bool vec16, BodyVec body_vec, BodyOne body_one) {
  if (vec16) {
#pragma unroll
    for (int i = 0; i < PER_WG / (256 * W); ++i) {
      const int64_t e = e0 + ((int64_t)i * 256 + threadIdx.x) * W;
      if (e + W <= numel) body_vec(e);
      else for (int64_t k = e; k < numel; ++k) body_one(k);
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < PER_WG / 256; ++i) {
      const int64_t k = e0 + (int64_t)i * 256 + threadIdx.x;
      if (k < numel) body_one(k);
    }
  }
}
