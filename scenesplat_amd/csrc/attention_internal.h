// Internal interface between the packed-layout attention files: attention.hip (the C-ABI entry points) calls the launchers
// of attention_simt.hip, attention_mfma.hip, attention_mfma32.hip and attention_rpe.hip declared here.
#pragma once
#include "common.h"
#define SS_ATTN_MFMA_MAX_WINDOW 2048   // = FA_IDX_CAP of attention_frag.h; longer windows run on the SIMT kernels

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }   // workspace parts start 256-byte aligned

// ---- relative position encoding (ss_window_attn_rpe_*) ----
// largest pos_bnd whose 3 * (2 * pos_bnd + 1) table column fits the kernels' LDS copy
#define SS_ATTN_RPE_MAX_POS_BND 64   // patch sizes up to 8192: int((4 * 8192) ** (1 / 3) * 2)
#define RPE_MAX_BINS (3 * (2 * SS_ATTN_RPE_MAX_POS_BND + 1))
#define RPE_LOG2E 1.44269504088896340736f
// table index of one axis: qp = query coordinate + pos_bnd (or kc = key coordinate - pos_bnd), result in [0, 2 pos_bnd]
__device__ __forceinline__ int rpe_bin(int qp_minus_k, int pb2) { return min(max(qp_minus_k, 0), pb2); }
// RPE operands of a launch.  slab (backward only): per-workgroup partial sums of dtable, (nslab, H, 3 * (2 pos_bnd + 1)) f32
struct SsAttnRpe { const int32_t* gc; const float* table; int pos_bnd; float* slab; };
// the workspace holds one slab per (window, 128-query chunk of the MFMA dQ kernel); the SIMT dQ kernel fills one per window
#define SS_ATTN_RPE_BQ 128
static inline int ss_attn_rpe_chunks(int max_window) { return max_window > 0 ? (max_window + SS_ATTN_RPE_BQ - 1) / SS_ATTN_RPE_BQ : 1; }

// ---- attention_simt.hip: rpe == nullptr runs the plain kernels ----
int ss_attn_fwd_simt(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int W,
                     void* out, float* lse, int C, int H, float scale, int dtype, const SsAttnRpe* rpe, hipStream_t st);
int ss_attn_delta(const void* out, const void* dout, const int32_t* sidx, float* delta, int64_t n_pad, int C, int H,
                  int dtype, hipStream_t st);
int ss_attn_fix_borrowed(const int32_t* gidx, const int32_t* sidx, int64_t n_pad, const void* extra, void* dqkv, int C,
                         int dtype, hipStream_t st);
int ss_attn_bwd_simt(const void* qkv, const void* dout, const float* lse, const float* delta, const int32_t* gidx,
                     const int32_t* sidx, const int32_t* win_start, int W, void* dqkv, void* extra, int C, int H,
                     float scale, int dtype, const SsAttnRpe* rpe, hipStream_t st);
// ---- attention_mfma.hip ----
int ss_attn_fwd_mfma(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int W,
                     int max_window, void* out, float* lse, int C, int H, float scale, hipStream_t st);
// delta (n_pad, H) is an OUTPUT of the dQ kernel here (rowsum(out o dout), consumed by the dK/dV kernel): no ss_attn_delta pass
int ss_attn_bwd_mfma(const void* qkv, const void* dout, const void* out, const float* lse, float* delta, const int32_t* gidx,
                     const int32_t* sidx, const int32_t* win_start, int W, int max_window, void* dqkv, void* extra,
                     int C, int H, float scale, hipStream_t st);
// 32x32x16 re-tiling of the forward (attention_mfma32.hip); same contract as ss_attn_fwd_mfma
int ss_attn_fwd_mfma32(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int W,
                       int max_window, void* out, float* lse, int C, int H, float scale, hipStream_t st);
// ---- attention_rpe.hip: the MFMA kernels with RPE, contracts of ss_attn_fwd_mfma / ss_attn_bwd_mfma; the backward fills
// W * ss_attn_rpe_chunks(max_window) slabs.  ss_attn_rpe_dtable_reduce overwrites dtable with the sum of nslab slabs
// (zeros for nslab = 0), after either backward.
int ss_attn_rpe_fwd_mfma(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int W,
                         int max_window, void* out, float* lse, int C, int H, float scale, const SsAttnRpe& rpe, hipStream_t st);
int ss_attn_rpe_bwd_mfma(const void* qkv, const void* dout, const void* out, const float* lse, float* delta, const int32_t* gidx,
                         const int32_t* sidx, const int32_t* win_start, int W, int max_window, void* dqkv, void* extra,
                         int C, int H, float scale, const SsAttnRpe& rpe, hipStream_t st);
int ss_attn_rpe_dtable_reduce(const float* slab, int nslab, int H, int pos_bnd, float* dtable, hipStream_t st);
