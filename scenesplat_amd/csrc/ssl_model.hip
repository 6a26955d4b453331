// Kernels of the SimDINO pretraining model (pointcept/models/simdinov2.py:191-302 update_teacher / mask_generator,
// point_transformer_v3m1_ssl.py:733-737 the mask token).  All HBM-bound row passes: one thread per element or row, grid-stride, at most
// SSLM_MAX_BLOCKS workgroups.  Reductions are per-block partials in a fixed order plus a one-workgroup finish: no float atomics, the same
// bits on every run.
//   mask generator   keys (sample, z, y, x) of the mask cells -> [ss_argsort_i64 + ss_pool_partition give the dense cell rank] -> patch
//                    starts / counts per sample -> [host draws one byte per patch] -> point mask, ascending masked-row index and the
//                    per-row fp16 weights, compacted by a three-pass ordered scan.
//   mask token       out = mask ? token : x, and its backward (dx, dtoken).
//   grouped EMA      teacher = m * teacher + (1 - m) * student over a descriptor table, the layout of ss_adamw_group (csrc/optim.hip).
#include "grouped.h"

namespace {

constexpr int SSLM_BLOCK = 256;
constexpr int SSLM_MAX_BLOCKS = 1024;

inline int sslm_blocks(int64_t n) {
  const int64_t b = (n + SSLM_BLOCK - 1) / SSLM_BLOCK;
  return (int)(b < 1 ? 1 : (b > SSLM_MAX_BLOCKS ? SSLM_MAX_BLOCKS : b));
}

// sample of row i: the first b with offset[b] > i (offset = inclusive row ends, ascending; empty samples are skipped)
__device__ __forceinline__ int sample_of(const int32_t* __restrict__ offset, int num_batches, int64_t i) {
  int lo = 0, hi = num_batches - 1;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)offset[mid] > i) hi = mid; else lo = mid + 1; }
  return lo;
}

// ---- mask generator, step 1a: sort keys -----------------------------------------------------------------------------------------
// cell = floor(float(grid_coord) / mask_grid_size) in fp32 with an IEEE divide, what torch computes for an int tensor divided by a Python
// float.  The dense patch id of the reference is the rank of voxel_grid's cluster index x + y * ex + z * ex * ey among the sample's
// occupied cells (x fastest; extents max + 1 after the per-sample minimum is subtracted).  torch_cluster is not part of this project's
// environment: that order is taken from its documented formula, not from a run of it.  The rank by that index is the rank by (z, y, x)
// compared lexicographically, which needs neither the minimum nor the extents, so the key is sample | z | y | x with 12 + 3 x 17 bits.
// A cell outside [0, 2^17) or more than 4096 samples sets status[0] (every thread that writes it writes 1).
constexpr int CELL_BITS = 17;
constexpr int MASK_MAX_SAMPLES = 4096;

__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_keys(const int32_t* __restrict__ gc, const int32_t* __restrict__ offset, int num_batches, int64_t n, float size,
            int64_t* __restrict__ keys, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * SSLM_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSLM_BLOCK) {
    const int b = sample_of(offset, num_batches, i);
    int64_t key = (int64_t)b;
    bool bad = false;
#pragma unroll
    for (int a = 2; a >= 0; --a) {
      const float c = floorf(__fdiv_rn((float)gc[i * 3 + a], size));
      bad = bad || !(c >= 0.0f && c < (float)(1 << CELL_BITS));
      key = (key << CELL_BITS) | (int64_t)(bad ? 0 : (int)c);
    }
    keys[i] = key;
    if (bad) status[0] = 1;
  }
}

// ---- step 1b: patch_start (B + 1), patch_count (B) from the global cell rank ----------------------------------------------------------
// The rows of sample b are the sorted positions [offset[b-1], offset[b]) (the sample is the key's top field and the sort is stable), so its
// first patch is the cluster of the row at sorted position offset[b-1]; an empty sample starts where the next one does.
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_patch_starts(const int32_t* __restrict__ cluster, const int32_t* __restrict__ order, const int32_t* __restrict__ offset,
                    int num_batches, int64_t n, const int32_t* __restrict__ n_out, int32_t* __restrict__ patch_start,
                    int32_t* __restrict__ patch_count) {
  for (int b = blockIdx.x * SSLM_BLOCK + threadIdx.x; b <= num_batches; b += gridDim.x * SSLM_BLOCK) {
    const int64_t r0 = b == 0 ? 0 : (int64_t)offset[b - 1];
    const int s0 = (b < num_batches && r0 < n) ? cluster[order[r0]] : n_out[0];
    patch_start[b] = s0;
    if (b < num_batches) {
      const int64_t r1 = (int64_t)offset[b];
      const int s1 = (b + 1 < num_batches && r1 < n) ? cluster[order[r1]] : n_out[0];
      patch_count[b] = s1 - s0;
    }
  }
}

// patch_id[i] = cluster[i] - patch_start[sample of i]
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_patch_ids(const int32_t* __restrict__ cluster, const int32_t* __restrict__ offset, int num_batches, int64_t n,
                 const int32_t* __restrict__ patch_start, int32_t* __restrict__ patch_id) {
  for (int64_t i = (int64_t)blockIdx.x * SSLM_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSLM_BLOCK)
    patch_id[i] = cluster[i] - patch_start[sample_of(offset, num_batches, i)];
}

// ---- step 2: point mask + ordered compaction --------------------------------------------------------------------------------------------
// Workgroup w owns the rows [w * span, (w + 1) * span), span a multiple of the block size, and walks them in tiles of 256 in order.
// pass A writes mask[i] and the workgroup's count; pass B (one workgroup) turns the counts into exclusive bases and the total; pass C walks
// the same rows again and writes index / weight at base + (rank inside the workgroup): ascending row order, no atomics.
__device__ __forceinline__ bool mask_of(const uint8_t* __restrict__ selected, const int32_t* __restrict__ patch_id,
                                        const int32_t* __restrict__ patch_start, int b, int64_t i) {
  return patch_id ? selected[(int64_t)patch_start[b] + patch_id[i]] != 0 : selected[i] != 0;
}

__device__ __forceinline__ int block_count(bool p, int* lds) {
  const unsigned long long bal = __ballot(p);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  const int c = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return c;
}

__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_apply(const uint8_t* __restrict__ selected, const int32_t* __restrict__ patch_id, const int32_t* __restrict__ patch_start,
             const int32_t* __restrict__ offset, int num_batches, int64_t n, int64_t span, uint8_t* __restrict__ mask,
             int32_t* __restrict__ counts) {
  __shared__ int lds[4];
  const int64_t r0 = (int64_t)blockIdx.x * span, r1 = r0 + span < n ? r0 + span : n;
  int total = 0;
  for (int64_t t = r0; t < r1; t += SSLM_BLOCK) {
    const int64_t i = t + threadIdx.x;
    bool p = false;
    if (i < r1) {
      p = mask_of(selected, patch_id, patch_start, sample_of(offset, num_batches, i), i);
      mask[i] = p ? 1 : 0;
    }
    total += block_count(p, lds);
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts (nb <= SSLM_MAX_BLOCKS) -> exclusive bases in place, total -> count_out[0]
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_scan(int32_t* __restrict__ counts, int nb, int32_t* __restrict__ count_out) {
  __shared__ int part[SSLM_BLOCK];
  constexpr int PER = SSLM_MAX_BLOCKS / SSLM_BLOCK;
  int v[PER], s = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { const int j = threadIdx.x * PER + k; v[k] = j < nb ? counts[j] : 0; s += v[k]; }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < SSLM_BLOCK; ++t) { const int c = part[t]; part[t] = run; run += c; }
    count_out[0] = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
#pragma unroll
  for (int k = 0; k < PER; ++k) { const int j = threadIdx.x * PER + k; if (j < nb) counts[j] = run; run += v[k]; }
}

__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_compact(const uint8_t* __restrict__ mask, const int32_t* __restrict__ offset, int num_batches, int64_t n, int64_t span,
               const int32_t* __restrict__ bases, const uint16_t* __restrict__ sample_weight, int32_t* __restrict__ index,
               uint16_t* __restrict__ weight) {
  __shared__ int lds[4];
  const int64_t r0 = (int64_t)blockIdx.x * span, r1 = r0 + span < n ? r0 + span : n;
  int base = bases[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t t = r0; t < r1; t += SSLM_BLOCK) {
    const int64_t i = t + threadIdx.x;
    const bool p = i < r1 && mask[i] != 0;
    const unsigned long long bal = __ballot(p);
    if (lane == 0) lds[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += lds[w];
    const int tile = lds[0] + lds[1] + lds[2] + lds[3];
    if (p) {
      const int pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      index[pos] = (int32_t)i;
      weight[pos] = sample_weight[sample_of(offset, num_batches, i)];
    }
    base += tile;
    __syncthreads();
  }
}

// ---- mask token ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_token_fwd(const T* __restrict__ x, const uint8_t* __restrict__ mask, const float* __restrict__ token, int64_t n, int C,
                 T* __restrict__ out) {
  const int64_t total = n * C;
  for (int64_t e = (int64_t)blockIdx.x * SSLM_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SSLM_BLOCK) {
    const int64_t i = e / C;
    if (mask[i]) ElemIO<T>::store(out + e, token[e - i * C]);
    else out[e] = x[e];
  }
}

// dx = mask ? 0 : g, and partial[w][c] = sum of the masked g[i][c] of workgroup w's rows.  A workgroup of 256 threads holds R = 256 / C
// row slots of C channels (thread t = slot * C + c: consecutive threads read consecutive addresses); slot s of workgroup w adds rows
// r0 + s, r0 + s + R, ... of [w * span, (w + 1) * span) in that order, then channel c adds its R slots in slot order.
template <typename T>
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_token_bwd(const T* __restrict__ g, const uint8_t* __restrict__ mask, int64_t n, int C, int64_t span, T* __restrict__ dx,
                 float* __restrict__ partial) {
  __shared__ float lds[SSLM_BLOCK];
  const int R = SSLM_BLOCK / C;
  const int slot = threadIdx.x / C, c = threadIdx.x - slot * C;
  const int64_t r0 = (int64_t)blockIdx.x * span, r1 = r0 + span < n ? r0 + span : n;
  float acc = 0.0f;
  if (slot < R) {
    for (int64_t i = r0 + slot; i < r1; i += R) {
      const T v = g[i * C + c];
      if (mask[i]) { acc = __fadd_rn(acc, ElemIO<T>::load(&v)); ElemIO<T>::store(dx + i * C + c, 0.0f); }
      else dx[i * C + c] = v;
    }
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < C) {
    float s = lds[threadIdx.x];
    for (int k = 1; k < R; ++k) s = __fadd_rn(s, lds[k * C + threadIdx.x]);
    partial[(int64_t)blockIdx.x * C + threadIdx.x] = s;
  }
}

// dtoken[c] = partial[0][c] + partial[1][c] + ... in workgroup order
__global__ void __launch_bounds__(SSLM_BLOCK)
k_mask_token_finish(const float* __restrict__ partial, int nb, int C, float* __restrict__ dtoken) {
  const int c = blockIdx.x * SSLM_BLOCK + threadIdx.x;
  if (c >= C) return;
  float s = partial[c];
  for (int w = 1; w < nb; ++w) s = __fadd_rn(s, partial[(int64_t)w * C + c]);
  dtoken[c] = s;
}

// ---- grouped EMA ---------------------------------------------------------------------------------------------------------------------------
// desc: 4 int64 words per pair = {teacher f32 pointer, student f32 pointer, numel, flags}; flags as in optim.hip.  The arithmetic
// is torch._foreach_mul_(t, m) followed by torch._foreach_add_(t, s, alpha = 1 - m) with every rounding kept: (m * t) + (alpha * s), three
// fp32 roundings, never contracted into an fma.
#define EMA_PER_WG 8192

__device__ __forceinline__ float ema_elem(float t, float s, float m, float alpha) {
  return __fadd_rn(__fmul_rn(t, m), __fmul_rn(alpha, s));
}

__global__ void __launch_bounds__(256)
k_ema_group(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob, float m, float alpha) {
  const int b = blockIdx.x;
  const int lo = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)lo * 4;
  gf32* t = reinterpret_cast<gf32*>(d[0]);
  cgf32* s = reinterpret_cast<cgf32*>(d[1]);
  group_span<EMA_PER_WG, 4>(
      (int64_t)(b - wg_start[lo]) * EMA_PER_WG, d[2], d[3] & 1,
      [&](int64_t e) {
        f32x4_t tv = ld4(t + e);
        const f32x4_t sv = ld4(s + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) tv[k] = ema_elem(tv[k], sv[k], m, alpha);
        st4(t + e, tv);
      },
      [&](int64_t k) { t[k] = ema_elem(t[k], s[k], m, alpha); });
}

// rows per workgroup of the ordered passes: the rows split evenly over the workgroups, rounded up to whole tiles
inline int64_t sslm_span(int64_t n, int nb) {
  const int64_t per = (n + nb - 1) / nb;
  return (per + SSLM_BLOCK - 1) / SSLM_BLOCK * SSLM_BLOCK;
}

}  // namespace

extern "C" int ss_mask_max_samples(void) { return MASK_MAX_SAMPLES; }
extern "C" int ss_mask_key_bits(void) { return 12 + 3 * CELL_BITS; }

extern "C" int ss_mask_keys(const int32_t* grid_coord, const int32_t* offset, int num_batches, int64_t n, float mask_grid_size,
                            int64_t* keys, int32_t* status, hipStream_t stream) {
  if (n < 0 || num_batches < 0 || !status || !(mask_grid_size > 0.0f)) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!grid_coord || !offset || !keys || num_batches < 1 || num_batches > MASK_MAX_SAMPLES || n >= (1ll << 31)) return SS_ERR_ARG;
  SS_LAUNCH(k_mask_keys, dim3(sslm_blocks(n)), dim3(SSLM_BLOCK), 0, stream, grid_coord, offset, num_batches, n, mask_grid_size, keys, status);
  return SS_OK;
}

extern "C" int ss_mask_patches(const int32_t* cluster, const int32_t* order, const int32_t* offset, int num_batches, int64_t n,
                               const int32_t* n_out, int32_t* patch_start, int32_t* patch_count, int32_t* patch_id, hipStream_t stream) {
  if (n < 0 || num_batches < 1 || !offset || !n_out || !patch_start || !patch_count) return SS_ERR_ARG;
  if (n > 0 && (!cluster || !order || !patch_id)) return SS_ERR_ARG;
  SS_LAUNCH(k_mask_patch_starts, dim3(sslm_blocks(num_batches + 1)), dim3(SSLM_BLOCK), 0, stream, cluster, order, offset, num_batches, n,
            n_out, patch_start, patch_count);
  if (n > 0)
    SS_LAUNCH(k_mask_patch_ids, dim3(sslm_blocks(n)), dim3(SSLM_BLOCK), 0, stream, cluster, offset, num_batches, n, patch_start, patch_id);
  return SS_OK;
}

extern "C" int ss_mask_select_blocks(int64_t n) { return sslm_blocks(n); }

extern "C" int ss_mask_select(const uint8_t* selected, const int32_t* patch_id, const int32_t* patch_start, const int32_t* offset,
                              int num_batches, int64_t n, const uint16_t* sample_weight, uint8_t* mask, int32_t* index,
                              uint16_t* weight, int32_t* count, int32_t* block_counts, hipStream_t stream) {
  if (n < 0 || !count) return SS_ERR_ARG;
  const int nb = sslm_blocks(n);
  if (n > 0 && (!selected || !offset || num_batches < 1 || !sample_weight || !mask || !index || !weight || !block_counts)) return SS_ERR_ARG;
  if (n > 0 && patch_id && !patch_start) return SS_ERR_ARG;
  if (n == 0) {
    (void)hipGetLastError();
    if (hipMemsetAsync(count, 0, sizeof(int32_t), stream) != hipSuccess) return SS_ERR_LAUNCH;
    return SS_OK;
  }
  const int64_t span = sslm_span(n, nb);
  SS_LAUNCH(k_mask_apply, dim3(nb), dim3(SSLM_BLOCK), 0, stream, selected, patch_id, patch_start, offset, num_batches, n, span, mask, block_counts);
  SS_LAUNCH(k_mask_scan, dim3(1), dim3(SSLM_BLOCK), 0, stream, block_counts, nb, count);
  SS_LAUNCH(k_mask_compact, dim3(nb), dim3(SSLM_BLOCK), 0, stream, mask, offset, num_batches, n, span, block_counts, sample_weight, index, weight);
  return SS_OK;
}

extern "C" int ss_mask_token_fwd(const void* x, int dtype, const uint8_t* mask, const float* token, int64_t n, int channels, void* out,
                                 hipStream_t stream) {
  if (n < 0 || channels < 1 || (dtype != SS_F32 && dtype != SS_BF16)) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!x || !mask || !token || !out) return SS_ERR_ARG;
  const int nb = sslm_blocks(n * channels);
  if (dtype == SS_F32)
    SS_LAUNCH(k_mask_token_fwd<float>, dim3(nb), dim3(SSLM_BLOCK), 0, stream, (const float*)x, mask, token, n, channels, (float*)out);
  else
    SS_LAUNCH(k_mask_token_fwd<unsigned short>, dim3(nb), dim3(SSLM_BLOCK), 0, stream, (const unsigned short*)x, mask, token, n, channels,
              (unsigned short*)out);
  return SS_OK;
}

#define MASK_TOKEN_BWD_MAX_BLOCKS 256
extern "C" int ss_mask_token_bwd_blocks(int64_t n) {
  const int64_t b = (n + SSLM_BLOCK - 1) / SSLM_BLOCK;
  return (int)(b < 1 ? 1 : (b > MASK_TOKEN_BWD_MAX_BLOCKS ? MASK_TOKEN_BWD_MAX_BLOCKS : b));
}
extern "C" int64_t ss_mask_token_bwd_span(int64_t n) { return sslm_span(n < 1 ? 1 : n, ss_mask_token_bwd_blocks(n)); }

extern "C" int ss_mask_token_bwd(const void* g, int dtype, const uint8_t* mask, int64_t n, int channels, void* dx, float* partial,
                                 float* dtoken, hipStream_t stream) {
  if (n < 0 || channels < 1 || channels > SSLM_BLOCK || (dtype != SS_F32 && dtype != SS_BF16) || !dtoken) return SS_ERR_ARG;
  if (n == 0) {
    (void)hipGetLastError();
    if (hipMemsetAsync(dtoken, 0, sizeof(float) * channels, stream) != hipSuccess) return SS_ERR_LAUNCH;
    return SS_OK;
  }
  if (!g || !mask || !dx || !partial) return SS_ERR_ARG;
  const int nb = ss_mask_token_bwd_blocks(n);
  const int64_t span = sslm_span(n, nb);
  if (dtype == SS_F32)
    SS_LAUNCH(k_mask_token_bwd<float>, dim3(nb), dim3(SSLM_BLOCK), 0, stream, (const float*)g, mask, n, channels, span, (float*)dx, partial);
  else
    SS_LAUNCH(k_mask_token_bwd<unsigned short>, dim3(nb), dim3(SSLM_BLOCK), 0, stream, (const unsigned short*)g, mask, n, channels, span,
              (unsigned short*)dx, partial);
  SS_LAUNCH(k_mask_token_finish, dim3(1), dim3(SSLM_BLOCK), 0, stream, partial, nb, channels, dtoken);
  return SS_OK;
}

extern "C" int ss_ema_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, float m, float alpha,
                            hipStream_t stream) {
  SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups);
  SS_LAUNCH(k_ema_group, dim3((unsigned)total_workgroups), dim3(256), 0, stream, desc, wg_start, nprob, m, alpha);
  return SS_OK;
}
