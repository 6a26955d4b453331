// Scene chunking: pointcept/datasets/preprocessing/sampling_chunking_data_gs.py::chunking_scene over a scene arena on the device.
//   extent / recentre   column min / max of coord (per-block partials + a finish step, no atomics) and coord - min (fp32, rounded once)
//   lang normalise      lang_feat[valid] /= its L2 norm: one wave per row, fp32 sums, one rounding to the storage dtype
//   grid subsample      cell keys (IEEE division) -> radix argsort + ss_pool_partition (serialize.hip) -> per cell the smallest row and
//                       the pick; a second argsort by smallest row puts the cells in the reference's first-occurrence order
//   membership          every row writes the chunks it lies in into its `slots` key slots; ONE stable argsort of the slots lists the
//                       rows of every chunk in ascending row order (no atomic decides a position), integer atomics only count
//   grouped gather      (chunk, asset) problems in one launch: dst[i] = src[pick[idx[i]]], 16 / 4 / 2 / 1-byte words by alignment
// Everything here is bound by memory; only the gather moves more than a few bytes per row.
#include "grouped.h"

typedef __attribute__((ext_vector_type(4))) unsigned int ck_u32x4;

// ---- extent and recentre ----------------------------------------------------------------------------------------------------------
#define CK_EXT_ROWS_PER_WG 4096
#define CK_EXT_MAX_WG 1024

static inline int ck_extent_blocks(int64_t m) {
  const int64_t b = (m + CK_EXT_ROWS_PER_WG - 1) / CK_EXT_ROWS_PER_WG;
  return (int)(b < 1 ? 1 : b > CK_EXT_MAX_WG ? CK_EXT_MAX_WG : b);
}

// the six extremes of a workgroup's threads -> out6 (thread 0 writes); min / max are exact, so the order of the tree does not matter
__device__ __forceinline__ void ck_block_minmax(float (&lo)[3], float (&hi)[3], float* __restrict__ out6) {
  __shared__ float sh[4][6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { sh[wave][c] = lo[c]; sh[wave][3 + c] = hi[c]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    float v = sh[0][c];
    for (int w = 1; w < 4; ++w) v = c < 3 ? fminf(v, sh[w][c]) : fmaxf(v, sh[w][c]);
    out6[c] = v;
  }
}

__global__ void __launch_bounds__(256)
k_chunk_extent(const float* __restrict__ x, const int32_t* __restrict__ idx, int64_t m, float* __restrict__ partials) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const int64_t r = idx ? (int64_t)idx[i] : i;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float v = x[r * 3 + c]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
  }
  ck_block_minmax(lo, hi, partials + (int64_t)blockIdx.x * 6);
}

__global__ void __launch_bounds__(256)
k_chunk_extent_finish(const float* __restrict__ partials, int blocks, float* __restrict__ out6) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], partials[b * 6 + c]); hi[c] = fmaxf(hi[c], partials[b * 6 + 3 + c]); }
  }
  ck_block_minmax(lo, hi, out6);
}

__global__ void __launch_bounds__(256)
k_chunk_recentre(const float* __restrict__ coord, const float* __restrict__ ext6, int64_t n3, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n3) out[e] = __fsub_rn(coord[e], ext6[e % 3]);
}

extern "C" int ss_chunk_extent_blocks(int64_t m) { return ck_extent_blocks(m); }
extern "C" int ss_chunk_extent(const float* x, const int32_t* idx, int64_t m, float* partials, float* out6, hipStream_t stream) {
  if (m < 1 || !x || !partials || !out6) return SS_ERR_ARG;
  const int blocks = ck_extent_blocks(m);
  SS_LAUNCH(k_chunk_extent, dim3(blocks), dim3(256), 0, stream, x, idx, m, partials);
  SS_LAUNCH(k_chunk_extent_finish, dim3(1), dim3(256), 0, stream, (const float*)partials, blocks, out6);
  return SS_OK;
}
extern "C" int ss_chunk_recentre(const float* coord, const float* ext6, int64_t n, float* out, hipStream_t stream) {
  if (n < 0 || (n > 0 && (!coord || !ext6 || !out))) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  SS_LAUNCH(k_chunk_recentre, dim3(ss_div_up(n * 3, 256)), dim3(256), 0, stream, coord, ext6, n * 3, out);
  return SS_OK;
}

// ---- lang_feat row normalisation ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
k_chunk_lang_normalize(T* __restrict__ feat, const uint8_t* __restrict__ valid, int64_t n, int width) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);    // one wave per row: the branch below is uniform over the wave
  if (row >= n || !valid[row]) return;
  const int lane = threadIdx.x & 63;
  T* __restrict__ p = feat + row * width;
  float acc = 0.f;
  for (int j = lane; j < width; j += 64) { const float v = (float)p[j]; acc = fmaf(v, v, acc); }
  const float norm = __fsqrt_rn(wave_reduce_sum(acc));                  // (the butterfly leaves the same bits in every lane)
  for (int j = lane; j < width; j += 64) p[j] = (T)__fdiv_rn((float)p[j], norm);
}

extern "C" int ss_chunk_lang_normalize(void* feat, int dtype, const uint8_t* valid, int64_t n, int width, hipStream_t stream) {
  if (n < 0 || width < 1 || (dtype != SS_CHUNK_F16 && dtype != SS_CHUNK_F32) || (n > 0 && (!feat || !valid))) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  const dim3 g(ss_div_up(n, 4)), b(256);
  if (dtype == SS_CHUNK_F16) SS_LAUNCH(k_chunk_lang_normalize<_Float16>, g, b, 0, stream, (_Float16*)feat, valid, n, width);
  else SS_LAUNCH(k_chunk_lang_normalize<float>, g, b, 0, stream, (float*)feat, valid, n, width);
  return SS_OK;
}

// ---- grid subsample ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_chunk_cell_keys(const float* __restrict__ rec, int64_t n, float g, int bx, int by, int bz, int64_t* __restrict__ keys,
                  int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float cx = floorf(__fdiv_rn(rec[i * 3 + 0], g)), cy = floorf(__fdiv_rn(rec[i * 3 + 1], g)), cz = floorf(__fdiv_rn(rec[i * 3 + 2], g));
  // (the comparisons are false for NaN: such a row is flagged too)
  const bool ok = cx >= 0.f && cx < (float)(1ll << bx) && cy >= 0.f && cy < (float)(1ll << by) && cz >= 0.f && cz < (float)(1ll << bz);
  int64_t key = 0;
  if (ok) key = ((int64_t)cx << (by + bz)) | ((int64_t)cy << bz) | (int64_t)cz;
  else atomicOr(status, 1);
  keys[i] = key;
}

__global__ void __launch_bounds__(256)
k_chunk_cell_pick(const int32_t* __restrict__ order, const int32_t* __restrict__ idx_ptr, int64_t n_cells,
                  const uint8_t* __restrict__ valid, uint64_t seed, int64_t* __restrict__ first, int32_t* __restrict__ pick) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  const int s = idx_ptr[c], e = idx_ptr[c + 1];
  const int head = order[s];                                          // the sort is stable: a cell's rows come ascending
  int chosen = head;
  if (valid) {
    uint32_t nvalid = 0;
    for (int j = s; j < e; ++j) nvalid += valid[order[j]] ? 1u : 0u;
    if (nvalid) {
      uint32_t w[4] = {(uint32_t)head, 0u, 0x43484e4bu, 0u};
      philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
      uint32_t k = w[0] % nvalid;
      for (int j = s; j < e; ++j) {
        const int r = order[j];
        if (valid[r]) { if (k == 0) { chosen = r; break; } --k; }
      }
    }
  }
  first[c] = head;
  pick[c] = chosen;
}

extern "C" int ss_chunk_cell_keys(const float* rec, int64_t n, float grid_size, int bits_x, int bits_y, int bits_z, int64_t* keys,
                                  int32_t* status, hipStream_t stream) {
  if (n < 0 || !(grid_size > 0.f) || bits_x < 1 || bits_y < 1 || bits_z < 1 || bits_x + bits_y + bits_z > 63) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!rec || !keys || !status) return SS_ERR_ARG;
  SS_LAUNCH(k_chunk_cell_keys, dim3(ss_div_up(n, 256)), dim3(256), 0, stream, rec, n, grid_size, bits_x, bits_y, bits_z, keys, status);
  return SS_OK;
}
extern "C" int ss_chunk_cell_pick(const int32_t* order, const int32_t* idx_ptr, int64_t n_cells, const uint8_t* valid, uint64_t seed,
                                  int64_t* first, int32_t* pick, hipStream_t stream) {
  if (n_cells < 0) return SS_ERR_ARG;
  if (n_cells == 0) return SS_OK;
  if (!order || !idx_ptr || !first || !pick) return SS_ERR_ARG;
  SS_LAUNCH(k_chunk_cell_pick, dim3(ss_div_up(n_cells, 256)), dim3(256), 0, stream, order, idx_ptr, n_cells, valid, seed, first, pick);
  return SS_OK;
}

// ---- membership ----------------------------------------------------------------------------------------------------------------------
#define CK_MEM_ROWS_PER_WG 1024
#define CK_MEM_LDS_BINS 2048

// the last origin t with lo[t] <= v, -1 when there is none (also for NaN)
__device__ __forceinline__ int ck_last_le(const double* __restrict__ lo, int count, double v) {
  int a = 0, b = count;                                               // the answer + 1 lies in [a, b]
  while (a < b) { const int mid = (a + b) >> 1; if (lo[mid] <= v) a = mid + 1; else b = mid; }
  return a - 1;
}

__global__ void __launch_bounds__(256)
k_chunk_membership(const float* __restrict__ rec, const int32_t* __restrict__ pick, int64_t m, const double* __restrict__ bounds,
                   int nx, int ny, int slots, int64_t* __restrict__ slot_keys, int32_t* __restrict__ counts,
                   int32_t* __restrict__ status) {
  __shared__ int32_t hist[CK_MEM_LDS_BINS];
  const int nchunk = nx * ny;
  const bool lds = nchunk <= CK_MEM_LDS_BINS;
  if (lds) {
    for (int c = threadIdx.x; c < nchunk; c += 256) hist[c] = 0;
    __syncthreads();
  }
  const double* __restrict__ lo_x = bounds;
  const double* __restrict__ hi_x = bounds + nx;
  const double* __restrict__ lo_y = bounds + 2 * nx;
  const double* __restrict__ hi_y = bounds + 2 * nx + ny;
  const int64_t i0 = (int64_t)blockIdx.x * CK_MEM_ROWS_PER_WG;
  for (int t = 0; t < CK_MEM_ROWS_PER_WG / 256; ++t) {
    const int64_t i = i0 + t * 256 + threadIdx.x;
    if (i >= m) break;
    const int64_t r = pick ? (int64_t)pick[i] : i;
    const double x = (double)rec[r * 3 + 0], y = (double)rec[r * 3 + 1];
    const int tx = ck_last_le(lo_x, nx, x), ty = ck_last_le(lo_y, ny, y);
    int64_t* __restrict__ out = slot_keys + i * slots;
    int used = 0;
    // hi = lo + range ascends with lo: below the first origin whose upper edge the row has passed there is no member left
    for (int ix = tx; ix >= 0 && x < hi_x[ix]; --ix)
      for (int iy = ty; iy >= 0 && y < hi_y[iy]; --iy) {
        const int chunk = ix * ny + iy;
        if (used < slots) {
          out[used++] = chunk;
          if (lds) atomicAdd(&hist[chunk], 1); else atomicAdd(&counts[chunk], 1);
        } else {
          atomicOr(status, 1);
        }
      }
    for (; used < slots; ++used) out[used] = nchunk;
  }
  if (lds) {
    __syncthreads();
    for (int c = threadIdx.x; c < nchunk; c += 256) { const int v = hist[c]; if (v) atomicAdd(&counts[c], v); }
  }
}

// exclusive running sum of counts: one workgroup, tiles of 256 with a carry
__global__ void __launch_bounds__(256)
k_chunk_offsets(const int32_t* __restrict__ counts, int nchunk, int64_t* __restrict__ offsets) {
  __shared__ int64_t sh[256];
  int64_t carry = 0;
  for (int base = 0; base < nchunk; base += 256) {
    const int c = base + threadIdx.x;
    const int64_t v = c < nchunk ? (int64_t)counts[c] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int64_t add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    if (c < nchunk) offsets[c] = carry + sh[threadIdx.x] - v;
    carry += sh[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[nchunk] = carry;
}

__global__ void __launch_bounds__(256)
k_chunk_slot_rows(const int32_t* __restrict__ slot_order, int64_t total, int slots, int32_t* __restrict__ rows) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < total) rows[p] = slot_order[p] / slots;
}

extern "C" int ss_chunk_membership(const float* rec, const int32_t* pick, int64_t m, const void* bounds, int nx, int ny, int slots,
                                   int64_t* slot_keys, int32_t* counts, int32_t* status, hipStream_t stream) {
  if (m < 0 || nx < 1 || ny < 1 || slots < 1 || (int64_t)nx * ny >= (1ll << 31) || m * slots >= (1ll << 31)) return SS_ERR_ARG;
  if (m == 0) return SS_OK;
  if (!rec || !bounds || !slot_keys || !counts || !status) return SS_ERR_ARG;
  SS_LAUNCH(k_chunk_membership, dim3(ss_div_up(m, CK_MEM_ROWS_PER_WG)), dim3(256), 0, stream, rec, pick, m, (const double*)bounds, nx, ny,
            slots, slot_keys, counts, status);
  return SS_OK;
}
extern "C" int ss_chunk_offsets(const int32_t* counts, int nchunk, int64_t* offsets, hipStream_t stream) {
  if (nchunk < 0 || !offsets || (nchunk > 0 && !counts)) return SS_ERR_ARG;
  SS_LAUNCH(k_chunk_offsets, dim3(1), dim3(256), 0, stream, counts, nchunk, offsets);
  return SS_OK;
}
extern "C" int ss_chunk_slot_rows(const int32_t* slot_order, int64_t total, int slots, int32_t* rows, hipStream_t stream) {
  if (total < 0 || slots < 1) return SS_ERR_ARG;
  if (total == 0) return SS_OK;
  if (!slot_order || !rows) return SS_ERR_ARG;
  SS_LAUNCH(k_chunk_slot_rows, dim3(ss_div_up(total, 256)), dim3(256), 0, stream, slot_order, total, slots, rows);
  return SS_OK;
}

// ---- grouped row gather --------------------------------------------------------------------------------------------------------------
#define CK_GATHER_BYTES_PER_WG 32768
#define CK_GATHER_MAX_ROWS_PER_WG 4096

static inline int ck_gather_rows_per_wg(int64_t row_bytes) {
  if (row_bytes < 1) return CK_GATHER_MAX_ROWS_PER_WG;
  const int64_t r = CK_GATHER_BYTES_PER_WG / row_bytes;
  return (int)(r < 1 ? 1 : r > CK_GATHER_MAX_ROWS_PER_WG ? CK_GATHER_MAX_ROWS_PER_WG : r);
}

// rows [r0, r1) of one problem in words of type W: consecutive threads take consecutive words of a row, then of the next row
template <typename W>
__device__ __forceinline__ void ck_gather_span(const int64_t* __restrict__ d, int64_t r0, int64_t r1) {
  typedef __attribute__((address_space(1))) const W gS;
  typedef __attribute__((address_space(1))) W gD;
  typedef __attribute__((address_space(1))) const int32_t gI;
  const int64_t rb = d[4], src_rows = d[6], pick_rows = d[7];
  gI* idx = reinterpret_cast<gI*>(d[2]);
  gI* pick = reinterpret_cast<gI*>(d[5]);
  const uint32_t words = (uint32_t)(rb / (int64_t)sizeof(W));         // per row
  const uint32_t items = (uint32_t)(r1 - r0) * words;                 // <= max(CK_GATHER_BYTES_PER_WG, row_bytes) < 2^31
  if (src_rows < 1 || (d[5] != 0 && pick_rows < 1)) return;           // no index can be followed
  // U words per thread in flight: the three dependent loads (idx, pick, the row) are issued U at a time.  An index outside its
  // table is never followed: the load goes to row 0 instead (it exists, by the line above) and the word is not stored.
  constexpr int U = 4;
  for (uint32_t it0 = threadIdx.x; it0 < items; it0 += 256 * U) {
    uint32_t lr[U], w[U];
    int64_t r[U];
    bool ok[U];
    W v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t it = it0 + u * 256;
      ok[u] = it < items;
      lr[u] = ok[u] ? it / words : 0;
      w[u] = ok[u] ? it - lr[u] * words : 0;
      r[u] = idx[r0 + lr[u]];
    }
    if (d[5] != 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = (uint64_t)r[u] < (uint64_t)pick_rows;
        ok[u] = ok[u] && in;
        r[u] = pick[in ? r[u] : 0];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = (uint64_t)r[u] < (uint64_t)src_rows;
      ok[u] = ok[u] && in;
      v[u] = *(reinterpret_cast<gS*>(d[0] + (in ? r[u] : 0) * rb) + w[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u]) *(reinterpret_cast<gD*>(d[1] + (int64_t)(r0 + lr[u]) * rb) + w[u]) = v[u];
  }
}

__global__ void __launch_bounds__(256)
k_chunk_gather_group(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob) {
  const int b = blockIdx.x;
  const int p = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)p * 8;
  const int64_t n_rows = d[3], rb = d[4];
  if (rb < 1) return;
  const int64_t per = CK_GATHER_BYTES_PER_WG / rb;
  const int64_t rows_per = per < 1 ? 1 : per > CK_GATHER_MAX_ROWS_PER_WG ? CK_GATHER_MAX_ROWS_PER_WG : per;
  const int64_t r0 = (int64_t)(b - wg_start[p]) * rows_per;
  const int64_t r1 = r0 + rows_per < n_rows ? r0 + rows_per : n_rows;
  if (r0 >= r1) return;
  const int64_t align = d[0] | d[1] | rb;                             // uniform over the workgroup
  if ((align & 15) == 0) ck_gather_span<ck_u32x4>(d, r0, r1);
  else if ((align & 3) == 0) ck_gather_span<uint32_t>(d, r0, r1);
  else if ((align & 1) == 0) ck_gather_span<uint16_t>(d, r0, r1);
  else ck_gather_span<uint8_t>(d, r0, r1);
}

extern "C" int ss_chunk_gather_rows_per_workgroup(int64_t row_bytes) { return ck_gather_rows_per_wg(row_bytes); }
extern "C" int ss_chunk_gather_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, hipStream_t stream) {
  SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups);
  SS_LAUNCH(k_chunk_gather_group, dim3((unsigned)total_workgroups), dim3(256), 0, stream, desc, wg_start, nprob);
  return SS_OK;
}
