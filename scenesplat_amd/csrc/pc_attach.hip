// Labelled point cloud -> chunk folders: pointcept/datasets/preprocessing/adding_pc_label_to_gs_chunk.py (SceneCache.slice and
// semseg_label_slice) for a BATCH of chunks of one scene, after ONE k-NN search of all their Gaussian centres in the scene cloud.
//   mark      one lane per (Gaussian, neighbour) pair: fp64 distance of the fp32 coordinates, compared with the limit; a hit sets the
//             bit of its cloud row in the chunk's bitmap (integer OR: the result does not depend on arrival order).  The lane of
//             column 0 also writes the Gaussian's nearest row, or -1 beyond the limit (the 1-NN search of semseg_label_slice).
//   compact   np.unique without a sort: popcount per tile of bitmap words, ONE exclusive scan over the tiles of all chunks (a chunk's
//             tiles are consecutive, so chunk 0's rows come first, then chunk 1's, ...), per-chunk counts for the host's one read,
//             then an emit pass that writes every set bit's row at tile base + rank inside the tile.  No atomic orders anything.
// The gather of the labelled arrays through `rows` is ss_chunk_gather_group (chunking.hip).
// Everything here is bound by memory: mark reads 4 B of idx and (through the caches) 12 B of a cloud row per pair.
#include "common.h"
// the distance of ss_pc_mark is stated operation by operation (numpy's): no product may fuse into a sum anywhere in this file
#pragma clang fp contract(off)

#define PC_THREADS 256
#define PC_MAX_WG 4096                 // grid-stride beyond: 16 workgroups per CU
#define PC_TILE_WORDS 1024             // bitmap words of one compact tile: 4 steps of one word per thread

// the chunk of query row r: the LAST c with q_offset[c] <= r, searched in [0, nc): in range whatever the table holds
__device__ __forceinline__ int pc_chunk_of(const int32_t* __restrict__ q_offset, int nc, int64_t r) {
  int lo = 0, hi = nc - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int64_t)q_offset[mid] <= r) lo = mid; else hi = mid - 1; }
  return lo;
}

__global__ void __launch_bounds__(PC_THREADS)
k_pc_clear(uint32_t* __restrict__ words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PC_THREADS) words[i] = 0u;
}

__global__ void __launch_bounds__(PC_THREADS)
k_pc_mark(const float* __restrict__ pc, int64_t M, const float* __restrict__ q, int64_t m, const int32_t* __restrict__ q_offset, int nc,
          const int32_t* __restrict__ idx, int k, double dist_limit, int64_t words_per_chunk, uint32_t* __restrict__ bitmap,
          int32_t* __restrict__ nearest, int32_t* __restrict__ status) {
  const int64_t pairs = m * k;
  for (int64_t p = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * PC_THREADS) {
    const int64_t row = (uint32_t)p / (uint32_t)k;                     // (pairs < 2^31: the entry point refuses more)
    const int j = (int)(p - row * k);
    const int64_t id = idx[p];
    bool hit = false;
    if (id >= M) {
      atomicOr(status, 1);                                             // never followed
    } else if (id >= 0) {
      // the expression of the module docstring: three fp64 differences, squares added in x, y, z order, no contraction, IEEE sqrt
      const double dx = (double)q[row * 3 + 0] - (double)pc[id * 3 + 0];
      const double dy = (double)q[row * 3 + 1] - (double)pc[id * 3 + 1];
      const double dz = (double)q[row * 3 + 2] - (double)pc[id * 3 + 2];
      const double d = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);        // (contraction is off: five roundings, then the root's)
      hit = d <= dist_limit;                                           // (false for NaN)
      if (hit) {
        const int c = pc_chunk_of(q_offset, nc, row);
        uint32_t* w = bitmap + (int64_t)c * words_per_chunk + (id >> 5);
        const uint32_t bit = 1u << (id & 31);
        // neighbouring Gaussians share neighbours: most bits are set already.  A stale read only costs a redundant atomic.
        if (!(*(volatile uint32_t*)w & bit)) atomicOr(w, bit);
      }
    }
    if (j == 0) nearest[row] = hit ? (int32_t)id : -1;
  }
}

// exclusive scan of one int per thread over the workgroup; *total = the sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ int pc_block_scan(int v, int* total) {
  __shared__ int wave_sum[PC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
  __syncthreads();                                                     // the previous call's reads of wave_sum are over
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < PC_THREADS / 64; ++w) { const int s = wave_sum[w]; if (w < wave) base += s; tot += s; }
  *total = tot;
  return base + inc - v;
}

// word `wi` of a chunk's bitmap, without the bits of rows >= M in a partial last word; 0 beyond the chunk
__device__ __forceinline__ uint32_t pc_word(const uint32_t* __restrict__ chunk_words, int64_t wi, int64_t words_per_chunk, int tail_bits) {
  if (wi >= words_per_chunk) return 0u;
  uint32_t w = chunk_words[wi];
  if (tail_bits && wi == words_per_chunk - 1) w &= (1u << tail_bits) - 1u;
  return w;
}

// tile t = chunk (t / tiles_per_chunk), words [(t % tiles_per_chunk) * PC_TILE_WORDS, + PC_TILE_WORDS) of it
__global__ void __launch_bounds__(PC_THREADS)
k_pc_tile_count(const uint32_t* __restrict__ bitmap, int64_t words_per_chunk, int tail_bits, int tiles_per_chunk, int ntiles,
                int32_t* __restrict__ tile_count) {
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t* __restrict__ words = bitmap + (int64_t)(t / tiles_per_chunk) * words_per_chunk;
    const int64_t w0 = (int64_t)(t % tiles_per_chunk) * PC_TILE_WORDS;
    int n = 0;
#pragma unroll
    for (int s = 0; s < PC_TILE_WORDS / PC_THREADS; ++s) n += __popc(pc_word(words, w0 + s * PC_THREADS + threadIdx.x, words_per_chunk, tail_bits));
    int total;
    pc_block_scan(n, &total);
    if (threadIdx.x == 0) tile_count[t] = total;
  }
}

// tile_base (ntiles + 1) = exclusive running sum of tile_count: one workgroup, pieces of 256 with a carry
__global__ void __launch_bounds__(PC_THREADS)
k_pc_tile_scan(const int32_t* __restrict__ tile_count, int ntiles, int32_t* __restrict__ tile_base) {
  int carry = 0;
  for (int base = 0; base < ntiles; base += PC_THREADS) {
    const int t = base + threadIdx.x;
    const int v = t < ntiles ? tile_count[t] : 0;
    int total;
    const int excl = pc_block_scan(v, &total);
    if (t < ntiles) tile_base[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) tile_base[ntiles] = carry;
}

__global__ void __launch_bounds__(PC_THREADS)
k_pc_chunk_counts(const int32_t* __restrict__ tile_base, int tiles_per_chunk, int nc, int32_t* __restrict__ counts) {
  for (int c = blockIdx.x * PC_THREADS + threadIdx.x; c < nc; c += gridDim.x * PC_THREADS)
    counts[c] = tile_base[(int64_t)(c + 1) * tiles_per_chunk] - tile_base[(int64_t)c * tiles_per_chunk];
}

__global__ void __launch_bounds__(PC_THREADS)
k_pc_emit(const uint32_t* __restrict__ bitmap, int64_t words_per_chunk, int tail_bits, int tiles_per_chunk, int ntiles,
          const int32_t* __restrict__ tile_base, int32_t* __restrict__ rows, int64_t capacity) {
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t* __restrict__ words = bitmap + (int64_t)(t / tiles_per_chunk) * words_per_chunk;
    const int64_t w0 = (int64_t)(t % tiles_per_chunk) * PC_TILE_WORDS;
    int64_t carry = tile_base[t];
    for (int s = 0; s < PC_TILE_WORDS / PC_THREADS; ++s) {
      const int64_t wi = w0 + s * PC_THREADS + threadIdx.x;
      uint32_t w = pc_word(words, wi, words_per_chunk, tail_bits);
      int total;
      int64_t pos = carry + pc_block_scan(__popc(w), &total);
      while (w) {
        const int b = __ffs(w) - 1;
        if (pos < capacity) rows[pos] = (int32_t)(wi * 32 + b);        // (a capacity below the scan's total only loses rows)
        ++pos;
        w &= w - 1u;
      }
      carry += total;
    }
  }
}

static inline int pc_grid(int64_t items) {
  const int64_t b = (items + PC_THREADS - 1) / PC_THREADS;
  return (int)(b < 1 ? 1 : b > PC_MAX_WG ? PC_MAX_WG : b);
}
static inline int64_t pc_words(int64_t M) { return (M + 31) / 32; }
static inline int64_t pc_tiles_per_chunk(int64_t M) { return (pc_words(M) + PC_TILE_WORDS - 1) / PC_TILE_WORDS; }
// every row index and every position of `rows` is an int32, and so is the tile count
static inline bool pc_sizes_ok(int64_t M, int nc) {
  return M >= 1 && nc >= 1 && M < (1ll << 31) && (int64_t)nc * pc_words(M) * 32 < (1ll << 31) && (int64_t)nc * pc_tiles_per_chunk(M) < (1ll << 24);
}

extern "C" int64_t ss_pc_bitmap_words(int64_t M) { return M < 0 ? 0 : pc_words(M); }
extern "C" int64_t ss_pc_compact_tiles(int64_t M, int nc) { return M < 1 || nc < 1 ? 0 : (int64_t)nc * pc_tiles_per_chunk(M); }

extern "C" int ss_pc_mark(const float* pc, int64_t M, const float* q, int64_t m, const int32_t* q_offset, int nc, const int32_t* idx, int k,
                          const double* h_dist_limit, uint32_t* bitmap, int32_t* nearest, int32_t* status, hipStream_t stream) {
  if (!pc_sizes_ok(M, nc) || m < 0 || k < 1 || m * k >= (1ll << 31) || !h_dist_limit || !pc || !q_offset || !bitmap || !status) return SS_ERR_ARG;
  if (m > 0 && (!q || !idx || !nearest)) return SS_ERR_ARG;
  const int64_t words = (int64_t)nc * pc_words(M);
  SS_LAUNCH(k_pc_clear, dim3(pc_grid(words)), dim3(PC_THREADS), 0, stream, bitmap, words);
  SS_LAUNCH(k_pc_clear, dim3(1), dim3(PC_THREADS), 0, stream, (uint32_t*)status, (int64_t)1);
  if (m == 0) return SS_OK;
  SS_LAUNCH(k_pc_mark, dim3(pc_grid(m * k)), dim3(PC_THREADS), 0, stream, pc, M, q, m, q_offset, nc, idx, k, *h_dist_limit, pc_words(M),
            bitmap, nearest, status);
  return SS_OK;
}

extern "C" int ss_pc_compact_scan(const uint32_t* bitmap, int64_t M, int nc, int32_t* tile_base, int32_t* counts, hipStream_t stream) {
  if (!pc_sizes_ok(M, nc) || !bitmap || !tile_base || !counts) return SS_ERR_ARG;
  const int tpc = (int)pc_tiles_per_chunk(M), ntiles = nc * tpc;
  // tile_base holds 2 * ntiles + 1 words: the bases (ntiles + 1), then the per-tile counts the scan reads
  SS_LAUNCH(k_pc_tile_count, dim3(ntiles < PC_MAX_WG ? ntiles : PC_MAX_WG), dim3(PC_THREADS), 0, stream, bitmap, pc_words(M), (int)(M & 31), tpc,
            ntiles, tile_base + ntiles + 1);
  SS_LAUNCH(k_pc_tile_scan, dim3(1), dim3(PC_THREADS), 0, stream, (const int32_t*)(tile_base + ntiles + 1), ntiles, tile_base);
  SS_LAUNCH(k_pc_chunk_counts, dim3(pc_grid(nc)), dim3(PC_THREADS), 0, stream, (const int32_t*)tile_base, tpc, nc, counts);
  return SS_OK;
}

extern "C" int ss_pc_compact(const uint32_t* bitmap, int64_t M, int nc, const int32_t* tile_base, int32_t* rows, int64_t capacity,
                             hipStream_t stream) {
  if (!pc_sizes_ok(M, nc) || capacity < 0 || !bitmap || !tile_base) return SS_ERR_ARG;
  if (capacity == 0) return SS_OK;
  if (!rows) return SS_ERR_ARG;
  const int tpc = (int)pc_tiles_per_chunk(M), ntiles = nc * tpc;
  SS_LAUNCH(k_pc_emit, dim3(ntiles < PC_MAX_WG ? ntiles : PC_MAX_WG), dim3(PC_THREADS), 0, stream, bitmap, pc_words(M), (int)(M & 31), tpc, ntiles,
            tile_base, rows, capacity);
  return SS_OK;
}
