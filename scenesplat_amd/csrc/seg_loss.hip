// Semantic-segmentation losses and metric on the device (gfx950): CrossEntropyLoss + multiclass Lovasz-softmax, and the
// per-class intersection / union / target counts of the evaluator.
//
// Reference (pointcept/models/losses/misc.py:35-62, losses/lovasz.py:121-256, utils/misc.py:167-179): Lovasz-softmax loops in
// Python over labels.unique() (a device->host sync), then sorts each present class's errors with its own torch.sort.  Here the
// loss pair is a fixed sequence of launches with no host read, so it can sit inside a captured training step:
//   1. k_seg_softmax_ce   one pass over the logits: per-row max / sum-exp (kept for the backward), the CE term on valid rows
//                         (per-block partials), the per-class foreground counts (LDS histogram + one integer atomic per class
//                         and block) and the Lovasz sort keys, class-major (C, n):
//                             key = fg << 32 | ~float_bits(|fg - p_c|)      (ignored rows: 0xFFFFFFFF = error 0, sorts last)
//                         The errors lie in [0, 1], so the ascending order of the low 32 bits is descending error; fg rides
//                         along in bit 32, above the bits the sort looks at.
//   2. ss_argsort_i64     stable LSD radix sort of the C segments on the low 32 bits (ties: row index).
//   3. k_lovasz_tile_count / k_lovasz_tile_scan / k_lovasz_scan
//                         segmented scan per present class in sorted order: I = gts - cumsum(fg), U = gts + cumsum(1 - fg)
//                         (integer counts, exact), J = 1 - I/U in fp32, g_k = J_k - J_{k-1}; loss_c = sum e_k g_k (per-tile
//                         partials); g is written back to (class, row) through the permutation.
//   4. k_seg_loss_finish  one block: fixed-order sums -> [ce_sum, n_valid, lovasz_sum over present classes, n_present].
// The backward (k_seg_loss_bwd) is one pass per row.  No float atomics anywhere: two runs give bitwise-equal results.
#include "common.h"

#define SL_THREADS 256
#define SL_MAX_BLOCKS 1024
#define SL_ITEMS 16
#define SL_TILE (SL_THREADS * SL_ITEMS)
#define SL_MAX_CLASSES 256

static inline size_t sl_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int sl_blocks(int64_t n) {
  int64_t b = (n + SL_THREADS - 1) / SL_THREADS;
  return (int)(b < 1 ? 1 : (b > SL_MAX_BLOCKS ? SL_MAX_BLOCKS : b));
}
static inline int sl_tiles(int64_t n) { return ss_div_up(n > 0 ? n : 1, SL_TILE); }

template <typename T> __device__ __forceinline__ float sl_ld(const T* p, int64_t i) { return ElemIO<T>::load(p + i); }

// fixed-order block sum (256 threads = 4 waves); every thread gets the result
__device__ __forceinline__ float sl_block_sum(float v, float* sh /*[4]*/) {
  v = wave_reduce_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ bool sl_valid(int64_t lab, int64_t ignore, int C) { return lab != ignore && lab >= 0 && lab < C; }

// ---- 1. softmax, CE, foreground counts, sort keys ----------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SL_THREADS) void k_seg_softmax_ce(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                int64_t n, int C, int64_t ignore, float* __restrict__ rowstat,
                                                                int64_t* __restrict__ keys, float* __restrict__ part,
                                                                int* __restrict__ fgcount) {
  __shared__ int hist[SL_MAX_CLASSES];
  __shared__ float red[4];
  for (int c = threadIdx.x; c < C; c += SL_THREADS) hist[c] = 0;
  __syncthreads();
  float ce = 0.f, nv = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_THREADS) {
    const T* row = logits + i * C;
    const int64_t lab = labels[i];
    const bool valid = sl_valid(lab, ignore, C);
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, sl_ld(row, c));
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(sl_ld(row, c) - m);
    rowstat[2 * i] = m;
    rowstat[2 * i + 1] = s;
    if (valid) {
      ce += logf(s) + m - sl_ld(row, lab);
      nv += 1.f;
      atomicAdd(&hist[lab], 1);
    }
    if (keys) {
      for (int c = 0; c < C; ++c) {
        uint64_t key = 0xFFFFFFFFull;
        if (valid) {
          const float p = expf(sl_ld(row, c) - m) / s;
          const bool fg = (lab == c);
          const float e = fabsf((fg ? 1.f : 0.f) - p);
          key = ((uint64_t)fg << 32) | (uint64_t)(~__float_as_uint(e));
        }
        keys[(int64_t)c * n + i] = (int64_t)key;
      }
    }
  }
  const float ce_b = sl_block_sum(ce, red);
  const float nv_b = sl_block_sum(nv, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = ce_b; part[2 * blockIdx.x + 1] = nv_b; }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SL_THREADS)
    if (hist[c]) atomicAdd(&fgcount[c], hist[c]);
}

__device__ __forceinline__ bool sl_present(const int* fgcount, const unsigned char* seen, int c) {
  return fgcount[c] > 0 && (seen == nullptr || seen[c] != 0);
}

// ---- 3a. foreground count per sorted tile --------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void k_lovasz_tile_count(const int64_t* __restrict__ skeys, int64_t n, int tiles,
                                                                   const int* __restrict__ fgcount, const unsigned char* __restrict__ seen,
                                                                   int* __restrict__ tilecnt) {
  __shared__ float red[4];
  const int c = blockIdx.y;
  if (!sl_present(fgcount, seen, c)) return;
  const int64_t* seg = skeys + (int64_t)c * n;
  const int64_t base = (int64_t)blockIdx.x * SL_TILE;
  int cnt = 0;
  for (int j = threadIdx.x; j < SL_TILE; j += SL_THREADS)
    if (base + j < n) cnt += (int)((seg[base + j] >> 32) & 1);
  const float tot = sl_block_sum((float)cnt, red);      // <= 4096: exact in fp32
  if (threadIdx.x == 0) tilecnt[(int64_t)c * tiles + blockIdx.x] = (int)tot;
}

// ---- 3b. exclusive scan of the tile counts of one class (one block per class) ----------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void k_lovasz_tile_scan(int* __restrict__ tilecnt, int tiles, const int* __restrict__ fgcount,
                                                                  const unsigned char* __restrict__ seen) {
  __shared__ int sh[SL_THREADS];
  __shared__ int carry;
  const int c = blockIdx.x;
  if (!sl_present(fgcount, seen, c)) return;
  int* t = tilecnt + (int64_t)c * tiles;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b = 0; b < tiles; b += SL_THREADS) {
    const int j = b + threadIdx.x;
    const int v = j < tiles ? t[j] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    int acc = v;
    for (int o = 1; o < SL_THREADS; o <<= 1) {
      const int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      acc += add;
      sh[threadIdx.x] = acc;
      __syncthreads();
    }
    if (j < tiles) t[j] = carry + acc - v;
    __syncthreads();
    if (threadIdx.x == SL_THREADS - 1) carry += acc;
    __syncthreads();
  }
}

// ---- 3c. the Lovasz gradient and the per-tile loss partials ----------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void k_lovasz_scan(const int64_t* __restrict__ skeys, const int32_t* __restrict__ order,
                                                             int64_t n, int tiles, const int* __restrict__ tilecnt,
                                                             const int* __restrict__ fgcount, const unsigned char* __restrict__ seen,
                                                             float* __restrict__ glov, float* __restrict__ lpart) {
  __shared__ int sh[SL_THREADS];
  __shared__ float red[4];
  const int c = blockIdx.y;
  if (!sl_present(fgcount, seen, c)) return;
  const int64_t* seg = skeys + (int64_t)c * n;
  const int32_t* ord = order + (int64_t)c * n;
  const int64_t k0 = (int64_t)blockIdx.x * SL_TILE + (int64_t)threadIdx.x * SL_ITEMS;
  // this thread's SL_ITEMS consecutive elements: foreground bits, then a block exclusive scan of their counts
  unsigned fgbits = 0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SL_ITEMS; ++j) {
    const int64_t k = k0 + j;
    const unsigned f = k < n ? (unsigned)((seg[k] >> 32) & 1) : 0u;
    fgbits |= f << j;
    cnt += (int)f;
  }
  sh[threadIdx.x] = cnt;
  __syncthreads();
  int acc = cnt;
  for (int o = 1; o < SL_THREADS; o <<= 1) {
    const int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    acc += add;
    sh[threadIdx.x] = acc;
    __syncthreads();
  }
  const float gts = (float)fgcount[c];
  int cf = tilecnt[(int64_t)c * tiles + blockIdx.x] + acc - cnt;      // cumsum(fg) before this thread's first element
  float loss = 0.f;
#pragma unroll
  for (int j = 0; j < SL_ITEMS; ++j) {
    const int64_t k = k0 + j;
    if (k >= n) break;
    const int f = (int)((fgbits >> j) & 1u);
    const int cfp = cf;                                                // cumsum(fg) through k - 1
    cf += f;
    const float J = 1.f - (gts - (float)cf) / (gts + (float)(k + 1 - cf));
    const float Jp = k == 0 ? 0.f : 1.f - (gts - (float)cfp) / (gts + (float)(k - cfp));
    const float g = J - Jp;
    const float e = __uint_as_float(~(unsigned)(seg[k] & 0xFFFFFFFFll));
    loss += e * g;
    glov[(int64_t)c * n + ord[k]] = g;
  }
  const float tot = sl_block_sum(loss, red);
  if (threadIdx.x == 0) lpart[(int64_t)c * tiles + blockIdx.x] = tot;
}

// ---- 4. fixed-order totals ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void k_seg_loss_finish(const float* __restrict__ part, int nb, const float* __restrict__ lpart,
                                                                 int tiles, const int* __restrict__ fgcount,
                                                                 const unsigned char* __restrict__ seen, int C, int lovasz,
                                                                 int32_t* __restrict__ present, float* __restrict__ sums) {
  __shared__ float red[4];
  float ce = 0.f, nv = 0.f;
  for (int b = threadIdx.x; b < nb; b += SL_THREADS) { ce += part[2 * b]; nv += part[2 * b + 1]; }
  float ls = 0.f, np = 0.f;
  for (int c = threadIdx.x; c < C; c += SL_THREADS) {
    const bool pr = lovasz && sl_present(fgcount, seen, c);
    if (present) present[c] = pr ? 1 : 0;
    if (pr) {
      float s = 0.f;
      for (int t = 0; t < tiles; ++t) s += lpart[(int64_t)c * tiles + t];
      ls += s;
      np += 1.f;
    }
  }
  ce = sl_block_sum(ce, red);
  nv = sl_block_sum(nv, red);
  ls = sl_block_sum(ls, red);
  np = sl_block_sum(np, red);
  if (threadIdx.x == 0) { sums[0] = ce; sums[1] = nv; sums[2] = ls; sums[3] = np; }
}

// ---- backward: one pass per row ----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SL_THREADS) void k_seg_loss_bwd(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              int64_t n, int C, int64_t ignore, const float* __restrict__ rowstat,
                                                              const float* __restrict__ glov, const int32_t* __restrict__ present,
                                                              const float* __restrict__ coef, T* __restrict__ dlogits) {
  __shared__ unsigned char pres[SL_MAX_CLASSES];
  for (int c = threadIdx.x; c < C; c += SL_THREADS) pres[c] = (glov && present && present[c]) ? 1 : 0;
  __syncthreads();
  const float c_ce = coef[0], c_lov = coef[1];
  for (int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_THREADS) {
    const T* row = logits + i * C;
    T* drow = dlogits + i * C;
    const int64_t lab = labels[i];
    const bool valid = sl_valid(lab, ignore, C);
    if (!valid) {
      for (int c = 0; c < C; ++c) ElemIO<T>::store(drow + c, 0.f);
      continue;
    }
    const float m = rowstat[2 * i], s = rowstat[2 * i + 1];
    // Lovasz: v_c = g_c sign(p_c - fg_c) (sign(0) = 0), through the softmax Jacobian: p_c (v_c - sum_j p_j v_j)
    float dot = 0.f;
    if (glov) {
      for (int c = 0; c < C; ++c) {
        if (!pres[c]) continue;
        const float p = expf(sl_ld(row, c) - m) / s;
        const float d = p - (lab == c ? 1.f : 0.f);
        const float v = glov[(int64_t)c * n + i] * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        dot += p * v;
      }
    }
    for (int c = 0; c < C; ++c) {
      const float p = expf(sl_ld(row, c) - m) / s;
      const float d = p - (lab == c ? 1.f : 0.f);
      float out = c_ce * d;
      if (glov) {
        const float v = pres[c] ? glov[(int64_t)c * n + i] * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 0.f;
        out += c_lov * p * (v - dot);
      }
      ElemIO<T>::store(drow + c, out);
    }
  }
}

// ---- metric: arg-max + intersection / union / target histograms ----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SL_THREADS) void k_seg_iou(const T* __restrict__ logits, const int32_t* __restrict__ pred,
                                                         const int64_t* __restrict__ target, int64_t n, int C, int64_t ignore,
                                                         unsigned long long* __restrict__ out) {
  __shared__ unsigned hi[SL_MAX_CLASSES], ho[SL_MAX_CLASSES], ht[SL_MAX_CLASSES];
  for (int c = threadIdx.x; c < C; c += SL_THREADS) { hi[c] = 0; ho[c] = 0; ht[c] = 0; }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_THREADS) {
    int64_t o;
    if (pred) {
      o = pred[i];
    } else {
      const T* row = logits + i * C;
      float best = sl_ld(row, 0);
      int arg = 0;
      for (int c = 1; c < C; ++c) {
        const float x = sl_ld(row, c);
        if (x > best) { best = x; arg = c; }            // equal maxima: the lowest index
      }
      o = arg;
    }
    const int64_t t = target[i];
    if (t == ignore) o = ignore;                          // output[target == ignore_index] = ignore_index
    const bool oin = o >= 0 && o < C, tin = t >= 0 && t < C;
    if (oin) atomicAdd(&ho[o], 1u);
    if (tin) atomicAdd(&ht[t], 1u);
    if (oin && o == t) atomicAdd(&hi[o], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SL_THREADS) {
    if (hi[c]) atomicAdd(&out[c], (unsigned long long)hi[c]);
    if (ho[c] + ht[c] - hi[c]) atomicAdd(&out[C + c], (unsigned long long)(ho[c] + ht[c] - hi[c]));
    if (ht[c]) atomicAdd(&out[2 * C + c], (unsigned long long)ht[c]);
  }
}

// ---- C-ABI ----------------------------------------------------------------------------------------------------------------
struct SlWs {
  int64_t *keys, *skeys;
  int32_t* order;
  int* fgcount;
  int* tilecnt;
  float *part, *lpart;
  void* sort_ws;
  size_t sort_bytes;
};

static size_t sl_layout(int64_t n, int C, char* base, SlWs* w) {
  const int64_t cn = (int64_t)C * n;
  const int tiles = sl_tiles(n), nb = sl_blocks(n);
  const size_t sizes[8] = {sl_align((size_t)cn * 8), sl_align((size_t)cn * 8), sl_align((size_t)cn * 4), sl_align((size_t)C * 4),
                           sl_align((size_t)C * tiles * 4), sl_align((size_t)nb * 2 * 4), sl_align((size_t)C * tiles * 4),
                           sl_align(ss_argsort_workspace_bytes(n > 0 ? n : 1, C))};
  size_t off = 0, offs[8];
  for (int k = 0; k < 8; ++k) { offs[k] = off; off += sizes[k]; }
  if (w) {
    w->keys = (int64_t*)(base + offs[0]); w->skeys = (int64_t*)(base + offs[1]); w->order = (int32_t*)(base + offs[2]);
    w->fgcount = (int*)(base + offs[3]); w->tilecnt = (int*)(base + offs[4]); w->part = (float*)(base + offs[5]);
    w->lpart = (float*)(base + offs[6]); w->sort_ws = base + offs[7]; w->sort_bytes = sizes[7];
  }
  return off;
}

extern "C" size_t ss_seg_loss_workspace_bytes(int64_t n, int num_classes) {
  if (n < 0 || num_classes < 1) return 0;
  return sl_layout(n, num_classes, nullptr, nullptr);
}

extern "C" int ss_seg_loss_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int num_classes,
                               int64_t ignore_index, const unsigned char* class_seen, int lovasz, float* rowstat, float* glov,
                               int32_t* present, float* sums, void* workspace, size_t workspace_bytes, ss_stream_t stream) {
  const int C = num_classes;
  if (n < 0 || C < 1 || C > SL_MAX_CLASSES || (dtype != SS_F32 && dtype != SS_BF16) || !sums) return SS_ERR_ARG;
  if (n > 0 && (!logits || !labels || !rowstat)) return SS_ERR_ARG;
  if (lovasz && (!glov || !present || (int64_t)C * n >= (1LL << 31))) return SS_ERR_ARG;
  if (!workspace || workspace_bytes < ss_seg_loss_workspace_bytes(n, C)) return SS_ERR_WORKSPACE;
  SlWs w;
  sl_layout(n, C, (char*)workspace, &w);
  const int nb = sl_blocks(n), tiles = sl_tiles(n);
  if (hipMemsetAsync(w.fgcount, 0, (size_t)C * 4, stream) != hipSuccess) return SS_ERR_LAUNCH;
  if (n == 0) {
    if (hipMemsetAsync(w.part, 0, (size_t)nb * 2 * 4, stream) != hipSuccess) return SS_ERR_LAUNCH;
  } else if (dtype == SS_F32) {
    SS_LAUNCH(k_seg_softmax_ce<float>, dim3(nb), dim3(SL_THREADS), 0, stream, (const float*)logits, labels, n, C, ignore_index,
              rowstat, lovasz ? w.keys : (int64_t*)nullptr, w.part, w.fgcount);
  } else {
    SS_LAUNCH(k_seg_softmax_ce<unsigned short>, dim3(nb), dim3(SL_THREADS), 0, stream, (const unsigned short*)logits, labels, n, C,
              ignore_index, rowstat, lovasz ? w.keys : (int64_t*)nullptr, w.part, w.fgcount);
  }
  if (lovasz && n > 0) {
    int rc = ss_argsort_i64(w.keys, C, n, 32, w.order, nullptr, w.skeys, w.sort_ws, w.sort_bytes, stream);
    if (rc != SS_OK) return rc;
    SS_LAUNCH(k_lovasz_tile_count, dim3(tiles, C), dim3(SL_THREADS), 0, stream, (const int64_t*)w.skeys, n, tiles,
              (const int*)w.fgcount, class_seen, w.tilecnt);
    SS_LAUNCH(k_lovasz_tile_scan, dim3(C), dim3(SL_THREADS), 0, stream, w.tilecnt, tiles, (const int*)w.fgcount, class_seen);
    SS_LAUNCH(k_lovasz_scan, dim3(tiles, C), dim3(SL_THREADS), 0, stream, (const int64_t*)w.skeys, (const int32_t*)w.order, n, tiles,
              (const int*)w.tilecnt, (const int*)w.fgcount, class_seen, glov, w.lpart);
  }
  SS_LAUNCH(k_seg_loss_finish, dim3(1), dim3(SL_THREADS), 0, stream, (const float*)w.part, nb, (const float*)w.lpart, tiles,
            (const int*)w.fgcount, class_seen, C, (lovasz && n > 0) ? 1 : 0, present, sums);
  return SS_OK;
}

extern "C" int ss_seg_loss_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int num_classes, int64_t ignore_index,
                               const float* rowstat, const float* glov, const int32_t* present, const float* coef, void* dlogits,
                               ss_stream_t stream) {
  const int C = num_classes;
  if (n < 0 || C < 1 || C > SL_MAX_CLASSES || (dtype != SS_F32 && dtype != SS_BF16) || !coef) return SS_ERR_ARG;
  if (glov && !present) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!logits || !labels || !rowstat || !dlogits) return SS_ERR_ARG;
  const int nb = sl_blocks(n);
  if (dtype == SS_F32)
    SS_LAUNCH(k_seg_loss_bwd<float>, dim3(nb), dim3(SL_THREADS), 0, stream, (const float*)logits, labels, n, C, ignore_index, rowstat,
              glov, present, coef, (float*)dlogits);
  else
    SS_LAUNCH(k_seg_loss_bwd<unsigned short>, dim3(nb), dim3(SL_THREADS), 0, stream, (const unsigned short*)logits, labels, n, C,
              ignore_index, rowstat, glov, present, coef, (unsigned short*)dlogits);
  return SS_OK;
}

extern "C" int ss_seg_iou(const void* logits, int dtype, const int32_t* pred, const int64_t* target, int64_t n, int num_classes,
                          int64_t ignore_index, int64_t* out, ss_stream_t stream) {
  const int C = num_classes;
  if (n < 0 || C < 1 || C > SL_MAX_CLASSES || !out || (!pred && dtype != SS_F32 && dtype != SS_BF16)) return SS_ERR_ARG;
  if (hipMemsetAsync(out, 0, (size_t)3 * C * 8, stream) != hipSuccess) return SS_ERR_LAUNCH;
  if (n == 0) return SS_OK;
  if (!target || (!pred && !logits)) return SS_ERR_ARG;
  const int nb = sl_blocks(n);
  if (pred || dtype == SS_F32)
    SS_LAUNCH(k_seg_iou<float>, dim3(nb), dim3(SL_THREADS), 0, stream, (const float*)logits, pred, target, n, C, ignore_index,
              (unsigned long long*)out);
  else
    SS_LAUNCH(k_seg_iou<unsigned short>, dim3(nb), dim3(SL_THREADS), 0, stream, (const unsigned short*)logits, pred, target, n, C,
              ignore_index, (unsigned long long*)out);
  return SS_OK;
}
