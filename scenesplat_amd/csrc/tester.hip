// The steps of the open-vocabulary test stage that follow the fragment accumulation (pointcept/engines/test.py:372-394 and
// pointcept/utils/misc.py:98-125), over every original Gaussian and without leaving the device:
//   ss_vocab_finish   (n, C) accumulated probabilities -> the k best classes per row (+ confidence threshold for k = 1), the
//                     pred_label_mapping table, and the grid -> origin expansion pred[inverse]
//   ss_cluster_vote   every instance takes its most frequent prediction (np.unique + argmax per instance in the reference)
// All counters are integers: the results are exact and bitwise reproducible whatever the order of the atomics.
#include "common.h"

#define TS_THREADS 256
#define TS_MAX_CLASSES 256
#define TS_MAX_K 8

static inline size_t ts_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- ss_vocab_finish ------------------------------------------------------------------------------------------------------
// A value as an unsigned key of the same order: -0 is folded into +0 and NaN into -inf first, so equal values give equal keys
// and every real key is > 0.  Key 0 marks a slot outside the row or a class already taken.
__device__ __forceinline__ unsigned ts_key(float v) {
  v = (v != v) ? -INFINITY : v + 0.0f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ts_key_value(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// all-reduce over the 16 lanes of a DPP row by rotations (row_ror:8,4,2,1): VALU only, every lane ends with the result
template <int CTRL>
__device__ __forceinline__ unsigned ts_row_ror(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned ts_row_max(unsigned v) {
  unsigned o;
  o = ts_row_ror<0x128>(v); v = o > v ? o : v;
  o = ts_row_ror<0x124>(v); v = o > v ? o : v;
  o = ts_row_ror<0x122>(v); v = o > v ? o : v;
  o = ts_row_ror<0x121>(v); v = o > v ? o : v;
  return v;
}
__device__ __forceinline__ unsigned ts_row_min(unsigned v) {
  unsigned o;
  o = ts_row_ror<0x128>(v); v = o < v ? o : v;
  o = ts_row_ror<0x124>(v); v = o < v ? o : v;
  o = ts_row_ror<0x122>(v); v = o < v ? o : v;
  o = ts_row_ror<0x121>(v); v = o < v ? o : v;
  return v;
}

// Sixteen lanes per row (four rows per wave), E slots per lane.  VEC: slot e of lane t is class 4 (t + 16 (e / 4)) + e % 4, from
// E / 4 loads of 16 bytes; otherwise class t + 16 e.  Either way the class grows with e inside a lane, so the strict compare of the
// local pass keeps the lowest class among equal values.  k rounds: the row's largest key not taken yet, then the lowest class that
// holds it; lane 0 of the row writes the label.  Rows past n repeat row n - 1 and write nothing (no lane leaves before the DPP ops).
template <bool VEC, int E>
__global__ __launch_bounds__(TS_THREADS) void k_vocab_rank(const float* __restrict__ pred, int64_t n, int C, int k, float threshold,
                                                            int ignore_index, const int32_t* __restrict__ lut,
                                                            int32_t* __restrict__ labels) {
  const int t = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * (TS_THREADS / 16) + (threadIdx.x >> 4);
  const float* p = pred + (row < n ? row : n - 1) * C;
  unsigned key[E];
  if (VEC) {
#pragma unroll
    for (int i = 0; i < E / 4; ++i) {
      const int c = 4 * (t + 16 * i);
      if (c < C) {                                                 // C % 4 == 0: the whole quad is inside the row
        const float4 v = *reinterpret_cast<const float4*>(p + c);
        key[4 * i] = ts_key(v.x); key[4 * i + 1] = ts_key(v.y); key[4 * i + 2] = ts_key(v.z); key[4 * i + 3] = ts_key(v.w);
      } else {
        key[4 * i] = key[4 * i + 1] = key[4 * i + 2] = key[4 * i + 3] = 0u;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = t + 16 * e;
      key[e] = c < C ? ts_key(p[c]) : 0u;
    }
  }
  const int c0 = VEC ? 4 * t : t;                                  // class of slot 0; slot e is at c0 + step(e)
  for (int r = 0; r < k; ++r) {
    unsigned best = 0u, bc = 0x7fffffffu;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int step = VEC ? 64 * (e >> 2) + (e & 3) : 16 * e;
      if (key[e] > best) { best = key[e]; bc = (unsigned)(c0 + step); }
    }
    const unsigned top = ts_row_max(best);                         // > 0: k <= C leaves a class to take in every round
    const unsigned win = ts_row_min(best == top ? bc : 0x7fffffffu);
    const int d = (int)win - c0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int step = VEC ? 64 * (e >> 2) + (e & 3) : 16 * e;
      key[e] = d == step ? 0u : key[e];
    }
    if (t == 0 && row < n) {
      int label = (int)win;
      const bool ignored = (k == 1) && (ts_key_value(top) < threshold);         // strict, as max_probs < confidence_threshold
      if (lut) label = lut[ignored ? 0 : label + 1];
      else if (ignored) label = ignore_index;
      labels[row * k + r] = label;
    }
  }
}

// out[j, :] = labels[inverse[j], :]: k ints per output row (an inverse outside [0, n) gives the image of ignore_index)
__global__ __launch_bounds__(TS_THREADS) void k_vocab_expand(const int32_t* __restrict__ labels, const int64_t* __restrict__ inverse,
                                                              int64_t n, int64_t m, int k, int ignore_index,
                                                              const int32_t* __restrict__ lut, int32_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (t >= m * k) return;
  const int64_t j = t / k;
  const int c = (int)(t - j * k);
  const int64_t src = inverse[j];
  out[t] = (src >= 0 && src < n) ? labels[src * k + c] : (lut ? lut[0] : ignore_index);
}

extern "C" size_t ss_vocab_finish_workspace_bytes(int64_t n, int k, int64_t m) {
  (void)m;
  if (n <= 0 || k <= 0) return 256;
  return ts_align((size_t)n * (size_t)k * sizeof(int32_t));
}

extern "C" int ss_vocab_finish(const float* pred, int64_t n, int num_classes, int k, float threshold, int32_t ignore_index,
                               const int64_t* inverse, int64_t m, const int32_t* lut, int32_t* out, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  const int C = num_classes;
  if (n < 0 || m < 0 || C < 1 || C > TS_MAX_CLASSES || k < 1 || k > TS_MAX_K || k > C) return SS_ERR_ARG;
  if (!inverse) m = n;
  if (n == 0 || m == 0) return SS_OK;
  if (!pred || !out) return SS_ERR_ARG;
  if ((n + 15) / 16 > 0x7fffffffLL || (m * k + TS_THREADS - 1) / TS_THREADS > 0x7fffffffLL) return SS_ERR_ARG;
  int32_t* labels = out;
  if (inverse) {
    if (!workspace) return SS_ERR_ARG;
    if (workspace_bytes < (size_t)n * (size_t)k * sizeof(int32_t)) return SS_ERR_WORKSPACE;
    labels = (int32_t*)workspace;
  }
  const dim3 grid(ss_div_up(n, TS_THREADS / 16)), block(TS_THREADS);
  const bool vec = (C % 4 == 0) && (((uintptr_t)pred) % 16 == 0);
#define TS_RANK(V, E_) SS_LAUNCH((k_vocab_rank<V, E_>), grid, block, 0, stream, pred, n, C, k, threshold, (int)ignore_index, lut, labels)
  if (C <= 64) { if (vec) TS_RANK(true, 4); else TS_RANK(false, 4); }
  else { if (vec) TS_RANK(true, 16); else TS_RANK(false, 16); }
#undef TS_RANK
  if (inverse) {
    SS_LAUNCH(k_vocab_expand, dim3(ss_div_up(m * k, TS_THREADS)), block, 0, stream, (const int32_t*)labels, inverse, n, m, k,
              (int)ignore_index, lut, out);
  }
  return SS_OK;
}

// ---- ss_cluster_vote ------------------------------------------------------------------------------------------------------
// A (num_instances, C + 1) table of counts.  The slots of an instance are in the NUMERIC order of the values they stand for
// (ignore_index where it sorts among 0 .. C-1), so "first slot with the largest count" is np.unique + argmax.
__device__ __forceinline__ int ts_slot(int v, int C, int ignore_index) {
  if (ignore_index < 0) return v == ignore_index ? 0 : (v >= 0 && v < C ? v + 1 : -1);
  if (ignore_index >= C) return v == ignore_index ? C : (v >= 0 && v < C ? v : -1);
  return (v >= 0 && v < C) ? v : -1;                               // ignore_index is one of the classes
}
__device__ __forceinline__ int ts_slot_value(int s, int C, int ignore_index) {
  if (ignore_index < 0) return s == 0 ? ignore_index : s - 1;
  if (ignore_index >= C) return s == C ? ignore_index : s;
  return s;
}

// Rows of an instance tend to be neighbours: a run of equal (instance, slot) keys inside a wave is counted by its first lane
// with one atomic of the run's length.
__global__ __launch_bounds__(TS_THREADS) void k_cluster_count(const int32_t* __restrict__ pred, const int32_t* __restrict__ inst,
                                                               int64_t m, int num_instances, int C, int ignore_index,
                                                               unsigned* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int cell = -1;
  if (i < m) {
    const int g = inst[i];
    const int s = ts_slot(pred[i], C, ignore_index);
    if (g >= 0 && g < num_instances && s >= 0) cell = g * (C + 1) + s;
  }
  const int prev = __shfl_up(cell, 1, 64);
  const bool head = lane == 0 || prev != cell;
  const unsigned long long heads = __ballot(head);
  if (head && cell >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int len = above ? __ffsll((long long)above) : 64 - lane;
    atomicAdd(&table[cell], (unsigned)len);
  }
}

// one wave per instance: the first slot with the largest count
__global__ __launch_bounds__(TS_THREADS) void k_cluster_argmax(const unsigned* __restrict__ table, int num_instances, int C,
                                                                int ignore_index, int32_t* __restrict__ winner) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (TS_THREADS / 64) + (threadIdx.x >> 6);
  if (g >= num_instances) return;
  const unsigned* row = table + (int64_t)g * (C + 1);
  unsigned long long best = 0ull;                                  // count << 32 | ~slot
  for (int s = lane; s <= C; s += 64) {
    const unsigned long long key = ((unsigned long long)row[s] << 32) | (unsigned)(~s);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) winner[g] = ts_slot_value((int)(~(unsigned)(best & 0xffffffffull)), C, ignore_index);
}

__global__ __launch_bounds__(TS_THREADS) void k_cluster_bcast(const int32_t* __restrict__ pred, const int32_t* __restrict__ inst,
                                                               const int32_t* __restrict__ winner, int64_t m, int num_instances,
                                                               int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (i >= m) return;
  const int g = inst[i];
  out[i] = (g >= 0 && g < num_instances) ? winner[g] : pred[i];
}

static inline size_t ts_table_bytes(int num_instances, int num_classes) {
  return ts_align((size_t)num_instances * (size_t)(num_classes + 1) * sizeof(unsigned));
}

extern "C" size_t ss_cluster_vote_workspace_bytes(int num_instances, int num_classes) {
  if (num_instances <= 0 || num_classes <= 0) return 256;
  return ts_table_bytes(num_instances, num_classes) + ts_align((size_t)num_instances * sizeof(int32_t));
}

extern "C" int ss_cluster_vote(const int32_t* pred, const int32_t* instance_dense, int64_t m, int num_instances, int num_classes,
                               int32_t ignore_index, int32_t* out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const int C = num_classes;
  if (m < 0 || num_instances < 0 || C < 1 || C > TS_MAX_CLASSES) return SS_ERR_ARG;
  if (m == 0) return SS_OK;
  if (!pred || !instance_dense || !out) return SS_ERR_ARG;
  if ((int64_t)num_instances * (C + 1) > 0x7fffffffLL || (m + TS_THREADS - 1) / TS_THREADS > 0x7fffffffLL) return SS_ERR_ARG;
  const dim3 block(TS_THREADS), rows(ss_div_up(m, TS_THREADS));
  int32_t* winner = nullptr;
  if (num_instances > 0) {
    if (!workspace) return SS_ERR_ARG;
    if (workspace_bytes < ss_cluster_vote_workspace_bytes(num_instances, C)) return SS_ERR_WORKSPACE;
    const size_t tb = ts_table_bytes(num_instances, C);
    unsigned* table = (unsigned*)workspace;
    winner = (int32_t*)((char*)workspace + tb);
    (void)hipGetLastError();
    if (hipMemsetAsync(table, 0, tb, stream) != hipSuccess) return SS_ERR_LAUNCH;
    SS_LAUNCH(k_cluster_count, rows, block, 0, stream, pred, instance_dense, m, num_instances, C, (int)ignore_index, table);
    SS_LAUNCH(k_cluster_argmax, dim3(ss_div_up(num_instances, TS_THREADS / 64)), block, 0, stream, (const unsigned*)table,
              num_instances, C, (int)ignore_index, winner);
  }
  SS_LAUNCH(k_cluster_bcast, rows, block, 0, stream, pred, instance_dense, (const int32_t*)winner, m, num_instances, out);
  return SS_OK;
}
