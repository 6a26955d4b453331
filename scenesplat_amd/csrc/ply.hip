// 3DGS checkpoint decode: the vertex block of a binary little-endian .ply (interleaved records, `stride` bytes apart) -> the five
// arrays of a scene folder, in ONE pass (scripts/preprocess_gs.py::read_gaussian_attributes of the reference: fourteen strided column
// extractions, then exp, a sigmoid, a row norm, a sign flip and a colour quantisation as separate numpy passes).
//
// A workgroup of PLY_ROWS threads owns PLY_ROWS consecutive records.
//   1. The tile's bytes (rows * stride, contiguous in memory) come in with coalesced loads and go to LDS as they are: 16-byte loads
//      where the tile's first byte is 16-byte aligned, 8-byte loads where it is 8-byte aligned, 4-byte loads otherwise and for the
//      tail; several loads per thread are in flight before the first LDS store.  PLY_ROWS * stride is a multiple of 512, so every
//      tile of a call has the alignment of `records`: the 8- and 4-byte forms serve a caller that decodes records where they lie
//      inside a larger buffer (record k of a 248-byte stream starts 0 or 8 mod 16); the package's loader copies every piece to the
//      start of its staging buffer and always takes the 16-byte form.  A stride above PLY_MAX_LDS_STRIDE does not fit the tile into
//      LDS; its rows are read straight from memory, one thread per row (the wanted words only).
//   2. Thread r reads the wanted words of record r from LDS (ds_read_b32 at r * stride / 4 + offset: for the standard 62-word record
//      two rows of a 32-lane group share a bank -- a 2-way conflict on 14 reads per row, accepted: the pass is bound by the HBM read
//      of step 1 and a padded image would give up the 16-byte LDS stores of the linear copy) and computes its outputs in registers.
//   3. The outputs go back to LDS in array order (the tile is dead by then) and every array is written with consecutive lanes on
//      consecutive words (bytes for the colours).
// No atomics.  The offsets travel as kernel arguments.
//
// Values: coord copied.  color, quat: every fp32 operation rounded on its own, in numpy's order (contraction is off for this file), IEEE
// division and square root.  scale, opacity: fp64 exp, ONE rounding to fp32.
#include "common.h"

#pragma clang fp contract(off)

#define PLY_ROWS 128
#define PLY_MAX_LDS_STRIDE 512                       // PLY_ROWS * 512 B = 64 KiB of LDS
#define PLY_OUT_ROW_BYTES 52                         // 3 + 1 + 4 + 4 floats and 3 colour bytes, rounded up to a word
#define PLY_MAX_OFFS 15                              // x y z, f_dc_0..2, opacity, <= 4 scale, <= 4 rot

struct PlyOffsets { int32_t w[PLY_MAX_OFFS]; };      // WORD offsets inside a record, in the order of the header's h_offsets

typedef uint32_t __attribute__((ext_vector_type(4))) ply_u32x4;
typedef uint32_t __attribute__((ext_vector_type(2))) ply_u32x2;

// `count` elements of type V from memory to LDS, thread t taking elements t, t + PLY_ROWS, ...: U loads are issued before the first
// LDS store of a batch (a load -> store pair per trip would pay one memory round trip per element)
template <typename V, int U>
__device__ __forceinline__ void ply_copy(const uint32_t* __restrict__ g, uint32_t* l, int count, int t) {
  const V* gv = reinterpret_cast<const V*>(g);
  V* lv = reinterpret_cast<V*>(l);
  for (int base = t; base < count; base += U * PLY_ROWS) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * PLY_ROWS < count) v[u] = gv[base + u * PLY_ROWS];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * PLY_ROWS < count) lv[base + u * PLY_ROWS] = v[u];
  }
}

__global__ void __launch_bounds__(PLY_ROWS)
k_ply_decode(const uint32_t* __restrict__ rec, int64_t n, int stride_w, PlyOffsets off, int n_scale, int n_rot, int use_lds,
             float* __restrict__ coord, uint8_t* __restrict__ color, float* __restrict__ opacity, float* __restrict__ scale,
             float* __restrict__ quat) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * PLY_ROWS;
  const int rows = (int)((n - row0) < PLY_ROWS ? (n - row0) : PLY_ROWS);       // >= 1: the grid is ceil(n / PLY_ROWS)
  const uint32_t* tile = rec + row0 * stride_w;
  const int words = rows * stride_w;                                           // <= 128 * 128

  const uint32_t* src;                                                         // where thread t finds its record
  if (use_lds) {
    const int align = (int)((uintptr_t)tile & 15);                             // uniform over the workgroup
    int done = 0;
    if (align == 0) {
      done = (words >> 2) << 2;
      ply_copy<ply_u32x4, 16>(tile, lds, words >> 2, t);
    } else if (align == 8) {                                                   // e.g. an odd record number of a 248-byte stream
      done = (words >> 1) << 1;
      ply_copy<ply_u32x2, 16>(tile, lds, words >> 1, t);
    }
    ply_copy<uint32_t, 16>(tile + done, lds + done, words - done, t);          // the tail, or the whole tile of a 4-byte start
    __syncthreads();
    src = lds + t * stride_w;
  } else {
    src = tile + (int64_t)t * stride_w;
  }

  float c[3], col[3], op = 0.f, sc[4], q[4];
  if (t < rows) {
    for (int a = 0; a < 3; ++a) c[a] = __uint_as_float(src[off.w[a]]);
    for (int a = 0; a < 3; ++a) {
      float v = __uint_as_float(src[off.w[3 + a]]) * 0.28209479177387814f;     // one rounding per operation (contract off)
      v = v + 0.5f;
      v = v < 0.f ? 0.f : v;                                                   // ordered compares: NaN passes, as in np.clip
      v = v > 1.f ? 1.f : v;
      col[a] = v * 255.f;
    }
    op = (float)(1.0 / (1.0 + exp(-(double)__uint_as_float(src[off.w[6]]))));
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_scale) sc[a] = (float)exp((double)__uint_as_float(src[off.w[7 + a]]));
    float ss = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_rot) {
        q[a] = __uint_as_float(src[off.w[7 + n_scale + a]]);
        const float p = q[a] * q[a];
        ss = a == 0 ? p : ss + p;
      }
    const float den = sqrtf(ss) + 1e-9f;
    float sign = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_rot) {
        q[a] = q[a] / den;
        if (a == 0) sign = q[0] > 0.f ? 1.f : q[0] < 0.f ? -1.f : q[0] == 0.f ? 0.f : q[0];      // np.sign: NaN stays NaN
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_rot) q[a] = q[a] * sign;
  }
  if (use_lds) __syncthreads();                                                // every record has been read: the tile is dead

  // LDS image of the outputs: coord (3 R), opacity (R), scale (n_scale R), quat (n_rot R) floats, then 3 R colour bytes
  float* lf = reinterpret_cast<float*>(lds);
  float* l_op = lf + 3 * PLY_ROWS;
  float* l_sc = l_op + PLY_ROWS;
  float* l_q = l_sc + n_scale * PLY_ROWS;
  uint8_t* l_col = reinterpret_cast<uint8_t*>(l_q + n_rot * PLY_ROWS);
  if (t < rows) {
    for (int a = 0; a < 3; ++a) lf[t * 3 + a] = c[a];
    l_op[t] = op;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_scale) l_sc[t * n_scale + a] = sc[a];
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < n_rot) l_q[t * n_rot + a] = q[a];
    for (int a = 0; a < 3; ++a) l_col[t * 3 + a] = (uint8_t)(int)col[a];       // truncation; values are in [0, 255] unless NaN
  }
  __syncthreads();
  for (int i = t; i < rows * 3; i += PLY_ROWS) coord[row0 * 3 + i] = lf[i];
  if (t < rows) opacity[row0 + t] = l_op[t];
  for (int i = t; i < rows * n_scale; i += PLY_ROWS) scale[row0 * n_scale + i] = l_sc[i];
  for (int i = t; i < rows * n_rot; i += PLY_ROWS) quat[row0 * n_rot + i] = l_q[i];
  for (int i = t; i < rows * 3; i += PLY_ROWS) color[row0 * 3 + i] = l_col[i];
}

extern "C" int ss_ply_decode_rows_per_workgroup(void) { return PLY_ROWS; }

extern "C" int ss_ply_decode(const void* records, int64_t n, int stride_bytes, const int32_t* h_offsets, int n_scale, int n_rot,
                             float* coord, uint8_t* color, float* opacity, float* scale, float* quat, hipStream_t stream) {
  if (n < 0 || n_scale < 1 || n_scale > 4 || n_rot < 1 || n_rot > 4 || !h_offsets) return SS_ERR_ARG;
  if (stride_bytes < 4 || (stride_bytes & 3)) return SS_ERR_ARG;
  PlyOffsets off;
  for (int i = 0; i < PLY_MAX_OFFS; ++i) off.w[i] = 0;
  for (int i = 0; i < 7 + n_scale + n_rot; ++i) {
    if (h_offsets[i] < 0 || (h_offsets[i] & 3) || (int64_t)h_offsets[i] + 4 > stride_bytes) return SS_ERR_ARG;
    off.w[i] = h_offsets[i] >> 2;
  }
  if (n == 0) return SS_OK;
  if (!records || !coord || !color || !opacity || !scale || !quat || ((uintptr_t)records & 3)) return SS_ERR_ARG;
  const int64_t grid = (n + PLY_ROWS - 1) / PLY_ROWS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  const int use_lds = stride_bytes <= PLY_MAX_LDS_STRIDE;
  const int tile_bytes = use_lds ? PLY_ROWS * stride_bytes : 0;
  const int out_bytes = PLY_ROWS * PLY_OUT_ROW_BYTES;
  const size_t shmem = (size_t)(tile_bytes > out_bytes ? tile_bytes : out_bytes);
  SS_LAUNCH(k_ply_decode, dim3((unsigned)grid), dim3(PLY_ROWS), shmem, stream, reinterpret_cast<const uint32_t*>(records), n,
            stride_bytes >> 2, off, n_scale, n_rot, use_lds, coord, color, opacity, scale, quat);
  return SS_OK;
}
