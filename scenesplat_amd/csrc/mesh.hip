// ScanNet mesh converter (pointcept/datasets/preprocessing/scannet/preprocess_scannet.py and preprocess_scannet_gs.py of the reference):
// the vertex and face blocks of a binary little-endian .ply, the area-weighted vertex normals and the label lookup, on the device.
//
//   decode    A workgroup of MESH_ROWS threads owns MESH_ROWS consecutive records.  The tile's bytes come in as the aligned words that
//             cover them (16-byte loads where the first covering word is 16-byte aligned, 4-byte loads otherwise and for the tail;
//             MESH_ROWS * stride is a multiple of 256, so every tile of a call has the alignment of `records`) and go to LDS as they
//             are; thread r then reads its fields at byte r * stride + offset, a field that straddles two words funnelled out of both.
//             So a record may start at ANY byte: the face block of a mesh starts at header + n * stride, and its records are 13 bytes.
//             The outputs go back to LDS in array order and leave with consecutive lanes on consecutive words (bytes for the colours).
//             A vertex stride above MESH_MAX_LDS_STRIDE is read where it lies, one thread per record.
//   normals   `vertex_normal` of the two scripts, bit for bit: per face the term nf * area with every fp32 operation rounded on its own
//             (contraction is off for this file, IEEE division and square root); per vertex the terms of its incident faces added in
//             ascending face index into ONE fp32 accumulator per component.  The incidence is the 3F (vertex, pair) entries,
//             pair = 3 * face + corner, under a stable radix argsort by vertex (ss_argsort_i64) with ss_pool_partition's run
//             boundaries: one lane per run walks it.  No floating-point atomics: the order of the additions is the result.
//   labels    one pass: seg = seg_indices[src ? src[i] : i], g = seg_to_group[seg], three per-group tables; -1 where there is none.
#include "common.h"

#pragma clang fp contract(off)

#define MESH_ROWS 256
#define MESH_MAX_LDS_STRIDE 128                      // MESH_ROWS * 128 B = 32 KiB of LDS
#define MESH_FACE_BYTES 13                           // uchar count + 3 x int32
#define MESH_VERTEX_OUT_BYTES (MESH_ROWS * 15)       // 3 floats and 3 colour bytes per row
#define MESH_BAD_COUNT 1
#define MESH_BAD_INDEX 2

typedef uint32_t __attribute__((ext_vector_type(4))) mesh_u32x4;

// the 32 bits at byte b of a word array, little endian; b of any alignment.  The second word is read only where the value reaches
// into it, so nothing beyond the words that cover the value is touched.
__device__ __forceinline__ uint32_t mesh_u32_at(const uint32_t* w, int64_t b) {
  const uint32_t lo = w[b >> 2];
  const int sh = (int)(b & 3) * 8;
  if (sh == 0) return lo;
  return (lo >> sh) | (w[(b >> 2) + 1] << (32 - sh));
}
__device__ __forceinline__ uint32_t mesh_u8_at(const uint32_t* w, int64_t b) { return (w[b >> 2] >> ((int)(b & 3) * 8)) & 0xffu; }

// `count` elements of type V from memory to LDS, thread t taking t, t + MESH_ROWS, ...; U loads in flight before the first LDS store
template <typename V, int U>
__device__ __forceinline__ void mesh_copy(const uint32_t* __restrict__ g, uint32_t* l, int count, int t) {
  const V* gv = reinterpret_cast<const V*>(g);
  V* lv = reinterpret_cast<V*>(l);
  for (int base = t; base < count; base += U * MESH_ROWS) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * MESH_ROWS < count) v[u] = gv[base + u * MESH_ROWS];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * MESH_ROWS < count) lv[base + u * MESH_ROWS] = v[u];
  }
}

// bytes [a, a + nbytes) -> LDS: the aligned words that cover them, LDS byte (a & 3) + k = byte a[k].  -> a & 3
__device__ __forceinline__ int mesh_stage(const uint8_t* a, int nbytes, uint32_t* lds, int t) {
  const int shift = (int)((uintptr_t)a & 3);
  const uint32_t* g = reinterpret_cast<const uint32_t*>(a - shift);
  const int words = (shift + nbytes + 3) >> 2;
  int done = 0;
  if (((uintptr_t)g & 15) == 0) {                                              // uniform over the workgroup
    done = (words >> 2) << 2;
    mesh_copy<mesh_u32x4, 4>(g, lds, words >> 2, t);
  }
  mesh_copy<uint32_t, 4>(g + done, lds + done, words - done, t);
  return shift;
}

// ---- vertex block ---------------------------------------------------------------------------------------------------------------------
struct MeshVertexOffsets { int32_t xyz[3]; int32_t rgb[3]; };                  // BYTE offsets inside a record

__global__ void __launch_bounds__(MESH_ROWS)
k_mesh_decode_vertices(const uint8_t* __restrict__ rec, int64_t n, int stride, MeshVertexOffsets off, int use_lds,
                       float* __restrict__ coord, uint8_t* __restrict__ color) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * MESH_ROWS;
  const int rows = (int)((n - row0) < MESH_ROWS ? (n - row0) : MESH_ROWS);     // >= 1: the grid is ceil(n / MESH_ROWS)
  const uint8_t* tile = rec + row0 * stride;

  const uint32_t* src;                                                         // the words thread t reads its record from
  int64_t at;                                                                  // byte of the record's start in them
  if (use_lds) {
    const int shift = mesh_stage(tile, rows * stride, lds, t);
    __syncthreads();
    src = lds;
    at = shift + t * stride;
  } else {
    const int shift = (int)((uintptr_t)tile & 3);
    src = reinterpret_cast<const uint32_t*>(tile - shift);
    at = shift + (int64_t)t * stride;
  }
  uint32_t c[3] = {0, 0, 0}, col[3] = {0, 0, 0};
  if (t < rows) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = mesh_u32_at(src, at + off.xyz[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) col[a] = mesh_u8_at(src, at + off.rgb[a]);
  }
  if (use_lds) __syncthreads();                                                // every record has been read: the tile is dead

  uint8_t* l_col = reinterpret_cast<uint8_t*>(lds + 3 * MESH_ROWS);
  if (t < rows) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lds[t * 3 + a] = c[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) l_col[t * 3 + a] = (uint8_t)col[a];
  }
  __syncthreads();
  uint32_t* cw = reinterpret_cast<uint32_t*>(coord);
  for (int i = t; i < rows * 3; i += MESH_ROWS) cw[row0 * 3 + i] = lds[i];
  for (int i = t; i < rows * 3; i += MESH_ROWS) color[row0 * 3 + i] = l_col[i];
}

extern "C" int ss_mesh_decode_rows_per_workgroup(void) { return MESH_ROWS; }

extern "C" int ss_mesh_decode_vertices(const void* records, int64_t n, int stride_bytes, const int32_t* h_offsets, float* coord,
                                       uint8_t* color, hipStream_t stream) {
  if (n < 0 || stride_bytes < 15 || !h_offsets) return SS_ERR_ARG;
  MeshVertexOffsets off;
  for (int a = 0; a < 3; ++a) {
    const int32_t f = h_offsets[a], b = h_offsets[3 + a];
    if (f < 0 || (f & 3) || (int64_t)f + 4 > stride_bytes || b < 0 || b >= stride_bytes) return SS_ERR_ARG;
    off.xyz[a] = f;
    off.rgb[a] = b;
  }
  if (n == 0) return SS_OK;
  if (!records || !coord || !color) return SS_ERR_ARG;
  const int64_t grid = (n + MESH_ROWS - 1) / MESH_ROWS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  const int use_lds = stride_bytes <= MESH_MAX_LDS_STRIDE;
  const int tile_bytes = use_lds ? MESH_ROWS * stride_bytes + 16 : 0;          // + the bytes in front of an unaligned start, rounded up
  const size_t shmem = (size_t)(tile_bytes > MESH_VERTEX_OUT_BYTES ? tile_bytes : MESH_VERTEX_OUT_BYTES);
  SS_LAUNCH(k_mesh_decode_vertices, dim3((unsigned)grid), dim3(MESH_ROWS), shmem, stream, reinterpret_cast<const uint8_t*>(records), n,
            stride_bytes, off, use_lds, coord, color);
  return SS_OK;
}

// ---- face block ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_ROWS)
k_mesh_decode_faces(const uint8_t* __restrict__ rec, int64_t F, uint32_t n_vertices, int32_t* __restrict__ faces,
                    int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[(MESH_ROWS * MESH_FACE_BYTES) / 4 + 4];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * MESH_ROWS;
  const int rows = (int)((F - row0) < MESH_ROWS ? (F - row0) : MESH_ROWS);
  const int shift = mesh_stage(rec + row0 * MESH_FACE_BYTES, rows * MESH_FACE_BYTES, lds, t);
  __syncthreads();
  uint32_t v[3] = {0, 0, 0};
  if (t < rows) {
    const int at = shift + t * MESH_FACE_BYTES;
    int bad = mesh_u8_at(lds, at) != 3u ? MESH_BAD_COUNT : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = mesh_u32_at(lds, at + 1 + 4 * a);
      if (v[a] >= n_vertices) bad |= MESH_BAD_INDEX;                           // (a negative int is a large uint)
    }
    if (bad) atomicOr(status, bad);
  }
  __syncthreads();                                                             // the tile is dead
  if (t < rows) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lds[t * 3 + a] = v[a];
  }
  __syncthreads();
  for (int i = t; i < rows * 3; i += MESH_ROWS) faces[row0 * 3 + i] = (int32_t)lds[i];
}

extern "C" int ss_mesh_decode_faces(const void* records, int64_t n_faces, int64_t n_vertices, int32_t* faces, int32_t* status,
                                    hipStream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_vertices > 0x7fffffff) return SS_ERR_ARG;
  if (n_faces == 0) return SS_OK;
  if (!records || !faces || !status) return SS_ERR_ARG;
  const int64_t grid = (n_faces + MESH_ROWS - 1) / MESH_ROWS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  SS_LAUNCH(k_mesh_decode_faces, dim3((unsigned)grid), dim3(MESH_ROWS), 0, stream, reinterpret_cast<const uint8_t*>(records), n_faces,
            (uint32_t)n_vertices, faces, status);
  return SS_OK;
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------------------
// np.maximum(1e-8, r): a NaN passes
__device__ __forceinline__ float mesh_length(float r, int form) { return form == SS_MESH_FORM_PC ? r + 1e-8f : (r < 1e-8f ? 1e-8f : r); }

__global__ void k_mesh_face_terms(const float* __restrict__ coord, const int32_t* __restrict__ faces, int64_t F, uint32_t n_vertices,
                                  int form, float* __restrict__ terms, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const uint32_t i0 = (uint32_t)faces[3 * f], i1 = (uint32_t)faces[3 * f + 1], i2 = (uint32_t)faces[3 * f + 2];
  if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
    atomicOr(status, MESH_BAD_INDEX);
    terms[3 * f] = 0.f; terms[3 * f + 1] = 0.f; terms[3 * f + 2] = 0.f;
    return;
  }
  float a[3], u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = coord[3 * (int64_t)i0 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = coord[3 * (int64_t)i1 + k] - a[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = coord[3 * (int64_t)i2 + k] - a[k];
  float c[3];                                                                  // np.cross: mul, mul, sub
  { const float p = u[1] * w[2], q = u[2] * w[1]; c[0] = p - q; }
  { const float p = u[2] * w[0], q = u[0] * w[2]; c[1] = p - q; }
  { const float p = u[0] * w[1], q = u[1] * w[0]; c[2] = p - q; }
  const float sx = c[0] * c[0], sy = c[1] * c[1], sz = c[2] * c[2];
  const float sxy = sx + sy;
  const float r = sqrtf(sxy + sz);
  const float length = mesh_length(r, form);
  const float area = form == SS_MESH_FORM_PC ? length * 0.5f : 0.5f * r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float nf = c[k] / length;
    terms[3 * f + k] = nf * area;
  }
}

extern "C" int ss_mesh_face_terms(const float* coord, const int32_t* faces, int64_t n_faces, int64_t n_vertices, int form, float* terms,
                                  int32_t* status, hipStream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_vertices > 0x7fffffff || (form != SS_MESH_FORM_PC && form != SS_MESH_FORM_GS)) return SS_ERR_ARG;
  if (n_faces == 0) return SS_OK;
  if (!coord || !faces || !terms || !status) return SS_ERR_ARG;
  const int64_t grid = (n_faces + 255) / 256;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  SS_LAUNCH(k_mesh_face_terms, dim3((unsigned)grid), dim3(256), 0, stream, coord, faces, n_faces, (uint32_t)n_vertices, form, terms, status);
  return SS_OK;
}

// one lane per run of equal vertex along `order` (the stable argsort of the 3F corner entries by vertex): pairs ascend inside a run,
// so faces do.  PC: `nv[face[i]] += nf[i]` writes a vertex the face names twice ONCE; GS adds per corner.
__global__ void k_mesh_vertex_normals(const float* __restrict__ terms, const int32_t* __restrict__ faces, const int32_t* __restrict__ order,
                                      const int32_t* __restrict__ idx_ptr, const int32_t* __restrict__ head,
                                      const int32_t* __restrict__ n_runs, int64_t n_pairs, uint32_t n_vertices, int form,
                                      float* __restrict__ normal) {
  const int64_t run = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= *n_runs) return;
  const uint32_t h = (uint32_t)head[run];
  if (h >= (uint64_t)n_pairs) return;
  const uint32_t v = (uint32_t)faces[h];
  if (v >= n_vertices) return;
  int64_t j = idx_ptr[run], end = idx_ptr[run + 1];
  if (j < 0) j = 0;
  if (end > n_pairs) end = n_pairs;
  float acc[3] = {0.f, 0.f, 0.f};
  uint32_t prev = 0xffffffffu;
  for (; j < end; ++j) {
    const uint32_t p = (uint32_t)order[j];
    if (p >= (uint64_t)n_pairs) continue;
    const uint32_t f = p / 3u;
    if (form == SS_MESH_FORM_PC && f == prev) continue;
    prev = f;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + terms[3 * (int64_t)f + k];
  }
  const float sx = acc[0] * acc[0], sy = acc[1] * acc[1], sz = acc[2] * acc[2];
  const float sxy = sx + sy;
  const float length = mesh_length(sqrtf(sxy + sz), form);
#pragma unroll
  for (int k = 0; k < 3; ++k) normal[3 * (int64_t)v + k] = acc[k] / length;
}

extern "C" int ss_mesh_vertex_normals(const float* terms, const int32_t* faces, const int32_t* order, const int32_t* idx_ptr,
                                      const int32_t* head, const int32_t* n_runs, int64_t n_faces, int64_t n_vertices, int form,
                                      float* normal, hipStream_t stream) {
  if (n_faces < 0 || n_faces > 0x7fffffff / 3 || n_vertices < 0 || n_vertices > 0x7fffffff ||
      (form != SS_MESH_FORM_PC && form != SS_MESH_FORM_GS))
    return SS_ERR_ARG;
  if (n_faces == 0 || n_vertices == 0) return SS_OK;
  if (!terms || !faces || !order || !idx_ptr || !head || !n_runs || !normal) return SS_ERR_ARG;
  const int64_t pairs = 3 * n_faces;
  const int64_t most = pairs < n_vertices ? pairs : n_vertices;                // no more runs than vertices, nor than entries
  SS_LAUNCH(k_mesh_vertex_normals, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, stream, terms, faces, order, idx_ptr, head, n_runs,
            pairs, (uint32_t)n_vertices, form, normal);
  return SS_OK;
}

// ---- labels ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void k_mesh_labels(const int32_t* __restrict__ seg_indices, int64_t n_vertices, const int32_t* __restrict__ src,
                              const int32_t* __restrict__ seg_to_group, int64_t n_segments, const int32_t* __restrict__ t20,
                              const int32_t* __restrict__ t200, const int32_t* __restrict__ tinst, int n_groups, int64_t n,
                              T* __restrict__ s20, T* __restrict__ s200, T* __restrict__ inst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t row = src ? (int64_t)src[i] : i;
  int g = -1;
  if (row >= 0 && row < n_vertices) {
    const int64_t seg = seg_indices[row];
    if (seg >= 0 && seg < n_segments) g = seg_to_group[seg];
  }
  const bool have = g >= 0 && g < n_groups;
  s20[i] = (T)(have ? t20[g] : -1);
  s200[i] = (T)(have ? t200[g] : -1);
  inst[i] = (T)(have ? tinst[g] : -1);
}

extern "C" int ss_mesh_labels(const int32_t* seg_indices, int64_t n_vertices, const int32_t* src, const int32_t* seg_to_group,
                              int64_t n_segments, const int32_t* table20, const int32_t* table200, const int32_t* table_instance,
                              int n_groups, int64_t n, int out_bytes, void* segment20, void* segment200, void* instance, hipStream_t stream) {
  if (n < 0 || n_vertices < 0 || n_segments < 0 || n_groups < 0 || (out_bytes != 2 && out_bytes != 8)) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!segment20 || !segment200 || !instance || (n_vertices > 0 && !seg_indices) || (n_segments > 0 && !seg_to_group) ||
      (n_groups > 0 && (!table20 || !table200 || !table_instance)))
    return SS_ERR_ARG;
  const int64_t grid = (n + 255) / 256;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  if (out_bytes == 2)
    SS_LAUNCH(k_mesh_labels<int16_t>, dim3((unsigned)grid), dim3(256), 0, stream, seg_indices, n_vertices, src, seg_to_group, n_segments,
              table20, table200, table_instance, n_groups, n, (int16_t*)segment20, (int16_t*)segment200, (int16_t*)instance);
  else
    SS_LAUNCH(k_mesh_labels<int64_t>, dim3((unsigned)grid), dim3(256), 0, stream, seg_indices, n_vertices, src, seg_to_group, n_segments,
              table20, table200, table_instance, n_groups, n, (int64_t*)segment20, (int64_t*)segment200, (int64_t*)instance);
  return SS_OK;
}
