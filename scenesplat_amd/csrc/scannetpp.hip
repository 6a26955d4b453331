// ScanNet++ converter (pointcept/datasets/preprocessing/scannetpp/preprocess_scannetpp.py and preprocess_scannetpp_gs.py of the reference):
// the vertex normals in Open3D's definition and the top-3 label arrays, on the device.  The .ply blocks are decoded by csrc/mesh.hip.
//
//   normals   `TriangleMesh::ComputeVertexNormals(normalized = true)`: vertices held as doubles, per face the UNNORMALISED cross product
//             (v1 - v0) x (v2 - v0) in fp64 (mul, mul, sub: contraction is off for this file), per vertex the cross products of its
//             incident faces added in ascending face index, once per corner, into one fp64 accumulator per component, then
//             z = (x^2 + y^2) + z^2 and, where z > 0, a division by sqrt(z) (IEEE both); one rounding to fp32 at the end.  The incidence
//             is the sort and walk of csrc/mesh.hip: the 3F (vertex, 3 * face + corner) entries under a stable radix argsort by vertex
//             with ss_pool_partition's run boundaries, one lane per run.  No floating-point atomics: the order of the sums is the result.
//   labels    the reference's sequential loop over `segGroups` (a vertex takes up to three labels in group order, a group's size counts
//             the vertices it still found a free slot on, column 0 then goes to the smallest instance) restated per SEGMENT: every vertex
//             of a segment sees the same groups, so first3[s] = the first three valid groups that list s decides the slots of all its
//             vertices, and a vertex counts towards a group's size exactly when the group is in its segment's first3.
//             histogram of the segments -> per-group sizes -> one pass over the rows; integer atomics only, so no order shows.
#include "common.h"

#pragma clang fp contract(off)

#define SPP_BAD_INDEX 2                              // the status bit of csrc/mesh.hip
#define SPP_THREADS 256

// ---- vertex normals ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SPP_THREADS)
k_mesh_face_cross_f64(const float* __restrict__ coord, const int32_t* __restrict__ faces, int64_t F, uint32_t n_vertices,
                      double* __restrict__ cross, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const uint32_t i0 = (uint32_t)faces[3 * f], i1 = (uint32_t)faces[3 * f + 1], i2 = (uint32_t)faces[3 * f + 2];
  if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
    atomicOr(status, SPP_BAD_INDEX);
    cross[3 * f] = 0.0; cross[3 * f + 1] = 0.0; cross[3 * f + 2] = 0.0;
    return;
  }
  double a[3], u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = (double)coord[3 * (int64_t)i0 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = (double)coord[3 * (int64_t)i1 + k] - a[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = (double)coord[3 * (int64_t)i2 + k] - a[k];
  { const double p = u[1] * w[2], q = u[2] * w[1]; cross[3 * f] = p - q; }
  { const double p = u[2] * w[0], q = u[0] * w[2]; cross[3 * f + 1] = p - q; }
  { const double p = u[0] * w[1], q = u[1] * w[0]; cross[3 * f + 2] = p - q; }
}

extern "C" int ss_mesh_face_cross_f64(const float* coord, const int32_t* faces, int64_t n_faces, int64_t n_vertices, double* cross,
                                      int32_t* status, hipStream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_vertices > 0x7fffffff) return SS_ERR_ARG;
  if (n_faces == 0) return SS_OK;
  if (!coord || !faces || !cross || !status) return SS_ERR_ARG;
  const int64_t grid = (n_faces + SPP_THREADS - 1) / SPP_THREADS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  SS_LAUNCH(k_mesh_face_cross_f64, dim3((unsigned)grid), dim3(SPP_THREADS), 0, stream, coord, faces, n_faces, (uint32_t)n_vertices, cross,
            status);
  return SS_OK;
}

// one lane per run of equal vertex along `order`: entries ascend inside a run (the sort is stable), so faces do, and a face that names
// the vertex at two corners is added twice, as the loop over the triangles does
__global__ void __launch_bounds__(SPP_THREADS)
k_mesh_vertex_normals_f64(const double* __restrict__ cross, const int32_t* __restrict__ faces, const int32_t* __restrict__ order,
                          const int32_t* __restrict__ idx_ptr, const int32_t* __restrict__ head, const int32_t* __restrict__ n_runs,
                          int64_t n_pairs, uint32_t n_vertices, float* __restrict__ normal) {
  const int64_t run = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= *n_runs) return;
  const uint32_t h = (uint32_t)head[run];
  if (h >= (uint64_t)n_pairs) return;
  const uint32_t v = (uint32_t)faces[h];
  if (v >= n_vertices) return;
  int64_t j = idx_ptr[run], end = idx_ptr[run + 1];
  if (j < 0) j = 0;
  if (end > n_pairs) end = n_pairs;
  double acc[3] = {0.0, 0.0, 0.0};
  for (; j < end; ++j) {
    const uint32_t p = (uint32_t)order[j];
    if (p >= (uint64_t)n_pairs) continue;
    const uint32_t f = p / 3u;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + cross[3 * (int64_t)f + k];
  }
  const double sx = acc[0] * acc[0], sy = acc[1] * acc[1], sz = acc[2] * acc[2];
  const double sxy = sx + sy;
  const double z = sxy + sz;
  if (z > 0.0) {                                                               // a zero sum stays zero, a NaN stays as it is
    const double r = __dsqrt_rn(z);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = __ddiv_rn(acc[k], r);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) normal[3 * (int64_t)v + k] = (float)acc[k];
}

extern "C" int ss_mesh_vertex_normals_f64(const double* cross, const int32_t* faces, const int32_t* order, const int32_t* idx_ptr,
                                          const int32_t* head, const int32_t* n_runs, int64_t n_faces, int64_t n_vertices, float* normal,
                                          hipStream_t stream) {
  if (n_faces < 0 || n_faces > 0x7fffffff / 3 || n_vertices < 0 || n_vertices > 0x7fffffff) return SS_ERR_ARG;
  if (n_faces == 0 || n_vertices == 0) return SS_OK;
  if (!cross || !faces || !order || !idx_ptr || !head || !n_runs || !normal) return SS_ERR_ARG;
  const int64_t pairs = 3 * n_faces;
  const int64_t most = pairs < n_vertices ? pairs : n_vertices;                // no more runs than vertices, nor than entries
  SS_LAUNCH(k_mesh_vertex_normals_f64, dim3((unsigned)((most + SPP_THREADS - 1) / SPP_THREADS)), dim3(SPP_THREADS), 0, stream, cross, faces,
            order, idx_ptr, head, n_runs, pairs, (uint32_t)n_vertices, normal);
  return SS_OK;
}

// ---- labels ------------------------------------------------------------------------------------------------------------------------------
// (no LDS copy of the counters: a scan holds tens of thousands of segments, and the pass is a small share of the converter:
// profiles/scannetpp.md)
__global__ void __launch_bounds__(SPP_THREADS)
k_spp_segment_hist(const int32_t* __restrict__ seg_indices, int64_t n, int64_t n_segments, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t s = seg_indices[i];
  if (s >= 0 && s < n_segments) atomicAdd(count + s, 1);
}

extern "C" int ss_spp_segment_hist(const int32_t* seg_indices, int64_t n_vertices, int64_t n_segments, int32_t* count, hipStream_t stream) {
  if (n_vertices < 0 || n_vertices > 0x7fffffff || n_segments < 0) return SS_ERR_ARG;        // (a counter holds at most n_vertices)
  if (n_vertices == 0 || n_segments == 0) return SS_OK;
  if (!seg_indices || !count) return SS_ERR_ARG;
  const int64_t grid = (n_vertices + SPP_THREADS - 1) / SPP_THREADS;
  SS_LAUNCH(k_spp_segment_hist, dim3((unsigned)grid), dim3(SPP_THREADS), 0, stream, seg_indices, n_vertices, n_segments, count);
  return SS_OK;
}

__global__ void __launch_bounds__(SPP_THREADS)
k_spp_group_sizes(const int32_t* __restrict__ first3, const int32_t* __restrict__ count, int64_t n_segments, int n_groups,
                  int32_t* __restrict__ size) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_segments) return;
  const int32_t c = count[s];
  if (c == 0) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t g = first3[3 * s + k];
    if (g >= 0 && g < n_groups) atomicAdd(size + g, c);
  }
}

extern "C" int ss_spp_group_sizes(const int32_t* first3, const int32_t* count, int64_t n_segments, int n_groups, int32_t* size,
                                  hipStream_t stream) {
  if (n_segments < 0 || n_groups < 0) return SS_ERR_ARG;
  if (n_segments == 0 || n_groups == 0) return SS_OK;
  if (!first3 || !count || !size) return SS_ERR_ARG;
  const int64_t grid = (n_segments + SPP_THREADS - 1) / SPP_THREADS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  SS_LAUNCH(k_spp_group_sizes, dim3((unsigned)grid), dim3(SPP_THREADS), 0, stream, first3, count, n_segments, n_groups, size);
  return SS_OK;
}

struct SppRow { int32_t seg[3]; int32_t inst[3]; };

// the three labels of one row, column 0 swapped with the smallest instance's (np.argmin: the first of equal sizes)
__device__ __forceinline__ SppRow spp_row(int64_t i, const int32_t* __restrict__ seg_indices, int64_t n_vertices,
                                          const int32_t* __restrict__ src, const int32_t* __restrict__ first3, int64_t n_segments,
                                          const int32_t* __restrict__ table_label, const int32_t* __restrict__ table_object,
                                          const int32_t* __restrict__ size, int n_groups, int32_t empty) {
  SppRow r;
#pragma unroll
  for (int k = 0; k < 3; ++k) { r.seg[k] = empty; r.inst[k] = empty; }
  const int64_t row = src ? (int64_t)src[i] : i;
  if (row < 0 || row >= n_vertices) return r;
  const int64_t s = seg_indices[row];
  if (s < 0 || s >= n_segments) return r;
  int32_t g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = first3[3 * s + k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (g[k] >= n_groups) return r;                                            // a slot out of range: the row holds nothing
  int used = 0, p = 0;
  int64_t least = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (g[k] < 0) continue;                                                    // an empty slot: +inf, never the first smallest
    r.seg[k] = table_label[g[k]];
    r.inst[k] = table_object[g[k]];
    const int64_t sz = size[g[k]];
    if (used == 0 || sz < least) { least = sz; p = k; }
    ++used;
  }
  if (used > 1 && p != 0) {
    const int32_t a = r.seg[0], b = r.inst[0];
    r.seg[0] = r.seg[p]; r.inst[0] = r.inst[p];
    r.seg[p] = a; r.inst[p] = b;
  }
  return r;
}

__device__ __forceinline__ uint32_t spp_pack(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

struct SppWords { uint32_t x, y, z; };                 // 12 bytes at 4-byte alignment: one three-word store

// one lane per PAIR of rows: 12 bytes = three words per output, lanes on consecutive 12-byte pieces.  The last lane of an odd n writes
// its single row as three int16.
__global__ void __launch_bounds__(SPP_THREADS)
k_spp_labels(const int32_t* __restrict__ seg_indices, int64_t n_vertices, const int32_t* __restrict__ src,
             const int32_t* __restrict__ first3, int64_t n_segments, const int32_t* __restrict__ table_label,
             const int32_t* __restrict__ table_object, const int32_t* __restrict__ size, int n_groups, int64_t n, int32_t empty,
             int16_t* __restrict__ segment, int16_t* __restrict__ instance) {
  const int64_t pair = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = 2 * pair;
  if (i >= n) return;
  const SppRow a = spp_row(i, seg_indices, n_vertices, src, first3, n_segments, table_label, table_object, size, n_groups, empty);
  if (i + 1 < n) {
    const SppRow b = spp_row(i + 1, seg_indices, n_vertices, src, first3, n_segments, table_label, table_object, size, n_groups, empty);
    SppWords s, t;
    s.x = spp_pack(a.seg[0], a.seg[1]); s.y = spp_pack(a.seg[2], b.seg[0]); s.z = spp_pack(b.seg[1], b.seg[2]);
    t.x = spp_pack(a.inst[0], a.inst[1]); t.y = spp_pack(a.inst[2], b.inst[0]); t.z = spp_pack(b.inst[1], b.inst[2]);
    *reinterpret_cast<SppWords*>(segment + 3 * i) = s;                         // byte 6 * i = 12 * pair: a multiple of 4
    *reinterpret_cast<SppWords*>(instance + 3 * i) = t;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      segment[3 * i + k] = (int16_t)a.seg[k];
      instance[3 * i + k] = (int16_t)a.inst[k];
    }
  }
}

extern "C" int ss_spp_labels(const int32_t* seg_indices, int64_t n_vertices, const int32_t* src, const int32_t* first3, int64_t n_segments,
                             const int32_t* table_label, const int32_t* table_object, const int32_t* size, int n_groups, int64_t n,
                             int empty, int16_t* segment, int16_t* instance, hipStream_t stream) {
  if (n < 0 || n_vertices < 0 || n_segments < 0 || n_groups < 0 || empty < -32768 || empty > 32767) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!segment || !instance || (n_vertices > 0 && !seg_indices) || (n_segments > 0 && !first3) ||
      (n_groups > 0 && (!table_label || !table_object || !size)))
    return SS_ERR_ARG;
  if (((uintptr_t)segment & 3) || ((uintptr_t)instance & 3)) return SS_ERR_ARG;
  const int64_t grid = ((n + 1) / 2 + SPP_THREADS - 1) / SPP_THREADS;
  if (grid > 0x7fffffff) return SS_ERR_ARG;
  SS_LAUNCH(k_spp_labels, dim3((unsigned)grid), dim3(SPP_THREADS), 0, stream, seg_indices, n_vertices, src, first3, n_segments,
            table_label, table_object, size, n_groups, n, (int32_t)empty, segment, instance);
  return SS_OK;
}
