// Scene ingest: the astype / clip / reshape / [:, 0] block of the reference's dataset classes (pointcept/datasets/scannetgs.py:93-153
// and its siblings) for ALL assets of a scene in ONE grouped launch.  The host packs the .npy payloads, in their stored dtypes, into
// one arena (one upload); every problem of the launch turns one asset of the arena into its output tensor.
// desc: 8 int64 words per problem = {src, dst, n_out, src dtype | dst dtype << 8 | flags << 16, src row stride, column, lo, hi}
// (lo / hi: fp32 bit patterns in the low 32 bits).  A workgroup owns INGEST_PER_WG consecutive OUTPUT elements of one problem; the
// type pair is a property of the problem, so the dispatch branch is uniform over the workgroup.
// Values are numpy's, bit for bit: float narrowing is the hardware's round-to-nearest-even conversion (overflow to inf, subnormals
// kept), integer narrowing wraps, bool is "any bit set", and the clip is two ordered compares (NaN stays NaN, -0.0 passes lo = 0).
#include "grouped.h"

#define INGEST_PER_WG 4096
#define ING_F64 0
#define ING_F32 1
#define ING_F16 2
#define ING_U8 3
#define ING_I8 4
#define ING_I16 5
#define ING_I32 6
#define ING_I64 7
#define ING_BOOL 8
#define ING_HAS_LO 1
#define ING_HAS_HI 2
#define ING_PICK 4

template <int C> struct ing_type;
template <> struct ing_type<ING_F64> { typedef double T; };
template <> struct ing_type<ING_F32> { typedef float T; };
template <> struct ing_type<ING_F16> { typedef _Float16 T; };
template <> struct ing_type<ING_U8> { typedef uint8_t T; };
template <> struct ing_type<ING_I8> { typedef int8_t T; };
template <> struct ing_type<ING_I16> { typedef int16_t T; };
template <> struct ing_type<ING_I32> { typedef int32_t T; };
template <> struct ing_type<ING_I64> { typedef int64_t T; };
template <> struct ing_type<ING_BOOL> { typedef uint8_t T; };      // a numpy bool is one byte

template <typename T, int N> using ing_vec = T __attribute__((ext_vector_type(N)));

struct IngestClip { float lo, hi; int flags; };

// one value, as numpy's astype (then clip) computes it
template <int SC, int DC>
__device__ __forceinline__ typename ing_type<DC>::T ingest_one(typename ing_type<SC>::T v, const IngestClip& c) {
  typedef typename ing_type<DC>::T D;
  if constexpr (DC == ING_BOOL) {
    return (D)(v != 0);                                              // any bit set, not the low byte
  } else if constexpr (SC == ING_BOOL) {
    return (D)(v != 0 ? 1 : 0);
  } else if constexpr (DC == ING_F32) {
    float o = (float)v;
    if (c.flags & ING_HAS_LO) o = o < c.lo ? c.lo : o;               // ordered compares: NaN fails both and stays, -0.0 < 0 is false
    if (c.flags & ING_HAS_HI) o = o > c.hi ? c.hi : o;
    return o;
  } else {
    return (D)v;
  }
}

// V converted values -> memory in stores of at most 16 bytes (dst + e is aligned to min(16, V * sizeof(D)) on the vector path)
template <typename D, int V>
__device__ __forceinline__ void ingest_store(__attribute__((address_space(1))) D* p, const D (&o)[V]) {
  constexpr int W = (V * sizeof(D) >= 16) ? (int)(16 / sizeof(D)) : V;
#pragma unroll
  for (int i = 0; i < V; i += W) {
    ing_vec<D, W> t;
#pragma unroll
    for (int j = 0; j < W; ++j) t[j] = o[i + j];
    *reinterpret_cast<__attribute__((address_space(1))) ing_vec<D, W>*>(p + i) = t;
  }
}

template <int SC, int DC>
__device__ __forceinline__ void ingest_span(const int64_t* __restrict__ d, int64_t e0) {
  typedef typename ing_type<SC>::T S;
  typedef typename ing_type<DC>::T D;
  typedef __attribute__((address_space(1))) const S gS;
  typedef __attribute__((address_space(1))) D gD;
  constexpr int V = 16 / sizeof(S);                                  // source elements of one 16-byte load
  gS* src = reinterpret_cast<gS*>(d[0]);
  gD* dst = reinterpret_cast<gD*>(d[1]);
  const int64_t n = d[2];
  const int flags = (int)((d[3] >> 16) & 0xff);
  IngestClip c;
  c.lo = __int_as_float((int)(uint32_t)d[6]);
  c.hi = __int_as_float((int)(uint32_t)d[7]);
  c.flags = flags;
  if (flags & ING_PICK) {                                            // out[k] = src[k * stride + column]: one element per thread
    const int64_t stride = d[4], col = d[5];
#pragma unroll 4
    for (int i = 0; i < INGEST_PER_WG / 256; ++i) {
      const int64_t k = e0 + (int64_t)i * 256 + threadIdx.x;
      if (k < n) dst[k] = ingest_one<SC, DC>(src[k * stride + col], c);
    }
    return;
  }
  // e0 * sizeof(S) is a multiple of 16 (INGEST_PER_WG is), so the span is aligned when the two bases are
  const bool vec16 = ((d[0] | d[1]) & 15) == 0;
  group_span<INGEST_PER_WG, V>(
      e0, n, vec16,
      [&](int64_t e) {
        const ing_vec<S, V> a = *reinterpret_cast<__attribute__((address_space(1))) const ing_vec<S, V>*>(src + e);
        D o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = ingest_one<SC, DC>(a[j], c);
        ingest_store<D, V>(dst + e, o);
      },
      [&](int64_t k) { dst[k] = ingest_one<SC, DC>(src[k], c); });
}

// same dtype -> same dtype without a clip: a copy of BYTES-wide words (also the clone of a cached arena's asset)
template <int BYTES> struct ing_word;
template <> struct ing_word<1> { static constexpr int code = ING_U8; };
template <> struct ing_word<2> { static constexpr int code = ING_I16; };
template <> struct ing_word<4> { static constexpr int code = ING_I32; };
template <> struct ing_word<8> { static constexpr int code = ING_I64; };

__device__ __forceinline__ int ingest_bytes(int code) {
  return code == ING_F64 || code == ING_I64 ? 8 : code == ING_F32 || code == ING_I32 ? 4 : code == ING_F16 || code == ING_I16 ? 2 : 1;
}

__global__ void __launch_bounds__(256)
k_ingest_group(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob) {
  const int b = blockIdx.x;
  const int p = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)p * 8;
  const int64_t e0 = (int64_t)(b - wg_start[p]) * INGEST_PER_WG;
  const int sc = (int)(d[3] & 0xff), dc = (int)((d[3] >> 8) & 0xff);
  if (sc == dc && !(dc == ING_F32 && ((d[3] >> 16) & (ING_HAS_LO | ING_HAS_HI)))) {
    switch (ingest_bytes(sc)) {
      case 1: ingest_span<ing_word<1>::code, ing_word<1>::code>(d, e0); break;
      case 2: ingest_span<ing_word<2>::code, ing_word<2>::code>(d, e0); break;
      case 4: ingest_span<ing_word<4>::code, ing_word<4>::code>(d, e0); break;
      default: ingest_span<ing_word<8>::code, ing_word<8>::code>(d, e0); break;
    }
    return;
  }
#define ING_CASE(S, D) case ((S) | ((D) << 8)): ingest_span<S, D>(d, e0); break;
  switch (sc | (dc << 8)) {
    ING_CASE(ING_F64, ING_F32) ING_CASE(ING_F32, ING_F32) ING_CASE(ING_F16, ING_F32) ING_CASE(ING_U8, ING_F32) ING_CASE(ING_I8, ING_F32)
    ING_CASE(ING_I16, ING_F32) ING_CASE(ING_I32, ING_F32) ING_CASE(ING_I64, ING_F32) ING_CASE(ING_BOOL, ING_F32)
    ING_CASE(ING_F32, ING_F16)
    ING_CASE(ING_U8, ING_I32) ING_CASE(ING_I8, ING_I32) ING_CASE(ING_I16, ING_I32) ING_CASE(ING_I64, ING_I32) ING_CASE(ING_BOOL, ING_I32)
    ING_CASE(ING_U8, ING_BOOL) ING_CASE(ING_I8, ING_BOOL) ING_CASE(ING_I16, ING_BOOL) ING_CASE(ING_I32, ING_BOOL) ING_CASE(ING_I64, ING_BOOL)
    default: break;                                                  // (native.ingest_group refuses every other pair before the launch)
  }
#undef ING_CASE
}

extern "C" int ss_ingest_group_elems_per_workgroup(void) { return INGEST_PER_WG; }
extern "C" int ss_ingest_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, hipStream_t stream) {
  SS_GROUP_GUARD(desc, wg_start, nprob, total_workgroups);
  SS_LAUNCH(k_ingest_group, dim3((unsigned)total_workgroups), dim3(256), 0, stream, desc, wg_start, nprob);
  return SS_OK;
}
