// Fused tail of a pre-norm PTv3 Block (ptv3:318-338) at C <= 256: from the attention output to the end of the Block in ONE
// launch each way instead of six (proj | add + DropPath scale + LN2 | fc1 | GELU | fc2 | add + DropPath scale):
//     y1 = bf16(feat Wp^T + bp);  x_mid = x + rs1 y1;  h2 = bf16(LN2(x_mid));  u = bf16(h2 W1^T + b1);  a = bf16(gelu(u));
//     y2 = bf16(a W2^T + b2);     x_out = x_mid + rs2 y2            (every rounding where the six-launch chain rounds; the
//     biases are read as fp32 or as the bf16 shadows the chain's GEMMs read)
// backward: dy2 = bf16(rs2 g);  da = bf16(dy2 W2);  du = bf16(da gelu'(u));  dh2 = bf16(du W1);  g_mid = g + LN2'(dh2);
//           dy1 = bf16(rs1 g_mid);  dfeat = bf16(dy1 Wp);  per-workgroup partial rows of dgamma2 / dbeta2.  No atomics.
// One workgroup owns BT_R = 32 rows; the activations of the tile stay in LDS (bf16, rows padded by 16 bytes: the ds_read_b128 of
// an MFMA A fragment is then at most 2-way conflicted) or registers between the products.  The weights are K-contiguous, at
// most 1.2 MB per Block and L2-resident: a lane loads its 16-byte v_mfma_f32_16x16x32_bf16 B fragment straight from global
// memory, no LDS staging.  Products write their bf16 result to LDS; every global store is a coalesced row-wise pass.
// Waves per workgroup grow with C (4 / 4 / 8 / 16): at C = 256 a tile streams the whole 1.2 MB and the pooled levels have
// fewer tiles than CUs, so the time is one tile's weight stream -- shared out over more waves with more loads in flight.
#include "common.h"
#include "rowmath.h"

#define BT_R 32
#define BT_MAX_BWD_BLOCKS 1024
#define BT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

template <int C> struct BtCfg {
  static constexpr int NW = C <= 64 ? 4 : (C == 128 ? 8 : 16);   // waves per workgroup
  static constexpr int THREADS = NW * 64;
  static constexpr int LPR = C / 4;                // lanes per row in the row-wise passes (4 channels per lane)
  static constexpr int RPP = THREADS / LPR;        // rows per pass
  static constexpr int PASSES = BT_R / RPP;
  static constexpr int LDC = C + 8, LDH = 4 * C + 8;   // LDS row strides (elements)
  static_assert(BT_R % RPP == 0 && PASSES >= 1, "row passes must tile the row block");
};

// sOut[BT_R][N + 8] = bf16(sIn[BT_R][K + 8] . W^T + bias), W (N, K) bf16 row-major in global memory.  All NW waves of the
// workgroup call it; the caller puts a barrier before (sIn complete) and after (sOut complete).
template <int N, int K, int NW>
__device__ __forceinline__ void bt_gemm(const unsigned short* sIn, const unsigned short* __restrict__ W,
                                        const void* __restrict__ bias, int bias_dt, unsigned short* sOut) {
  constexpr int LDI = K + 8, LDO = N + 8, NT = N / 16;
  constexpr int RG = NT >= NW ? 2 : 1;             // row tiles (of 16) per work item: both when there are enough column tiles
  constexpr int ITEMS = NT * (2 / RG);
  constexpr int UNR = NW == 16 ? 4 : 8;            // B fragments in flight per wave (the 16-wave form has 128 VGPRs per lane)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  for (int it = wave; it < ITEMS; it += NW) {
    const int ct = it % NT, rt0 = (it / NT) * RG;
    f32x4_t acc[RG];
#pragma unroll
    for (int g = 0; g < RG; ++g) acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (K % 64 == 0) {
      // two k-steps per 64 columns of K: a lane owns 32 contiguous bytes of its weight row (k = 16 fq .. 16 fq + 15), so the 16
      // rows of a wave's load pair cover whole 128-byte lines; the first 8 feed one MFMA, the next 8 the other, and the A
      // fragments follow the same k order (a sum over k does not care which MFMA takes which k)
      const unsigned short* wrow = W + (size_t)(ct * 16 + fr) * K + fq * 16;
      const unsigned short* arow = sIn + (rt0 * 16 + fr) * LDI + fq * 16;
#pragma unroll UNR / 2
      for (int k0 = 0; k0 < K; k0 += 64) {
        const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(wrow + k0);
        const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(wrow + k0 + 8);
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          const bf16x8_t a0 = *reinterpret_cast<const bf16x8_t*>(arow + g * 16 * LDI + k0);
          const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t*>(arow + g * 16 * LDI + k0 + 8);
          acc[g] = BT_MFMA(a0, b0, acc[g]);
          acc[g] = BT_MFMA(a1, b1, acc[g]);
        }
      }
    } else {
      const unsigned short* wrow = W + (size_t)(ct * 16 + fr) * K + fq * 8;
      const unsigned short* arow = sIn + (rt0 * 16 + fr) * LDI + fq * 8;
#pragma unroll UNR
      for (int k0 = 0; k0 < K; k0 += 32) {
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(wrow + k0);
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(arow + g * 16 * LDI + k0);
          acc[g] = BT_MFMA(a, b, acc[g]);
        }
      }
    }
    const int col = ct * 16 + fr;
    const float bv = !bias ? 0.f : (bias_dt == SS_F32 ? reinterpret_cast<const float*>(bias)[col]
                                                     : bf16_to_f32(reinterpret_cast<const unsigned short*>(bias)[col]));
#pragma unroll
    for (int g = 0; g < RG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) sOut[((rt0 + g) * 16 + fq * 4 + i) * LDO + col] = f32_to_bf16(acc[g][i] + bv);
  }
}

__device__ __forceinline__ float4 bt_lds_ld4(const unsigned short* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ uint2 bt_pack4(const float4& v) {
  uint2 u; u.x = pack_bf16x2(v.x, v.y); u.y = pack_bf16x2(v.z, v.w);
  return u;
}

// global (rows, W) bf16 tile <-> LDS [BT_R][W + 8], 16 bytes per lane; rows past `rows` read as zeros / are not written
template <int W, int THREADS>
__device__ __forceinline__ void bt_tile_load(const unsigned short* __restrict__ src, unsigned short* s, int rows) {
  for (int i = threadIdx.x; i < BT_R * (W / 8); i += THREADS) {
    const int r = i / (W / 8), c = (i % (W / 8)) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < rows) v = *reinterpret_cast<const uint4*>(src + (int64_t)r * W + c);
    *reinterpret_cast<uint4*>(s + r * (W + 8) + c) = v;
  }
}
template <int W, int THREADS>
__device__ __forceinline__ void bt_tile_store(const unsigned short* s, unsigned short* __restrict__ dst, int rows) {
  for (int i = threadIdx.x; i < BT_R * (W / 8); i += THREADS) {
    const int r = i / (W / 8), c = (i % (W / 8)) * 8;
    if (r < rows) *reinterpret_cast<uint4*>(dst + (int64_t)r * W + c) = *reinterpret_cast<const uint4*>(s + r * (W + 8) + c);
  }
}

template <int C>
__global__ void __launch_bounds__(BtCfg<C>::THREADS)
k_block_tail_fwd(const unsigned short* __restrict__ feat, const float* __restrict__ x, const float* __restrict__ rs1,
                 const float* __restrict__ rs2, const unsigned short* __restrict__ Wp, const void* __restrict__ bp,
                 const unsigned short* __restrict__ W1, const void* __restrict__ b1, const unsigned short* __restrict__ W2,
                 const void* __restrict__ b2, int bias_dt, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                 float* __restrict__ x_mid, float* __restrict__ mean, float* __restrict__ rstd, unsigned short* __restrict__ h2,
                 unsigned short* __restrict__ u, unsigned short* __restrict__ a, float* __restrict__ x_out,
                 unsigned short* __restrict__ xcopy, int64_t n) {
  using Cf = BtCfg<C>;
  constexpr int H = 4 * C, LDC = Cf::LDC, LDH = Cf::LDH, T = Cf::THREADS;
  __shared__ __attribute__((aligned(16))) unsigned short sA[BT_R * LDC];    // feat, then h2
  __shared__ __attribute__((aligned(16))) unsigned short sB[BT_R * LDC];    // y1, then y2
  __shared__ __attribute__((aligned(16))) unsigned short sH[BT_R * LDH];    // u, then a
  const int64_t row0 = (int64_t)blockIdx.x * BT_R;
  const int rows = (int)((n - row0) < BT_R ? (n - row0) : BT_R);
  const int pr = threadIdx.x / Cf::LPR, pj = (threadIdx.x % Cf::LPR) * 4;    // this lane's (row of a pass, first channel)

  bt_tile_load<C, T>(feat + row0 * C, sA, rows);
  __syncthreads();
  bt_gemm<C, C, Cf::NW>(sA, Wp, bp, bias_dt, sB);
  __syncthreads();

  // x_mid = x + rs1 * y1; LN2 -> h2 (LDS + global)
  float4 xm[Cf::PASSES];
  const float4 gm = *reinterpret_cast<const float4*>(gamma + pj), bt = *reinterpret_cast<const float4*>(beta + pj);
#pragma unroll
  for (int p = 0; p < Cf::PASSES; ++p) {
    const int r = p * Cf::RPP + pr;
    const bool valid = r < rows;
    const int64_t g = (row0 + r) * C + pj;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
      v = *reinterpret_cast<const float4*>(x + g);
      const float s = rs1 ? rs1[row0 + r] : 1.f;
      const float4 y = bt_lds_ld4(sB + r * LDC + pj);
      v.x += s * y.x; v.y += s * y.y; v.z += s * y.z; v.w += s * y.w;
      *reinterpret_cast<float4*>(x_mid + g) = v;
    }
    xm[p] = v;
    const float mu = lanes_reduce_sum<Cf::LPR>(ln_sum4(v)) / C;
    const float rr = rsqrtf(lanes_reduce_sum<Cf::LPR>(ln_sqdev4(v, mu)) / C + eps);
    const uint2 hp = bt_pack4(ln_apply4(v, mu, rr, gm, bt));
    *reinterpret_cast<uint2*>(sA + r * LDC + pj) = hp;
    if (valid) {
      *reinterpret_cast<uint2*>(h2 + g) = hp;
      if (pj == 0) { mean[row0 + r] = mu; rstd[row0 + r] = rr; }
    }
  }
  __syncthreads();
  bt_gemm<H, C, Cf::NW>(sA, W1, b1, bias_dt, sH);
  __syncthreads();

  // u -> global; a = gelu(u) -> LDS (in place) + global
  for (int i = threadIdx.x; i < BT_R * (H / 8); i += T) {
    const int r = i / (H / 8), c = (i % (H / 8)) * 8;
    const uint4 uv = *reinterpret_cast<const uint4*>(sH + r * LDH + c);
    float f[8];
    bf8_unpack(uv, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = gelu_f(f[e]);
    const uint4 av = bf8_pack(f);
    *reinterpret_cast<uint4*>(sH + r * LDH + c) = av;
    if (r < rows) {
      const int64_t g = (row0 + r) * H + c;
      *reinterpret_cast<uint4*>(u + g) = uv;
      *reinterpret_cast<uint4*>(a + g) = av;
    }
  }
  __syncthreads();
  bt_gemm<C, H, Cf::NW>(sH, W2, b2, bias_dt, sB);
  __syncthreads();

  // x_out = x_mid + rs2 * y2 (+ bf16 copy)
#pragma unroll
  for (int p = 0; p < Cf::PASSES; ++p) {
    const int r = p * Cf::RPP + pr;
    if (r < rows) {
      const int64_t g = (row0 + r) * C + pj;
      const float s = rs2 ? rs2[row0 + r] : 1.f;
      const float4 y = bt_lds_ld4(sB + r * LDC + pj);
      float4 v = xm[p];
      v.x += s * y.x; v.y += s * y.y; v.z += s * y.z; v.w += s * y.w;
      *reinterpret_cast<float4*>(x_out + g) = v;
      if (xcopy) *reinterpret_cast<uint2*>(xcopy + g) = bt_pack4(v);
    }
  }
}

template <int C>
__global__ void __launch_bounds__(BtCfg<C>::THREADS)
k_block_tail_bwd(const float* __restrict__ g_xout, const unsigned short* __restrict__ g_xcopy, const float* __restrict__ x_mid,
                 const float* __restrict__ mean, const float* __restrict__ rstd, const unsigned short* __restrict__ u,
                 const float* __restrict__ rs1, const float* __restrict__ rs2, const float* __restrict__ gamma,
                 const unsigned short* __restrict__ Wpt, const unsigned short* __restrict__ W1t,
                 const unsigned short* __restrict__ W2t, float* __restrict__ g_mid, unsigned short* __restrict__ dfeat,
                 unsigned short* __restrict__ dy2, unsigned short* __restrict__ du, unsigned short* __restrict__ dy1,
                 float* __restrict__ part /* (2, gridDim.x, C): dgamma | dbeta */, int64_t n) {
  using Cf = BtCfg<C>;
  constexpr int H = 4 * C, LDC = Cf::LDC, LDH = Cf::LDH, T = Cf::THREADS;
  __shared__ __attribute__((aligned(16))) unsigned short sA[BT_R * LDC];    // dy2, then dy1
  __shared__ __attribute__((aligned(16))) unsigned short sB[BT_R * LDC];    // dh2, then dfeat
  __shared__ __attribute__((aligned(16))) unsigned short sH[BT_R * LDH];    // da, then du; at the end the column partials
  static_assert(2 * Cf::RPP * C * 4 <= BT_R * LDH * 2, "column partials must fit the hidden tile");
  const int pr = threadIdx.x / Cf::LPR, pj = (threadIdx.x % Cf::LPR) * 4;
  const float4 gm = *reinterpret_cast<const float4*>(gamma + pj);
  float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg;
  const int64_t ntiles = (n + BT_R - 1) / BT_R;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * BT_R;
    const int rows = (int)((n - row0) < BT_R ? (n - row0) : BT_R);
    // g = g_xout (+ g_xcopy), kept in registers; dy2 = bf16(rs2 * g)
    float4 gr[Cf::PASSES];
#pragma unroll
    for (int p = 0; p < Cf::PASSES; ++p) {
      const int r = p * Cf::RPP + pr;
      const int64_t g = (row0 + r) * C + pj;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      float s = 0.f;
      if (r < rows) {
        v = *reinterpret_cast<const float4*>(g_xout + g);
        if (g_xcopy) { const float4 e = ln_ld4(g_xcopy, SS_BF16, g); v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w; }
        s = rs2 ? rs2[row0 + r] : 1.f;
      }
      gr[p] = v;
      const uint2 d = bt_pack4(make_float4(s * v.x, s * v.y, s * v.z, s * v.w));
      *reinterpret_cast<uint2*>(sA + r * LDC + pj) = d;
      if (r < rows) *reinterpret_cast<uint2*>(dy2 + g) = d;
    }
    __syncthreads();
    bt_gemm<H, C, Cf::NW>(sA, W2t, nullptr, SS_F32, sH);
    __syncthreads();
    // du = bf16(da * gelu'(u)) -> LDS (in place) + global; four elements per lane and step (erff + expf of eight at once spilled
    // registers at the 128 a lane has in the 16-wave form)
    for (int i = threadIdx.x; i < BT_R * (H / 4); i += T) {
      const int r = i / (H / 4), c = (i % (H / 4)) * 4;
      const int64_t g = (row0 + r) * H + c;
      float4 f = bt_lds_ld4(sH + r * LDH + c);
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) z = ln_ld4(u, SS_BF16, g);
      f.x *= dgelu_exact(z.x); f.y *= dgelu_exact(z.y); f.z *= dgelu_exact(z.z); f.w *= dgelu_exact(z.w);
      const uint2 dv = bt_pack4(f);
      *reinterpret_cast<uint2*>(sH + r * LDH + c) = dv;
      if (r < rows) *reinterpret_cast<uint2*>(du + g) = dv;
    }
    __syncthreads();
    bt_gemm<C, H, Cf::NW>(sH, W1t, nullptr, SS_F32, sB);
    __syncthreads();
    // g_mid = g + LN2'(dh2); dy1 = bf16(rs1 * g_mid); column sums of dgamma / dbeta in registers
#pragma unroll
    for (int p = 0; p < Cf::PASSES; ++p) {
      const int r = p * Cf::RPP + pr;
      const bool valid = r < rows;
      const int64_t g = (row0 + r) * C + pj;
      float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), gh = xv;
      float mu = 0.f, rr = 0.f, s = 0.f;
      if (valid) {
        xv = *reinterpret_cast<const float4*>(x_mid + g);
        gh = bt_lds_ld4(sB + r * LDC + pj);
        mu = mean[row0 + r]; rr = rstd[row0 + r];
        s = rs1 ? rs1[row0 + r] : 1.f;
      }
      const float4 xh = ln_xhat4(xv, mu, rr);
      const float4 gy = make_float4(gh.x * gm.x, gh.y * gm.y, gh.z * gm.z, gh.w * gm.w);
      const float c1 = lanes_reduce_sum<Cf::LPR>(ln_sum4(gy)) / C;
      const float c2 = lanes_reduce_sum<Cf::LPR>(gy.x * xh.x + gy.y * xh.y + gy.z * xh.z + gy.w * xh.w) / C;
      float4 gv = ln_dx4(gy, xh, c1, c2, rr);
      gv.x += gr[p].x; gv.y += gr[p].y; gv.z += gr[p].z; gv.w += gr[p].w;
      dg.x += gh.x * xh.x; dg.y += gh.y * xh.y; dg.z += gh.z * xh.z; dg.w += gh.w * xh.w;
      db.x += gh.x; db.y += gh.y; db.z += gh.z; db.w += gh.w;
      const uint2 d = bt_pack4(make_float4(s * gv.x, s * gv.y, s * gv.z, s * gv.w));
      *reinterpret_cast<uint2*>(sA + r * LDC + pj) = d;
      if (valid) {
        *reinterpret_cast<float4*>(g_mid + g) = gv;
        *reinterpret_cast<uint2*>(dy1 + g) = d;
      }
    }
    __syncthreads();
    bt_gemm<C, C, Cf::NW>(sA, Wpt, nullptr, SS_F32, sB);
    __syncthreads();
    bt_tile_store<C, T>(sB, dfeat + row0 * C, rows);
    __syncthreads();                     // the next tile overwrites sA / sB
  }

  // column partials of this workgroup: the RPP lanes that own a channel are summed in a fixed order
  float* red = reinterpret_cast<float*>(sH);                  // [2][RPP][C]
  *reinterpret_cast<float4*>(red + (0 * Cf::RPP + pr) * C + pj) = dg;
  *reinterpret_cast<float4*>(red + (1 * Cf::RPP + pr) * C + pj) = db;
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * C; j += T) {
    const int k = j / C, c = j - k * C;
    float acc = 0.f;
    for (int q = 0; q < Cf::RPP; ++q) acc += red[(k * Cf::RPP + q) * C + c];
    part[((int64_t)k * gridDim.x + blockIdx.x) * C + c] = acc;
  }
}

extern "C" int ss_block_tail_rows(void) { return BT_R; }

extern "C" int ss_block_tail_bwd_blocks(int64_t n) {
  int64_t b = (n + BT_R - 1) / BT_R;
  if (b > BT_MAX_BWD_BLOCKS) b = BT_MAX_BWD_BLOCKS;
  return (int)(b < 1 ? 1 : b);
}

static bool bt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int ss_block_tail_fwd(const void* feat, const float* x, const float* rs1, const float* rs2, const void* wp,
                                 const void* bp, const void* w1, const void* b1, const void* w2, const void* b2, int bias_dtype,
                                 const float* gamma, const float* beta, float eps, float* x_mid, float* mean, float* rstd,
                                 void* h2, void* u, void* a, float* x_out, void* xcopy_bf16, int64_t n, int channels,
                                 hipStream_t stream) {
  if (n < 0 || !(channels == 32 || channels == 64 || channels == 128 || channels == 256)) return SS_ERR_ARG;
  if (bias_dtype != SS_F32 && bias_dtype != SS_BF16) return SS_ERR_ARG;
  if (!feat || !x || !wp || !bp || !w1 || !b1 || !w2 || !b2 || !gamma || !beta || !x_mid || !mean || !rstd || !h2 || !u || !a || !x_out)
    return SS_ERR_ARG;
  const void* al[] = {feat, x, wp, w1, w2, gamma, beta, x_mid, h2, u, a, x_out, xcopy_bf16};
  for (const void* p : al) if (!bt_aligned16(p)) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  const dim3 g((unsigned)((n + BT_R - 1) / BT_R));
#define SS_BT_FWD(CC) SS_LAUNCH(k_block_tail_fwd<CC>, g, dim3(BtCfg<CC>::THREADS), 0, stream, (const unsigned short*)feat, x, rs1, rs2, \
    (const unsigned short*)wp, bp, (const unsigned short*)w1, b1, (const unsigned short*)w2, b2, bias_dtype, gamma, beta, eps, x_mid, mean, rstd, \
    (unsigned short*)h2, (unsigned short*)u, (unsigned short*)a, x_out, (unsigned short*)xcopy_bf16, n)
  switch (channels) { case 32: SS_BT_FWD(32); break; case 64: SS_BT_FWD(64); break; case 128: SS_BT_FWD(128); break; default: SS_BT_FWD(256); break; }
#undef SS_BT_FWD
  return SS_OK;
}

extern "C" int ss_block_tail_bwd(const float* g_xout, const void* g_xcopy_bf16, const float* x_mid, const float* mean,
                                 const float* rstd, const void* u, const float* rs1, const float* rs2, const float* gamma,
                                 const void* wp_t, const void* w1_t, const void* w2_t, float* g_mid, void* dfeat, void* dy2,
                                 void* du, void* dy1, float* part, int64_t n, int channels, int nblocks, hipStream_t stream) {
  if (n < 0 || !(channels == 32 || channels == 64 || channels == 128 || channels == 256)) return SS_ERR_ARG;
  if (!g_xout || !x_mid || !mean || !rstd || !u || !gamma || !wp_t || !w1_t || !w2_t || !g_mid || !dfeat || !dy2 || !du || !dy1 || !part)
    return SS_ERR_ARG;
  if (nblocks < 1 || nblocks > BT_MAX_BWD_BLOCKS) return SS_ERR_ARG;
  const void* al[] = {g_xout, g_xcopy_bf16, x_mid, u, gamma, wp_t, w1_t, w2_t, g_mid, dfeat, dy2, du, dy1};
  for (const void* p : al) if (!bt_aligned16(p)) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  const dim3 g((unsigned)nblocks);
#define SS_BT_BWD(CC) SS_LAUNCH(k_block_tail_bwd<CC>, g, dim3(BtCfg<CC>::THREADS), 0, stream, g_xout, (const unsigned short*)g_xcopy_bf16, \
    x_mid, mean, rstd, (const unsigned short*)u, rs1, rs2, gamma, (const unsigned short*)wp_t, (const unsigned short*)w1_t, \
    (const unsigned short*)w2_t, g_mid, (unsigned short*)dfeat, (unsigned short*)dy2, (unsigned short*)du, (unsigned short*)dy1, part, n)
  switch (channels) { case 32: SS_BT_BWD(32); break; case 64: SS_BT_BWD(64); break; case 128: SS_BT_BWD(128); break; default: SS_BT_BWD(256); break; }
#undef SS_BT_BWD
  return SS_OK;
}
