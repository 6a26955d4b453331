// Serialized-window attention with PTv3's relative position encoding (enable_rpe=True, ptv3:29-48, 104-112, 199-201):
//   S[h,i,j] = (q_i * scale) . k_j + T[clamp(g_i.x - g_j.x) + pos_bnd, h] + T[rpe_num + clamp(g_i.y - g_j.y) + pos_bnd, h]
//                                  + T[2 rpe_num + clamp(g_i.z - g_j.z) + pos_bnd, h],   out = softmax(S) v
// g = grid_coord[gidx[slot]] (a borrowed slot carries the coordinates of the point it borrows from), clamp to
// [-pos_bnd, pos_bnd], rpe_num = 2 pos_bnd + 1, T = table (3 rpe_num, H) f32.  The bias is not scaled by `scale`.
//
// The (windows, H, K, K) bias never exists in memory: every workgroup (window, head[, query chunk]) stages the window's
// coordinates (three int32 planes, so that the four consecutive keys of an accumulator register quad are one ds_read_b128)
// and its head's table column in LDS, and adds the three lookups to each score while it sits in the accumulator registers,
// before the online-softmax maximum.  Indexing, padding and the dqkv / borrowed-slot contract are those of attention_simt.hip
// and attention_mfma.hip (packed (n, 3C) qkv layout).  This file holds the MFMA kernels: v_mfma_f32_16x16x32_bf16, head dims
// 16/32/48/64, windows up to SS_ATTN_MFMA_MAX_WINDOW; scores and bias in exp2 units (q.k * scale*log2(e) + T*log2(e)), same
// S^T orientation, fragment helpers and LDS images as attention_mfma.hip (attention_frag.h); they always take its generic
// score path (no shift folded into the contraction padding).  The fp32-math parity path for any window length is the RPE
// instantiation of the kernels in attention_simt.hip; the C-ABI entry points are in attention.hip.
// Backward: dS = P o (dP - delta), dbias = dS in fp32 (before any rounding to bf16).  dT without global atomics: the dQ
// kernel accumulates its workgroup's 3 rpe_num bins in LDS (LDS float adds), writes them with plain stores to its slab of the
// caller's workspace, and k_rpe_dtable_reduce sums the slabs in fixed order into dtable (overwritten; a bin that no pair
// indexes is exactly 0).
#include "attention_frag.h"

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

// dtable[b][h] = sum over slabs, in fixed order: thread (bx, sy) adds slabs sy, sy + 4, ... and the four partial sums of a
// bin are added in the order 0..3
__global__ void __launch_bounds__(256)
k_rpe_dtable_reduce(const float* __restrict__ slab, int nslab, int H, int nb, float* __restrict__ dtable) {
  __shared__ float part[4][64];
  const int bx = threadIdx.x & 63, sy = threadIdx.x >> 6;
  const int gid = blockIdx.x * 64 + bx;      // (head, bin) pair, bin fastest: consecutive lanes read consecutive floats
  const bool ok = gid < H * nb;
  float s = 0.f;
  if (ok) for (int i = sy; i < nslab; i += 4) s += slab[(int64_t)i * H * nb + gid];
  part[sy][bx] = s;
  __syncthreads();
  if (ok && sy == 0) {
    const int h = gid / nb, b = gid - h * nb;
    dtable[(int64_t)b * H + h] = ((part[0][bx] + part[1][bx]) + part[2][bx]) + part[3][bx];
  }
}

#define RPE_BIN_WORDS 6208                   // 32 copies of up to 194 bins (pos_bnd <= 31: windows up to 1024), else 16 of up to 387

// the window in LDS: gather rows as 16-byte offsets (row * 3C/8), the three coordinate planes (zero past the window end up to
// the next multiple of 64, so that a tile's tail reads are defined: FA_IDX_CAP is a multiple of 64), the head's table column
// in exp2 units
struct RpeWindow {
  int32_t gidx_s[FA_IDX_CAP];
  __attribute__((aligned(16))) int32_t cx[FA_IDX_CAP];
  __attribute__((aligned(16))) int32_t cy[FA_IDX_CAP];
  __attribute__((aligned(16))) int32_t cz[FA_IDX_CAP];
  float tab[RPE_MAX_BINS];
};
__device__ __forceinline__ void rpe_window_fill(RpeWindow& W, const int32_t* __restrict__ gidx, const int32_t* __restrict__ gc,
                                                const float* __restrict__ table, int p0, int L, int C, int H, int h, int rn,
                                                int tid, int nthreads) {
  const int Lr = (L + 63) & ~63;
  for (int i = tid; i < Lr; i += nthreads) {
    int x = 0, y = 0, z = 0;
    if (i < L) {
      const int32_t row = gidx[p0 + i];
      W.gidx_s[i] = (int32_t)((uint32_t)row * (uint32_t)(3 * C >> 3));
      x = gc[(int64_t)row * 3]; y = gc[(int64_t)row * 3 + 1]; z = gc[(int64_t)row * 3 + 2];
    }
    W.cx[i] = x; W.cy[i] = y; W.cz[i] = z;
  }
  for (int i = tid; i < 3 * rn; i += nthreads) W.tab[i] = table[(int64_t)i * H + h] * RPE_LOG2E;
}

// ---- forward: S^T = K Q^T (key rows 16kt + 4g + r, query lq on the lane), bias added in the accumulators, online softmax
// in exp2 units, O^T += V^T P^T with P^T taken from the S^T accumulators
template <int D>
__global__ void __launch_bounds__(FA_THREADS)
k_rpe_fwd_mfma(const unsigned short* __restrict__ qkv, const int32_t* __restrict__ gidx, const int32_t* __restrict__ sidx,
               const int32_t* __restrict__ win_start, const int32_t* __restrict__ gc, const float* __restrict__ table,
               int pos_bnd, unsigned short* __restrict__ out, float* __restrict__ lse, int C, int H, float scale, int qchunks) {
  using A = ACfg<D>;
  constexpr int NLD = (2 * 64 * A::CH + FA_THREADS - 1) / FA_THREADS;
  constexpr int KIMG = 64 * A::ROWB, VIMG = 64 * A::TRB;
  __shared__ __attribute__((aligned(16))) char smem[2 * (KIMG + VIMG)];
  __shared__ RpeWindow W;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, g = lane >> 4;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qc = lid % qchunks; const int t_ = lid / qchunks; const int h = t_ % H; const int w = t_ / H;
  const int p0 = win_start[w], L = win_start[w + 1] - p0;
  const int q0 = qc * FA_BQ;
  if (q0 >= L) return;
  const int rn = 2 * pos_bnd + 1, pb2 = 2 * pos_bnd;
  rpe_window_fill(W, gidx, gc, table, p0, L, C, H, h, rn, tid, FA_THREADS);
  const int64_t C3 = 3 * (int64_t)C;
  const float c2 = scale * RPE_LOG2E;
  auto Kbuf = [&](int b_) { return smem + b_ * (KIMG + VIMG); };
  auto Vbuf = [&](int b_) { return smem + b_ * (KIMG + VIMG) + KIMG; };
  if (A::CHP > A::CH) {     // zero the contraction padding of the K images once
    for (int e = tid; e < 2 * 64 * (A::CHP - A::CH); e += FA_THREADS) {
      int b = e / (64 * (A::CHP - A::CH)); int r = (e / (A::CHP - A::CH)) % 64; int ch = A::CH + e % (A::CHP - A::CH);
      *reinterpret_cast<uint4*>(Kbuf(b) + row_img_off<D>(r, ch)) = make_uint4(0, 0, 0, 0);
    }
  }
  __syncthreads();
  bf8_t qf[FA_NT][A::NKS];
  int qslot[FA_NT], qx[FA_NT], qy[FA_NT], qz[FA_NT];      // query coordinate + pos_bnd
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt) {
    int slot = q0 + wave * FA_WQ + qt * 16 + lq;
    qslot[qt] = slot;
    const bool ok = slot < L;
    int64_t row = ok ? gidx[p0 + slot] : -1;
    qx[qt] = (ok ? W.cx[slot] : 0) + pos_bnd; qy[qt] = (ok ? W.cy[slot] : 0) + pos_bnd; qz[qt] = (ok ? W.cz[slot] : 0) + pos_bnd;
#pragma unroll
    for (int ks = 0; ks < A::NKS; ++ks) {
      int d0 = 32 * ks + 8 * g;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row >= 0 && d0 < D) v = ld16(qkv + row * C3 + h * D + d0);
      qf[qt][ks] = as_bf8(v);
    }
  }
  // row sums ride the matrix pipe (row 0 of an all-ones A tile), on the same bf16-rounded P the PV product uses
  const bf8_t ones = as_bf8(lq == 0 ? make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u) : make_uint4(0, 0, 0, 0));
  float m[FA_NT];                       // running maximum, exp2 units
  f32x4_t o[A::NDT][FA_NT], lsum[FA_NT];
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt) {
    m[qt] = -1e30f; lsum[qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < A::NDT; ++dt) o[dt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  uint4 st[NLD];
  auto stage_write = [&](int b) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      int c = i * FA_THREADS + tid;
      int second = c >= 64 * A::CH;
      int cc = second ? c - 64 * A::CH : c;
      int r = cc / A::CH, ch = cc - r * A::CH;
      if (c >= 2 * 64 * A::CH) continue;
      if (second) *reinterpret_cast<uint4*>(Vbuf(b) + r * A::TRB + ch * 16) = st[i];
      else *reinterpret_cast<uint4*>(Kbuf(b) + row_img_off<D>(r, ch)) = st[i];
    }
  };
  const float* tabx = W.tab; const float* taby = W.tab + rn; const float* tabz = W.tab + 2 * rn;
  const int ntiles = (L + FA_BK - 1) / FA_BK;
  tile_load<D, NLD>(st, qkv, W.gidx_s, 0, L, C + h * D, 2 * C + h * D, tid);
  stage_write(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int b = t & 1, kv0 = t * FA_BK;
    if (t + 1 < ntiles) tile_load<D, NLD>(st, qkv, W.gidx_s, kv0 + FA_BK, L, C + h * D, 2 * C + h * D, tid);
    f32x4_t s[4][FA_NT];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int qt = 0; qt < FA_NT; ++qt) s[kt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < A::NKS; ++ks) {
        bf8_t a = lds_b128(Kbuf(b), row_img_off<D>(16 * kt + lq, 4 * ks + g));
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) s[kt][qt] = MFMA16(a, qf[qt][ks], s[kt][qt]);
      }
    }
    // ---- scores in exp2 units + bias: the 4 keys of a register quad are consecutive slots (one 16-byte read per plane)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int kb = kv0 + 16 * kt + 4 * g;
      const i32x4_t kx = *reinterpret_cast<const i32x4_t*>(&W.cx[kb]);
      const i32x4_t ky = *reinterpret_cast<const i32x4_t*>(&W.cy[kb]);
      const i32x4_t kz = *reinterpret_cast<const i32x4_t*>(&W.cz[kb]);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) {
          const float bias = tabx[rpe_bin(qx[qt] - kx[r], pb2)] + taby[rpe_bin(qy[qt] - ky[r], pb2)] + tabz[rpe_bin(qz[qt] - kz[r], pb2)];
          s[kt][qt][r] = __builtin_fmaf(s[kt][qt][r], c2, bias);
        }
    }
    if (kv0 + FA_BK > L) {   // mask the keys past the window end (last tile only; wave-uniform)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kv0 + 16 * kt + 4 * g + r >= L) {
#pragma unroll
            for (int qt = 0; qt < FA_NT; ++qt) s[kt][qt][r] = -INFINITY;
          }
    }
#pragma unroll
    for (int qt = 0; qt < FA_NT; ++qt) {
      float mx = s[0][qt][0];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][qt][r]);
      mx = xmax4(mx);
      float mn = fmaxf(m[qt], mx);
      if (__any(mn > m[qt])) {      // exact skip: when no lane's running maximum moved, alpha == 1 for the whole wave
        float alpha = __builtin_amdgcn_exp2f(m[qt] - mn);
        lsum[qt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < A::NDT; ++dt) o[dt][qt] *= alpha;
      }
      m[qt] = mn;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][qt][r] = __builtin_amdgcn_exp2f(s[kt][qt][r] - mn);
    }
    // ---- O^T += V^T P^T ; k index (g, j) of step kk <-> key 32kk + 16(j>>2) + 4g + (j&3)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf8_t pf[FA_NT];
#pragma unroll
      for (int qt = 0; qt < FA_NT; ++qt) {
        pf[qt] = pack8(s[2 * kk][qt], s[2 * kk + 1][qt]);
        lsum[qt] = MFMA16(ones, pf[qt], lsum[qt]);
      }
      const char* vbase = Vbuf(b) + (32 * kk + 4 * g + (lq >> 2)) * A::TRB + (lq & 3) * 8;
#pragma unroll
      for (int dt = 0; dt < A::NDT; ++dt) {
        bf8_t vf = cat_tr(lds_tr(vbase + dt * 32), lds_tr(vbase + 16 * A::TRB + dt * 32));
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) o[dt][qt] = MFMA16(vf, pf[qt], o[dt][qt]);
      }
    }
    if (t + 1 < ntiles) stage_write(b ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt) {
    float lt = __shfl(lsum[qt][0], lq, 64);   // row 0 of the ones tile lives in lane group 0
    int slot = qslot[qt];
    if (slot < L) {
      if (g == 0) lse[(int64_t)(p0 + slot) * H + h] = m[qt] * 0.69314718055994530942f + __logf(lt);
      int32_t srow = sidx[p0 + slot];
      if (srow >= 0) {
        float inv = 1.f / lt;
        unsigned short* op = out + (int64_t)srow * C + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < A::NDT; ++dt) {
          uint2 v;
          v.x = pack_bf16x2(o[dt][qt][0] * inv, o[dt][qt][1] * inv);
          v.y = pack_bf16x2(o[dt][qt][2] * inv, o[dt][qt][3] * inv);
          *reinterpret_cast<uint2*>(op + 16 * dt) = v;
        }
      }
    }
  }
}

// ---- backward, dQ + dT: query-stationary.  S^T and dP^T = V dO^T (key rows, query on the lane), dS^T = P^T o (dP^T - delta),
// dQ^T += K^T dS^T; every fp32 dS is also added to its three bins of the workgroup's LDS histogram, which goes to the
// workgroup's slab ((window, query chunk), head, 3 rpe_num) with plain stores.  delta is an OUTPUT (as in attention_mfma.hip).
template <int D>
__global__ void __launch_bounds__(FA_THREADS)
k_rpe_bwd_dq_mfma(const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ dout,
                  const unsigned short* __restrict__ outp, const float* __restrict__ lse, float* __restrict__ delta,
                  const int32_t* __restrict__ gidx, const int32_t* __restrict__ sidx, const int32_t* __restrict__ win_start,
                  const int32_t* __restrict__ gc, const float* __restrict__ table, int pos_bnd,
                  unsigned short* __restrict__ dqkv, float* __restrict__ slab, int C, int H, float scale, int qchunks) {
  using A = ACfg<D>;
  constexpr int NLD = (2 * 64 * A::CH + FA_THREADS - 1) / FA_THREADS;
  constexpr int RIMG = 64 * A::ROWB, TIMG = 64 * A::TRB;
  constexpr int BUF = 2 * RIMG + TIMG;      // K row image, V row image, K tr image
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ RpeWindow W;
  // dT histogram, one copy per lane (mod `copies`): element (bin, copy) at bin * copies + copy.  The lanes of a wave share their
  // key (16-lane group) or their query (lanes l, l + 16, ...), so with a single copy most of them add to the SAME word; the
  // copies take 9 % (d 48) to 13 % (d 16) off forward + backward.  The LDS float adds themselves remain the cost of this kernel
  // (profiles/attention_rpe.md).
  __shared__ float bins[RPE_BIN_WORDS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, g = lane >> 4;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qc = lid % qchunks; const int t_ = lid / qchunks; const int h = t_ % H; const int w = t_ / H;
  const int p0 = win_start[w], L = win_start[w + 1] - p0;
  const int q0 = qc * FA_BQ;
  const int rn = 2 * pos_bnd + 1, pb2 = 2 * pos_bnd, nb = 3 * rn;
  float* my = slab + ((int64_t)(w * qchunks + qc) * H + h) * nb;
  if (q0 >= L) {      // no queries here: the slab still has to be written
    for (int i = tid; i < nb; i += FA_THREADS) my[i] = 0.f;
    return;
  }
  rpe_window_fill(W, gidx, gc, table, p0, L, C, H, h, rn, tid, FA_THREADS);
  const int copies = nb * 32 <= RPE_BIN_WORDS ? 32 : 16, cp = lane & (copies - 1);
  for (int i = tid; i < nb * copies; i += FA_THREADS) bins[i] = 0.f;
  const int64_t C3 = 3 * (int64_t)C;
  const float c2 = scale * RPE_LOG2E;
  if (A::CHP > A::CH) {      // zero the contraction padding of the K and V row images
    for (int e = tid; e < 4 * 64 * (A::CHP - A::CH); e += FA_THREADS) {
      int img = e / (64 * (A::CHP - A::CH)); int r = (e / (A::CHP - A::CH)) % 64; int ch = A::CH + e % (A::CHP - A::CH);
      char* base = smem + (img >> 1) * BUF + (img & 1) * RIMG;
      *reinterpret_cast<uint4*>(base + row_img_off<D>(r, ch)) = make_uint4(0, 0, 0, 0);
    }
  }
  __syncthreads();
  bf8_t qf[FA_NT][A::NKS], gf[FA_NT][A::NKS];
  float lse2[FA_NT], dl[FA_NT];
  int32_t srow[FA_NT];
  int qx[FA_NT], qy[FA_NT], qz[FA_NT];
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt) {
    const int slot = q0 + wave * FA_WQ + qt * 16 + lq;
    const bool ok = slot < L;
    const int64_t qrow = ok ? gidx[p0 + slot] : -1;
    srow[qt] = ok ? sidx[p0 + slot] : -1;
    lse2[qt] = ok ? lse[(int64_t)(p0 + slot) * H + h] * RPE_LOG2E : 0.f;
    qx[qt] = (ok ? W.cx[slot] : 0) + pos_bnd; qy[qt] = (ok ? W.cy[slot] : 0) + pos_bnd; qz[qt] = (ok ? W.cz[slot] : 0) + pos_bnd;
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < A::NKS; ++ks) {
      const int d0 = 32 * ks + 8 * g;
      uint4 v = make_uint4(0, 0, 0, 0), u = v, ov = v;
      if (qrow >= 0 && d0 < D) v = ld16(qkv + qrow * C3 + h * D + d0);
      if (srow[qt] >= 0 && d0 < D) {
        u = ld16(dout + (int64_t)srow[qt] * C + h * D + d0); ov = ld16(outp + (int64_t)srow[qt] * C + h * D + d0);
      }
      qf[qt][ks] = as_bf8(v); gf[qt][ks] = as_bf8(u);
      const unsigned int* uu = reinterpret_cast<const unsigned int*>(&u);
      const unsigned int* uo = reinterpret_cast<const unsigned int*>(&ov);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dsum += __uint_as_float(uu[j] << 16) * __uint_as_float(uo[j] << 16);
        dsum += __uint_as_float(uu[j] & 0xffff0000u) * __uint_as_float(uo[j] & 0xffff0000u);
      }
    }
    dl[qt] = xsum4(dsum);      // delta = rowsum(O o dO), published for the dK/dV kernel
    if (ok && g == 0) delta[(int64_t)(p0 + slot) * H + h] = dl[qt];
  }
  f32x4_t dq[A::NDT][FA_NT];
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt)
#pragma unroll
    for (int dt = 0; dt < A::NDT; ++dt) dq[dt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  uint4 st[NLD];
  auto stage_write = [&](int b) {
    char* base = smem + b * BUF;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      int c = i * FA_THREADS + tid;
      int second = c >= 64 * A::CH;
      int cc = second ? c - 64 * A::CH : c;
      int r = cc / A::CH, ch = cc - r * A::CH;
      if (c >= 2 * 64 * A::CH) continue;
      if (second) *reinterpret_cast<uint4*>(base + RIMG + row_img_off<D>(r, ch)) = st[i];
      else {
        *reinterpret_cast<uint4*>(base + row_img_off<D>(r, ch)) = st[i];
        *reinterpret_cast<uint4*>(base + 2 * RIMG + r * A::TRB + ch * 16) = st[i];
      }
    }
  };
  const float* tabx = W.tab; const float* taby = W.tab + rn; const float* tabz = W.tab + 2 * rn;
  // a lane's keys follow the curve, so consecutive keys often share a coordinate (on a floor: z always, x or y every other key):
  // the dS of a run of equal bins is summed in registers and reaches LDS as one add (per query tile and axis: the open run)
  int run_bin[FA_NT][3];
  float run_sum[FA_NT][3];
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt)
#pragma unroll
    for (int a = 0; a < 3; ++a) { run_bin[qt][a] = -1; run_sum[qt][a] = 0.f; }
  auto bin_add = [&](int qt, int a, int bin, float ds) {
    if (bin != run_bin[qt][a]) {
      if (run_bin[qt][a] >= 0) atomicAdd(&bins[run_bin[qt][a] * copies + cp], run_sum[qt][a]);
      run_bin[qt][a] = bin; run_sum[qt][a] = 0.f;
    }
    run_sum[qt][a] += ds;
  };
  const int ntiles = (L + FA_BK - 1) / FA_BK;
  tile_load<D, NLD>(st, qkv, W.gidx_s, 0, L, C + h * D, 2 * C + h * D, tid);
  stage_write(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int b = t & 1, kv0 = t * FA_BK;
    const char* Kr = smem + b * BUF; const char* Vr = Kr + RIMG; const char* Kt = Kr + 2 * RIMG;
    if (t + 1 < ntiles) tile_load<D, NLD>(st, qkv, W.gidx_s, kv0 + FA_BK, L, C + h * D, 2 * C + h * D, tid);
    f32x4_t s[4][FA_NT], dp[4][FA_NT];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int qt = 0; qt < FA_NT; ++qt) { s[kt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dp[kt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int ks = 0; ks < A::NKS; ++ks) {
        int off = row_img_off<D>(16 * kt + lq, 4 * ks + g);
        bf8_t ka = lds_b128(Kr, off), va = lds_b128(Vr, off);
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) {
          s[kt][qt] = MFMA16(ka, qf[qt][ks], s[kt][qt]);
          dp[kt][qt] = MFMA16(va, gf[qt][ks], dp[kt][qt]);
        }
      }
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int kb = kv0 + 16 * kt + 4 * g;
      const i32x4_t kx = *reinterpret_cast<const i32x4_t*>(&W.cx[kb]);
      const i32x4_t ky = *reinterpret_cast<const i32x4_t*>(&W.cy[kb]);
      const i32x4_t kz = *reinterpret_cast<const i32x4_t*>(&W.cz[kb]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool kok = kb + r < L;
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) {
          const int ix = rpe_bin(qx[qt] - kx[r], pb2), iy = rpe_bin(qy[qt] - ky[r], pb2), iz = rpe_bin(qz[qt] - kz[r], pb2);
          const float bias = tabx[ix] + taby[iy] + tabz[iz];
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][qt][r], c2, bias - lse2[qt]));
          float ds = p * (dp[kt][qt][r] - dl[qt]);
          if (kok && srow[qt] >= 0) {      // dbias = dS in fp32; a borrowed query's dS is 0 (its dO is)
            bin_add(qt, 0, ix, ds); bin_add(qt, 1, rn + iy, ds); bin_add(qt, 2, 2 * rn + iz, ds);
          } else {
            ds = 0.f;
          }
          s[kt][qt][r] = ds;
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf8_t df[FA_NT];
#pragma unroll
      for (int qt = 0; qt < FA_NT; ++qt) df[qt] = pack8(s[2 * kk][qt], s[2 * kk + 1][qt]);
      const char* kbase = Kt + (32 * kk + 4 * g + (lq >> 2)) * A::TRB + (lq & 3) * 8;
#pragma unroll
      for (int dt = 0; dt < A::NDT; ++dt) {
        bf8_t kf = cat_tr(lds_tr(kbase + dt * 32), lds_tr(kbase + 16 * A::TRB + dt * 32));
#pragma unroll
        for (int qt = 0; qt < FA_NT; ++qt) dq[dt][qt] = MFMA16(kf, df[qt], dq[dt][qt]);
      }
    }
    if (t + 1 < ntiles) stage_write(b ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt) {
    if (srow[qt] >= 0) {
      unsigned short* op = dqkv + (int64_t)srow[qt] * C3 + h * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < A::NDT; ++dt) {
        uint2 v;
        v.x = pack_bf16x2(dq[dt][qt][0] * scale, dq[dt][qt][1] * scale);
        v.y = pack_bf16x2(dq[dt][qt][2] * scale, dq[dt][qt][3] * scale);
        *reinterpret_cast<uint2*>(op + 16 * dt) = v;
      }
    }
  }
#pragma unroll
  for (int qt = 0; qt < FA_NT; ++qt)
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (run_bin[qt][a] >= 0) atomicAdd(&bins[run_bin[qt][a] * copies + cp], run_sum[qt][a]);
  __syncthreads();
  for (int i = tid; i < nb; i += FA_THREADS) {      // every LDS add is retired; the copies are added in fixed order
    float acc = 0.f;
    for (int c = 0; c < copies; ++c) acc += bins[i * copies + c];
    my[i] = acc;
  }
}

// ---- backward, dK/dV: key-stationary (keys on the lane, 64-query tiles of Q and dO streamed through LDS as a row image
// for S / dP and a tr image for dV^T += dO^T P, dK^T += Q^T dS); the bias is recomputed from the coordinate planes
#define FA_BQ2 64
#define DKV_THREADS FA_THREADS
#define DKV_BKEYS FA_BQ
template <int D>
__global__ void __launch_bounds__(DKV_THREADS)
k_rpe_bwd_dkv_mfma(const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ dout,
                   const float* __restrict__ lse, const float* __restrict__ delta, const int32_t* __restrict__ gidx,
                   const int32_t* __restrict__ sidx, const int32_t* __restrict__ win_start, const int32_t* __restrict__ gc,
                   const float* __restrict__ table, int pos_bnd, unsigned short* __restrict__ dqkv,
                   unsigned short* __restrict__ extra, int C, int H, float scale, int kchunks) {
  using A = ACfg<D>;
  constexpr int TOT = 2 * FA_BQ2 * A::CH;                     // 16-B chunks per (Q, dO) tile
  constexpr int NLD = (TOT + DKV_THREADS - 1) / DKV_THREADS;
  constexpr int RIMG = FA_BQ2 * A::ROWB, TIMG = FA_BQ2 * A::TRB;
  constexpr int BUF = 2 * RIMG + 2 * TIMG + 2 * FA_BQ2 * 4;   // Q row, dO row, Q tr, dO tr, lse2[64], delta[64]
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ RpeWindow W;
  __shared__ int32_t sidx_s[FA_IDX_CAP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, g = lane >> 4;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int kc = lid % kchunks; const int t_ = lid / kchunks; const int h = t_ % H; const int w = t_ / H;
  const int p0 = win_start[w], L = win_start[w + 1] - p0;
  const int k0 = kc * DKV_BKEYS;
  if (k0 >= L) return;
  const int rn = 2 * pos_bnd + 1, pb2 = 2 * pos_bnd;
  rpe_window_fill(W, gidx, gc, table, p0, L, C, H, h, rn, tid, DKV_THREADS);
  for (int i = tid; i < L; i += DKV_THREADS) { const int32_t sr = sidx[p0 + i]; sidx_s[i] = sr >= 0 ? sr * (C >> 3) : -1; }
  const int64_t C3 = 3 * (int64_t)C;
  const float c2 = scale * RPE_LOG2E;
  if (A::CHP > A::CH) {
    for (int e = tid; e < 4 * FA_BQ2 * (A::CHP - A::CH); e += DKV_THREADS) {
      int img = e / (FA_BQ2 * (A::CHP - A::CH)); int r = (e / (A::CHP - A::CH)) % FA_BQ2; int ch = A::CH + e % (A::CHP - A::CH);
      char* base = smem + (img >> 1) * BUF + (img & 1) * RIMG;
      *reinterpret_cast<uint4*>(base + row_img_off<D>(r, ch)) = make_uint4(0, 0, 0, 0);
    }
  }
  __syncthreads();
  // K / V fragments as B operands: lane holds K[key = lq][d = 32ks + 8g ..]
  bf8_t kf[FA_NT][A::NKS], vf[FA_NT][A::NKS];
  int kslot[FA_NT], kx[FA_NT], ky[FA_NT], kz[FA_NT];      // key coordinate - pos_bnd
#pragma unroll
  for (int kt = 0; kt < FA_NT; ++kt) {
    kslot[kt] = k0 + wave * FA_WQ + kt * 16 + lq;
    const bool ok = kslot[kt] < L;
    const int64_t krow = ok ? gidx[p0 + kslot[kt]] : -1;
    kx[kt] = (ok ? W.cx[kslot[kt]] : 0) - pos_bnd; ky[kt] = (ok ? W.cy[kslot[kt]] : 0) - pos_bnd; kz[kt] = (ok ? W.cz[kslot[kt]] : 0) - pos_bnd;
#pragma unroll
    for (int ks = 0; ks < A::NKS; ++ks) {
      const int d0 = 32 * ks + 8 * g;
      uint4 a = make_uint4(0, 0, 0, 0), b = a;
      if (krow >= 0 && d0 < D) { a = ld16(qkv + krow * C3 + C + h * D + d0); b = ld16(qkv + krow * C3 + 2 * C + h * D + d0); }
      kf[kt][ks] = as_bf8(a); vf[kt][ks] = as_bf8(b);
    }
  }
  f32x4_t dk[A::NDT][FA_NT], dv[A::NDT][FA_NT];
#pragma unroll
  for (int kt = 0; kt < FA_NT; ++kt)
#pragma unroll
    for (int dt = 0; dt < A::NDT; ++dt) { dk[dt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[dt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
  uint4 stv[NLD];
  float st_l = 0.f, st_d = 0.f;
  auto stage_load = [&](int qb) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      int c = i * DKV_THREADS + tid;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c < TOT) {
        int second = c >= FA_BQ2 * A::CH;
        int cc = second ? c - FA_BQ2 * A::CH : c;
        int r = cc / A::CH, ch = cc - r * A::CH;
        if (qb + r < L) {
          if (!second) v = ld16(reinterpret_cast<const char*>(qkv + h * D + ch * 8) + ((uint64_t)(uint32_t)W.gidx_s[qb + r] << 4));
          else { int32_t sr = sidx_s[qb + r]; if (sr >= 0) v = ld16(reinterpret_cast<const char*>(dout + h * D + ch * 8) + ((uint64_t)(uint32_t)sr << 4)); }
        }
      }
      stv[i] = v;
    }
    if (tid < FA_BQ2) {
      bool ok = qb + tid < L;
      st_l = ok ? lse[(int64_t)(p0 + qb + tid) * H + h] * RPE_LOG2E : 1e30f;   // p = 0 for rows past the window
      st_d = ok ? delta[(int64_t)(p0 + qb + tid) * H + h] : 0.f;
    }
  };
  auto stage_write = [&](int b) {
    char* base = smem + b * BUF;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      int c = i * DKV_THREADS + tid;
      if (c < TOT) {
        int second = c >= FA_BQ2 * A::CH;
        int cc = second ? c - FA_BQ2 * A::CH : c;
        int r = cc / A::CH, ch = cc - r * A::CH;
        *reinterpret_cast<uint4*>(base + second * RIMG + row_img_off<D>(r, ch)) = stv[i];
        *reinterpret_cast<uint4*>(base + 2 * RIMG + second * TIMG + r * A::TRB + ch * 16) = stv[i];
      }
    }
    if (tid < FA_BQ2) {
      float* f = reinterpret_cast<float*>(base + 2 * RIMG + 2 * TIMG);
      f[tid] = st_l; f[FA_BQ2 + tid] = st_d;
    }
  };
  const float* tabx = W.tab; const float* taby = W.tab + rn; const float* tabz = W.tab + 2 * rn;
  const int ntiles = (L + FA_BQ2 - 1) / FA_BQ2;
  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int b = t & 1;
    if (t + 1 < ntiles) stage_load((t + 1) * FA_BQ2);
    const char* Qr = smem + b * BUF; const char* Gr = Qr + RIMG; const char* Qt = Qr + 2 * RIMG; const char* Gt = Qt + TIMG;
    const float* fl = reinterpret_cast<const float*>(Qr + 2 * RIMG + 2 * TIMG);
#pragma unroll
    for (int hq = 0; hq < FA_BQ2 / 32; ++hq) {
      const char* Qr_h = Qr + hq * 32 * A::ROWB; const char* Gr_h = Gr + hq * 32 * A::ROWB;
      // S[q][key], dP[q][key]: rows = queries 32hq + 16qt + 4g + r, col = key lq (tile kt)
      f32x4_t s[2][FA_NT], dp[2][FA_NT];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int kt = 0; kt < FA_NT; ++kt) { s[qt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dp[qt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int ks = 0; ks < A::NKS; ++ks) {
          int off = row_img_off<D>(16 * qt + lq, 4 * ks + g);
          bf8_t qa = lds_b128(Qr_h, off), ga = lds_b128(Gr_h, off);
#pragma unroll
          for (int kt = 0; kt < FA_NT; ++kt) {
            s[qt][kt] = MFMA16(qa, kf[kt][ks], s[qt][kt]);
            dp[qt][kt] = MFMA16(ga, vf[kt][ks], dp[qt][kt]);
          }
        }
      }
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int ql = 32 * hq + 16 * qt + 4 * g;             // first of the lane's 4 consecutive query slots of the tile
        const i32x4_t cqx = *reinterpret_cast<const i32x4_t*>(&W.cx[t * FA_BQ2 + ql]);
        const i32x4_t cqy = *reinterpret_cast<const i32x4_t*>(&W.cy[t * FA_BQ2 + ql]);
        const i32x4_t cqz = *reinterpret_cast<const i32x4_t*>(&W.cz[t * FA_BQ2 + ql]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float l2 = fl[ql + r], dd = fl[FA_BQ2 + ql + r];
#pragma unroll
          for (int kt = 0; kt < FA_NT; ++kt) {
            const float bias = tabx[rpe_bin(cqx[r] - kx[kt], pb2)] + taby[rpe_bin(cqy[r] - ky[kt], pb2)] + tabz[rpe_bin(cqz[r] - kz[kt], pb2)];
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[qt][kt][r], c2, bias - l2));
            s[qt][kt][r] = p;
            dp[qt][kt][r] = p * (dp[qt][kt][r] - dd);
          }
        }
      }
      // dV^T += dO^T P ; dK^T += Q^T dS ; k index (g, j) <-> query 16(j>>2) + 4g + (j&3)
      const char* gbase = Gt + (32 * hq + 4 * g + (lq >> 2)) * A::TRB + (lq & 3) * 8;
      const char* qbase = Qt + (32 * hq + 4 * g + (lq >> 2)) * A::TRB + (lq & 3) * 8;
      bf8_t pf[FA_NT], df[FA_NT];
#pragma unroll
      for (int kt = 0; kt < FA_NT; ++kt) { pf[kt] = pack8(s[0][kt], s[1][kt]); df[kt] = pack8(dp[0][kt], dp[1][kt]); }
#pragma unroll
      for (int dt = 0; dt < A::NDT; ++dt) {
        bf8_t ga = cat_tr(lds_tr(gbase + dt * 32), lds_tr(gbase + 16 * A::TRB + dt * 32));
        bf8_t qa = cat_tr(lds_tr(qbase + dt * 32), lds_tr(qbase + 16 * A::TRB + dt * 32));
#pragma unroll
        for (int kt = 0; kt < FA_NT; ++kt) {
          dv[dt][kt] = MFMA16(ga, pf[kt], dv[dt][kt]);
          dk[dt][kt] = MFMA16(qa, df[kt], dk[dt][kt]);
        }
      }
    }
    if (t + 1 < ntiles) stage_write(b ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int kt = 0; kt < FA_NT; ++kt) {
    int slot = kslot[kt];
    if (slot < L) {
      int32_t sr = sidx[p0 + slot];
      unsigned short* kp; unsigned short* vp;
      if (sr >= 0) { kp = dqkv + (int64_t)sr * C3 + C + h * D + 4 * g; vp = kp + C; }
      else { kp = extra + (int64_t)(-1 - sr) * 2 * C + h * D + 4 * g; vp = kp + C; }
#pragma unroll
      for (int dt = 0; dt < A::NDT; ++dt) {
        uint2 a, b2;
        a.x = pack_bf16x2(dk[dt][kt][0] * scale, dk[dt][kt][1] * scale);
        a.y = pack_bf16x2(dk[dt][kt][2] * scale, dk[dt][kt][3] * scale);
        b2.x = pack_bf16x2(dv[dt][kt][0], dv[dt][kt][1]);
        b2.y = pack_bf16x2(dv[dt][kt][2], dv[dt][kt][3]);
        *reinterpret_cast<uint2*>(kp + 16 * dt) = a;
        *reinterpret_cast<uint2*>(vp + 16 * dt) = b2;
      }
    }
  }
}

// =====================================================================================
// launchers (argument checks and the SIMT / MFMA choice: attention.hip)
// =====================================================================================
static_assert(FA_BQ == SS_ATTN_RPE_BQ, "the workspace holds one dT slab per FA_BQ-query chunk");

int ss_attn_rpe_fwd_mfma(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int W,
                         int max_window, void* out, float* lse, int C, int H, float scale, const SsAttnRpe& rpe, hipStream_t st) {
  const int qchunks = ss_attn_rpe_chunks(max_window);
  dim3 g((unsigned)(W * H * qchunks)), b(FA_THREADS);
  const unsigned short* q = (const unsigned short*)qkv; unsigned short* o = (unsigned short*)out;
#define SS_RM_CASE(DD) \
  case DD: SS_LAUNCH((k_rpe_fwd_mfma<DD>), g, b, 0, st, q, gidx, sidx, win_start, rpe.gc, rpe.table, rpe.pos_bnd, o, lse, C, H, scale, qchunks); break;
  switch (C / H) {
    SS_RM_CASE(16) SS_RM_CASE(32) SS_RM_CASE(48) SS_RM_CASE(64)
    default: return SS_ERR_ARG;
  }
#undef SS_RM_CASE
  return SS_OK;
}

int ss_attn_rpe_bwd_mfma(const void* qkv, const void* dout, const void* out, const float* lse, float* delta, const int32_t* gidx,
                         const int32_t* sidx, const int32_t* win_start, int W, int max_window, void* dqkv, void* extra,
                         int C, int H, float scale, const SsAttnRpe& rpe, hipStream_t st) {
  const int chunks = ss_attn_rpe_chunks(max_window);
  dim3 g((unsigned)(W * H * chunks)), b(FA_THREADS);
  const unsigned short* q = (const unsigned short*)qkv; const unsigned short* go = (const unsigned short*)dout;
  unsigned short* dq = (unsigned short*)dqkv; unsigned short* ex = (unsigned short*)extra;
#define SS_RMB_CASE(DD)                                                                                                   \
  case DD:                                                                                                                \
    SS_LAUNCH((k_rpe_bwd_dq_mfma<DD>), g, b, 0, st, q, go, (const unsigned short*)out, lse, delta, gidx, sidx, win_start, \
              rpe.gc, rpe.table, rpe.pos_bnd, dq, rpe.slab, C, H, scale, chunks);                                         \
    SS_LAUNCH((k_rpe_bwd_dkv_mfma<DD>), g, b, 0, st, q, go, lse, (const float*)delta, gidx, sidx, win_start, rpe.gc,      \
              rpe.table, rpe.pos_bnd, dq, ex, C, H, scale, chunks);                                                       \
    break;
  switch (C / H) {
    SS_RMB_CASE(16) SS_RMB_CASE(32) SS_RMB_CASE(48) SS_RMB_CASE(64)
    default: return SS_ERR_ARG;
  }
#undef SS_RMB_CASE
  return SS_OK;
}

int ss_attn_rpe_dtable_reduce(const float* slab, int nslab, int H, int pos_bnd, float* dtable, hipStream_t st) {
  const int nb = 3 * (2 * pos_bnd + 1);
  SS_LAUNCH(k_rpe_dtable_reduce, dim3((unsigned)ss_div_up((int64_t)H * nb, 64)), dim3(256), 0, st, slab, nslab, H, nb, dtable);
  return SS_OK;
}
