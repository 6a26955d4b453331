// Prompt arithmetic of ALL PDNorm layers of a model in one launch each way (prompt-driven normalisation,
// pointcept/models/point_prompt_training/prompt_driven_normalization.py:8-53).  The reference runs, per norm layer,
//   shift, scale = Linear(silu(context)).chunk(2);  feat = norm(feat) * (1 + scale) + shift
// with context (1, Cc): scale and shift are per-channel constants of the batch, so they fold into the affine pair of the norm,
//   gamma_eff = gamma * (1 + scale),   beta_eff = beta * (1 + scale) + shift        (gamma = 1, beta = 0 for an affine-free norm)
// and the fused norm kernels (norm.hip) run unchanged on gamma_eff / beta_eff.  What is left per layer is a (2C x Cc) matrix-vector
// product: 64 of them in the lang-pretrain backbone (18,720 channels), a few microseconds of launch each as separate ops.  Here: a descriptor table with one
// row per layer (a grouped launch, grouped.h), 16 channels per workgroup, 4 per wave; the lanes of a wave stride over Cc and the
// two rows of W that a channel needs (c: shift, C + c: scale) are read once, coalesced.  Sums have a fixed order (lane-strided,
// xor butterfly, waves in order, workgroup partials in order): no atomics, results are bitwise reproducible.
#include "grouped.h"

#define PDN_WORDS 14          // int64 words per table row, see scenesplat_hip.h
#define PDN_CH_PER_WG 16
#define PDN_CH_PER_WAVE 4

__device__ __forceinline__ float pdn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float pdn_silu(float x) { return x / (1.0f + expf(-x)); }

// V consecutive floats (V = 4: one 16-byte access; the host selects it only when Cc % 4 == 0 and every base is 16-byte aligned)
template <int V> struct PdnVec { float v[V]; };
template <int V> __device__ __forceinline__ PdnVec<V> pdn_ld(const float* p) {
  PdnVec<V> r;
  if constexpr (V == 4) { const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p); r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
  else r.v[0] = *p;
  return r;
}
template <int V> __device__ __forceinline__ PdnVec<V> pdn_ld(cgf32* p) {
  PdnVec<V> r;
  if constexpr (V == 4) {
    const f32x4_t t = ld4(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else r.v[0] = *p;
  return r;
}
template <int V> __device__ __forceinline__ void pdn_st(gf32* p, const PdnVec<V>& r) {
  if constexpr (V == 4) {
    const f32x4_t t = {r.v[0], r.v[1], r.v[2], r.v[3]};
    st4(p, t);
  } else *p = r.v[0];
}

// ---- forward: gamma_eff, beta_eff, 1 + scale of every channel of every layer -------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256)
k_pdnorm_mod_fwd(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob, const float* __restrict__ context,
                 int Cc) {
  const int b = blockIdx.x;
  const int lo = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)lo * PDN_WORDS;
  const int C = (int)d[0];
  cgf32* W = reinterpret_cast<cgf32*>(d[1]);
  cgf32* bias = reinterpret_cast<cgf32*>(d[2]);
  cgf32* gamma = reinterpret_cast<cgf32*>(d[3]);
  cgf32* beta = reinterpret_cast<cgf32*>(d[4]);
  gf32* gamma_eff = reinterpret_cast<gf32*>(d[5]);
  gf32* beta_eff = reinterpret_cast<gf32*>(d[6]);
  gf32* ops = reinterpret_cast<gf32*>(d[7]);
  const int lane = threadIdx.x & 63;
  const int c0 = (b - wg_start[lo]) * PDN_CH_PER_WG + (threadIdx.x >> 6) * PDN_CH_PER_WAVE;      // wave-uniform
  if (c0 >= C) return;
  int ch[PDN_CH_PER_WAVE];
#pragma unroll
  for (int j = 0; j < PDN_CH_PER_WAVE; ++j) ch[j] = min(c0 + j, C - 1);       // channels past the end repeat the last one and are not written
  float ash[PDN_CH_PER_WAVE] = {0.f, 0.f, 0.f, 0.f}, asc[PDN_CH_PER_WAVE] = {0.f, 0.f, 0.f, 0.f};
  for (int k = lane * V; k < Cc; k += 64 * V) {
    PdnVec<V> s = pdn_ld<V>(context + k);
#pragma unroll
    for (int i = 0; i < V; ++i) s.v[i] = pdn_silu(s.v[i]);
#pragma unroll
    for (int j = 0; j < PDN_CH_PER_WAVE; ++j) {
      const PdnVec<V> wsh = pdn_ld<V>(W + (int64_t)ch[j] * Cc + k), wsc = pdn_ld<V>(W + (int64_t)(C + ch[j]) * Cc + k);
#pragma unroll
      for (int i = 0; i < V; ++i) { ash[j] += wsh.v[i] * s.v[i]; asc[j] += wsc.v[i] * s.v[i]; }
    }
  }
#pragma unroll
  for (int j = 0; j < PDN_CH_PER_WAVE; ++j) { ash[j] = wave_reduce_sum(ash[j]); asc[j] = wave_reduce_sum(asc[j]); }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < PDN_CH_PER_WAVE; ++j) {
      const int c = c0 + j;
      if (c < C) {
        const float shift = ash[j] + bias[c], scale = asc[j] + bias[C + c];
        const float o = 1.0f + scale;
        const float g = gamma ? gamma[c] : 1.0f, be = beta ? beta[c] : 0.0f;
        gamma_eff[c] = g * o;
        beta_eff[c] = be * o + shift;
        ops[c] = o;
      }
    }
  }
}

// ---- backward: dgamma, dbeta, db, dW of every layer; per-workgroup partial sums of W^T db for dcontext ----------------------
template <int V>
__global__ void __launch_bounds__(256)
k_pdnorm_mod_bwd(const int64_t* __restrict__ desc, const int32_t* __restrict__ wg_start, int nprob, const float* __restrict__ context,
                 int Cc, float* __restrict__ partials) {
  __shared__ float lds[4][64 * V];
  const int b = blockIdx.x;
  const int lo = group_owner(wg_start, nprob, b);
  const int64_t* d = desc + (int64_t)lo * PDN_WORDS;
  const int C = (int)d[0];
  cgf32* W = reinterpret_cast<cgf32*>(d[1]);
  cgf32* gamma = reinterpret_cast<cgf32*>(d[3]);
  cgf32* beta = reinterpret_cast<cgf32*>(d[4]);
  cgf32* ops = reinterpret_cast<cgf32*>(d[7]);
  cgf32* dge = reinterpret_cast<cgf32*>(d[8]);
  cgf32* dbe = reinterpret_cast<cgf32*>(d[9]);
  gf32* dW = reinterpret_cast<gf32*>(d[10]);
  gf32* db = reinterpret_cast<gf32*>(d[11]);
  gf32* dgamma = reinterpret_cast<gf32*>(d[12]);
  gf32* dbeta = reinterpret_cast<gf32*>(d[13]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (b - wg_start[lo]) * PDN_CH_PER_WG + wave * PDN_CH_PER_WAVE;       // wave-uniform; may lie past C (the wave then only adds zeros)
  float dsh[PDN_CH_PER_WAVE], dsc[PDN_CH_PER_WAVE];
#pragma unroll
  for (int j = 0; j < PDN_CH_PER_WAVE; ++j) {
    const int c = c0 + j;
    dsh[j] = dsc[j] = 0.0f;
    if (c < C) {
      const float ge = dge ? dge[c] : 0.0f, be = dbe ? dbe[c] : 0.0f;       // a norm whose output nobody used sends no gradient
      const float g = gamma ? gamma[c] : 1.0f, bt = beta ? beta[c] : 0.0f;
      dsh[j] = be;
      dsc[j] = ge * g + be * bt;
      if (lane == 0) {
        const float o = ops[c];
        db[c] = dsh[j];
        db[C + c] = dsc[j];
        if (dgamma) dgamma[c] = ge * o;
        if (dbeta) dbeta[c] = be * o;
      }
    }
  }
  for (int k0 = 0; k0 < Cc; k0 += 64 * V) {             // uniform over the workgroup: every wave reaches both barriers
    const int k = k0 + lane * V;
    PdnVec<V> acc;
#pragma unroll
    for (int i = 0; i < V; ++i) acc.v[i] = 0.0f;
    if (k < Cc) {
      PdnVec<V> s = pdn_ld<V>(context + k);
#pragma unroll
      for (int i = 0; i < V; ++i) s.v[i] = pdn_silu(s.v[i]);
#pragma unroll
      for (int j = 0; j < PDN_CH_PER_WAVE; ++j) {
        const int c = c0 + j;
        if (c < C) {
          const int64_t rsh = (int64_t)c * Cc + k, rsc = (int64_t)(C + c) * Cc + k;
          const PdnVec<V> wsh = pdn_ld<V>(W + rsh), wsc = pdn_ld<V>(W + rsc);
          PdnVec<V> osh, osc;
#pragma unroll
          for (int i = 0; i < V; ++i) {
            acc.v[i] += wsh.v[i] * dsh[j];
            acc.v[i] += wsc.v[i] * dsc[j];
            osh.v[i] = dsh[j] * s.v[i];
            osc.v[i] = dsc[j] * s.v[i];
          }
          pdn_st<V>(dW + rsh, osh);
          pdn_st<V>(dW + rsc, osc);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) lds[wave][lane * V + i] = acc.v[i];
    __syncthreads();
    if (wave == 0 && k < Cc) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int q = lane * V + i;
        partials[(int64_t)b * Cc + k + i] = ((lds[0][q] + lds[1][q]) + lds[2][q]) + lds[3][q];
      }
    }
    __syncthreads();
  }
}

// dcontext[k] = silu'(context[k]) * sum over workgroups of partials[w][k] in a fixed order: 16 interleaved chains per part (chain j
// takes the part's workgroups j, j + 16, ...), then the chains in order.  16 context channels x 16 chains per workgroup: the full
// lang-pretrain backbone has 1,170 partial rows, a chain of ~75 dependent adds each.
// The workgroups [0, split) and [split, nwg) are summed apart and contribute silu' * A + silu' * B (two roundings of the products, one
// of the sum: no fma), which is bit for bit what two launches over the two parts add up to in autograd: a backward pass that is
// split in two calls (two groups of layers) gives the gradient of the unsplit one.
#define PDN_FIN_K 16
#define PDN_FIN_CHAINS 16
__global__ void __launch_bounds__(256)
k_pdnorm_mod_bwd_finish(const float* __restrict__ partials, int nwg, int split, const float* __restrict__ context, int Cc,
                        float* __restrict__ dcontext) {
  __shared__ float lds[2][PDN_FIN_CHAINS][PDN_FIN_K];
  const int kk = threadIdx.x % PDN_FIN_K, chain = threadIdx.x / PDN_FIN_K;
  const int k = blockIdx.x * PDN_FIN_K + kk;
  float acc0 = 0.0f, acc1 = 0.0f;
  if (k < Cc) {
    for (int w = chain; w < split; w += PDN_FIN_CHAINS) acc0 += partials[(int64_t)w * Cc + k];
    for (int w = split + chain; w < nwg; w += PDN_FIN_CHAINS) acc1 += partials[(int64_t)w * Cc + k];
  }
  lds[0][chain][kk] = acc0;
  lds[1][chain][kk] = acc1;
  __syncthreads();
  if (chain == 0 && k < Cc) {
    float t0 = lds[0][0][kk], t1 = lds[1][0][kk];
#pragma unroll
    for (int j = 1; j < PDN_FIN_CHAINS; ++j) { t0 += lds[0][j][kk]; t1 += lds[1][j][kk]; }
    const float x = context[k];
    const float sg = pdn_sigmoid(x);
    const float ds = sg * (1.0f + x * (1.0f - sg));
    float r = __fmul_rn(ds, split > 0 ? t0 : t1);
    if (split > 0 && split < nwg) r = __fadd_rn(r, __fmul_rn(ds, t1));
    dcontext[k] = r;
  }
}

extern "C" int ss_pdnorm_channels_per_workgroup(void) { return PDN_CH_PER_WG; }

extern "C" int ss_pdnorm_mod_fwd(const int64_t* table, const int32_t* wg_start, int num_layers, int total_workgroups, const float* context,
                                 int context_channels, int vec4, hipStream_t stream) {
  if (num_layers == 0) return SS_OK;
  if (!table || !wg_start || !context || context_channels <= 0 || num_layers < 0 || total_workgroups <= 0) return SS_ERR_ARG;
  if (vec4 && (context_channels % 4 != 0 || (reinterpret_cast<uintptr_t>(context) & 15))) return SS_ERR_ARG;
  if (vec4)
    SS_LAUNCH(k_pdnorm_mod_fwd<4>, dim3((unsigned)total_workgroups), dim3(256), 0, stream, table, wg_start, num_layers, context, context_channels);
  else
    SS_LAUNCH(k_pdnorm_mod_fwd<1>, dim3((unsigned)total_workgroups), dim3(256), 0, stream, table, wg_start, num_layers, context, context_channels);
  return SS_OK;
}

extern "C" int ss_pdnorm_mod_bwd(const int64_t* table, const int32_t* wg_start, int num_layers, int total_workgroups, const float* context,
                                 int context_channels, int vec4, int split_workgroup, float* partials, float* dcontext, hipStream_t stream) {
  if (num_layers == 0) return SS_OK;
  if (split_workgroup < 0 || split_workgroup > total_workgroups) return SS_ERR_ARG;
  if (!table || !wg_start || !context || !partials || !dcontext || context_channels <= 0 || num_layers < 0 || total_workgroups <= 0)
    return SS_ERR_ARG;
  if (vec4 && (context_channels % 4 != 0 || (reinterpret_cast<uintptr_t>(context) & 15))) return SS_ERR_ARG;
  if (vec4)
    SS_LAUNCH(k_pdnorm_mod_bwd<4>, dim3((unsigned)total_workgroups), dim3(256), 0, stream, table, wg_start, num_layers, context, context_channels,
              partials);
  else
    SS_LAUNCH(k_pdnorm_mod_bwd<1>, dim3((unsigned)total_workgroups), dim3(256), 0, stream, table, wg_start, num_layers, context, context_channels,
              partials);
  SS_LAUNCH(k_pdnorm_mod_bwd_finish, dim3((unsigned)((context_channels + PDN_FIN_K - 1) / PDN_FIN_K)), dim3(256), 0, stream, partials, total_workgroups, split_workgroup,
            context, context_channels, dcontext);
  return SS_OK;
}
