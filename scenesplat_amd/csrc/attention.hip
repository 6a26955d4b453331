// C-ABI entry points of the serialized-window attention on the packed (n, 3C) layout, plain (ss_window_attn_*) and with
// relative position encoding (ss_window_attn_rpe_*): one argument check, one SIMT / MFMA choice and one workspace layout,
// dispatching to the SIMT kernels (attention_simt.hip) or the MFMA kernels (attention_mfma.hip, attention_rpe.hip).
#include "attention_internal.h"

extern "C" int ss_version(void) { return 101; }

static bool args_ok(int num_windows, int channels, int num_heads, int64_t n, int64_t n_pad, int dtype, const SsAttnRpe* rpe) {
  if (num_windows < 0 || channels <= 0 || num_heads <= 0 || channels % num_heads || n_pad < n) return false;
  if (dtype != SS_F32 && dtype != SS_BF16) return false;
  return !rpe || (rpe->pos_bnd >= 0 && rpe->pos_bnd <= SS_ATTN_RPE_MAX_POS_BND);
}

// MFMA is asked for but cannot run: the kernels keep the window's row offsets (16-byte units, 32 bits) in LDS.  The RPE
// family (simt_for_unsupported) also sends a bf16 head dim outside 16/32/48/64, channels % 8 != 0 and an unknown window
// length to the SIMT kernels (which report the head dims they do not cover); the plain family hands such shapes to the
// MFMA launcher and returns its status.
static int pick_impl(int impl, int dtype, int max_window, int64_t n, int channels, int num_heads, bool simt_for_unsupported) {
  if (impl != SS_ATTN_MFMA) return impl;
  if (max_window > SS_ATTN_MFMA_MAX_WINDOW || n * (int64_t)(3 * channels / 8) >= (1LL << 31)) return SS_ATTN_SIMT;
  if (simt_for_unsupported) {
    const int d = channels / num_heads;
    if (max_window <= 0) return SS_ATTN_SIMT;
    if (dtype == SS_BF16 && (!(d == 16 || d == 32 || d == 48 || d == 64) || (channels & 7))) return SS_ATTN_SIMT;
  }
  return impl;
}

// backward workspace: delta (n_pad, H) f32 | dK/dV of the borrowed slots (n_pad - n, 2C) | with RPE the dT slabs
// ((window, query chunk), H, 3 rpe_num) f32
struct BwdWorkspace { size_t extra, slab, total; };
static BwdWorkspace bwd_workspace(int64_t n, int64_t n_pad, int channels, int num_heads, int dtype, size_t slab_floats) {
  BwdWorkspace w;
  w.extra = al256((size_t)n_pad * num_heads * 4);
  w.slab = w.extra + al256((size_t)(n_pad - n) * 2 * channels * (dtype == SS_F32 ? 4 : 2));
  w.total = w.slab + al256(slab_floats * 4);
  return w;
}
static size_t rpe_slab_floats(int num_windows, int max_window, int num_heads, int pos_bnd) {
  return (size_t)(num_windows > 0 ? num_windows : 0) * ss_attn_rpe_chunks(max_window) * num_heads * 3 *
         (2 * (size_t)(pos_bnd > 0 ? pos_bnd : 0) + 1);
}

static int attn_fwd(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int num_windows,
                    int max_window, int64_t n, int64_t n_pad, int channels, int num_heads, float scale, int dtype, int impl,
                    const SsAttnRpe* rpe, void* out, float* lse, hipStream_t stream) {
  if (!args_ok(num_windows, channels, num_heads, n, n_pad, dtype, rpe)) return SS_ERR_ARG;
  if (num_windows == 0) return SS_OK;
  impl = pick_impl(impl, dtype, max_window, n, channels, num_heads, rpe != nullptr);
  if (impl == SS_ATTN_SIMT)
    return ss_attn_fwd_simt(qkv, gidx, sidx, win_start, num_windows, out, lse, channels, num_heads, scale, dtype, rpe, stream);
  if (!(impl == SS_ATTN_MFMA && dtype == SS_BF16)) return SS_ERR_ARG;
  return rpe ? ss_attn_rpe_fwd_mfma(qkv, gidx, sidx, win_start, num_windows, max_window, out, lse, channels, num_heads, scale, *rpe, stream)
             : ss_attn_fwd_mfma(qkv, gidx, sidx, win_start, num_windows, max_window, out, lse, channels, num_heads, scale, stream);
}

// rpe (its slab is set here) and dtable together, or neither
static int attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* gidx,
                    const int32_t* sidx, const int32_t* win_start, int num_windows, int max_window, int64_t n, int64_t n_pad,
                    int channels, int num_heads, float scale, int dtype, int impl, SsAttnRpe* rpe, void* dqkv, float* dtable,
                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!args_ok(num_windows, channels, num_heads, n, n_pad, dtype, rpe)) return SS_ERR_ARG;
  const BwdWorkspace ws = bwd_workspace(n, n_pad, channels, num_heads, dtype,
                                        rpe ? rpe_slab_floats(num_windows, max_window, num_heads, rpe->pos_bnd) : 0);
  if (workspace_bytes < ws.total) return SS_ERR_WORKSPACE;
  float* delta = (float*)workspace;
  void* extra = (char*)workspace + ws.extra;
  if (rpe) rpe->slab = (float*)((char*)workspace + ws.slab);
  int nslab = 0, rc = SS_OK;
  if (num_windows > 0) {
    impl = pick_impl(impl, dtype, max_window, n, channels, num_heads, rpe != nullptr);
    if (impl == SS_ATTN_SIMT) {
      rc = ss_attn_delta(out, dout, sidx, delta, n_pad, channels, num_heads, dtype, stream);
      if (rc) return rc;
      rc = ss_attn_bwd_simt(qkv, dout, lse, delta, gidx, sidx, win_start, num_windows, dqkv, extra, channels, num_heads, scale,
                            dtype, rpe, stream);
      nslab = num_windows;
    } else if (impl == SS_ATTN_MFMA && dtype == SS_BF16) {      // the MFMA dQ kernel computes delta itself
      rc = rpe ? ss_attn_rpe_bwd_mfma(qkv, dout, out, lse, delta, gidx, sidx, win_start, num_windows, max_window, dqkv, extra,
                                      channels, num_heads, scale, *rpe, stream)
               : ss_attn_bwd_mfma(qkv, dout, out, lse, delta, gidx, sidx, win_start, num_windows, max_window, dqkv, extra,
                                  channels, num_heads, scale, stream);
      nslab = num_windows * ss_attn_rpe_chunks(max_window);
    } else {
      return SS_ERR_ARG;
    }
    if (rc) return rc;
    if (n_pad > n) rc = ss_attn_fix_borrowed(gidx, sidx, n_pad, extra, dqkv, channels, dtype, stream);
    if (rc) return rc;
  }
  // dtable is overwritten (all zeros when there is no window)
  return rpe ? ss_attn_rpe_dtable_reduce(rpe->slab, nslab, num_heads, rpe->pos_bnd, dtable, stream) : SS_OK;
}

extern "C" int ss_window_attn_fwd(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start,
                                  int num_windows, int max_window, int64_t n, int64_t n_pad, int channels, int num_heads,
                                  float scale, int dtype, int impl, void* out, float* lse, hipStream_t stream) {
  return attn_fwd(qkv, gidx, sidx, win_start, num_windows, max_window, n, n_pad, channels, num_heads, scale, dtype, impl, nullptr,
                  out, lse, stream);
}

extern "C" int ss_window_attn_rpe_fwd(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start,
                                      int num_windows, int max_window, int64_t n, int64_t n_pad, int channels,
                                      int num_heads, float scale, int dtype, int impl, const int32_t* grid_coord,
                                      const float* table, int pos_bnd, void* out, float* lse, hipStream_t stream) {
  const SsAttnRpe rpe = {grid_coord, table, pos_bnd, nullptr};
  return attn_fwd(qkv, gidx, sidx, win_start, num_windows, max_window, n, n_pad, channels, num_heads, scale, dtype, impl, &rpe,
                  out, lse, stream);
}

extern "C" size_t ss_window_attn_bwd_workspace_bytes(int64_t n, int64_t n_pad, int channels, int num_heads, int dtype) {
  return bwd_workspace(n, n_pad, channels, num_heads, dtype, 0).total;
}

extern "C" size_t ss_window_attn_rpe_bwd_workspace_bytes(int64_t n, int64_t n_pad, int channels, int num_heads, int dtype,
                                                         int num_windows, int max_window, int pos_bnd) {
  return bwd_workspace(n, n_pad, channels, num_heads, dtype, rpe_slab_floats(num_windows, max_window, num_heads, pos_bnd)).total;
}

extern "C" int ss_window_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                                  const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int num_windows,
                                  int max_window, int64_t n, int64_t n_pad, int channels, int num_heads, float scale,
                                  int dtype, int impl, void* dqkv, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream) {
  return attn_bwd(qkv, out, dout, lse, gidx, sidx, win_start, num_windows, max_window, n, n_pad, channels, num_heads, scale,
                  dtype, impl, nullptr, dqkv, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ss_window_attn_rpe_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                                      const int32_t* gidx, const int32_t* sidx, const int32_t* win_start, int num_windows,
                                      int max_window, int64_t n, int64_t n_pad, int channels, int num_heads, float scale,
                                      int dtype, int impl, const int32_t* grid_coord, const float* table, int pos_bnd,
                                      void* dqkv, float* dtable, void* workspace, size_t workspace_bytes,
                                      hipStream_t stream) {
  SsAttnRpe rpe = {grid_coord, table, pos_bnd, nullptr};
  return attn_bwd(qkv, out, dout, lse, gidx, sidx, win_start, num_windows, max_window, n, n_pad, channels, num_heads, scale,
                  dtype, impl, &rpe, dqkv, dtable, workspace, workspace_bytes, stream);
}
