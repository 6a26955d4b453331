/* scenesplat_hip.h -- C-ABI of libscenesplat_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the native ops behind SceneSplat's PTv3 hot path.  Every entry point
 * takes raw DEVICE pointers, explicit sizes and a HIP stream, returns an int status
 * (SS_OK = 0), allocates nothing and is re-entrant per stream; the caller owns all memory
 * (outputs and workspaces; sizes from the *_workspace_bytes queries).  It keeps no global state
 * except process-wide kernel-choice switches: the flag ss_wgrad_set_xcd_order sets, and the
 * environment variables SS_WGRAD_XCD_TRIPLE, SS_WGRAD_MINPER, SS_CONV_PIPE, SS_WGRAD_PIPE,
 * SS_ATTN_FWD32, SS_ATTN_FWD_NQ and SS_ATTN_DO_INPLACE, each read once, at the first call that
 * consults it.  No torch types appear here.  Reference interfaces replaced (paths under /root/reference):
 *
 *   ss_serialize_encode / ss_argsort_i64      pointcept/models/utils/structure.py:81-92
 *                                             (encode(): utils/serialization/default.py:8-24)
 *   ss_pool_partition / ss_pool_level_attrs   point_transformer_v3m1_base.py:384-398,422-427
 *   ss_window_index                           point_transformer_v3m1_base.py:114-170,184-185
 *   ss_subm_rulebook + ss_subm_conv_*         spconv.SubMConv3d (ptv3:278-284,499-506; structure.py:131-138)
 *   ss_segment_reduce / ss_segment_bcast      torch_scatter.segment_csr (ptv3:416-421)
 *   ss_gather_rows / ss_scatter_rows / ss_gather_add_rows   feat[idx] row indexing (ptv3:188,216,417,478)
 *   ss_window_attn_fwd / ss_window_attn_bwd   flash_attn.flash_attn_varlen_qkvpacked_func (ptv3:208-214)
 *   ss_linear_fwd_headmajor + ss_window_attn_hm_fwd / _bwd   the same call together with the qkv projection's output
 *                                             layout and the qkv[order] gather in front of it (ptv3:172-188, 208-216)
 *   ss_lang_head_fwd / ss_lang_head_bwd       models/default.py:98-109 (F.normalize), losses/misc.py:254-270
 *                                             (CosineSimilarity), :274-295 (L2Loss)
 *   ss_seg_loss_fwd / ss_seg_loss_bwd         losses/misc.py:35-62 (CrossEntropyLoss), losses/lovasz.py:121-256 (LovaszLoss, multiclass)
 *   ss_seg_iou                                utils/misc.py:167-179 (intersection_and_union_gpu), hooks/evaluator.py:106-240
 *   ss_aug_bbox ... ss_aug_color             pointcept/datasets/transform.py:446-816,1120-1178 (the per-sample augmentations
 *                                             in front of GridSample: CenterShift ... ChromaticJitter)
 *   ss_aug_hsv / ss_aug_moments               pointcept/datasets/transform.py:1037-1100 (HueSaturationTranslation), :424-434 (NormalizeCoord)
 *   ss_instance_boxes / ss_instance_scatter   pointcept/datasets/transform.py:1626-1664 (InstanceParser)
 *   ss_voxel_pick_labelled                    pointcept/datasets/transform.py:1245-1253 (GridSample's pick over pc_coord)
 *   ss_color_chain / ss_voxel_blur            pointcept/datasets/transform.py:820-1032 (RandomColorJitter, RandomColorGrayScale),
 *                                             :60-176 (GSGaussianBlurVoxelOpc)
 *   ss_knn_query ... ss_bfs_cluster           libs/pointops/src/pointops_api.cpp:15-31,
 *                                             libs/pointops2/src/pointops_api.cpp:17-44,
 *                                             libs/pointgroup_ops/src/bfs_cluster.cpp:140-145
 *   ss_splat_project ... ss_splat_composite   tools/visualize_scene.py:57-201 (the Open3D point cloud / ellipsoid meshes and the
 *                                             matplotlib scatter; docs/ROADMAP.md task 3), as a headless splat rasteriser
 */
#ifndef SCENESPLAT_HIP_H
#define SCENESPLAT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct ihipStream_t;
typedef struct ihipStream_t* ss_stream_t; /* == hipStream_t */

#define SS_MAX_ORDERS 8
enum { SS_ORDER_Z = 0, SS_ORDER_Z_TRANS = 1, SS_ORDER_HILBERT = 2, SS_ORDER_HILBERT_TRANS = 3 };
enum { SS_DTYPE_F32 = 0, SS_DTYPE_BF16 = 1 };
enum { SS_ATTN_SIMT = 0, SS_ATTN_MFMA = 1 };
/* the int status every entry point returns: 0 = ok, 1 bad argument, 2 launch failed, 3 workspace too small */
enum { SS_OK = 0, SS_ERR_ARG = 1, SS_ERR_LAUNCH = 2, SS_ERR_WORKSPACE = 3 };

int ss_version(void);

/* ---- serialization ------------------------------------------------------------------- */
/* codes[k][i] = (batch[i] << 3*depth) | key_{orders[k]}(grid_coord[i]); grid_coord (n,3) int32 >= 0 */
int ss_serialize_encode(const int32_t* grid_coord, const int32_t* batch, int64_t n, int depth, const int* orders,
                        int num_orders, int64_t* codes, ss_stream_t stream);
int ss_offsets_to_batch(const int32_t* offsets, int num_batches, int64_t n, int32_t* batch, ss_stream_t stream);
int ss_count_duplicates(const int64_t* sorted_keys, int64_t n, int32_t* count, ss_stream_t stream);
int ss_grid_coord_max(const int32_t* grid_coord, int64_t n, int32_t* out_max, ss_stream_t stream);
/* stable argsort of num_segments independent rows of n non-negative int64 keys (low key_bits
 * significant).  order_out (num_segments,n) int32; inverse_out / sorted_keys_out optional. */
size_t ss_argsort_workspace_bytes(int64_t n, int num_segments);
int ss_argsort_i64(const int64_t* keys, int num_segments, int64_t n, int key_bits, int32_t* order_out,
                   int32_t* inverse_out, int64_t* sorted_keys_out, void* workspace, size_t workspace_bytes,
                   ss_stream_t stream);

/* ---- grid pooling structure ---------------------------------------------------------- */
size_t ss_pool_partition_workspace_bytes(int64_t n);
/* cluster (n), idx_ptr (n+1 capacity), head (n capacity), n_out (1): clusters are the runs of
 * equal (code0 >> shift_bits) along order0; indices of segment_csr == order0. */
int ss_pool_partition(const int64_t* code0, const int32_t* order0, int64_t n, int shift_bits, int32_t* cluster,
                      int32_t* idx_ptr, int32_t* head, int32_t* n_out, void* workspace, size_t workspace_bytes,
                      ss_stream_t stream);
int ss_pool_level_attrs(const int32_t* head, int64_t n_out, int64_t n_in, const int32_t* grid_coord,
                        const int32_t* batch, const int64_t* codes, int num_orders, int pool_depth,
                        int32_t* grid_coord_out, int32_t* batch_out, int64_t* codes_out, ss_stream_t stream);
int ss_batch_offsets(const int32_t* batch, const int32_t* perm, int64_t n, int num_batches, int32_t* offsets,
                     ss_stream_t stream);

/* ---- attention windows ---------------------------------------------------------------- */
/* offsets / offsets_pad: (num_batches+1) int32 exclusive prefix sums (leading 0). */
int ss_window_index(const int32_t* order, const int32_t* offsets, const int32_t* offsets_pad, int num_batches,
                    int patch_size, int64_t n_pad, int32_t* gidx, int32_t* sidx, ss_stream_t stream);
/* qkv (n,3C); out (n,C); lse (n_pad,H) f32; win_start (num_windows+1) int32 = cu_seqlens */
int ss_window_attn_fwd(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start,
                       int num_windows, int max_window, int64_t n, int64_t n_pad, int channels, int num_heads,
                       float scale, int dtype, int impl, void* out, float* lse, ss_stream_t stream);
size_t ss_window_attn_bwd_workspace_bytes(int64_t n, int64_t n_pad, int channels, int num_heads, int dtype);
int ss_window_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* gidx,
                       const int32_t* sidx, const int32_t* win_start, int num_windows, int max_window, int64_t n,
                       int64_t n_pad, int channels, int num_heads, float scale, int dtype, int impl, void* dqkv,
                       void* workspace, size_t workspace_bytes, ss_stream_t stream);

/* ---- grouped launches: many small problems in ONE launch --------------------------------------------------------------------
 * Every entry point that takes (desc, wg_start, nprob, total_workgroups, ...) follows one contract.  desc: one row of int64 words
 * per problem, (nprob, words) row-major; wg_start: nprob + 1 int32, wg_start[p] = first workgroup of problem p = the running total
 * of the workgroup counts of the problems before it, wg_start[nprob] = total_workgroups < 2^31.  Both tables live in DEVICE memory.
 * wg_start is non-decreasing and starts at 0; a problem may own no workgroup.  Workgroup b belongs to the LAST problem p with
 * wg_start[p] <= b and works on that problem's piece b - wg_start[p].  nprob <= 0 or total_workgroups <= 0: SS_OK without a launch;
 * a NULL table: SS_ERR_ARG (exceptions are stated at the entry).  Each entry below gives its descriptor words and what one workgroup
 * owns (the unit that the workgroup count of a problem is rounded up in). */

/* fp32 -> bf16 cast of many tensors (the bf16 weight shadows; replaces one torch copy kernel per tensor).
 * desc: 3 words {src f32 pointer, dst bf16 pointer, numel}; a workgroup owns ss_cast_bf16_group_elems_per_workgroup() elements. */
int ss_cast_bf16_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
int ss_cast_bf16_group_elems_per_workgroup(void);

/* Scene ingest: every asset of a packed scene arena -> its output tensor, with numpy's astype / clip / reshape / [:, column] values
 * bit for bit (replaces one host conversion and one upload per .npy file of a dataset sample).
 * desc: 8 words {src pointer, dst pointer, n_out elements, src dtype | dst dtype << 8 | flags << 16, src row stride, column (both in
 * elements; read with flag 4 only: out[k] = src[k * stride + column]), lo, hi (fp32 bit patterns in the low 32 bits; dst f32 only)}.
 * dtype codes: 0 f64, 1 f32, 2 f16, 3 u8, 4 i8, 5 i16, 6 i32, 7 i64, 8 bool.  flags: 1 has_lo, 2 has_hi, 4 pick_column.
 * Pairs: any source -> f32 (then out = v < lo ? lo : v > hi ? hi : v, so NaN stays and -0.0 passes lo = 0); f32 | f16 -> f16
 * (round to nearest even, overflow to inf, subnormals kept); u8 | i8 | i16 | i32 | i64 | bool -> i32 (wraps) and -> bool (any bit
 * set); equal dtypes: a copy.  Any other pair writes nothing (the Python wrapper refuses it).  16-byte source loads when src and dst
 * are 16-byte aligned.  A workgroup owns ss_ingest_group_elems_per_workgroup() consecutive output elements. */
int ss_ingest_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
int ss_ingest_group_elems_per_workgroup(void);

/* ---- optimizer step: global gradient norm + AdamW update of all tensors of all parameter groups (replaces
 * torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step, pointcept/engines/train.py:196-232).  Grouped launches as above:
 * a workgroup owns ss_optim_group_elems_per_workgroup() elements; flags bit 0 = every pointer of the row is 16-byte aligned
 * (16-byte lanes; otherwise one element per lane).  No atomics: results are bitwise reproducible.
 * ss_grad_sqnorm_group: desc 3 words {g f32 pointer, numel, flags}; partials[w] = fp64 sum of squares of workgroup w.
 * ss_grad_norm_finish:  record[0] = total_norm = sqrt(sum of partials), record[1] = coef = min(1, max_norm / (total_norm + 1e-6)),
 *                       non-finite values propagating as in clip_grad_norm_(norm_type=2, error_if_nonfinite=False).
 * ss_adamw_group:       desc 10 words {p, g, m, v f32 pointers, numel, flags, then 8 fp32: 1 - lr*wd, 1 - beta1, beta2,
 *                       1 - beta2, sqrt(1 - beta2^t), eps, lr / (1 - beta1^t), 0}; record as written by ss_grad_norm_finish (its
 *                       coef scales g on the fly) or NULL for coef = 1.  Writes p, m, v; g is only read. */
int ss_optim_group_elems_per_workgroup(void);
int ss_grad_sqnorm_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, double* partials,
                         ss_stream_t stream);
int ss_grad_norm_finish(const double* partials, int num_partials, float max_norm, float* record, ss_stream_t stream);
int ss_adamw_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, const float* record,
                   ss_stream_t stream);

/* ---- PDNorm prompt modulation of ALL PDNorm layers of a model, one grouped launch each way (csrc/pdnorm.hip; reference:
 * pointcept/models/point_prompt_training/prompt_driven_normalization.py:8-53).  With s = silu(context) (context_channels fp32 values,
 * silu(x) = x / (1 + exp(-x))) and [shift | scale] = W s + b per layer (W (2C, context_channels) row-major, b (2C)):
 *   gamma_eff = gamma * (1 + scale),  beta_eff = beta * (1 + scale) + shift,  ops = 1 + scale      (gamma = 1 / beta = 0 where NULL).
 * table: 14 int64 per layer {C, W, b, gamma | 0, beta | 0, gamma_eff, beta_eff, ops, dgamma_eff | 0, dbeta_eff | 0, dW, db,
 * dgamma | 0, dbeta | 0}, all fp32 pointers; the forward reads words 0-7, the backward words 0-1, 3-4 and 7-13.  A grouped
 * launch (above) with one problem per layer; a workgroup owns ss_pdnorm_channels_per_workgroup() channels.  Unlike the other grouped
 * entries, num_layers < 0, and total_workgroups <= 0 with num_layers != 0, are SS_ERR_ARG.  vec4 != 0: 16-byte accesses; the caller guarantees context_channels % 4 == 0 and 16-byte aligned context, W and dW.
 * Backward: d_shift = dbeta_eff, d_scale = dgamma_eff * gamma + dbeta_eff * beta, db = [d_shift | d_scale], dW = db (x) s,
 * dgamma = dgamma_eff * ops, dbeta = dbeta_eff * ops, dcontext = silu'(context) * sum over layers of W^T db (a NULL dgamma_eff /
 * dbeta_eff counts as zeros).  partials: total_workgroups * context_channels floats of scratch; the sum over workgroups is finished
 * in a fixed order by a second small kernel: no atomics, bitwise reproducible.  split_workgroup in [0, total_workgroups]: the
 * workgroups below it and from it on are summed apart and contribute silu' * A + silu' * B, bit for bit the sum of two calls over
 * the two parts of the table (0 or total_workgroups: one part).  num_layers == 0: SS_OK without a launch. */
int ss_pdnorm_channels_per_workgroup(void);
int ss_pdnorm_mod_fwd(const int64_t* table, const int32_t* wg_start, int num_layers, int total_workgroups, const float* context,
                      int context_channels, int vec4, ss_stream_t stream);
int ss_pdnorm_mod_bwd(const int64_t* table, const int32_t* wg_start, int num_layers, int total_workgroups, const float* context,
                      int context_channels, int vec4, int split_workgroup, float* partials, float* dcontext, ss_stream_t stream);

/* ---- DropPath row scales (timm DropPath on (n, C) rows, ptv3:333-336) ------------------------------------
 * out[i] = Bernoulli(keep[i]) / keep[i] for the n rows of all residual seams of a forward; Philox4x32-10, counter = row index,
 * key = the 64-bit seed read from DEVICE memory (so a captured launch draws fresh masks per replay). */
int ss_row_keep_scales(const int64_t* seed, const float* keep, float* out, int64_t n, ss_stream_t stream);

/* ---- exact-erf GELU of the MLP (ptv3:225-248, nn.GELU()) on flat arrays ---------------------------------------
 * dy == NULL: out = gelu(x); else out = dy * gelu'(x).  dtype SS_DTYPE_F32 | SS_DTYPE_BF16 (math in fp32, one rounding); 16-byte aligned. */
int ss_gelu(const void* x, const void* dy, void* out, int64_t numel, int dtype, ss_stream_t stream);

/* ---- runtime queries -------------------------------------------------------------------- */
/* 0 = the stream is not capturing, 1 = capturing, 2 = its capture was invalidated (abandon it: never end it), < 0 = query failed */
int ss_stream_capture_status(ss_stream_t stream);
/* identity (> 0) of the capture the stream is actively recording into, 0 = none / unknown */
unsigned long long ss_stream_capture_id(ss_stream_t stream);

/* ---- head-major window attention (round 3) ------------------------------------------------------------
 * hm (sections = 3, num_heads, n_pad, head_dim) bf16: q / k / v of padded slot p of the curve order (slot p = point gidx[p]);
 * section 0 holds q * softmax_scale * log2(e).  Written by ss_linear_fwd_headmajor (the projection itself, LDS-DMA pipeline
 * GEMM; needs k % 64 == 0) or by ss_headmajor_pack from an existing (n, sections * channels) projection (fp32 or bf16).
 * out (n, channels) bf16 in memory row order (rows through sidx); neg_lse2 (num_heads, n_pad) fp32 = -log2 sum exp2(scores).
 * Backward: dqkv (n, 3 * channels) bf16 in memory row order, gradients w.r.t. the UNSCALED q, k, v. */
int ss_linear_fwd_headmajor(const void* x, const int32_t* row_index, const void* weight, const float* bias, void* out_hm,
                            int64_t m, int k, int n_out, int channels, int head_dim, float sec0_scale, ss_stream_t stream);
int ss_headmajor_pack(const void* src, int in_dtype, const int32_t* gidx, void* hm, int64_t n_pad, int channels,
                      int num_heads, int sections, float sec0_scale, ss_stream_t stream);
int ss_window_attn_hm_fwd(const void* hm, const int32_t* sidx, const int32_t* win_start, int num_windows, int max_window,
                          int64_t n, int64_t n_pad, int channels, int num_heads, void* out, float* neg_lse2,
                          ss_stream_t stream);
size_t ss_window_attn_hm_bwd_workspace_bytes(int64_t n, int64_t n_pad, int channels, int num_heads);
int ss_window_attn_hm_bwd(const void* hm, const void* out, const void* dout, const float* neg_lse2, const int32_t* gidx,
                          const int32_t* sidx, const int32_t* win_start, int num_windows, int max_window, int64_t n,
                          int64_t n_pad, int channels, int num_heads, float scale, void* dqkv, void* workspace,
                          size_t workspace_bytes, ss_stream_t stream);

/* ---- window attention with relative position encoding (PT-v3m1 enable_rpe; csrc/attention_rpe.hip) ----------------
 * ss_window_attn_fwd / _bwd with a learned bias added to every score before the softmax:
 *   bias[h][i][j] = sum over the axes a of table[a * rpe_num + clamp(g_i[a] - g_j[a], -pos_bnd, pos_bnd) + pos_bnd][h],
 * g = grid_coord[gidx[slot]], rpe_num = 2 * pos_bnd + 1 (0 <= pos_bnd <= 64).  grid_coord (n, 3) int32; table (3 * rpe_num,
 * num_heads) f32; the bias is not multiplied by `scale`; lse includes it.  impl = SS_ATTN_MFMA (bf16) runs head dims
 * 16/32/48/64 and windows up to 2048 on the matrix cores; longer windows and other shapes run on the SIMT kernels.
 * Backward: dqkv as ss_window_attn_bwd; dtable (3 * rpe_num, num_heads) f32 is OVERWRITTEN with the gradient of the table
 * (no global atomics: per-workgroup partial sums in the workspace, added in a fixed order; a row no (query, key) pair
 * indexes is exactly 0).  The workspace needs no initialisation. */
int ss_window_attn_rpe_fwd(const void* qkv, const int32_t* gidx, const int32_t* sidx, const int32_t* win_start,
                           int num_windows, int max_window, int64_t n, int64_t n_pad, int channels, int num_heads,
                           float scale, int dtype, int impl, const int32_t* grid_coord, const float* table, int pos_bnd,
                           void* out, float* lse, ss_stream_t stream);
size_t ss_window_attn_rpe_bwd_workspace_bytes(int64_t n, int64_t n_pad, int channels, int num_heads, int dtype,
                                              int num_windows, int max_window, int pos_bnd);
int ss_window_attn_rpe_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* gidx,
                           const int32_t* sidx, const int32_t* win_start, int num_windows, int max_window, int64_t n,
                           int64_t n_pad, int channels, int num_heads, float scale, int dtype, int impl,
                           const int32_t* grid_coord, const float* table, int pos_bnd, void* dqkv, float* dtable,
                           void* workspace, size_t workspace_bytes, ss_stream_t stream);

/* ---- submanifold convolution ------------------------------------------------------------ */
/* nbr (k^3, n) int32 (tap-major), -1 = no site; zkeys_sorted/zorder: z (or z-trans, swap_xy=1) codes sorted */
int ss_subm_rulebook(const int32_t* grid_coord, const int32_t* batch, int64_t n, int depth,
                     const int64_t* zkeys_sorted, const int32_t* zorder, int swap_xy, int kernel_size, int32_t* nbr,
                     ss_stream_t stream);
/* keys (n) int64 for regrouping the conv walk order: tap-presence mask of site order[p] (taps <= 27 bits) below the coarse
 * block id p >> coarse_bits; a stable sort of them gives the walk of scenesplat_amd.plan.Level.conv_rowperm */
int ss_subm_tap_mask_keys(const int32_t* nbr, const int32_t* order, int64_t n, int taps, int coarse_bits, int64_t* keys,
                          ss_stream_t stream);
/* same table through an open-addressing hash of the voxel keys (no sorted keys needed); workspace >= 12 *
 * ss_subm_rulebook_table_size(n) bytes */
int64_t ss_subm_rulebook_table_size(int64_t n);
int ss_subm_rulebook_hashed(const int32_t* grid_coord, const int32_t* batch, int64_t n, int depth, int kernel_size, int32_t* nbr,
                            void* workspace, size_t workspace_bytes, ss_stream_t stream);

/* bf16 MFMA implicit GEMM.  in (n,cin) bf16; weight (cout,taps,cin) bf16 (the reference's
 * (Cout,k,k,k,Cin) layout flattened); bias (cout) f32 or NULL; rowperm (n) = site walk order (z-order)
 * or NULL; out (n,cout) bf16 / f32.  cin % 8 == 0.  dgrad = same call on dout with the tap-mirrored
 * transposed weight (cin,taps,cout). */
int ss_subm_conv_fwd(const void* in, const void* weight, const float* bias, const int32_t* nbr, const int32_t* rowperm,
                     void* out, int64_t n, int cin, int cout, int taps, int out_dtype, ss_stream_t stream);
/* bf16 weight of the dgrad pass: wt (cin, taps, cout)[ci][T-1-t][co] = w (cout, taps, cin)[co][t][ci] */
int ss_subm_weight_mirror(const void* w, void* wt, int cout, int taps, int cin, ss_stream_t stream);
/* stream restricted to the CUs set in mask (hipExtStreamCreateWithCUMask); used for the deferred weight gradients */
int ss_stream_create_cu_mask(int nwords, const uint32_t* mask, void** stream_out);
/* im2col of a submanifold conv for small levels: dst (n, taps, row_bytes) = src rows through the rulebook, zero rows for
 * missing neighbours; row_bytes % 16 == 0.  The conv is then one plain GEMM over K = taps * Cin (spconv's gather-GEMM,
 * ptv3:278-284, without the per-tap loop). */
int ss_subm_im2col(const void* src, const int32_t* nbr, void* dst, int64_t n, int taps, int64_t row_bytes, ss_stream_t stream);
/* 256 x 256 LDS-DMA pipeline GEMM (csrc/gemm8.hip).  ss_gemm8_ok: shapes it accepts (k % 64 == 0, k <= 4096, n % 4 == 0,
 * taps <= 27).  ss_subm_conv_fwd_pipe: same contract as ss_subm_conv_fwd (which dispatches to it for wide, large levels).
 * ss_linear_fwd: out (m,n) = x (m,k) bf16 @ weight (n,k)^T bf16 + bias (n) f32 or NULL  -- torch.nn.functional.linear as
 * PTv3 uses it (ptv3:131-133 qkv/proj, ptv3:224-228 MLP). */
int ss_gemm8_ok(int64_t m, int k, int n, int taps);
int ss_subm_conv_fwd_pipe(const void* in, const void* weight, const float* bias, const int32_t* nbr, const int32_t* rowperm,
                          void* out, int64_t n, int cin, int cout, int taps, int out_dtype, ss_stream_t stream);
/* the rulebook in WALK order (nbr_walk[t][k] = nbr[t][rowperm[k]]; rowperm NULL: nbr itself): the pipeline kernel then reads its
 * 256-site slice as contiguous words.  ss_subm_conv_fwd_walk = ss_subm_conv_fwd that hands nbr_walk to the pipeline kernel when it
 * dispatches there (ss_subm_conv_fwd_uses_pipe) and nbr to the other kernels; nbr_walk NULL: plain ss_subm_conv_fwd. */
int ss_subm_conv_fwd_pipe_walk(const void* in, const void* weight, const float* bias, const int32_t* nbr_walk, const int32_t* rowperm,
                               void* out, int64_t n, int cin, int cout, int taps, int out_dtype, ss_stream_t stream);
int ss_subm_conv_fwd_uses_pipe(int64_t n, int cin, int cout, int taps);
int ss_subm_conv_fwd_walk(const void* in, const void* weight, const float* bias, const int32_t* nbr, const int32_t* nbr_walk,
                          const int32_t* rowperm, void* out, int64_t n, int cin, int cout, int taps, int out_dtype, ss_stream_t stream);
int ss_linear_fwd(const void* x, const void* weight, const float* bias, void* out, int64_t m, int k, int n, int out_dtype,
                  ss_stream_t stream);
/* weight gradients on the same pipeline (csrc/wgrad8.hip); dweight must be ZERO on entry (fp32 atomics).
 * ss_subm_conv_wgrad_pipe: contract of ss_subm_conv_wgrad (which dispatches to it for wide, large levels).
 * ss_linear_wgrad: dweight (n_out,k_in) f32 += dy (m,n_out)^T @ x (m,k_in), both bf16 -- the nn.Linear weight gradient;
 * dbias (n_out) f32, ZERO on entry, += column sums of dy (the bias gradient), or NULL. */
/* 1: the weight-gradient kernels order their output tiles XCD-aware (runs of 3 tiles that stream the same rows go to one XCD) */
int ss_wgrad_xcd_order(void);
int ss_wgrad_set_xcd_order(int on);   /* tuning knob (default: off; environment SS_WGRAD_XCD_TRIPLE=1 turns it on) */
int ss_wgrad8_ok(int64_t n, int cin, int cout, int taps);
int ss_subm_conv_wgrad_pipe(const void* in, const void* dout, const int32_t* nbr, const int32_t* rowperm,
                            const int32_t* blk_count, const int32_t* blk_list, float* dweight, int64_t n, int cin, int cout,
                            int taps, ss_stream_t stream);
int ss_linear_wgrad(const void* x, const void* dy, float* dweight, float* dbias, int64_t m, int k_in, int n_out,
                    ss_stream_t stream);
/* Grouped launch (see "grouped launches") of up to 128 independent nn.Linear weight gradients (the blocks of a pooled stage);
 * nprob > 128: SS_ERR_ARG.  desc: 8 words {x, dy, dweight, dbias | 0, m, and three words filled by ss_linear_wgrad_group_plan}; a
 * problem owns the workgroup count that ss_linear_wgrad_group_plan returns (host call, no launch; 0 = shape not eligible); every
 * dweight / dbias zeroed. */
int ss_linear_wgrad_group_plan(int64_t m, int k_in, int n_out, int64_t* desc_words);
/* ..._plan2: the same with launch_tiles = sum over the launch's problems of ss_linear_wgrad_tiles(k_in, n_out) (256 x 256 output
 * tiles): the K dimension of every problem is split so that the whole GROUP is one round of workgroups (one per CU). */
int ss_linear_wgrad_tiles(int k_in, int n_out);
int ss_linear_wgrad_group_plan2(int64_t m, int k_in, int n_out, int launch_tiles, int64_t* desc_words);
int ss_linear_wgrad_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
/* The same group on a CAPPED grid of min(total_items, max_workgroups) persistent workgroups: workgroup b runs the items b, b + grid,
 * b + 2 grid, ... (an item = what a workgroup is in ss_linear_wgrad_group).  A workgroup fills a CU, so a cap of CUs - R leaves R CUs
 * to the kernels of another stream.  ..._plan_capped: the plan for such a launch -- K is split into up to four rounds of equally long
 * items (never below 8 K-tiles of 64 rows per item), so that every workgroup gets the same number of items, give or take one. */
int ss_linear_wgrad_group_plan_capped(int64_t m, int k_in, int n_out, int launch_tiles, int max_workgroups, int64_t* desc_words);
int ss_linear_wgrad_group_capped(const int64_t* desc, const int32_t* wg_start, int nprob, int total_items, int max_workgroups,
                                 ss_stream_t stream);
/* small levels: split-K over tap ranges; acc32 (n,cout) f32 zeroed by the caller, receives out (+bias) */
int ss_subm_conv_splits(int64_t n, int cout, int taps);
int ss_subm_conv_fwd_splitk(const void* in, const void* weight, const float* bias, const int32_t* nbr, const int32_t* rowperm,
                            float* acc32, int64_t n, int cin, int cout, int taps, int splits, ss_stream_t stream);
/* per tap, the 64-site blocks (in rowperm order) that hold at least one pair: blk_count (taps), blk_list (taps, ceil(n/64)) */
int ss_subm_block_lists(const int32_t* nbr, const int32_t* rowperm, int64_t n, int taps, int32_t* blk_count,
                        int32_t* blk_list, ss_stream_t stream);
/* dweight (cout,taps,cin) f32, ACCUMULATED into (caller zeroes it); cin % 8 == 0, cout % 8 == 0 */
int ss_subm_conv_wgrad(const void* in, const void* dout, const int32_t* nbr, const int32_t* rowperm,
                       const int32_t* blk_count, const int32_t* blk_list, float* dweight, int64_t n, int cin, int cout,
                       int taps, ss_stream_t stream);

/* ---- first-stage submanifold conv in exact fp32 on v_mfma_f32_32x32x2_f32 (csrc/subm_f32.hip) ---------------------
 * Replaces spconv.SubMConv3d (pointcept/models/modules.py:64-75, fp32 under AMP) for the 32-channel stage:
 * stem (ptv3:572-590 Embedding, k = 5, 6..11 -> 32) and the enc0 cpe convs (ptv3:271-289, k = 3, 32 -> 32).
 * in (n, cin_padded) f32 with cin_padded 16 or 32 (zero-padded channels); cout == 32.
 * wq = weights re-laid [tap][cin_padded / 8][2][32 co][4] f32: wq[t][q][h][co][e] = W[co][t][8 q + 4 h + e].
 * nbr_walk (taps, n): the rulebook in WALK order, nbr_walk[t][k] = nbr[t][rowperm[k]] (rowperm NULL: nbr itself).
 * dgrad = the same entry on (dout, tap-mirrored transposed weights). */
int ss_subm_f32_ok(int cin_padded, int cout);
int ss_subm_f32_fwd(const float* in, const float* wq, const float* bias, const int32_t* nbr_walk, const int32_t* rowperm,
                    float* out, int64_t n, int cin_padded, int cout, int taps, ss_stream_t stream);
/* dgrad of the same conv on a level with DUPLICATE voxels (Mix3D batches, pointcept/datasets/utils.py:43-47; spconv leaves their
 * semantics open, this library resolves a voxel to its lowest row): dout_folded = ss_dup_fold_rows(dout), wq = tap-mirrored
 * transposed weights; rows that are not the winner of their voxel receive zeros.  taps must be odd. */
int ss_subm_f32_dgrad_dup(const float* dout_folded, const float* wq, const int32_t* nbr_walk, const int32_t* rowperm, float* din,
                          int64_t n, int cin_padded, int cout, int taps, ss_stream_t stream);
/* dweight (32, taps, cin) f32 ACCUMULATED into (caller zeroes it); blk_* from ss_subm_block_lists with the same rowperm */
int ss_subm_f32_wgrad(const float* in, const float* dout, const int32_t* nbr_walk, const int32_t* rowperm,
                      const int32_t* blk_count, const int32_t* blk_list, float* dweight, int64_t n, int cin_padded,
                      int cin, int cout, int taps, ss_stream_t stream);

/* weight gradient with the walk-order rulebook beside the plain one (see ss_subm_conv_fwd_walk); nbr_walk NULL = ss_subm_conv_wgrad */
int ss_subm_conv_wgrad_pipe_walk(const void* in, const void* dout, const int32_t* nbr_walk, const int32_t* rowperm,
                                 const int32_t* blk_count, const int32_t* blk_list, float* dweight, int64_t n, int cin, int cout,
                                 int taps, ss_stream_t stream);
int ss_subm_conv_wgrad_uses_pipe(int64_t n, int cin, int cout, int taps);
/* The pipeline weight gradient on a CAPPED grid of min(items, max_workgroups) persistent workgroups (a workgroup fills a CU, so a cap of
 * CUs - R leaves R CUs to the kernels of another stream).  An item is what a workgroup is in ss_subm_conv_wgrad_pipe (K share, tap,
 * output tile); the workgroups draw item ids from `counter`, ONE int32 that must be zero when the kernel starts (zero it on `stream`
 * in front of every launch; the launch leaves items + workgroups in it).  nbr: the rulebook (taps, n), in walk order when walk != 0
 * (see ss_subm_conv_wgrad_pipe_walk).  min_per: K-tiles of 64 sites per share, 0 = what the plain launch takes.  dweight ZERO on entry.
 * ss_subm_conv_wgrad_pipe_items: the item count of such a launch (host arithmetic, no launch; 0 = shape not eligible). */
int ss_subm_conv_wgrad_pipe_capped(const void* in, const void* dout, const int32_t* nbr, const int32_t* rowperm,
                                   const int32_t* blk_count, const int32_t* blk_list, float* dweight, int32_t* counter, int64_t n,
                                   int cin, int cout, int taps, int walk, int min_per, int max_workgroups, ss_stream_t stream);
int64_t ss_subm_conv_wgrad_pipe_items(int64_t n, int cin, int cout, int taps, int min_per);
int ss_subm_conv_wgrad_walk(const void* in, const void* dout, const int32_t* nbr, const int32_t* nbr_walk, const int32_t* rowperm,
                            const int32_t* blk_count, const int32_t* blk_list, float* dweight, int64_t n, int cin, int cout,
                            int taps, ss_stream_t stream);

/* ---- fused residual add (+ DropPath row scale) + LayerNorm (ptv3:318-338 seams) ------------------------
 * v = x + rowscale*y; xout = v (f32/bf16) [+ bf16 copy]; h = LN(v)*gamma+beta.  NULL = absent.  C % 4 == 0, C <= 1024. */
int ss_add_layernorm_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* rowscale,
                         const float* gamma, const float* beta, float eps, void* xout, int xout_dtype, void* xcopy_bf16,
                         void* h, int h_dtype, float* mean, float* rstd, int64_t n, int channels, ss_stream_t stream);
/* First seam of a pre-norm Block in one pass (ptv3:318-325): xout = x + LN0(t), h = LN1(xout).  stats (n,4) f32 = mean0, rstd0,
 * mean1, rstd1.  Backward: g_x = g_xout + LN1'(g_h), g_t = LN0'(g_x); part (4, nblocks, C) f32 = per-block partial sums of
 * dgamma0, dbeta0, dgamma1, dbeta1 (nblocks = ss_add_layernorm_bwd_blocks(n)); either of g_xout / g_h may be NULL. */
int ss_ln_add_ln_fwd(const void* x, int x_dtype, const void* t, int t_dtype, const float* gamma0, const float* beta0, float eps0,
                     const float* gamma1, const float* beta1, float eps1, float* xout, void* h, int h_dtype, float* stats,
                     int64_t n, int channels, ss_stream_t stream);
int ss_ln_add_ln_bwd(const float* g_xout, const void* g_h, int g_h_dtype, const float* xout, const void* t, int t_dtype,
                     const float* stats, const float* gamma0, const float* gamma1, void* g_x, int g_x_dtype, void* g_t,
                     int g_t_dtype, float* part, int64_t n, int channels, int nblocks, ss_stream_t stream);
int ss_add_layernorm_bwd_blocks(int64_t n);

/* ---- fused tail of a pre-norm Block at C in {32, 64, 128, 256}, hidden = 4C (ptv3:318-338): proj + residual + LN2 + fc1 + GELU +
 * fc2 + residual in ONE launch each way.  feat (n, C) bf16 = attention output, x (n, C) f32 = residual stream, rs1 / rs2 (n) f32
 * DropPath row scales or NULL; wp (C, C), w1 (4C, C), w2 (C, 4C) bf16 row-major; gamma / beta f32; the three biases all f32 or all
 * bf16 (bias_dtype SS_DTYPE_F32 | SS_DTYPE_BF16: the bf16 shadows today's GEMMs read), added in fp32 to the fp32 accumulator.
 *   y1 = bf16(feat wp^T + bp); x_mid = x + rs1 y1; h2 = bf16(LN(x_mid) gamma + beta); u = bf16(h2 w1^T + b1); a = bf16(gelu(u));
 *   y2 = bf16(a w2^T + b2); x_out = x_mid + rs2 y2 [+ bf16 copy, NULL = none].  Written: x_mid, mean, rstd, h2, u, a, x_out.
 * Backward: g = g_xout (+ g_xcopy); dy2 = bf16(rs2 g); da = bf16(dy2 w2); du = bf16(da gelu'(u)); dh2 = bf16(du w1);
 *   g_mid = g + LN'(dh2); dy1 = bf16(rs1 g_mid); dfeat = bf16(dy1 wp).  wp_t / w1_t / w2_t are the (in, out) copies of the weights.
 *   part (2, nblocks, C) f32 = per-workgroup partial sums of dgamma, dbeta with nblocks = ss_block_tail_bwd_blocks(n); no atomics.
 * One workgroup owns ss_block_tail_rows() rows.  Every tensor 16-byte aligned. */
int ss_block_tail_rows(void);
int ss_block_tail_bwd_blocks(int64_t n);
int ss_block_tail_fwd(const void* feat, const float* x, const float* rs1, const float* rs2, const void* wp, const void* bp,
                      const void* w1, const void* b1, const void* w2, const void* b2, int bias_dtype, const float* gamma, const float* beta,
                      float eps, float* x_mid, float* mean, float* rstd, void* h2, void* u, void* a, float* x_out,
                      void* xcopy_bf16, int64_t n, int channels, ss_stream_t stream);
int ss_block_tail_bwd(const float* g_xout, const void* g_xcopy_bf16, const float* x_mid, const float* mean, const float* rstd,
                      const void* u, const float* rs1, const float* rs2, const float* gamma, const void* wp_t, const void* w1_t,
                      const void* w2_t, float* g_mid, void* dfeat, void* dy2, void* du, void* dy1, float* part, int64_t n,
                      int channels, int nblocks, ss_stream_t stream);
/* Grouped launch reducing many partial-sum blocks (the dgamma / dbeta partials of a whole stage): desc 4 words {part (K, nb, C) f32,
 * dst (K*C) f32, nb, C | (K*C) << 32}; a workgroup owns ss_group_partial_sums_outputs_per_workgroup() of the K*C outputs;
 * dst[k*C + c] = sum_b part[k][b][c]. */
int ss_group_partial_sums_outputs_per_workgroup(void);
int ss_group_partial_sums(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
/* ss_transpose16_group: dst (cols, rows) = src (rows, cols)^T of 2-byte elements for many matrices in one grouped launch (transposed bf16
 * copies of nn.Linear weights: hipBLASLt's NT form of the dgrad GEMM dx = dy @ W, reference call site torch.nn.functional.linear backward
 * under point_transformer_v3m1_base.py:225-248).  desc 4 words {src, dst, rows, cols}; a workgroup owns one 64 x 64 tile (row-major over
 * ceil(rows / 64) x ceil(cols / 64)). */
int ss_transpose16_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
/* ss_subm_weight_mirror_group: ss_subm_weight_mirror for many conv weights in one grouped launch; desc 5 words {w, wt, cout, taps, cin};
 * a workgroup owns one (tap, T x T) tile of (cout x cin) with T = ss_subm_weight_mirror_group_tile(): taps * ceil(cout / T) *
 * ceil(cin / T) workgroups per problem. */
int ss_subm_weight_mirror_group_tile(void);
int ss_subm_weight_mirror_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
/* g_v = g_xout + g_xcopy + LN'(g_h); g_x = g_v; g_y = rowscale*g_v; dgamma/dbeta partials (nblocks, C) */
int ss_add_layernorm_bwd(const void* g_xout, int g_xout_dtype, const void* g_xcopy, int g_xcopy_dtype, const void* g_h,
                         int g_h_dtype, const void* v, int v_dtype, const float* mean, const float* rstd,
                         const float* gamma, const float* rowscale, void* g_x, int g_x_dtype, void* g_y, int g_y_dtype,
                         float* dgamma_part, float* dbeta_part, int64_t n, int channels, int nblocks, ss_stream_t stream);

/* ---- fused BatchNorm1d (+ exact GELU when act = 1) over (n, C) rows; mean/rstd per channel from the caller --------
 * ss_col_stats: per-block partial column sums of (x - shift) and (x - shift)^2 -> psum/psq (nblocks, C), with shift = row 0 of x
 * (a value of the batch conditions the one-pass variance whatever the column means are); shift_out (C f32, may be NULL) receives it */
int ss_col_stats(const void* x, int x_dtype, float* shift_out, float* psum, float* psq, int64_t n, int channels,
                 int nblocks, ss_stream_t stream);
/* ss_bn_stats_finish: (psum, psq) partials of ss_col_stats (stored as part (2, nblocks, C)) and its shift_out (NULL: the sums are
 * of plain x) -> batch mean = shift + s/n, rstd = rsqrt(q/n - (s/n)^2 + eps) and, when
 * running_mean / running_var are given, nn.BatchNorm1d's training-mode update (momentum, unbiased variance; reference:
 * torch.nn.BatchNorm1d as used by pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py:499-506,385-386);
 * num_batches (int64, may be NULL) is incremented.  ss_bn_bwd_finish: partials of ss_bn_act_bwd_reduce -> sums (2, C) =
 * (sum dz, sum dz*xhat) and coef (2, C) = sums / n (NULL in eval mode). */
int ss_bn_stats_finish(const float* part, const float* shift, int nblocks, int channels, int64_t n, float momentum, float eps,
                       float* running_mean, float* running_var, int64_t* num_batches, float* mean, float* rstd,
                       ss_stream_t stream);
int ss_bn_bwd_finish(const float* part, int nblocks, int channels, int64_t n, float* sums, float* coef, ss_stream_t stream);
int ss_bn_act_fwd(const void* x, int x_dtype, const float* mean, const float* rstd, const float* gamma, const float* beta,
                  int act, void* y, int y_dtype, int64_t n, int channels, ss_stream_t stream);
int ss_bn_act_bwd_reduce(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, int act, float* pdz, float* pdzx, int64_t n, int channels,
                         int nblocks, ss_stream_t stream);
int ss_bn_act_bwd_apply(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int act, const float* c1, const float* c2, void* dx,
                        int dx_dtype, int64_t n, int channels, ss_stream_t stream);

/* ---- open-vocabulary scan (evaluator.py:793-800, test.py:335-351) ----------------------------------------
 * feat (n, dim) bf16 unit rows, text (num_classes <= 256, dim) bf16.  max_prob/argmax (n) = max / arg-max of
 * sigmoid(feat text^T) (ties: lowest class), and/or pred_accum[idx ? idx[i] : i][c] += sigmoid(logit). */
int ss_feat_text_scan(const void* feat_bf16, const void* text_bf16, int64_t n, int dim, int num_classes, float* max_prob,
                      int32_t* argmax, const int32_t* idx, float* pred_accum, ss_stream_t stream);

/* ---- vision-language distillation head (models/default.py:98-109; losses/misc.py:254-295) ----------------
 * One pass over feat / target (n, C) rows, C % 4 == 0, C <= 2048, dtypes SS_DTYPE_*:
 *   p = feat / max(|feat|, 1e-12) when normalize (else p = feat); p_out optional (NULL to skip);
 *   sums (3) f32 = [ sum_valid (1 - cos(p, t)), sum_valid |p - t|^2, #valid ], cos with eps 1e-8 on each norm
 *   (torch.nn.CosineSimilarity); mask (n) bytes, non-zero = valid.  target NULL: normalisation only (mask, part,
 *   sums unused).  rowstat (n, 4) f32 is kept for the backward; part = ss_lang_head_blocks(n) * 3 floats of scratch.
 * Backward: coef (2) f32 DEVICE values dL/dsums[0..1]; dp_extra optional gradient arriving at p from other
 *   consumers (the contrastive loss); dfeat (n, C).
 * n == 0 is a no-op each way (the forward clears sums when given), also with the NULL data pointers of empty tensors;
 *   the width is checked first. */
int ss_lang_head_blocks(int64_t n);
int ss_lang_head_fwd(const void* feat, int feat_dtype, const void* target, int target_dtype, const unsigned char* mask,
                     int normalize, void* p_out, int p_dtype, float* rowstat, float* part, float* sums, int64_t n,
                     int channels, ss_stream_t stream);
int ss_lang_head_bwd(const void* feat, int feat_dtype, const void* target, int target_dtype, const unsigned char* mask,
                     int normalize, const float* rowstat, const float* coef, const void* dp_extra, int dp_dtype,
                     void* dfeat, int dfeat_dtype, int64_t n, int channels, ss_stream_t stream);

/* ---- semantic segmentation: CrossEntropyLoss + multiclass Lovasz-softmax, and the evaluator's counts (csrc/seg_loss.hip) -------
 * logits (n, C) SS_DTYPE_*, C <= 256; labels (n) int64; a row is valid when its label != ignore_index and lies in [0, C) (the caller
 * asserts the range).  All arithmetic fp32, no float atomics: two runs give bitwise-equal results.
 * Forward: rowstat (n, 2) f32 = per-row max and sum of exp (kept for the backward); sums (4) f32 = [sum over valid rows of
 *   -log softmax[label], #valid, sum over contributing classes of the Lovasz loss, #contributing classes].  A class contributes when
 *   it has a valid foreground row and class_seen (C bytes, NULL = all) marks it.  lovasz = 0 skips the Lovasz part (glov / present
 *   unused, sums[2..3] = 0); else glov (C, n) f32 = the Lovasz gradient with respect to each error (rows of non-contributing classes
 *   are not written) and present (C) int32 = the contributing flags.  lovasz needs C * n < 2^31.  Workspace from the query.
 * Backward: coef (2) f32 DEVICE values = dL/dsums[0], dL/dsums[2]; dlogits (n, C) in the logits' dtype (glov NULL: CE only).
 * ss_seg_iou: out (3, C) int64 = [intersection, union, target] of intersection_and_union_gpu(pred, target, C, ignore_index), with
 *   pred = the arg-max of the logits (equal maxima: the lowest class) or the given pred (n) int32. */
size_t ss_seg_loss_workspace_bytes(int64_t n, int num_classes);
int ss_seg_loss_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int num_classes, int64_t ignore_index,
                    const unsigned char* class_seen, int lovasz, float* rowstat, float* glov, int32_t* present, float* sums,
                    void* workspace, size_t workspace_bytes, ss_stream_t stream);
int ss_seg_loss_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int num_classes, int64_t ignore_index,
                    const float* rowstat, const float* glov, const int32_t* present, const float* coef, void* dlogits,
                    ss_stream_t stream);
int ss_seg_iou(const void* logits, int dtype, const int32_t* pred, const int64_t* target, int64_t n, int num_classes,
               int64_t ignore_index, int64_t* out, ss_stream_t stream);

/* ---- row movement ------------------------------------------------------------------------ */
int ss_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_dst, int64_t row_bytes, ss_stream_t stream);
int ss_scatter_rows(const void* src, const int32_t* idx, void* dst, int64_t n_src, int64_t row_bytes, ss_stream_t stream);
int ss_gather_add_rows(const void* a, const void* b, const int32_t* idx, void* dst, int64_t n, int channels, int dtype,
                       ss_stream_t stream);
/* Duplicate voxels: adjoint of "every site of a voxel reads the voxel's winner (lowest) row" -- the fold in front of a submanifold
 * conv's dgrad (structure.py:104-140 / spconv pairs with Mix3D-merged batch elements).  sorted_keys (n) = the codes of one curve in
 * sorted order, order (n) = its stable argsort (ss_argsort_i64): runs of equal keys list a voxel's rows ascending.
 * dst[winner] = sum of src over the run (fp32 accumulate, run order), dst[every other row] = 0; src != dst; row bytes % 16 == 0. */
int ss_dup_fold_rows(const void* src, const int64_t* sorted_keys, const int32_t* order, void* dst, int64_t n, int channels,
                     int dtype, ss_stream_t stream);
/* x[row] = 0 for every row that is not the winner of its voxel (in place) */
int ss_dup_zero_rows(const int64_t* sorted_keys, const int32_t* order, void* x, int64_t n, int64_t row_bytes, ss_stream_t stream);
int ss_segment_reduce(const void* src, const int32_t* indices, const int32_t* idx_ptr, void* out, int64_t n_seg,
                      int channels, int dtype, int mean, ss_stream_t stream);
/* reduce = "min" / "max" of torch_scatter.segment_csr: out (n_seg,C) and arg (n_seg,C) int32 = source row attaining it
 * (NULL to skip; -1 for an empty segment, whose out is 0).  Backward: dsrc (ZEROED) [arg[s][c]][c] = dout[s][c]. */
int ss_segment_minmax(const void* src, const int32_t* indices, const int32_t* idx_ptr, void* out, int32_t* arg, int64_t n_seg,
                      int channels, int dtype, int is_max, ss_stream_t stream);
int ss_segment_minmax_bwd(const void* dout, const int32_t* arg, void* dsrc, int64_t n_seg, int channels, int dtype,
                          ss_stream_t stream);
int ss_segment_bcast(const void* dout, const int32_t* cluster, const int32_t* idx_ptr, void* dsrc, int64_t n,
                     int channels, int dtype, int mean, ss_stream_t stream);


/* ---- per-sample Gaussian augmentations (csrc/augment.hip) ------------------------------------------------------------------
 * One pass over HBM each, fp32, in place.  Pointers named `h_*` are HOST pointers to a few floats that travel as kernel arguments
 * (NULL = that part is off); everything else is a device pointer. */
/* out6 = {min x, min y, min z, max x, max y, max z} of A x + b (h_affine = A row-major (9) then b (3)) or of x itself (h_affine
 * NULL: exact).  Deterministic: per-block partials (ss_aug_bbox_blocks(n) * 6 floats) and a finish step, no atomics.  n >= 1. */
int ss_aug_bbox_blocks(int64_t n);
int ss_aug_bbox(const float* x, int64_t n, const float* h_affine, float* partials, float* out6, ss_stream_t stream);
/* The fused rigid pass of CenterShift / RandomRotate / RandomScale / RandomShift / RandomFlip / RandomJitter.  coord (n,3), quat (n,4,
 * wxyz), scale (n,3), normal (n,3): each optional (NULL = absent).
 *   coord  <- A x + b (h_affine; NULL = identity), then + clip(sigma * N(0,1), +-clip) per component when jitter != 0: N from
 *             noise (n,3) when given, else Philox4x32-10 keyed by seed with the point index as counter (Box-Muller)
 *   quat   <- normalise, r (x) q (h_rquat, unit, wxyz; Hamilton product), then for flip (bit 0: x, bit 1: y) the conjugation
 *             F R F = (w, x, -y, -z) | (w, -x, y, -z) | (w, -x, -y, z) and the sign that scipy's Rotation.from_matrix gives: the
 *             component that wins arg-max [M00, M11, M22, trace] (for a unit quaternion: the first largest of x^2, y^2, z^2, w^2)
 *             is made positive.  Rows of zero norm are left unchanged.
 *   scale  <- scale * h_scale_mul (3)
 *   normal <- L normal (h_lin, row-major 9: rotation and reflection only) */
int ss_aug_gaussians(float* coord, float* quat, float* scale, float* normal, int64_t n, const float* h_affine,
                     const float* h_rquat, int flip, const float* h_scale_mul, const float* h_lin, int jitter, float jitter_sigma,
                     float jitter_clip, const float* noise, uint64_t seed, ss_stream_t stream);
/* ElasticDistortion's application: coord += trilinear(noise, coord) * magnitude; noise (d0,d1,d2,3), node i of an axis at
 * origin + i * granularity, 0 outside the grid */
int ss_aug_elastic(float* coord, int64_t n, const float* noise, int d0, int d1, int d2, const float* h_origin, float granularity,
                   float magnitude, ss_stream_t stream);
/* color (n,3) on the 0..255 scale.  flags bit 0: c <- (1 - blend) c + blend (c - lo) 255 / (hi - lo); bit 1: c <- clip(c + tr, 0, 255);
 * bit 2: c <- clip(c + N * jitter_std * 255, 0, 255), N from noise (n,3) or Philox (as above); then normalize != 0: c / 127.5 - 1 */
int ss_aug_color(float* color, int64_t n, int flags, const float* h_lo, const float* h_hi, float blend, const float* h_tr,
                 float jitter_std, const float* noise, uint64_t seed, int normalize, ss_stream_t stream);
/* HueSaturationTranslation (transform.py:1037-1100) on color (n,3), fp32 on the 0..255 scale, in place; h_hue_sat = 2 HOST doubles
 * {hue_val, sat_ratio} (doubles travel behind a host pointer: the ABI has no double by value).  Per point, in fp64, uncontracted
 * and in the reference's operation order, with IEEE division:
 *   rgb -> hsv   v = max, s = (max - min) / max, h = ((bc - gc | 2 + rc - bc | 4 + gc - rc) / 6) % 1 by the ordered branches
 *                r == max, else g == max, else b; xc = (max - x) / (max - min); max == min gives h = s = 0
 *   shift        h <- (hue_val + h + 1) % 1, s <- clip(sat_ratio * s, 0, 1); a % 1 is numpy's: fmod, + 1 when negative, and may
 *                round to exactly 1.0 (sector 6 = sector 0)
 *   hsv -> rgb   i = uint8(h * 6), f = h * 6 - i, p = v (1 - s), q = v (1 - s f), t = v (1 - s (1 - f)); s == 0: (v, v, v), else by
 *                i % 6: 1 (q,v,p)  2 (p,v,t)  3 (p,q,v)  4 (t,p,v)  5 (v,p,q)  0 (v,t,p)
 * and writes the results truncated to integers (the reference's astype("uint8")) back as fp32.  Inputs are on 0..255; outside that
 * range numpy's cast is undefined and this one saturates to 0 / 255 (NaN -> 0). */
int ss_aug_hsv(float* color, int64_t n, const double* h_hue_sat, ss_stream_t stream);
/* NormalizeCoord's reductions over p = A x + b (h_affine = 12 HOST doubles, A row-major then b; NULL: p = x), x (n,3) fp32, in fp64:
 * out4 = {sum p_x, sum p_y, sum p_z, max |p|^2}, p_i = ((a_i0 x + a_i1 y) + a_i2 z) + b_i and |p|^2 = (p_x^2 + p_y^2) + p_z^2 without
 * contraction, so the maximum is bit-equal to that expression in numpy.  Deterministic: per-block partials (ss_aug_moments_blocks(n) * 4
 * doubles) and a one-wave finish, no atomics.  n >= 1. */
int ss_aug_moments_blocks(int64_t n);
int ss_aug_moments(const float* x, int64_t n, const double* h_affine, double* partials, double* out4, ss_stream_t stream);
/* InstanceParser (transform.py:1626-1664).  order / idx_ptr / cluster: what ss_argsort_i64 (stable) and ss_pool_partition wrote for the
 * rows' instance ids, the rows to ignore keyed past every id: run k < K is instance k and holds rows order[idx_ptr[k] .. idx_ptr[k+1]),
 * ascending.
 * ss_instance_boxes: one workgroup per instance; bbox (K,8) = {(max + min) / 2 (3), max - min (3), 0, class} in fp32 with exact min /
 *   max, class = segment[first row of the run] - #{v in h_vacancy : class > v} (h_vacancy: num_vacancy <= 16 HOST int64, the non-negative
 *   segment ignore indices); centroid (K,3) = the fp64 sum of the run's coordinates in a fixed tree order / count, rounded once to fp32.
 *   segment (int64) and coord (n,3) are indexed by row.  K == 0: SS_OK without a launch.
 * ss_instance_scatter: per row, instance[row] (int64 when instance_is_i64, else int32) <- cluster[row] and instance_centroid[row] <-
 *   centroid[cluster[row]]; rows of a run >= K get ignore_index in both.  K == 0: every row does (cluster / centroid not looked at). */
int ss_instance_boxes(const float* coord, const int64_t* segment, const int32_t* order, const int32_t* idx_ptr, int64_t K,
                      const int64_t* h_vacancy, int num_vacancy, float* bbox, float* centroid, ss_stream_t stream);
int ss_instance_scatter(const int32_t* cluster, int64_t n, int64_t K, const float* centroid, void* instance, int instance_is_i64,
                        int64_t ignore_index, float* instance_centroid, ss_stream_t stream);
/* GridSample(apply_to_pc=True) over the point cloud beside the Gaussians (transform.py:1245-1253).  order / idx_ptr: the CSR that
 * ss_pool_partition wrote over a stable argsort of the cell keys (cell c holds rows order[idx_ptr[c] .. idx_ptr[c+1]), ascending).
 * chosen[c] = the first of them whose label (int64, indexed by row) differs from ignore_index; the first member when the cell has
 * none or label is NULL.  n_cells == 0: SS_OK without a launch (pointers are not looked at). */
int ss_voxel_pick_labelled(const int32_t* order, const int32_t* idx_ptr, int64_t n_cells, const int64_t* label,
                           int64_t ignore_index, int32_t* chosen, ss_stream_t stream);

/* ---- the self-supervised view generator's colour and blur transforms (csrc/ssl_views.hip) -----------------------------------------
 * RandomColorJitter / RandomColorGrayScale (transform.py:820-1032) as ONE pass over color (n,3), fp32 on the 0..255 scale, in place.
 * h_codes / h_factors: num_steps <= 8 HOST (code, factor) pairs applied per point in the given order:
 *   1 brightness  c <- clip(f c, 0, 255)
 *   2 contrast    c <- clip(f c + (1 - f) mean, 0, 255), mean = the mean over all n points of 0.2989 r + 0.587 g + 0.114 b of the colours
 *                 as they are when the step is reached
 *   3 saturation  the same blend against the point's own gray
 *   4 hue         rgb / 255 -> hsv (ties: maxc == r, then maxc == g), h <- (h + f) mod 1 (non-negative), hsv -> rgb * 255; p, q, t are
 *                 clipped to [0, 1], v and the result are not; -0.5 <= f <= 0.5; evaluated in fp64 as the reference's promotion has it
 *   5 grayscale   r, g, b <- gray (the factor is ignored)
 * Each contrast step costs one reduction pass that re-applies the steps in front of it in registers and writes nothing to color: per-block
 * partials (ss_color_chain_blocks(n) floats) and a one-wave fp64 finish, no atomics, the same bits on every run.  The means stay in
 * `means` (8 floats, device; slot k belongs to step k) for the apply pass: no readback.  partials / means may be NULL without a contrast step. */
int ss_color_chain_blocks(int64_t n);
int ss_color_chain(float* color, int64_t n, int num_steps, const int* h_codes, const float* h_factors, float* partials, float* means,
                   ss_stream_t stream);
/* GSGaussianBlurVoxelOpc (transform.py:60-176) without the dense grid.  grid_coord (n,3) int32, unique rows, any origin; mask (n) bytes
 * (NULL = every row).  The masked voxels go into an open-addressing hash (ss_voxel_blur_table_size(n) slots >= 2 n); every masked row then
 * sums w(dx) w(dy) w(dz) * value and w(dx) w(dy) w(dz) over the (2r+1)^3 neighbours that are masked voxels, r = int(2 sigma + 0.5) <= 8,
 * w(x) = exp(-x^2 / 2 sigma^2) / sum w (scipy's kernel at truncate = 2.0), indices outside [0, size) folded back by scipy's `reflect` rule
 * with size = max - min + 1 of grid_coord over ALL rows (a device reduction), and is overwritten by sum / (wsum + 1e-7), accumulated in
 * fp64.  color (n,3) always; opacity (n,1), scale (n,3), quat (n,4), normal (n,3) when not NULL.  normalize_quat != 0: afterwards EVERY
 * row of quat is divided by its norm (rows of zero norm are left as they are).  No readback, O(n) workspace; its int32 word 6 is a status
 * the caller may look at: != 0 when an axis spans 2^21 cells or more, in which case nothing was blurred. */
int64_t ss_voxel_blur_table_size(int64_t n);
size_t ss_voxel_blur_workspace_bytes(int64_t n);
int ss_voxel_blur(const int32_t* grid_coord, const uint8_t* mask, int64_t n, float* color, float* opacity, float* scale, float* quat,
                  float* normal, int normalize_quat, float sigma, void* workspace, size_t workspace_bytes, ss_stream_t stream);

/* ---- SimDINO pretraining model (csrc/ssl_model.hip; pointcept/models/simdinov2.py:191-302, point_transformer_v3m1_ssl.py:733-737) ----
 * Mask generator.  offset (num_batches) int32 = inclusive row ends of the samples, num_batches <= ss_mask_max_samples().
 * ss_mask_keys: keys[i] = sample | z | y | x (ss_mask_key_bits() bits) of cell = floor(float(grid_coord) / mask_grid_size), IEEE divide;
 *   sorting them orders a sample's cells as torch_cluster's grid index does (x fastest).  status[0] is set to 1 when a cell leaves
 *   [0, 2^17) (the caller zeroes it and reads it with the patch counts).
 * ss_mask_patches: cluster / n_out as ss_pool_partition wrote them over a stable argsort `order` of the keys -> patch_start
 *   (num_batches + 1), patch_count (num_batches), patch_id (n) = rank of the row's cell among the occupied cells of its sample.
 * ss_mask_select: mask[i] = selected[patch_start[b] + patch_id[i]] (patch_id NULL: selected[i], the `splats` mode); index = the masked
 *   rows ascending, weight[j] = sample_weight[sample of index[j]] (fp16 bits), count[0] = how many; index / weight have capacity n,
 *   block_counts ss_mask_select_blocks(n) int32.  Ordered three-pass compaction: no atomics. */
int ss_mask_max_samples(void);
int ss_mask_key_bits(void);
int ss_mask_keys(const int32_t* grid_coord, const int32_t* offset, int num_batches, int64_t n, float mask_grid_size, int64_t* keys,
                 int32_t* status, ss_stream_t stream);
int ss_mask_patches(const int32_t* cluster, const int32_t* order, const int32_t* offset, int num_batches, int64_t n, const int32_t* n_out,
                    int32_t* patch_start, int32_t* patch_count, int32_t* patch_id, ss_stream_t stream);
int ss_mask_select_blocks(int64_t n);
int ss_mask_select(const uint8_t* selected, const int32_t* patch_id, const int32_t* patch_start, const int32_t* offset, int num_batches,
                   int64_t n, const uint16_t* sample_weight, uint8_t* mask, int32_t* index, uint16_t* weight, int32_t* count,
                   int32_t* block_counts, ss_stream_t stream);
/* Mask token.  x / out / g / dx (n, channels) f32 or bf16 (dtype), mask (n) bytes, token (channels) f32.
 * fwd: out[i] = mask[i] ? token : x[i].  bwd: dx[i] = mask[i] ? 0 : g[i]; dtoken[c] = sum of the masked g[i][c] in fp32: workgroup w of
 * ss_mask_token_bwd_blocks(n) owns ss_mask_token_bwd_span(n) consecutive rows, 256 / channels row slots add every (256 / channels)-th row
 * in order, the slots are added in order, then the workgroups in order (partial: blocks x channels floats).  channels <= 256. */
int ss_mask_token_fwd(const void* x, int dtype, const uint8_t* mask, const float* token, int64_t n, int channels, void* out,
                      ss_stream_t stream);
int ss_mask_token_bwd_blocks(int64_t n);
int64_t ss_mask_token_bwd_span(int64_t n);
int ss_mask_token_bwd(const void* g, int dtype, const uint8_t* mask, int64_t n, int channels, void* dx, float* partial, float* dtoken,
                      ss_stream_t stream);
/* Grouped EMA of the teacher: t = (m * t) + (alpha * s) for every pair in one launch, each product and the sum rounded to fp32
 * (torch._foreach_mul_ + torch._foreach_add_(alpha=)).  desc 4 words {t, s f32 pointers, numel, flags}; workgroup size and flags
 * as ss_adamw_group. */
int ss_ema_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, float m, float alpha, ss_stream_t stream);

/* ---- libs/pointops, pointops2, pointgroup_ops (fp32 features, int32 indices, offset batches) ------- */
/* libs/pointops/src/knn_query/knn_query_cuda.cpp:7-16; nsample <= 128; idx -1 / dist2 1e10 padding */
int ss_knn_query(int m, int nsample, const float* xyz, const float* new_xyz, const int32_t* offset,
                 const int32_t* new_offset, int num_batches, int32_t* idx, float* dist2, ss_stream_t stream);
size_t ss_ball_query_workspace_bytes(int m);
int ss_ball_query(int m, int nsample, float min_radius, float max_radius, const float* xyz, const float* new_xyz,
                  const int32_t* offset, const int32_t* new_offset, int num_batches, int32_t* idx, float* dist2,
                  void* workspace, size_t workspace_bytes, ss_stream_t stream);
int ss_random_ball_query(int m, int nsample, float min_radius, float max_radius, const int32_t* order, const float* xyz,
                         const float* new_xyz, const int32_t* offset, const int32_t* new_offset, int num_batches,
                         int32_t* idx, float* dist2, ss_stream_t stream);
/* tmp (n) f32 initialised to 1e10 by the caller (libs/pointops/functions/sampling.py:19) */
int ss_farthest_point_sampling(int num_batches, const float* xyz, const int32_t* offset, const int32_t* new_offset,
                               float* tmp, int32_t* idx, ss_stream_t stream);
int ss_grouping_fwd(int m, int nsample, int c, const float* input, const int32_t* idx, float* output, ss_stream_t stream);
int ss_grouping_bwd(int m, int nsample, int c, const float* grad_output, const int32_t* idx, float* grad_input, ss_stream_t stream);
int ss_subtraction_fwd(int n, int nsample, int c, const float* input1, const float* input2, const int32_t* idx, float* output, ss_stream_t stream);
int ss_subtraction_bwd(int n, int nsample, int c, const int32_t* idx, const float* grad_output, float* grad_input1, float* grad_input2, ss_stream_t stream);
int ss_aggregation_fwd(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int32_t* idx, float* output, ss_stream_t stream);
int ss_aggregation_bwd(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int32_t* idx, const float* grad_output, float* grad_input, float* grad_position, float* grad_weight, ss_stream_t stream);
int ss_interpolation_fwd(int n, int c, int k, const float* input, const int32_t* idx, const float* weight, float* output, ss_stream_t stream);
int ss_interpolation_bwd(int n, int c, int k, const float* grad_output, const int32_t* idx, const float* weight, float* grad_input, ss_stream_t stream);
/* weight == NULL: pointops2 attention_step1 (q . k per edge and head) */
int ss_attention_relation_fwd(int m, int g, int c, const float* query, const float* key, const float* weight, const int32_t* index_target, const int32_t* index_refer, float* output, ss_stream_t stream);
int ss_attention_relation_bwd(int m, int g, int c, const float* query, float* grad_query, const float* key, float* grad_key, const float* weight, float* grad_weight, const int32_t* index_target, const int32_t* index_refer, const float* grad_output, ss_stream_t stream);
/* == pointops2 attention_step2; output / grad_value / grad_* are ACCUMULATED into (caller zeroes) */
int ss_attention_fusion_fwd(int m, int g, int c, const float* weight, const float* value, const int32_t* index_target, const int32_t* index_refer, float* output, ss_stream_t stream);
int ss_attention_fusion_bwd(int m, int g, int c, const float* weight, float* grad_weight, const float* value, float* grad_value, const int32_t* index_target, const int32_t* index_refer, const float* grad_output, ss_stream_t stream);
int ss_rpe_dot_prod_fwd(int n, int m, int h, int hdim, const float* q, const int32_t* index, const float* table, const int32_t* rel_idx, float* output, ss_stream_t stream);
int ss_rpe_dot_prod_bwd(int n, int m, int h, int hdim, const float* grad_out, const float* q, const int32_t* index, const float* table, const int32_t* rel_idx, float* grad_q, float* grad_table, ss_stream_t stream);
int ss_rpe_attn_step2_fwd(int n, int m, int h, int hdim, const float* attn, const float* v, const int32_t* index0, const int32_t* index1, const float* table, const int32_t* rel_idx, float* output, ss_stream_t stream);
int ss_rpe_attn_step2_bwd(int n, int m, int h, int hdim, const float* grad_out, const int32_t* index0, const int32_t* index1, const float* attn, const float* v, const float* table, const int32_t* rel_idx, float* grad_attn, float* grad_v, float* grad_table, ss_stream_t stream);
/* Exact kNN on a uniform hash grid (csrc/knn_grid.hip): the result of ss_knn_query -- libs/pointops/src/knn_query/
 * knn_query_cuda_kernel.cu:60-104, called by the zero-shot evaluator's neighbour voting with k = 25 over ~10^6 Gaussians
 * (pointcept/engines/hooks/evaluator.py:697-739; the reference runs scipy's cKDTree on the CPU there) -- without the O(m n) scan.
 *   1. ss_knn_grid_keys      keys[i] = batch << 48 | cx << 32 | cy << 16 | cz, cell = floor((p - origin) / cell_size) clamped to 16 bits
 *   2. ss_argsort_i64        (sorted keys, order)
 *   3. ss_knn_grid_build     workspace <- hash table key -> [start, end) + the points in cell order; ncell (1) = occupied cells
 *   4. ss_knn_grid_query     one wave per query, rings of cells until the k-th distance is inside the searched region; nsample <= 64.
 * qorder (m) or NULL = processing order of the queries; dim* = the largest cell index of the data per axis. */
int64_t ss_knn_grid_table_size(int64_t n);
size_t ss_knn_grid_workspace_bytes(int64_t n);
int ss_knn_grid_keys(const float* xyz, const int32_t* offset, int num_batches, int64_t n, float origin_x, float origin_y, float origin_z,
                     float cell_size, int64_t* keys, ss_stream_t stream);
int ss_knn_grid_build(const float* xyz, const int64_t* sorted_keys, const int32_t* order, int64_t n, void* workspace,
                      size_t workspace_bytes, int32_t* ncell, ss_stream_t stream);
int ss_knn_grid_query(int m, int nsample, const float* new_xyz, const int32_t* qorder, const int32_t* offset, const int32_t* new_offset,
                      int num_batches, float origin_x, float origin_y, float origin_z, float cell_size, int dimx, int dimy, int dimz,
                      int64_t n, const void* workspace, int32_t* idx, float* dist2, ss_stream_t stream);
/* ss_ball_query's result on the grid built by ss_knn_grid_build (libs/pointops/src/ball_query/ball_query_cuda_kernel.cu:58-123): one wave
 * per query collects the candidates of the cells within the ball's reach into LDS, sorts them there and writes all of them or the
 * strided subsample; max_radius <= 8 cells.  xyz = the original coordinates (crowded balls fall back to the index-order rule). */
int ss_ball_grid_query(int m, int nsample, float min_radius, float max_radius, const float* xyz, const float* new_xyz,
                       const int32_t* qorder, const int32_t* offset, const int32_t* new_offset, int num_batches, float origin_x,
                       float origin_y, float origin_z, float cell_size, int dimx, int dimy, int dimz, int64_t n, const void* workspace,
                       int32_t* idx, float* dist2, ss_stream_t stream);
/* neighbour majority vote of the zero-shot evaluator (pointcept/utils/misc.py:17-51): ties -> smallest label, k <= 64 */
int ss_majority_vote(const int32_t* nn_idx, const int32_t* labels, int64_t m, int k, int ignore_label, int num_classes,
                     int32_t* out, ss_stream_t stream);
/* ---- open-vocabulary test stage, after the fragment accumulation (csrc/tester.hip) -------------------------------------------
 * ss_vocab_finish: pointcept/engines/test.py:372-394 in one pass over pred (n, C) f32, 1 <= C <= 256, 1 <= k <= min(C, 8).
 *   labels (n, k)  the k classes of a row by descending value, equal values: the lower class first (16 lanes per row).  k == 1: a
 *                  row whose maximum is < threshold (strict) gives ignore_index; k > 1: no threshold (the ScanNet++ top-3 form).
 *   lut            (C + 1) int32 or NULL: entry 0 = the image of ignore_index, entry c + 1 = the image of class c (pred_label_mapping)
 *   out (m, k)     out[j, :] = labels[inverse[j], :]; inverse (m) int64 or NULL (m = n, labels are written to out directly).
 * pred is read once whatever m is; the workspace holds the (n, k) labels when inverse is given.  n == 0 or m == 0: no-op. */
size_t ss_vocab_finish_workspace_bytes(int64_t n, int k, int64_t m);
int ss_vocab_finish(const float* pred, int64_t n, int num_classes, int k, float threshold, int32_t ignore_index,
                    const int64_t* inverse, int64_t m, const int32_t* lut, int32_t* out, void* workspace,
                    size_t workspace_bytes, ss_stream_t stream);
/* ss_cluster_vote: clustering_voting (pointcept/utils/misc.py:98-125).  instance_dense[i] in [0, num_instances) or < 0 = no instance
 * (the row keeps its pred); pred[i] in {ignore_index} U [0, num_classes), num_classes <= 256.  Every row of an instance gets the
 * instance's most frequent pred value; ignore_index counts as a value like any other, and on equal counts the numerically smallest
 * value wins (np.unique sorts, argmax takes the first).  Integer counters: exact and reproducible. */
size_t ss_cluster_vote_workspace_bytes(int num_instances, int num_classes);
int ss_cluster_vote(const int32_t* pred, const int32_t* instance_dense, int64_t m, int num_instances, int num_classes,
                    int32_t ignore_index, int32_t* out, void* workspace, size_t workspace_bytes, ss_stream_t stream);
/* libs/pointgroup_ops/src/bfs_cluster.cpp:140-145.  total (1) device int = number of pairs found */
int ss_ballquery_batch_p(int n, int mean_active, float radius, const float* xyz, const int32_t* batch_idxs, const int32_t* batch_offsets, int32_t* idx, int32_t* start_len, int32_t* total, ss_stream_t stream);
/* HOST pointers (CPU BFS, as the reference) */
int ss_bfs_cluster(const int32_t* semantic_label, const int32_t* ball_query_idxs, const int32_t* start_len, int n, int threshold, int32_t* cluster_idxs, int64_t cap_points, int32_t* cluster_offsets, int64_t cap_clusters, int32_t* n_clusters, int32_t* n_points);

/* ---- scene chunking (csrc/chunking.hip; pointcept/datasets/preprocessing/sampling_chunking_data_gs.py::chunking_scene) ----------
 * The steps of chunking_scene over a scene arena on the device, values as numpy's bit for bit where the reference is deterministic.
 * ss_chunk_extent: out6 = {min x, y, z, max x, y, z} of the rows x[idx[i]] (idx NULL: x[i]) of x (., 3) f32, i < m, m >= 1.
 *   Deterministic: per-block partials (ss_chunk_extent_blocks(m) * 6 floats), then a finish step; no atomics.  NaN is skipped.
 * ss_chunk_recentre: out[i][c] = coord[i][c] - ext6[c], one correctly rounded fp32 subtraction (ext6 is read on the device). */
int ss_chunk_extent_blocks(int64_t m);
int ss_chunk_extent(const float* x, const int32_t* idx, int64_t m, float* partials, float* out6, ss_stream_t stream);
int ss_chunk_recentre(const float* coord, const float* ext6, int64_t n, float* out, ss_stream_t stream);
/* lang_feat[valid == 1] /= norm(lang_feat[valid == 1], axis=1): rows (n, width) of dtype SS_CHUNK_F16 | SS_CHUNK_F32, in place; valid (n)
 * bytes, a row is touched when its byte is non-zero.  One wave per row: fp32 sum of squares (lane l adds elements l, l + 64, ... in
 * order, then a 6-level butterfly), correctly rounded sqrt and division, ONE rounding to the storage dtype.  A valid all-zero row
 * becomes NaN, as in numpy. */
enum { SS_CHUNK_F16 = 2, SS_CHUNK_F32 = 1 };
int ss_chunk_lang_normalize(void* feat, int dtype, const uint8_t* valid, int64_t n, int width, ss_stream_t stream);
/* Grid subsample.  ss_chunk_cell_keys: keys[i] = cx << (bits_y + bits_z) | cy << bits_z | cz with c = floor(x / grid_size), a correctly
 * rounded fp32 division of the recentred coordinate.  bits_* >= 1; their sum above 63, or grid_size <= 0: SS_ERR_ARG.  status[0]
 * (caller-zeroed int32) is set to 1 when a cell falls outside [0, 2^bits) of its axis (its key is then 0).
 * ss_chunk_cell_pick: order / idx_ptr = the CSR that ss_pool_partition wrote over a stable argsort of the keys (cell c holds rows
 *   order[idx_ptr[c] .. idx_ptr[c+1]), ascending).  first[c] = the cell's smallest row (int64: the key of the sort that puts the cells
 *   in first-occurrence order); pick[c] = that row when valid is NULL or the cell has no valid row, else its valid row number
 *   Philox4x32-10(key = seed; counter = {first[c] low, first[c] high, 0x43484e4b, 0}) word 0 mod n_valid, counted in ascending row order. */
int ss_chunk_cell_keys(const float* rec, int64_t n, float grid_size, int bits_x, int bits_y, int bits_z, int64_t* keys,
                       int32_t* status, ss_stream_t stream);
int ss_chunk_cell_pick(const int32_t* order, const int32_t* idx_ptr, int64_t n_cells, const uint8_t* valid, uint64_t seed,
                       int64_t* first, int32_t* pick, ss_stream_t stream);
/* Chunk membership of the rows rec[pick[i]] (pick NULL: rec[i]), i < m, for ALL chunk origins at once.  bounds: fp64,
 * {lo_x (nx), hi_x (nx), lo_y (ny), hi_y (ny)}, lo ascending, hi = lo + range: row i lies in chunk ix * ny + iy when
 * lo_x[ix] <= x < hi_x[ix] and lo_y[iy] <= y < hi_y[iy], the fp32 coordinate converted to fp64 (numpy's promotion).
 * slot_keys (m, slots): the row's chunks, in any order, and nx * ny in the unused slots; a stable
 * sort of slot_keys lists every chunk's rows (sorted position / slots) in ascending row order, chunk after chunk.  slots >= the most
 * chunks one row can lie in (ceil(range / stride) per axis, multiplied); a row in more chunks than that sets status[0] = 1 (caller-
 * zeroed).  counts (nx * ny) int32, caller-zeroed: integer atomics (an LDS histogram per workgroup when nx * ny <= 2048). */
int ss_chunk_membership(const float* rec, const int32_t* pick, int64_t m, const void* bounds, int nx, int ny, int slots,
                        int64_t* slot_keys, int32_t* counts, int32_t* status, ss_stream_t stream);
/* offsets (nchunk + 1) int64 = exclusive running sum of counts (one workgroup) */
int ss_chunk_offsets(const int32_t* counts, int nchunk, int64_t* offsets, ss_stream_t stream);
/* rows[p] = slot_order[p] / slots for the first `total` positions of the sorted slots (= offsets[nchunk]) */
int ss_chunk_slot_rows(const int32_t* slot_order, int64_t total, int slots, int32_t* rows, ss_stream_t stream);
/* Grouped row gather (a grouped launch, contract above): for every (chunk, asset) problem dst[i] = src[r], r = idx[i], or
 * r = pick[idx[i]] when pick is given (the composition with a grid subsample: the subsampled scene is never materialised).
 * desc: 8 words {src pointer, dst pointer, idx pointer (int32), n_rows, row_bytes < 2^31, pick pointer (int32) | 0, src_rows,
 * pick_rows}; a row whose idx[i] lies outside [0, pick_rows) or whose r lies outside [0, src_rows) is not written.  Word size of the
 * copy: 16 bytes when src, dst and row_bytes are multiples of 16, else 4, 2 or 1 by the same rule.  A workgroup owns
 * ss_chunk_gather_rows_per_workgroup(row_bytes) rows; n_rows = 0 is legal. */
int ss_chunk_gather_group(const int64_t* desc, const int32_t* wg_start, int nprob, int total_workgroups, ss_stream_t stream);
int ss_chunk_gather_rows_per_workgroup(int64_t row_bytes);

/* ---- labelled point cloud of a batch of chunks (csrc/pc_attach.hip; pointcept/datasets/preprocessing/adding_pc_label_to_gs_chunk.py::
 * SceneCache.slice and semseg_label_slice) ---------------------------------------------------------------------------------------------
 * pc (M, 3) f32: the scene cloud.  q (m, 3) f32: the Gaussian centres of nc chunks, concatenated; chunk c owns the query rows
 * q_offset[c] .. q_offset[c + 1] (q_offset (nc + 1) int32, ascending, q_offset[0] = 0).  idx (m, k) int32: the k nearest cloud rows of
 * every query, nearest first, -1 in unfilled slots (ss_knn_query / ss_knn_grid_query).
 * Limits (anything else: SS_ERR_ARG): 1 <= M < 2^31, nc >= 1, nc * ss_pc_bitmap_words(M) * 32 < 2^31, m * k < 2^31.
 * ss_pc_mark: clears bitmap (nc, ss_pc_bitmap_words(M)) uint32 and status (1) itself, then per (query, j) pair: idx < 0 is skipped;
 *   idx >= M sets status[0] = 1 and is never followed; else d = sqrt(dx * dx + dy * dy + dz * dz) in fp64 from the fp32 coordinates
 *   (d? = (double)q? - (double)p?; every operation rounded on its own, the squares added in x, y, z order) and, where
 *   d <= *h_dist_limit (a HOST double; it travels as a kernel argument), bit idx & 31 of bitmap[c][idx >> 5] is set with an integer
 *   atomic OR (skipped when a plain load shows the bit set).  nearest[row] = idx[row][0] where its d <= limit, else -1.
 *   The result does not depend on the order of arrival: two runs are byte-equal.
 * ss_pc_compact_scan: popcounts per tile of 1,024 words (a chunk's tiles are consecutive; a partial last word counts no row >= M),
 *   one exclusive scan over all tiles -> tile_base, and counts[c] (nc) int32 = the distinct rows of chunk c.  tile_base is a caller
 *   buffer of 2 * ss_pc_compact_tiles(M, nc) + 1 int32 (the bases, then the per-tile counts).
 * ss_pc_compact: rows[tile base + rank] = the cloud row of every set bit: the ascending rows of chunk 0, then of chunk 1, ...
 *   (np.unique per chunk without a sort; chunk c's rows start at the running sum of counts).  capacity = the room of `rows`
 *   (the sum of counts); nothing is written at or beyond it. */
int64_t ss_pc_bitmap_words(int64_t M);
int64_t ss_pc_compact_tiles(int64_t M, int nc);
int ss_pc_mark(const float* pc, int64_t M, const float* q, int64_t m, const int32_t* q_offset, int nc, const int32_t* idx, int k,
               const double* h_dist_limit, uint32_t* bitmap, int32_t* nearest, int32_t* status, ss_stream_t stream);
int ss_pc_compact_scan(const uint32_t* bitmap, int64_t M, int nc, int32_t* tile_base, int32_t* counts, ss_stream_t stream);
int ss_pc_compact(const uint32_t* bitmap, int64_t M, int nc, const int32_t* tile_base, int32_t* rows, int64_t capacity,
                  ss_stream_t stream);

/* ---- 3DGS checkpoint decode (csrc/ply.hip; scripts/preprocess_gs.py::read_gaussian_attributes, and read_gaussian_attribute of
 * pointcept/datasets/preprocessing/holicity/preprocess_holicity_gs.py) -------------------------------------------------------------
 * records: n whole vertex records of a binary little-endian .ply on the DEVICE, stride_bytes apart, 4-byte aligned.  h_offsets: a HOST
 * table of 7 + n_scale + n_rot byte offsets inside a record, of the float32 properties x, y, z, f_dc_0..2, opacity,
 * scale_0..n_scale-1, rot_0..n_rot-1; it travels as kernel arguments.  1 <= n_scale, n_rot <= 4.  The stride and every offset are
 * multiples of 4 and offset + 4 <= stride; anything else: SS_ERR_ARG.  n == 0: SS_OK without a launch.
 * Outputs, arrays of their own, contiguous:
 *   coord (n, 3) f32     a copy
 *   color (n, 3) u8      u8(clip(f32(f_dc * f32(0.28209479177387814)) + 0.5f, 0, 1) * 255): every operation rounded to fp32 on its
 *                        own (no fma), the conversion truncates; NaN passes the clip
 *   opacity (n) f32      1 / (1 + exp(-x)) in fp64, rounded once
 *   scale (n, n_scale)   exp(x) in fp64, rounded once
 *   quat (n, n_rot)      q / (sqrt(((q0^2 + q1^2) + q2^2) + q3^2) + f32(1e-9)) * sign(q0 of the quotient): fp32 steps in that order,
 *                        IEEE square root and division; sign(0) = 0, so a record with rot_0 == 0 gives zeros (kept as the reference
 *                        has it)
 * A workgroup owns ss_ply_decode_rows_per_workgroup() consecutive records; a tile whose first byte is 16-byte aligned comes in with
 * 16-byte loads, an 8-byte aligned one with 8-byte loads, any other with 4-byte loads. */
int ss_ply_decode_rows_per_workgroup(void);
int ss_ply_decode(const void* records, int64_t n, int stride_bytes, const int32_t* h_offsets, int n_scale, int n_rot, float* coord,
                  uint8_t* color, float* opacity, float* scale, float* quat, ss_stream_t stream);

/* ---- ScanNet mesh converter (csrc/mesh.hip; pointcept/datasets/preprocessing/scannet/preprocess_scannet.py and
 * preprocess_scannet_gs.py: read_plymesh, vertex_normal, the label loop of handle_process) ---------------------------------------------
 * ss_mesh_decode_vertices: n whole vertex records of a binary little-endian .ply on the DEVICE, stride_bytes apart, starting at ANY
 * byte.  h_offsets: a HOST table of six byte offsets inside a record: the float32 properties x, y, z (multiples of 4, offset + 4 <=
 * stride) and the uchar properties red, green, blue (anywhere).  -> coord (n, 3) f32 and color (n, 3) u8, copies.
 * ss_mesh_decode_faces: n_faces records of 13 bytes (a uchar count, then three int32 or uint32 indices), starting at ANY byte ->
 * faces (n_faces, 3) int32.  A count other than 3 ORs 1 into *status, an index outside [0, n_vertices) ORs 2; the caller zeroes
 * status before the first piece and reads it once.  Both read the aligned 4-byte words that cover the records, so up to 3 bytes in
 * front of `records` and behind the last record must belong to the same allocation.  A workgroup owns
 * ss_mesh_decode_rows_per_workgroup() records; a caller that decodes in pieces hands in outputs advanced to the piece's first row. */
enum { SS_MESH_FORM_PC = 0, SS_MESH_FORM_GS = 1 };
int ss_mesh_decode_rows_per_workgroup(void);
int ss_mesh_decode_vertices(const void* records, int64_t n, int stride_bytes, const int32_t* h_offsets, float* coord, uint8_t* color,
                            ss_stream_t stream);
int ss_mesh_decode_faces(const void* records, int64_t n_faces, int64_t n_vertices, int32_t* faces, int32_t* status, ss_stream_t stream);
/* Vertex normals, bit-equal to the scripts' numpy: every fp32 operation rounded on its own, IEEE division and square root.
 * ss_mesh_face_terms: terms (n_faces, 3) f32 = (vec / length) * area of every face, vec = cross(v1 - v0, v2 - v0) as mul, mul, sub,
 * r = sqrt((x^2 + y^2) + z^2);  SS_MESH_FORM_PC: length = r + 1e-8f, area = length * 0.5f;  SS_MESH_FORM_GS: area = 0.5f * r,
 * length = max(1e-8f, r).  An index outside [0, n_vertices) ORs 2 into *status and gives a zero term.
 * ss_mesh_vertex_normals: order / idx_ptr / head / n_runs = what ss_argsort_i64 (stable) and ss_pool_partition wrote for the 3 *
 * n_faces keys faces[face][corner] (entry p = 3 * face + corner).  One lane per run adds the terms of the run's faces in ascending
 * face index into one fp32 accumulator per component (PC: a face once per vertex, GS: once per corner) and writes
 * normal[v] = acc / length(sqrt((x^2 + y^2) + z^2)) with the form's length rule.  Rows of vertices in no face are NOT written: the
 * caller zeroes normal (n_vertices, 3), which is their value in both forms.  No atomics. */
int ss_mesh_face_terms(const float* coord, const int32_t* faces, int64_t n_faces, int64_t n_vertices, int form, float* terms,
                       int32_t* status, ss_stream_t stream);
int ss_mesh_vertex_normals(const float* terms, const int32_t* faces, const int32_t* order, const int32_t* idx_ptr, const int32_t* head,
                           const int32_t* n_runs, int64_t n_faces, int64_t n_vertices, int form, float* normal, ss_stream_t stream);
/* ss_mesh_labels: for row i < n: seg = seg_indices[src ? src[i] : i] (seg_indices: n_vertices int32), g = seg_to_group[seg]
 * (n_segments int32, -1 = no group), outputs table20[g], table200[g], table_instance[g] (n_groups int32 each); -1 where the row, the
 * segment or the group is out of range.  out_bytes 2: int16 outputs, 8: int64.  src: optional (n) int32 rows, or NULL. */
int ss_mesh_labels(const int32_t* seg_indices, int64_t n_vertices, const int32_t* src, const int32_t* seg_to_group, int64_t n_segments,
                   const int32_t* table20, const int32_t* table200, const int32_t* table_instance, int n_groups, int64_t n,
                   int out_bytes, void* segment20, void* segment200, void* instance, ss_stream_t stream);

/* ---- ScanNet++ converter (csrc/scannetpp.hip; pointcept/datasets/preprocessing/scannetpp/preprocess_scannetpp.py and
 * preprocess_scannetpp_gs.py: Open3D's compute_vertex_normals(normalized=True) and the top-3 label loop of parse_scene) ---------------
 * Vertex normals in Open3D's definition: fp64 throughout, every operation rounded on its own, IEEE division and square root.
 * ss_mesh_face_cross_f64: cross (n_faces, 3) f64 = (v1 - v0) x (v2 - v0) of the fp32 coordinates widened to fp64, each component mul,
 * mul, sub.  An index outside [0, n_vertices) ORs 2 into *status and gives a zero row.
 * ss_mesh_vertex_normals_f64: order / idx_ptr / head / n_runs as for ss_mesh_vertex_normals.  One lane per run adds the cross products
 * of the run's entries in ascending face index, once per corner, into three fp64 accumulators; z = (x^2 + y^2) + z^2; where z > 0 each
 * component is divided by sqrt(z); the result is rounded once to fp32.  Rows of vertices in no face are NOT written: the caller zeroes
 * normal (n_vertices, 3).  No atomics. */
int ss_mesh_face_cross_f64(const float* coord, const int32_t* faces, int64_t n_faces, int64_t n_vertices, double* cross, int32_t* status,
                           ss_stream_t stream);
int ss_mesh_vertex_normals_f64(const double* cross, const int32_t* faces, const int32_t* order, const int32_t* idx_ptr,
                               const int32_t* head, const int32_t* n_runs, int64_t n_faces, int64_t n_vertices, float* normal,
                               ss_stream_t stream);
/* The top-3 labels.  first3 (n_segments, 3) int32: per segment id the first three groups, in segGroups order, that carry a valid label
 * and list the segment; -1 = an empty slot; slots fill from 0.  table_label / table_object (n_groups) int32.  The caller zeroes count
 * (n_segments) and size (n_groups); the three run back to back on one stream, nothing is read on the host in between.
 * ss_spp_segment_hist: count[s] += 1 for s = seg_indices[i] in [0, n_segments), i < n_vertices (at most 2^31 - 1).
 * ss_spp_group_sizes: size[g] += count[s] for every slot g of first3[s] in [0, n_groups).  Integer atomics in both.
 * ss_spp_labels: for row i < n: s = seg_indices[src ? src[i] : i], slots g_k = first3[s][k]; segment[i][k] = table_label[g_k],
 * instance[i][k] = table_object[g_k], `empty` where the slot is empty.  With two or more used slots, p = the first slot of the smallest
 * size[g_k], and columns 0 and p are swapped in both outputs.  A row or segment out of range, or a slot >= n_groups, gives `empty` in
 * all three columns.  segment / instance: (n, 3) int16 at 4-byte aligned addresses, written a pair of rows (12 bytes) per lane. */
int ss_spp_segment_hist(const int32_t* seg_indices, int64_t n_vertices, int64_t n_segments, int32_t* count, ss_stream_t stream);
int ss_spp_group_sizes(const int32_t* first3, const int32_t* count, int64_t n_segments, int n_groups, int32_t* size, ss_stream_t stream);
int ss_spp_labels(const int32_t* seg_indices, int64_t n_vertices, const int32_t* src, const int32_t* first3, int64_t n_segments,
                  const int32_t* table_label, const int32_t* table_object, const int32_t* size, int n_groups, int64_t n, int empty,
                  int16_t* segment, int16_t* instance, ss_stream_t stream);

/* ---- minimal oriented bounding box and the points inside it (csrc/obb.hip; Open3D's get_minimal_oriented_bounding_box and
 * get_point_indices_within_bounding_box as preprocess_scannet_gs.py / preprocess_scannetpp_gs.py call them; the definition: DESIGN.md
 * 8q) -------------------------------------------------------------------------------------------------------------------------------
 * points (N, 3) f32 on the device, 1 <= N < 2^31.  A box is 15 doubles: center (3), R (3, 3) row-major with the axes as COLUMNS,
 * extent (3).  Bitmaps are ss_pc_bitmap_words(N) uint32 words, bit r & 31 of word r >> 5 = row r, every word written (bits of rows
 * >= N are 0): the (1, words) bitmap ss_pc_compact_scan / ss_pc_compact turn into ascending rows.
 * ss_obb_extremes: dirs (K, 3) f64 on the device, 1 <= K <= 1024.  rows_max[d] / rows_min[d] (K) int32 = the row of the largest /
 *   smallest fp64 projection p . dirs[d]; equal values go to the lower row (pairs are compared as a whole in both reduction stages, so
 *   two runs agree); -1 where no projection compares (NaN).  workspace: ss_obb_extremes_workspace_bytes(N, K), else SS_ERR_WORKSPACE.
 * ss_obb_filter: planes (F, 4) f64 on the device (n . p + d <= 0 inside the polytope), F >= 1; *h_tol a HOST double >= 0 (it travels as
 *   a kernel argument).  Bit r is CLEARED only when n . p + d < -tol for every plane; a NaN keeps the row.
 * ss_obb_search: verts (H, 3) f64 hull vertices, tris (T, 3) int32 rows of verts, both on the device.  Candidate 3 t + k: corners a, b,
 *   c of triangle t cyclically from corner k; u = unit(b - a), w = unit(u x (c - a)), v = unit(w x u), unit(x) = x / sqrt((x0^2 + x1^2) +
 *   x2^2); q = ((dx * r0 + dy * r1) + dz * r2) per axis r of d = p - a over all H vertices; extent = hi - lo, volume = (e0 * e1) * e2.
 *   Every operation is rounded on its own (no fma), IEEE square root and division.  volumes (3 T) f64: every candidate's (NaN for a
 *   triangle with a row outside [0, H) or without an area).  best_index (1) int32: the candidate of least volume, equal volumes go to
 *   the lowest index, NaN never wins; -1 when none compares.  box (15): center = a + ((u m0 + v m1) + w m2), m = (lo + hi) * 0.5, R = [u
 *   v w], extent.  No atomics.
 * ss_obb_within: h_box: a HOST box (kernel arguments).  Bit r is set when |((dx * R[0][k] + dy * R[1][k]) + dz * R[2][k])| <=
 *   extent[k] * 0.5 for k = 0, 1, 2, d = (double)p - center.  M == 0: SS_OK without a launch. */
size_t ss_obb_extremes_workspace_bytes(int64_t N, int K);
int ss_obb_extremes(const float* points, int64_t N, const double* dirs, int K, int32_t* rows_max, int32_t* rows_min, void* workspace,
                    size_t workspace_bytes, ss_stream_t stream);
int ss_obb_filter(const float* points, int64_t N, const double* planes, int F, const double* h_tol, uint32_t* bitmap, ss_stream_t stream);
int ss_obb_search(const double* verts, int H, const int32_t* tris, int T, double* volumes, int32_t* best_index, double* box,
                  ss_stream_t stream);
int ss_obb_within(const float* points, int64_t M, const double* h_box, uint32_t* bitmap, ss_stream_t stream);

/* ---- PCA colours of a feature matrix (csrc/feature_pca.hip; the reference's tools/visualize_features_pca.py; the definition:
 * DESIGN.md 8r) ------------------------------------------------------------------------------------------------------------------
 * x (N, D) on the device, rows contiguous, dtype SS_DTYPE_F32 / SS_DTYPE_BF16 / SS_DTYPE_F16; 1 <= N < 2^31, 1 <= D <= SS_PCA_MAX_DIM
 * (any D: edge tiles are padded in the kernels; rows are read with 16- / 8-byte accesses when D % 4 == 0 and x is aligned to them).
 * shift (D) f32 on the device or NULL (zeros).  x - shift is the fp32 difference: ONE rounding of the exact value.  No float atomics:
 * sums that cross a workgroup go through per-workgroup partials in the workspace, added in index order, so two runs agree bit for bit.
 * A workspace below the size its *_workspace_bytes function names: SS_ERR_WORKSPACE.
 * ss_pca_col_sums: sums (D) f64 = sum_r ((double)x[r][d] - (double)shift[d]).
 * ss_pca_gram: gram (D, D) f64 = (x - shift)^T (x - shift), both triangles (pairs ti <= tj of 128-column tiles are computed, the lower
 *   triangle is their mirror).  Products on v_mfma_f32_32x32x2_f32: an entry is a sum of fp32 fmaf chains over at most
 *   SS_PCA_GRAM_CHAIN consecutive rows each (in row order, starting at multiples of SS_PCA_GRAM_CHAIN), added in fp64.  Rows are staged
 *   SS_PCA_GRAM_ROWS at a time and shared out in runs of ss_pca_gram_share_rows(N, D) rows (a multiple of SS_PCA_GRAM_CHAIN, at least
 *   SS_PCA_GRAM_SHARE_MIN) to ceil(N / that) workgroups per tile pair.
 * ss_pca_project: comp (k, D) f32, off (k) f32 or NULL, k = 1..3, k <= D.  y (N, k) f32 = sum_d (x[r][d] - shift[d]) * comp[c][d] (fp32
 *   fmaf, a fixed order) - off[c]; extremes (2 k) f32: the k minima, then the k maxima, of the written y (fminf / fmaxf: a NaN is
 *   skipped).  A workgroup takes rows in blocks of SS_PCA_PROJECT_ROWS.
 * ss_pca_colors: colors (N, 3) f32 from y (N, k) and extremes (2 k): p = min(max((y - mn) / r, 0), 1), r = mx - mn, r = 1 where r == 0,
 *   every operation rounded on its own; k = 3: p; k = 2: (p0, p1, 0.5); k = 1: (p0, p0, p0). */
enum { SS_DTYPE_F16 = 2 };
#define SS_PCA_MAX_DIM 1024
#define SS_PCA_GRAM_CHAIN 256
#define SS_PCA_GRAM_ROWS 32
#define SS_PCA_GRAM_SHARE_MIN 512
#define SS_PCA_PROJECT_ROWS 256
size_t ss_pca_col_sums_workspace_bytes(int64_t N, int D);
int ss_pca_col_sums(const void* x, int dtype, int64_t N, int D, const float* shift, double* sums, void* workspace, size_t workspace_bytes,
                    ss_stream_t stream);
size_t ss_pca_gram_workspace_bytes(int64_t N, int D);
int64_t ss_pca_gram_share_rows(int64_t N, int D);
int ss_pca_gram(const void* x, int dtype, int64_t N, int D, const float* shift, double* gram, void* workspace, size_t workspace_bytes,
                ss_stream_t stream);
size_t ss_pca_project_workspace_bytes(int64_t N);
int ss_pca_project(const void* x, int dtype, int64_t N, int D, const float* shift, const float* comp, const float* off, int k, float* y,
                   float* extremes, void* workspace, size_t workspace_bytes, ss_stream_t stream);
int ss_pca_colors(const float* y, const float* extremes, int64_t N, int k, float* colors, ss_stream_t stream);

/* ---- text queries on scene features (csrc/text_query.hip; the definition: DESIGN.md 8t) ------------------------------------------
 * x (N, D) on the device as for the PCA entries (any D and alignment; wide loads when D % 4 == 0 and x is aligned to them), 1 <= N <
 * 2^31, 1 <= D <= SS_QUERY_MAX_DIM.  t_hat (Q, D) f32 on the device: the UNIT text embeddings (the caller normalises them in fp64),
 * 1 <= Q <= SS_QUERY_MAX_QUERIES.  valid (N) bytes on the device or NULL.  Anything outside the limits: SS_ERR_ARG; a workspace below
 * the size its *_workspace_bytes function names: SS_ERR_WORKSPACE.  No float atomics anywhere: two runs agree bit for bit.
 * ss_query_scores: scores (Q, N) f32, query-major: (sum_d x[r][d] * t_hat[q][d]) / max(sqrt(sum_d x[r][d]^2), 1e-12) in fp32, the sums
 *   as fmaf chains in a fixed order (v_mfma_f32_32x32x2_f32 for the products).  A row with valid[r] == 0, a zero norm or a score that
 *   is not finite is DEAD: -inf for every query.  -0.0 is written as +0.0.  stats (Q, 3) f64 = {live rows, sum s, sum s^2} over the
 *   live rows, from the fp32 scores.  A workgroup takes rows in blocks of SS_QUERY_ROWS; its fp64 partials are added in index order.
 * ss_query_select: scores (Q, N) as written above.  h_tau (Q) f32 and h_m (Q) int32 are HOST arrays (they travel as kernel arguments).
 *   The candidates of query q are the live rows (s > -inf) with s >= h_tau[q] (-inf: every live row).  h_m[q] < 0: all C of them are
 *   selected; else the min(h_m[q], C) best: descending score, the lower row first among equal scores, -0.0 equal to +0.0 (an exact
 *   radix select on the fp32 scores; rows are shared out in segments of SS_QUERY_SELECT_ROWS).  bitmap (Q, ss_pc_bitmap_words(N))
 *   uint32, every word written: what ss_pc_compact_scan / ss_pc_compact (nc = Q) turn into ascending rows.  counts (Q) int32: the
 *   selected rows.  tau_out (Q) f32: h_tau[q], but the score of the last row kept when the cap binds (h_m[q] < C) or when h_m[q] >= 0
 *   and h_tau[q] == -inf (+inf when nothing is kept).
 * ss_query_best: best (N) int32 = among the queries whose bitmap holds row r the one of highest score (the lowest q among equals), -1
 *   when none does. */
#define SS_QUERY_MAX_DIM 1024
#define SS_QUERY_MAX_QUERIES 32
#define SS_QUERY_ROWS 256
#define SS_QUERY_SELECT_ROWS 2048
size_t ss_query_scores_workspace_bytes(int64_t N, int Q);
int ss_query_scores(const void* x, int dtype, int64_t N, int D, const float* t_hat, int Q, const uint8_t* valid, float* scores,
                    double* stats, void* workspace, size_t workspace_bytes, ss_stream_t stream);
size_t ss_query_select_workspace_bytes(int64_t N, int Q);
int ss_query_select(const float* scores, int64_t N, int Q, const float* h_tau, const int32_t* h_m, uint32_t* bitmap, float* tau_out,
                    int32_t* counts, void* workspace, size_t workspace_bytes, ss_stream_t stream);
int ss_query_best(const float* scores, const uint32_t* bitmap, int64_t N, int Q, int32_t* best, ss_stream_t stream);

/* ---- headless Gaussian-splat rendering (csrc/splat.hip; the definition is DESIGN.md 8u) -----------------------------------------------
 * A scene's rows -- coord (N, 3), scale (N, 3) (exponentiated), quat (N, 4) = w, x, y, z, opacity (N), color (N, 3) in 0..1, all f32 on
 * the device -- become an image by EWA splatting: project, count the (Gaussian, tile) pairs, sort them by (tile, depth) with
 * ss_argsort_i64, composite front to back.  Forward only.  No atomics of any kind: two runs give the same bits.  Every buffer is the
 * caller's.  Limits (anything else: SS_ERR_ARG): 1 <= N < 2^31, 1 <= width, height <= SS_SPLAT_MAX_DIM, 1 <= P < 2^31.
 * Preconditions the kernels do not check: ss_splat_keys, ss_splat_ranges and ss_splat_composite take rect / tiles_touched / depth as
 *   ss_splat_project wrote them for the same camera, offsets and P as ss_splat_offsets wrote them for those tiles_touched, and keys /
 *   order / ranges / sorted_rows as the step before wrote them (ss_splat_keys alone guards its writes against P).
 * h_camera: a HOST block of SS_SPLAT_CAMERA_WORDS 32-bit words (it travels as a kernel argument): f32 R[9] (world to camera, row
 *   major), t[3], fx, fy, cx, cy, near, limx, limy (1.3 tan(fov / 2) per axis), then int32 width, height, then zeros.  The camera looks
 *   down +z, x right, y down; pixel (i, j) has its centre at (i + 0.5, j + 0.5); tiles are SS_SPLAT_TILE square.
 * ss_splat_project: per row mean2d (N, 2) f32, conic_opacity (N, 4) f32 = {conic xx, xy, yy, opacity}, depth (N) f32 = p_c.z,
 *   rect (N, 4) int32 = {x0, y0, x1, y1} in tiles (x1, y1 exclusive), radius (N) int32 or NULL, tiles_touched (N) int32 = the
 *   rectangle's area; all 0 for a culled row (a non-finite input, |q| == 0, p_c.z <= near, det <= 0 or NaN, a derived value that is
 *   not finite, an empty rectangle).  mode SS_SPLAT_MODE_POINTCLOUD: the 2-D covariance is (point_size / 3)^2 I and the opacity 1.
 * ss_splat_offsets: offsets (N) int64 = the exclusive running sum of tiles_touched; totals (2) int64 = {P, rows with tiles_touched
 *   > 0}.  Two levels over blocks of SS_SPLAT_SCAN_ROWS rows; workspace ss_splat_offsets_workspace_bytes(N), else SS_ERR_WORKSPACE.
 * ss_splat_keys: keys (P) int64 = (tile << 32) | bits(depth) with tile = y * tiles_x + x, rows (P) int32 = the pair's row, at
 *   offsets[row] + the tile's rank in the rectangle (y major).  Sort them with ss_argsort_i64 (key_bits = 32 + ceil(log2(tiles))).
 * ss_splat_ranges: sorted_keys / order = what the sort wrote.  ranges (num_tiles, 2) int32 = [start, end) of each tile in the sorted
 *   pairs ({0, 0} for a tile without any), sorted_rows (P) int32 = rows[order[i]].
 * ss_splat_composite: one workgroup per tile, one pixel per lane, the tile's Gaussians staged SS_SPLAT_BATCH at a time.  Per pixel,
 *   from T = 1: power = -0.5 d^T conic d (> 0 skips), alpha = min(0.99, o exp(power)) (< 1/255 skips), T' = T (1 - alpha) (< 1e-4
 *   stops the pixel before adding), else C += c alpha T, Z += depth alpha T, T = T'.  image (H, W, 3) = C + T background, alpha (H, W)
 *   = 1 - T, depth_out (H, W) = Z.  h_background: 3 HOST floats. */
#define SS_SPLAT_TILE 16
#define SS_SPLAT_BATCH 256
#define SS_SPLAT_MAX_DIM 4096
#define SS_SPLAT_CAMERA_WORDS 24
#define SS_SPLAT_SCAN_ROWS 2048
#define SS_SPLAT_MODE_GAUSSIANS 0
#define SS_SPLAT_MODE_POINTCLOUD 1
int ss_splat_project(const float* coord, const float* scale, const float* quat, const float* opacity, const float* color, int64_t N,
                     const void* h_camera, int mode, float scale_modifier, float point_size, float* mean2d, float* conic_opacity,
                     float* depth, int32_t* rect, int32_t* radius, int32_t* tiles_touched, ss_stream_t stream);
size_t ss_splat_offsets_workspace_bytes(int64_t N);
int ss_splat_offsets(const int32_t* tiles_touched, int64_t N, int64_t* offsets, int64_t* totals, void* workspace,
                     size_t workspace_bytes, ss_stream_t stream);
int ss_splat_keys(const float* depth, const int32_t* rect, const int32_t* tiles_touched, const int64_t* offsets, int64_t N, int64_t P,
                  int tiles_x, int tiles_y, int64_t* keys, int32_t* rows, ss_stream_t stream);
int ss_splat_ranges(const int64_t* sorted_keys, const int32_t* order, const int32_t* rows, int64_t P, int num_tiles, int32_t* ranges,
                    int32_t* sorted_rows, ss_stream_t stream);
int ss_splat_composite(const float* mean2d, const float* conic_opacity, const float* color, const float* depth, const int32_t* ranges,
                       const int32_t* sorted_rows, int64_t N, int64_t P, int width, int height, const float* h_background, float* image,
                       float* alpha, float* depth_out, ss_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCENESPLAT_HIP_H */
