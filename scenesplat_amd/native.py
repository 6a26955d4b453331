"""Tensor-level wrappers over the C-ABI (include/scenesplat_hip.h).

PyTorch supplies device memory and the current HIP stream only; every call here lands in a
hand-written HIP kernel.  Operands are validated on the host (device, dtype, contiguity,
shape) before any launch; a CPU tensor is an error -- there is no fallback path."""
import ctypes

import numpy as np
import torch

from . import _lib, grouped
from ._lib import check

_C = _lib.CONSTANTS      # the enums of the header
F32, BF16 = _C["SS_DTYPE_F32"], _C["SS_DTYPE_BF16"]
ATTN_SIMT, ATTN_MFMA = _C["SS_ATTN_SIMT"], _C["SS_ATTN_MFMA"]
HAVE_MFMA_ATTN = True  # bf16 MFMA window attention (csrc/attention_mfma.hip)
ORDER_IDS = {name: _C["SS_ORDER_" + name.upper().replace("-", "_")] for name in ("z", "z-trans", "hilbert", "hilbert-trans")}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, dtype=None, name="tensor", shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: scenesplat_amd ops need a GPU tensor (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _req_dense_f32(t, n, dev, name):
    """A tensor a grouped kernel may touch through its raw pointer: dense fp32, contiguous, n elements (None: any), on `dev`."""
    _req(t, torch.float32, name)
    if t.layout is not torch.strided or t.device != dev or (n is not None and t.numel() != n):
        raise RuntimeError(f"{name}: expected a dense tensor" + (f" of {n} elements" if n is not None else "") + f" on {dev}")


def _div_up(a, b):
    return (a + b - 1) // b


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise RuntimeError(f"unsupported feature dtype {t.dtype} (float32 / bfloat16 only)")


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def lib():
    return _lib.load()


# ---- serialization ------------------------------------------------------------------------
def grid_coord_max(gc32):
    _req(gc32, torch.int32, "grid_coord")
    out = torch.empty(1, dtype=torch.int32, device=gc32.device)
    check(lib().ss_grid_coord_max(_p(gc32), gc32.shape[0], _p(out), _stream()), "ss_grid_coord_max")
    return out


def offsets_to_batch(offsets32, n):
    _req(offsets32, torch.int32, "offsets")
    batch = torch.empty(n, dtype=torch.int32, device=offsets32.device)
    check(lib().ss_offsets_to_batch(_p(offsets32), offsets32.numel(), n, _p(batch), _stream()), "ss_offsets_to_batch")
    return batch


def serialize_encode(gc32, batch32, depth, order_names):
    n = gc32.shape[0]
    _req(gc32, torch.int32, "grid_coord", (n, 3))
    if batch32 is not None:
        _req(batch32, torch.int32, "batch", (n,))
    k = len(order_names)
    ids = (ctypes.c_int * k)(*[ORDER_IDS[o] for o in order_names])
    codes = torch.empty((k, n), dtype=torch.int64, device=gc32.device)
    check(lib().ss_serialize_encode(_p(gc32), _p(batch32), n, int(depth), ids, k, _p(codes), _stream()),
          "ss_serialize_encode")
    return codes


def argsort_i64(keys, key_bits, want_inverse=True, want_sorted=True):
    """keys (K, n) int64 >= 0 -> order (K,n) int32 [, inverse (K,n) int32, sorted keys (K,n) int64]; stable."""
    _req(keys, torch.int64, "keys")
    K, n = keys.shape
    dev = keys.device
    order = torch.empty((K, n), dtype=torch.int32, device=dev)
    inverse = torch.empty((K, n), dtype=torch.int32, device=dev) if want_inverse else None
    skeys = torch.empty((K, n), dtype=torch.int64, device=dev) if want_sorted else None
    nb = lib().ss_argsort_workspace_bytes(n, K)
    ws = _ws(nb, dev)
    check(lib().ss_argsort_i64(_p(keys), K, n, int(max(1, min(64, key_bits))), _p(order), _p(inverse), _p(skeys),
                               _p(ws), ws.numel(), _stream()), "ss_argsort_i64")
    return order, inverse, skeys


def count_duplicates(sorted_keys_row):
    _req(sorted_keys_row, torch.int64, "sorted_keys")
    cnt = torch.empty(1, dtype=torch.int32, device=sorted_keys_row.device)
    check(lib().ss_count_duplicates(_p(sorted_keys_row), sorted_keys_row.numel(), _p(cnt), _stream()),
          "ss_count_duplicates")
    return cnt


def pool_partition(code0, order0, shift_bits):
    n = code0.numel()
    _req(code0, torch.int64, "code0", (n,)); _req(order0, torch.int32, "order0", (n,))
    dev = code0.device
    cluster = torch.empty(n, dtype=torch.int32, device=dev)
    idx_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    head = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _ws(lib().ss_pool_partition_workspace_bytes(n), dev)
    check(lib().ss_pool_partition(_p(code0), _p(order0), n, int(shift_bits), _p(cluster), _p(idx_ptr), _p(head),
                                  _p(n_out), _p(ws), ws.numel(), _stream()), "ss_pool_partition")
    return cluster, idx_ptr, head, n_out


def pool_level_attrs(head, n_out, gc32, batch32, codes, pool_depth):
    K, n_in = codes.shape
    _req(codes, torch.int64, "codes"); _req(gc32, torch.int32, "grid_coord", (n_in, 3)); _req(batch32, torch.int32, "batch", (n_in,))
    _req(head, torch.int32, "head")
    if head.numel() < n_out:
        raise RuntimeError("head shorter than n_out")
    dev = codes.device
    gco = torch.empty((n_out, 3), dtype=torch.int32, device=dev)
    bo = torch.empty(n_out, dtype=torch.int32, device=dev)
    co = torch.empty((K, n_out), dtype=torch.int64, device=dev)
    check(lib().ss_pool_level_attrs(_p(head), n_out, n_in, _p(gc32), _p(batch32), _p(codes), K, int(pool_depth),
                                    _p(gco), _p(bo), _p(co), _stream()), "ss_pool_level_attrs")
    return gco, bo, co


def window_index(order_row, offsets, offsets_pad, patch, n_pad):
    _req(order_row, torch.int32, "order"); _req(offsets, torch.int32, "offsets"); _req(offsets_pad, torch.int32, "offsets_pad")
    B = offsets.numel() - 1
    dev = order_row.device
    gidx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    sidx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    check(lib().ss_window_index(_p(order_row), _p(offsets), _p(offsets_pad), B, int(patch), n_pad, _p(gidx), _p(sidx),
                                _stream()), "ss_window_index")
    return gidx, sidx


RULEBOOK_HASHED = True    # hash-table lookups (ss_subm_rulebook_hashed) instead of binary search in the sorted z keys


def subm_rulebook(gc32, batch32, depth, zkeys_sorted, zorder, swap_xy, ksize):
    n = gc32.shape[0]
    _req(gc32, torch.int32, "grid_coord", (n, 3)); _req(batch32, torch.int32, "batch", (n,))
    nbr = torch.empty((ksize ** 3, n), dtype=torch.int32, device=gc32.device)
    if RULEBOOK_HASHED and n < (1 << 30):
        ws = _ws(12 * lib().ss_subm_rulebook_table_size(n), gc32.device)
        check(lib().ss_subm_rulebook_hashed(_p(gc32), _p(batch32), n, int(depth), int(ksize), _p(nbr), _p(ws), ws.numel(), _stream()),
              "ss_subm_rulebook_hashed")
        return nbr
    _req(zkeys_sorted, torch.int64, "zkeys_sorted", (n,)); _req(zorder, torch.int32, "zorder", (n,))
    check(lib().ss_subm_rulebook(_p(gc32), _p(batch32), n, int(depth), _p(zkeys_sorted), _p(zorder), int(swap_xy),
                                 int(ksize), _p(nbr), _stream()), "ss_subm_rulebook")
    return nbr


def subm_tap_mask_keys(nbr, order, coarse_bits):
    """(taps,n) rulebook + walk order -> (n,) int64 sort keys: tap mask | coarse block id << taps."""
    taps, n = nbr.shape
    _req(nbr, torch.int32, "nbr"); _req(order, torch.int32, "order", (n,))
    keys = torch.empty(n, dtype=torch.int64, device=nbr.device)
    check(lib().ss_subm_tap_mask_keys(_p(nbr), _p(order), n, taps, int(coarse_bits), _p(keys), _stream()), "ss_subm_tap_mask_keys")
    return keys


def subm_conv_fwd_uses_pipe(n, cin, cout, taps):
    """Does subm_conv_fwd run this shape on the pipeline kernel (the one that profits from a walk-order rulebook)?"""
    return bool(lib().ss_subm_conv_fwd_uses_pipe(n, cin, cout, taps)) and lib().ss_subm_conv_splits(n, cout, taps) <= 1


def subm_conv_fwd(x, w, bias, nbr, rowperm, out_dtype=torch.bfloat16, nbr_walk=None):
    """x (n,cin) bf16, w (cout,taps,cin) bf16, bias (cout) f32|None, nbr (taps,n) -> (n,cout).
    nbr_walk: the rulebook in walk order (subm_walk_rulebook), read by the pipeline kernel where the shape runs on it."""
    n, cin = x.shape
    cout, taps, cin2 = w.shape
    _req(x, torch.bfloat16, "x"); _req(w, torch.bfloat16, "w"); _req(nbr, torch.int32, "nbr", (taps, n))
    if cin2 != cin or cin % 8:
        raise RuntimeError(f"subm_conv_fwd: cin mismatch / not a multiple of 8 ({cin}, {cin2})")
    if bias is not None:
        _req(bias, torch.float32, "bias", (cout,))
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    splits = lib().ss_subm_conv_splits(n, cout, taps)
    if splits > 1:      # small level: tap ranges in parallel, fp32 atomics, one conversion pass
        acc = torch.zeros((n, cout), dtype=torch.float32, device=x.device)
        check(lib().ss_subm_conv_fwd_splitk(_p(x), _p(w), _p(bias), _p(nbr), _p(rowperm), _p(acc), n, cin, cout, taps, splits,
                                            _stream()), "ss_subm_conv_fwd_splitk")
        return acc if out_dtype == torch.float32 else acc.to(out_dtype)
    out = torch.empty((n, cout), dtype=out_dtype, device=x.device)
    if nbr_walk is not None:
        _req(nbr_walk, torch.int32, "nbr_walk", (taps, n))
        check(lib().ss_subm_conv_fwd_walk(_p(x), _p(w), _p(bias), _p(nbr), _p(nbr_walk), _p(rowperm), _p(out), n, cin, cout, taps,
                                          dtype_code(out), _stream()), "ss_subm_conv_fwd_walk")
        return out
    check(lib().ss_subm_conv_fwd(_p(x), _p(w), _p(bias), _p(nbr), _p(rowperm), _p(out), n, cin, cout, taps,
                                 dtype_code(out), _stream()), "ss_subm_conv_fwd")
    return out


def subm_weight_mirror(w):
    """w (cout,taps,cin) bf16 -> wt (cin,taps,cout) bf16 with wt[ci][T-1-t][co] = w[co][t][ci] (dgrad weight)."""
    cout, taps, cin = w.shape
    _req(w, torch.bfloat16, "w")
    wt = torch.empty((cin, taps, cout), dtype=torch.bfloat16, device=w.device)
    check(lib().ss_subm_weight_mirror(_p(w), _p(wt), cout, taps, cin, _stream()), "ss_subm_weight_mirror")
    return wt


def subm_im2col(x, nbr):
    """x (n,c) bf16 with c % 8 == 0, nbr (taps,n) -> (n, taps*c): neighbour rows side by side, zeros where missing."""
    n, c = x.shape
    taps = nbr.shape[0]
    _req(x, torch.bfloat16, "x"); _req(nbr, torch.int32, "nbr", (taps, n))
    if c % 8:
        raise RuntimeError("subm_im2col: channels must be a multiple of 8")
    out = torch.empty((n, taps * c), dtype=torch.bfloat16, device=x.device)
    check(lib().ss_subm_im2col(_p(x), _p(nbr), _p(out), n, taps, c * 2, _stream()), "ss_subm_im2col")
    return out


def subm_conv_fwd_pipe(x, w, bias, nbr, rowperm, out_dtype=torch.bfloat16):
    """The LDS-DMA pipeline kernel directly (tests / benches); subm_conv_fwd dispatches to it for wide, large levels."""
    n, cin = x.shape
    cout, taps = w.shape[0], w.shape[1]
    out = torch.empty((n, cout), dtype=out_dtype, device=x.device)
    check(lib().ss_subm_conv_fwd_pipe(_p(x), _p(w), _p(bias), _p(nbr), _p(rowperm), _p(out), n, cin, cout, taps,
                                      dtype_code(out), _stream()), "ss_subm_conv_fwd_pipe")
    return out


def linear_fwd(x, w, bias=None, out_dtype=torch.bfloat16):
    """out = x @ w.T + bias on the pipeline GEMM.  x (m,k) bf16, w (n,k) bf16, bias (n) f32 or None."""
    m, k = x.shape
    n = w.shape[0]
    out = torch.empty((m, n), dtype=out_dtype, device=x.device)
    check(lib().ss_linear_fwd(_p(x), _p(w), _p(bias), _p(out), m, k, n, dtype_code(out), _stream()), "ss_linear_fwd")
    return out


def subm_block_lists(nbr, rowperm):
    """Per tap the compacted list of 64-site blocks with at least one pair: (count (taps), list (taps, nblocks))."""
    taps, n = nbr.shape
    _req(nbr, torch.int32, "nbr")
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    nb = (n + 63) // 64
    cnt = torch.empty(taps, dtype=torch.int32, device=nbr.device)
    lst = torch.empty((taps, nb), dtype=torch.int32, device=nbr.device)
    check(lib().ss_subm_block_lists(_p(nbr), _p(rowperm), n, taps, _p(cnt), _p(lst), _stream()), "ss_subm_block_lists")
    return cnt, lst


# ---- zero-initialised fp32 arena for the weight-gradient accumulators -------------------------------
# The wgrad kernels accumulate with fp32 atomics into ZEROED outputs; ~80 separate torch.zeros per backward cost
# ~0.9 ms of fill kernels and as many launches.  A model may reserve one zero-filled block per step
# (zero_arena_begin) from which the accumulators are carved; without a reservation each call allocates its own.
_ARENA = {"buf": None, "off": 0}


def zero_arena_begin(numel, device):
    """Reserve `numel` zero-filled fp32 elements (one fill kernel) for this step's wgrad accumulators."""
    _ARENA["buf"] = torch.zeros(int(numel), dtype=torch.float32, device=device) if numel > 0 else None
    _ARENA["off"] = 0


def zeros_f32(numel, device):
    """numel zero fp32 elements: a slice of the step's arena when it has room (16-byte aligned), else a fresh tensor."""
    buf, off = _ARENA["buf"], _ARENA["off"]
    if buf is not None and buf.device == device and off + numel <= buf.numel():
        _ARENA["off"] = off + ((numel + 3) & ~3)
        return buf[off:off + numel]
    return torch.zeros(int(numel), dtype=torch.float32, device=device)


def subm_conv_wgrad(x, dout, nbr, rowperm, blocks, out=None, nbr_walk=None):
    """-> dW (cout,taps,cin) f32 = sum_i dout[i] (x) x[nbr[t][i]].  blocks = subm_block_lists(nbr, rowperm).
    out: a ZEROED (cout,taps,cin) f32 accumulator to add into (deferred launches).
    nbr_walk: the rulebook in walk order (subm_walk_rulebook), read by the pipeline kernel where the shape runs on it."""
    n, cin = x.shape
    cout = dout.shape[1]
    taps = nbr.shape[0]
    _req(x, torch.bfloat16, "x"); _req(dout, torch.bfloat16, "dout", (n, cout)); _req(nbr, torch.int32, "nbr", (taps, n))
    if cin % 8 or cout % 8:
        raise RuntimeError("subm_conv_wgrad: channels must be multiples of 8")
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    dw = zeros_f32(cout * taps * cin, x.device).view(cout, taps, cin) if out is None else _req(out, torch.float32, "out", (cout, taps, cin))
    cnt, lst = blocks
    _req(cnt, torch.int32, "blk_count", (taps,)); _req(lst, torch.int32, "blk_list", (taps, (n + 63) // 64))
    if nbr_walk is not None:
        _req(nbr_walk, torch.int32, "nbr_walk", (taps, n))
    check(lib().ss_subm_conv_wgrad_walk(_p(x), _p(dout), _p(nbr), _p(nbr_walk), _p(rowperm), _p(cnt), _p(lst), _p(dw), n, cin, cout, taps,
                                        _stream()), "ss_subm_conv_wgrad_walk")
    return dw


def subm_conv_wgrad_capped(x, dout, nbr, rowperm, blocks, out=None, nbr_walk=None, max_workgroups=None, min_per=0, stream=None):
    """subm_conv_wgrad's result from the pipeline kernel on at most max_workgroups PERSISTENT workgroups (ss_subm_conv_wgrad_pipe_capped:
    a workgroup fills a CU, the other CUs stay free for another stream; None: one per CU).  The shape must be one the pipeline kernel
    takes.  out: a ZEROED (cout,taps,cin) f32 accumulator; min_per: K-tiles per share (0: the plain launch's); stream: launch there
    instead of on the current stream (the caller orders the streams).  The ticket counter is a fresh zero word per call."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return subm_conv_wgrad_capped(x, dout, nbr, rowperm, blocks, out, nbr_walk, max_workgroups, min_per)
    n, cin = x.shape
    cout = dout.shape[1]
    taps = nbr.shape[0]
    _req(x, torch.bfloat16, "x"); _req(dout, torch.bfloat16, "dout", (n, cout)); _req(nbr, torch.int32, "nbr", (taps, n))
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    cnt, lst = blocks
    _req(cnt, torch.int32, "blk_count", (taps,)); _req(lst, torch.int32, "blk_list", (taps, (n + 63) // 64))
    if nbr_walk is not None:
        _req(nbr_walk, torch.int32, "nbr_walk", (taps, n))
    if max_workgroups is None:
        max_workgroups = torch.cuda.get_device_properties(x.device).multi_processor_count
    dw = torch.zeros((cout, taps, cin), dtype=torch.float32, device=x.device) if out is None else _req(out, torch.float32, "out", (cout, taps, cin))
    counter = torch.zeros(1, dtype=torch.int32, device=x.device)
    rule = nbr if nbr_walk is None else nbr_walk
    check(lib().ss_subm_conv_wgrad_pipe_capped(_p(x), _p(dout), _p(rule), _p(rowperm), _p(cnt), _p(lst), _p(dw), _p(counter), n, cin, cout,
                                               taps, int(nbr_walk is not None), int(min_per), int(max_workgroups), _stream()),
          "ss_subm_conv_wgrad_pipe_capped")
    return dw


def subm_f32_weight_layout(w, mirror=False):
    """w (32, taps, c) f32 -> the fp32-MFMA conv's operand layout [tap][cp / 8][2][32][4] (cp = c padded to 16 or 32).
    mirror: the dgrad operand, w'[ci][T-1-t][co] = w[co][t][ci] (needs c == 32)."""
    w = w.float()
    if mirror:
        w = w.flip(1).permute(2, 1, 0)
    co, taps, c = w.shape
    cp = 16 if c <= 16 else 32
    if co != 32 or c > 32:
        raise RuntimeError("subm_f32: 32 output channels, at most 32 input channels")
    if cp != c:
        w = torch.nn.functional.pad(w, (0, cp - c))
    return w.reshape(32, taps, cp // 8, 2, 4).permute(1, 2, 3, 0, 4).contiguous()


def subm_walk_rulebook(nbr, rowperm):
    """The rulebook in walk order: (taps, n) with [t][k] = nbr[t][rowperm[k]] (rowperm None: nbr itself)."""
    return nbr if rowperm is None else nbr.index_select(1, rowperm).contiguous()


def subm_f32_fwd(x, wq, bias, nbr, rowperm, winners_only=False):
    """x (n, cp) f32 (cp 16 | 32), wq from subm_f32_weight_layout, nbr = subm_walk_rulebook(...) -> (n, 32) f32, exact fp32
    products (v_mfma_f32_32x32x2_f32).  winners_only: the dgrad form for a level with duplicate voxels -- x = dup_fold_rows(dout),
    rows that are not the winner of their voxel come out as zeros."""
    n, cp = x.shape
    taps = nbr.shape[0]
    _req(x, torch.float32, "x"); _req(wq, torch.float32, "wq", (taps, cp // 8, 2, 32, 4)); _req(nbr, torch.int32, "nbr", (taps, n))
    if bias is not None:
        _req(bias, torch.float32, "bias", (32,))
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    out = torch.empty((n, 32), dtype=torch.float32, device=x.device)
    if winners_only:
        if bias is not None:
            raise RuntimeError("subm_f32_fwd: the dgrad form takes no bias")
        check(lib().ss_subm_f32_dgrad_dup(_p(x), _p(wq), _p(nbr), _p(rowperm), _p(out), n, cp, 32, taps, _stream()), "ss_subm_f32_dgrad_dup")
        return out
    check(lib().ss_subm_f32_fwd(_p(x), _p(wq), _p(bias), _p(nbr), _p(rowperm), _p(out), n, cp, 32, taps, _stream()), "ss_subm_f32_fwd")
    return out


def dup_runs_from_rulebook(nbr):
    """(sorted keys (n) int64, order (n) int32) naming the duplicate-voxel runs of a level, derived from a rulebook alone: the centre
    tap of nbr (taps, n) is every site's winner row, a stable sort by it lists each voxel's rows ascending behind their winner.
    (A ScenePlan level hands out its curve codes instead: Level.dup_runs.)"""
    keys, order = torch.sort(nbr[nbr.shape[0] // 2].long(), stable=True)
    return keys.contiguous(), order.to(torch.int32).contiguous()


def dup_fold_rows(src, runs):
    """Adjoint of "every site of a voxel reads the voxel's winner row": out[winner] = sum of src over the voxel's rows (fp32
    accumulate, deterministic), out[other rows] = 0.  src (n, C) f32 | bf16 with 16-byte rows; runs = (sorted keys, order)."""
    keys, order = runs
    n, C = src.shape
    _req(src, None, "src"); _req(keys, torch.int64, "sorted_keys", (n,)); _req(order, torch.int32, "order", (n,))
    out = torch.empty_like(src)
    check(lib().ss_dup_fold_rows(_p(src), _p(keys), _p(order), _p(out), n, C, dtype_code(src), _stream()), "ss_dup_fold_rows")
    return out


def dup_zero_rows_(x, runs):
    """In place: rows of x (n, C) that are not the winner of their voxel := 0."""
    keys, order = runs
    n = x.shape[0]
    _req(x, None, "x"); _req(keys, torch.int64, "sorted_keys", (n,)); _req(order, torch.int32, "order", (n,))
    check(lib().ss_dup_zero_rows(_p(keys), _p(order), _p(x), n, x.shape[1] * x.element_size(), _stream()), "ss_dup_zero_rows")
    return x


def subm_f32_wgrad(x, dout, nbr, rowperm, blocks, cin):
    """-> dW (32, taps, cin) f32 = sum_i dout[i] (x) x[nbr[t][i]][:cin]; x (n, cp) f32, dout (n, 32) f32; nbr in walk order
    (subm_walk_rulebook), blocks = subm_block_lists(original nbr, rowperm)."""
    n, cp = x.shape
    taps = nbr.shape[0]
    _req(x, torch.float32, "x"); _req(dout, torch.float32, "dout", (n, 32)); _req(nbr, torch.int32, "nbr", (taps, n))
    if rowperm is not None:
        _req(rowperm, torch.int32, "rowperm", (n,))
    cnt, lst = blocks
    _req(cnt, torch.int32, "blk_count", (taps,)); _req(lst, torch.int32, "blk_list", (taps, (n + 63) // 64))
    dw = zeros_f32(32 * taps * cin, x.device).view(32, taps, cin)
    check(lib().ss_subm_f32_wgrad(_p(x), _p(dout), _p(nbr), _p(rowperm), _p(cnt), _p(lst), _p(dw), n, cp, cin, 32, taps, _stream()),
          "ss_subm_f32_wgrad")
    return dw


def subm_conv_wgrad_pipe(x, dout, nbr, rowperm, blocks):
    """The pipeline weight-gradient kernel directly (tests / benches)."""
    n, cin = x.shape
    cout, taps = dout.shape[1], nbr.shape[0]
    dw = torch.zeros((cout, taps, cin), dtype=torch.float32, device=x.device)
    cnt, lst = blocks
    check(lib().ss_subm_conv_wgrad_pipe(_p(x), _p(dout), _p(nbr), _p(rowperm), _p(cnt), _p(lst), _p(dw), n, cin, cout, taps,
                                        _stream()), "ss_subm_conv_wgrad_pipe")
    return dw


def linear_wgrad_alloc(k, nout, want_bias, device):
    """Zeroed fp32 accumulators (dW (nout,k), db (nout) | None) sharing one allocation."""
    buf = zeros_f32(nout * k + (nout if want_bias else 0), device)
    return buf[:nout * k].view(nout, k), (buf[nout * k:] if want_bias else None)


def linear_wgrad_into(x, dy, dw, db):
    """dw += dy^T @ x, db += column sums of dy (db may be None); dw / db must be zero on the first call."""
    m, k = x.shape
    nout = dy.shape[1]
    _req(x, torch.bfloat16, "x"); _req(dy, torch.bfloat16, "dy", (m, nout)); _req(dw, torch.float32, "dw", (nout, k))
    check(lib().ss_linear_wgrad(_p(x), _p(dy), _p(dw), _p(db), m, k, nout, _stream()), "ss_linear_wgrad")


_CAPPED_TILES = {}


def _capped_launch_tiles(shapes, cap):
    """The `launch_tiles` argument of ss_linear_wgrad_group_plan_capped for every problem of a capped launch.  The planner gives a tile
    4 * cap / launch_tiles shares, i.e. equally long items when every problem has the same m.  For problems of different m the launch's
    work is stated in tiles of THIS problem's K extent (sum of tiles x K-tiles over the launch / this problem's K-tiles), which makes the
    items equally long across problems; and of 2 .. 8 rounds the count is taken at which the static deal (workgroup b runs items b,
    b + grid, ...) ends earliest, an item costing its K-tiles plus about 8 for the pipeline fill and the 256-KiB atomic epilogue."""
    key = (shapes, cap)
    if key in _CAPPED_TILES:
        return _CAPPED_TILES[key]
    tiles = [lib().ss_linear_wgrad_tiles(k, n) for _, k, n in shapes]
    kt = [_div_up(m, 64) for m, _, _ in shapes]
    work = sum(t * b for t, b in zip(tiles, kt))
    words = np.zeros(8, dtype=np.int64)
    best = None
    for rounds in (4, 2, 3, 5, 6, 8):
        cand = [max(1, _div_up(work * 4, rounds * b)) for b in kt]
        lengths = []
        for (m, k, n), lt, t, b in zip(shapes, cand, tiles, kt):
            if lib().ss_linear_wgrad_group_plan_capped(m, k, n, lt, cap, ctypes.c_void_p(words.ctypes.data)) <= 0:
                continue
            shares, per = int(words[7]) & 0xffffffff, int(words[7]) >> 32
            lengths += [min(per, b - s * per) + 8 for s in range(shares) for _ in range(t)]
        grid = max(1, min(cap, len(lengths)))
        span = max(sum(lengths[b::grid]) for b in range(grid)) if lengths else 0
        if best is None or span < best[0]:
            best = (span, cand)
    if len(_CAPPED_TILES) > 64:
        _CAPPED_TILES.clear()
    _CAPPED_TILES[key] = best[1]
    return best[1]


def linear_wgrad_group(items, max_workgroups=None, stream=None):
    """ONE launch for many nn.Linear weight gradients.  items: list of (x (m,k) bf16, dy (m,n) bf16, dw (n,k) f32 ZEROED,
    db (n) f32 ZEROED | None).  Problems the pipeline kernel cannot take are run one by one.
    max_workgroups: run the group on at most that many persistent workgroups (ss_linear_wgrad_group_capped: a workgroup fills a CU, the
    other CUs stay free for another stream); stream: launch there instead of on the current stream (the caller orders the streams)."""
    if not items:
        return
    if stream is not None:
        with torch.cuda.stream(stream):
            return linear_wgrad_group(items, max_workgroups)
    dev = items[0][0].device
    desc = np.zeros((len(items), 8), dtype=np.int64)
    counts = []
    # the CUs are shared out over the output tiles of the whole group (one round of workgroups for the launch)
    launch_tiles = sum(lib().ss_linear_wgrad_tiles(x.shape[1], dy.shape[1]) for x, dy, _, _ in items)
    if max_workgroups is not None:
        capped_tiles = _capped_launch_tiles(tuple((x.shape[0], x.shape[1], dy.shape[1]) for x, dy, _, _ in items[:128]), int(max_workgroups))
    for x, dy, dw, db in items:
        _req(x, torch.bfloat16, "x"); _req(dy, torch.bfloat16, "dy", (x.shape[0], dy.shape[1]))
        _req(dw, torch.float32, "dw", (dy.shape[1], x.shape[1]))
        if db is not None:
            _req(db, torch.float32, "db", (dy.shape[1],))
        j = len(counts)
        words = ctypes.c_void_p(desc[j].ctypes.data)
        if max_workgroups is None:
            nwg = lib().ss_linear_wgrad_group_plan2(x.shape[0], x.shape[1], dy.shape[1], launch_tiles, words)
        else:
            nwg = lib().ss_linear_wgrad_group_plan_capped(x.shape[0], x.shape[1], dy.shape[1], capped_tiles[len(counts)], int(max_workgroups), words)
        if nwg <= 0 or j >= 128:
            linear_wgrad_into(x, dy, dw, db)
            continue
        desc[j, 0], desc[j, 1], desc[j, 2] = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
        desc[j, 3] = db.data_ptr() if db is not None else 0
        desc[j, 4] = x.shape[0]
        counts.append(nwg)
    if counts and max_workgroups is None:
        grouped.launch("ss_linear_wgrad_group", desc[:len(counts)].copy(), grouped.starts(counts), dev)
    elif counts:
        grouped.launch("ss_linear_wgrad_group_capped", desc[:len(counts)].copy(), grouped.starts(counts), dev, int(max_workgroups))


def linear_wgrad(x, dy, want_bias=False):
    """dW (n_out,k_in) f32 = dy^T @ x on the pipeline kernel (and db (n_out) f32 = column sums of dy when want_bias).
    x (m,k_in) bf16, dy (m,n_out) bf16.  dW and db share one zero-filled allocation."""
    m, k = x.shape
    nout = dy.shape[1]
    _req(x, torch.bfloat16, "x"); _req(dy, torch.bfloat16, "dy", (m, nout))
    buf = zeros_f32(nout * k + (nout if want_bias else 0), x.device)
    dw = buf[:nout * k].view(nout, k)
    db = buf[nout * k:] if want_bias else None
    check(lib().ss_linear_wgrad(_p(x), _p(dy), _p(dw), _p(db), m, k, nout, _stream()), "ss_linear_wgrad")
    return (dw, db) if want_bias else dw


# ---- fused add + layernorm ----------------------------------------------------------------------
def _dt(t):
    return dtype_code(t) if t is not None else 0


def add_layernorm_fwd(x, y, rowscale, gamma, beta, eps, want_xout, want_copy, h_dtype):
    """v = x + rowscale*y -> (xout f32 | None, xcopy bf16 | None, h | None, mean, rstd)."""
    n, C = x.shape
    _req(x, None, "x")
    if y is not None:
        _req(y, None, "y", (n, C))
    if rowscale is not None:
        _req(rowscale, torch.float32, "rowscale", (n,))
    dev = x.device
    xout = torch.empty((n, C), dtype=torch.float32, device=dev) if want_xout else None
    xcopy = torch.empty((n, C), dtype=torch.bfloat16, device=dev) if want_copy else None
    h = mean = rstd = None
    if gamma is not None:
        _req(gamma, torch.float32, "gamma", (C,)); _req(beta, torch.float32, "beta", (C,))
        h = torch.empty((n, C), dtype=h_dtype, device=dev)
        mean = torch.empty(n, dtype=torch.float32, device=dev); rstd = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().ss_add_layernorm_fwd(_p(x), _dt(x), _p(y), _dt(y), _p(rowscale), _p(gamma), _p(beta), float(eps), _p(xout), F32,
                                     _p(xcopy), _p(h), _dt(h), _p(mean), _p(rstd), n, C, _stream()), "ss_add_layernorm_fwd")
    return xout, xcopy, h, mean, rstd


def ln_add_ln_fwd(x, t, gamma0, beta0, eps0, gamma1, beta1, eps1, h_dtype):
    """xout = x + LN0(t), h = LN1(xout) in one pass -> (xout f32, h, stats (n,4) f32)."""
    n, C = x.shape
    _req(x, None, "x"); _req(t, None, "t", (n, C))
    for p_, nm in ((gamma0, "gamma0"), (beta0, "beta0"), (gamma1, "gamma1"), (beta1, "beta1")):
        _req(p_, torch.float32, nm, (C,))
    dev = x.device
    xout = torch.empty((n, C), dtype=torch.float32, device=dev)
    h = torch.empty((n, C), dtype=h_dtype, device=dev)
    stats = torch.empty((n, 4), dtype=torch.float32, device=dev)
    check(lib().ss_ln_add_ln_fwd(_p(x), _dt(x), _p(t), _dt(t), _p(gamma0), _p(beta0), float(eps0), _p(gamma1), _p(beta1), float(eps1),
                                 _p(xout), _p(h), _dt(h), _p(stats), n, C, _stream()), "ss_ln_add_ln_fwd")
    return xout, h, stats


def group_partial_sums(items):
    """ONE launch for many partial-sum reductions.  items: list of (part (K, nb, C) f32, dst (K, C) f32): dst = part.sum(1)."""
    if not items:
        return
    dev = items[0][0].device
    desc = np.zeros((len(items), 4), dtype=np.int64)
    per = lib().ss_group_partial_sums_outputs_per_workgroup()
    for j, (part, dst) in enumerate(items):
        K, nb, C = part.shape
        _req(part, torch.float32, "part"); _req(dst, torch.float32, "dst", (K, C))
        desc[j] = (part.data_ptr(), dst.data_ptr(), nb, C | ((K * C) << 32))
    grouped.launch("ss_group_partial_sums", desc, grouped.starts(_div_up(desc[:, 3] >> 32, per)), dev)


def subm_weight_mirror_group(pairs):
    """ONE launch: wt (cin, taps, cout) = tap-mirrored transpose of w (cout, taps, cin) for every (w, wt) bf16 pair."""
    if not pairs:
        return
    dev = pairs[0][0].device
    desc = np.zeros((len(pairs), 5), dtype=np.int64)
    tile = lib().ss_subm_weight_mirror_group_tile()
    for j, (w, wt) in enumerate(pairs):
        cout, taps, cin = w.shape
        _req(w, torch.bfloat16, "w"); _req(wt, torch.bfloat16, "wt", (cin, taps, cout))
        desc[j] = (w.data_ptr(), wt.data_ptr(), cout, taps, cin)
    starts = grouped.starts(desc[:, 3] * _div_up(desc[:, 2], tile) * _div_up(desc[:, 4], tile))
    grouped.launch("ss_subm_weight_mirror_group", desc, starts, dev)


def transpose16_group(pairs):
    """ONE launch: dst (cols, rows) = src (rows, cols)^T for every (src, dst) pair of 2-byte tensors (bf16 weight copies)."""
    if not pairs:
        return
    dev = pairs[0][0].device
    desc = np.zeros((len(pairs), 4), dtype=np.int64)
    for j, (src, dst) in enumerate(pairs):
        r, c = src.shape
        if src.element_size() != 2 or dst.element_size() != 2 or tuple(dst.shape) != (c, r) or not (src.is_contiguous() and dst.is_contiguous()):
            raise RuntimeError("transpose16_group: contiguous 2-byte (rows, cols) -> (cols, rows) pairs")
        desc[j] = (src.data_ptr(), dst.data_ptr(), r, c)
    grouped.launch("ss_transpose16_group", desc, grouped.starts(_div_up(desc[:, 2], 64) * _div_up(desc[:, 3], 64)), dev)


def ln_add_ln_bwd(g_xout, g_h, xout, t, stats, gamma0, gamma1, gx_dtype, gt_dtype, reduce=True):
    """-> (g_x, g_t, dgamma0, dbeta0, dgamma1, dbeta1); reduce=False: (g_x, g_t, part (4, nb, C)) for a grouped reduction"""
    n, C = xout.shape
    dev = xout.device
    if g_xout is not None:
        _req(g_xout, torch.float32, "g_xout", (n, C))
    if g_h is not None:
        _req(g_h, None, "g_h", (n, C))
    g_x = torch.empty((n, C), dtype=gx_dtype, device=dev)
    g_t = torch.empty((n, C), dtype=gt_dtype, device=dev)
    nb = lib().ss_add_layernorm_bwd_blocks(n)
    part = torch.empty((4, nb, C), dtype=torch.float32, device=dev)
    check(lib().ss_ln_add_ln_bwd(_p(g_xout), _p(g_h), _dt(g_h), _p(xout), _p(t), _dt(t), _p(stats), _p(gamma0), _p(gamma1), _p(g_x),
                                 _dt(g_x), _p(g_t), _dt(g_t), _p(part), n, C, nb, _stream()), "ss_ln_add_ln_bwd")
    if not reduce:
        return g_x, g_t, part
    red = part.sum(1)
    return g_x, g_t, red[0], red[1], red[2], red[3]


def add_layernorm_bwd(g_xout, g_xcopy, g_h, v, mean, rstd, gamma, rowscale, gx_dtype, gy_dtype, reduce=True):
    """-> (g_x | None, g_y | None, dgamma | None, dbeta | None); reduce=False: (g_x, g_y, part (2, nb, C) | None, None)"""
    ref = g_h if g_h is not None else (g_xout if g_xout is not None else g_xcopy)
    n, C = ref.shape
    dev = ref.device
    for t, nm in ((g_xout, "g_xout"), (g_xcopy, "g_xcopy"), (g_h, "g_h")):
        if t is not None:
            _req(t, None, nm, (n, C))
    g_x = torch.empty((n, C), dtype=gx_dtype, device=dev) if gx_dtype is not None else None
    g_y = torch.empty((n, C), dtype=gy_dtype, device=dev) if gy_dtype is not None else None
    nb = lib().ss_add_layernorm_bwd_blocks(n)
    dgp = dbp = None
    if g_h is not None:
        part = torch.empty((2, nb, C), dtype=torch.float32, device=dev)     # one allocation, ONE reduction for both
        dgp, dbp = part[0], part[1]
        _req(v, None, "v", (n, C))
    check(lib().ss_add_layernorm_bwd(_p(g_xout), _dt(g_xout), _p(g_xcopy), _dt(g_xcopy), _p(g_h), _dt(g_h), _p(v), _dt(v),
                                     _p(mean), _p(rstd), _p(gamma), _p(rowscale), _p(g_x), _dt(g_x), _p(g_y), _dt(g_y),
                                     _p(dgp), _p(dbp), n, C, nb, _stream()), "ss_add_layernorm_bwd")
    if g_h is not None:
        if not reduce:
            return g_x, g_y, part, None
        red = part.sum(1)
        return g_x, g_y, red[0], red[1]
    return g_x, g_y, None, None


# ---- fused batchnorm (+GELU) ----------------------------------------------------------------------
def col_stats(x):
    """-> (shift, sum, sumsq): shift = row 0 of x (fp32) and the column sums of (x - shift), (x - shift)^2, fp32 (partials
    reduced here).  mean = shift + sum / n; biased variance = sumsq / n - (sum / n)^2."""
    n, C = x.shape
    _req(x, None, "x")
    nb = lib().ss_add_layernorm_bwd_blocks(n)
    part = torch.empty((2, nb, C), dtype=torch.float32, device=x.device)
    shift = torch.empty(C, dtype=torch.float32, device=x.device)
    check(lib().ss_col_stats(_p(x), _dt(x), _p(shift), _p(part[0]), _p(part[1]), n, C, nb, _stream()), "ss_col_stats")
    red = part.sum(1)
    return shift, red[0], red[1]


def bn_batch_stats(x, running_mean, running_var, num_batches, momentum, eps):
    """Training-mode BatchNorm statistics in two launches: -> (mean, rstd) of the batch (fp32, biased variance), with the
    running statistics (fp32 buffers, in place; momentum update with the unbiased variance) and the batch counter updated
    the way nn.BatchNorm1d does.  The one-pass variance is conditioned on the batch itself: the statistics pass sums
    x - x[0] per column and hands row 0 to the finishing launch, so the result does not depend on how far the running
    mean is from the batch mean (it is 0 in a fresh model)."""
    n, C = x.shape
    _req(x, None, "x")
    _req(running_mean, torch.float32, "running_mean", (C,)); _req(running_var, torch.float32, "running_var", (C,))
    nb = lib().ss_add_layernorm_bwd_blocks(n)
    part = torch.empty((2, nb, C), dtype=torch.float32, device=x.device)
    small = torch.empty((3, C), dtype=torch.float32, device=x.device)             # shift | mean | rstd
    shift, out = small[0], small[1:]
    check(lib().ss_col_stats(_p(x), _dt(x), _p(shift), _p(part[0]), _p(part[1]), n, C, nb, _stream()), "ss_col_stats")
    if num_batches is not None:
        _req(num_batches, torch.int64, "num_batches_tracked")
    check(lib().ss_bn_stats_finish(_p(part), _p(shift), nb, C, n, float(momentum), float(eps), _p(running_mean),
                                   _p(running_var), _p(num_batches), _p(out[0]), _p(out[1]), _stream()), "ss_bn_stats_finish")
    return out[0], out[1]


def bn_act_fwd(x, mean, rstd, gamma, beta, act, out_dtype):
    n, C = x.shape
    y = torch.empty((n, C), dtype=out_dtype, device=x.device)
    check(lib().ss_bn_act_fwd(_p(x), _dt(x), _p(mean), _p(rstd), _p(gamma), _p(beta), int(act), _p(y), _dt(y), n, C, _stream()),
          "ss_bn_act_fwd")
    return y


def bn_act_bwd(dy, x, mean, rstd, gamma, beta, act, training):
    """-> dx (x.dtype), dgamma, dbeta (fp32)"""
    n, C = x.shape
    _req(dy, None, "dy", (n, C))
    nb = lib().ss_add_layernorm_bwd_blocks(n)
    part = torch.empty((2, nb, C), dtype=torch.float32, device=x.device)
    pz, pzx = part[0], part[1]
    check(lib().ss_bn_act_bwd_reduce(_p(dy), _dt(dy), _p(x), _dt(x), _p(mean), _p(rstd), _p(gamma), _p(beta), int(act), _p(pz),
                                     _p(pzx), n, C, nb, _stream()), "ss_bn_act_bwd_reduce")
    sums = torch.empty((2 if not training else 4, C), dtype=torch.float32, device=x.device)
    check(lib().ss_bn_bwd_finish(_p(part), nb, C, n, _p(sums), _p(sums[2:]) if training else None, _stream()), "ss_bn_bwd_finish")
    sdz, sdzx = sums[0], sums[1]
    c1, c2 = (sums[2], sums[3]) if training else (None, None)
    dx = torch.empty_like(x)
    check(lib().ss_bn_act_bwd_apply(_p(dy), _dt(dy), _p(x), _dt(x), _p(mean), _p(rstd), _p(gamma), _p(beta), int(act), _p(c1),
                                    _p(c2), _p(dx), _dt(dx), n, C, _stream()), "ss_bn_act_bwd_apply")
    return dx, sdzx, sdz


# ---- open-vocabulary scan ----------------------------------------------------------------------------
def feat_text_scan(feat, text, want_max=True, idx=None, pred_accum=None):
    """feat (n, D), text (C, D) -> (max_prob (n) f32, argmax (n) int32) and/or pred_accum[idx] += sigmoid(feat text^T)."""
    f = _req(feat.to(torch.bfloat16).contiguous(), torch.bfloat16, "feat")
    t = _req(text.to(torch.bfloat16).contiguous(), torch.bfloat16, "text")
    n, D = f.shape
    C = t.shape[0]
    if t.shape[1] != D or D % 8 or C > 256:
        raise RuntimeError("feat_text_scan: need matching dim (multiple of 8) and <= 256 classes")
    mp = torch.empty(n, dtype=torch.float32, device=f.device) if want_max else None
    am = torch.empty(n, dtype=torch.int32, device=f.device) if want_max else None
    if pred_accum is not None:
        _req(pred_accum, torch.float32, "pred_accum")
        if pred_accum.shape[1] != C:
            raise RuntimeError("pred_accum must be (rows, num_classes)")
    if idx is not None:
        _req(idx, torch.int32, "idx", (n,))
    check(lib().ss_feat_text_scan(_p(f), _p(t), n, D, C, _p(mp), _p(am), _p(idx), _p(pred_accum), _stream()), "ss_feat_text_scan")
    return mp, am


# ---- distillation head ------------------------------------------------------------------------
def _mask_bytes(mask, n):
    m = mask if mask.dtype in (torch.bool, torch.uint8) else (mask > 0)
    m = _req(m.contiguous(), None, "valid_feat_mask", (n,))
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def lang_head_fwd(feat, target, mask, normalize, want_p=True, p_dtype=torch.float32):
    """-> (p | None, sums (3) f32 | None, rowstat (n,4) f32).  feat / target (n, C) f32 | bf16."""
    _req(feat, None, "feat")
    n, C = feat.shape
    if C % 4 or C > 2048:
        raise RuntimeError("lang_head: channels must be a multiple of 4 and <= 2048")
    dev = feat.device
    p = torch.empty((n, C), dtype=p_dtype, device=dev) if want_p else None
    rowstat = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sums = part = m8 = None
    if target is not None:
        _req(target, None, "target", (n, C))
        m8 = _mask_bytes(mask, n)
        part = torch.empty(lib().ss_lang_head_blocks(n) * 3, dtype=torch.float32, device=dev)
        sums = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib().ss_lang_head_fwd(_p(feat), dtype_code(feat), _p(target), dtype_code(target) if target is not None else 0, _p(m8),
                                 int(bool(normalize)), _p(p), dtype_code(p) if p is not None else 0, _p(rowstat), _p(part), _p(sums),
                                 n, C, _stream()), "ss_lang_head_fwd")
    return p, sums, rowstat


def lang_head_bwd(feat, target, mask, normalize, rowstat, coef, dp_extra):
    """-> dfeat (n, C) in feat's dtype.  coef (2) f32 on the device (dL/dsums[0:2]) or None; dp_extra (n, C) or None."""
    _req(feat, None, "feat"); _req(rowstat, torch.float32, "rowstat")
    n, C = feat.shape
    m8 = None
    if target is not None:
        _req(target, None, "target", (n, C)); _req(coef, torch.float32, "coef")
        m8 = _mask_bytes(mask, n)
    if dp_extra is not None:
        _req(dp_extra, None, "dp", (n, C))
    dfeat = torch.empty_like(feat)
    check(lib().ss_lang_head_bwd(_p(feat), dtype_code(feat), _p(target), dtype_code(target) if target is not None else 0, _p(m8),
                                 int(bool(normalize)), _p(rowstat), _p(coef), _p(dp_extra),
                                 dtype_code(dp_extra) if dp_extra is not None else 0, _p(dfeat), dtype_code(dfeat), n, C, _stream()),
          "ss_lang_head_bwd")
    return dfeat


# ---- semantic segmentation losses and metric ------------------------------------------------------------------
SEG_MAX_CLASSES = 256


def _seg_operands(logits, labels):
    _req(logits, None, "logits")
    if logits.dim() != 2 or not 1 <= logits.shape[1] <= SEG_MAX_CLASSES:
        raise RuntimeError(f"seg_loss: logits must be (n, C) with C <= {SEG_MAX_CLASSES}")
    n = logits.shape[0]
    _req(labels, torch.int64, "labels", (n,))
    return n, logits.shape[1]


def seg_loss_fwd(logits, labels, ignore_index, class_seen=None, lovasz=True):
    """logits (n, C) f32 | bf16, labels (n) int64 -> (sums (4) f32 = [ce_sum, n_valid, lovasz_sum, n_present], rowstat (n, 2),
    glov (C, n) | None, present (C) int32 | None).  class_seen: (C) uint8 mask on the device or None."""
    n, C = _seg_operands(logits, labels)
    dev = logits.device
    if class_seen is not None:
        _req(class_seen, torch.uint8, "class_seen", (C,))
    rowstat = torch.empty((n, 2), dtype=torch.float32, device=dev)
    glov = torch.empty((C, n), dtype=torch.float32, device=dev) if lovasz else None
    present = torch.empty(C, dtype=torch.int32, device=dev) if lovasz else None
    sums = torch.empty(4, dtype=torch.float32, device=dev)
    ws = _ws(lib().ss_seg_loss_workspace_bytes(n, C), dev)
    check(lib().ss_seg_loss_fwd(_p(logits), dtype_code(logits), _p(labels), n, C, int(ignore_index), _p(class_seen), int(bool(lovasz)),
                                _p(rowstat), _p(glov), _p(present), _p(sums), _p(ws), ws.numel(), _stream()), "ss_seg_loss_fwd")
    return sums, rowstat, glov, present


def seg_loss_bwd(logits, labels, ignore_index, rowstat, glov, present, coef):
    """-> dlogits (n, C) in the logits' dtype.  coef (2) f32 on the device = dL/d[ce_sum, lovasz_sum]."""
    n, C = _seg_operands(logits, labels)
    _req(rowstat, torch.float32, "rowstat", (n, 2)); _req(coef, torch.float32, "coef", (2,))
    if glov is not None:
        _req(glov, torch.float32, "glov", (C, n)); _req(present, torch.int32, "present", (C,))
    dlogits = torch.empty_like(logits)
    check(lib().ss_seg_loss_bwd(_p(logits), dtype_code(logits), _p(labels), n, C, int(ignore_index), _p(rowstat), _p(glov),
                                _p(present), _p(coef), _p(dlogits), _stream()), "ss_seg_loss_bwd")
    return dlogits


def seg_iou(target, num_classes, ignore_index, logits=None, pred=None):
    """-> (3, C) int64 [intersection, union, target] of intersection_and_union_gpu(pred | argmax(logits), target, C, ignore_index)."""
    n = target.shape[0]
    _req(target, torch.int64, "target", (n,))
    C = int(num_classes)
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise RuntimeError(f"seg_iou: 1 <= num_classes <= {SEG_MAX_CLASSES}")
    if pred is not None:
        _req(pred, torch.int32, "pred", (n,))
        dt = F32
    else:
        _req(logits, None, "logits", (n, C))
        dt = dtype_code(logits)
    out = torch.empty((3, C), dtype=torch.int64, device=target.device)
    check(lib().ss_seg_iou(_p(logits), dt, _p(pred), _p(target), n, C, int(ignore_index), _p(out), _stream()), "ss_seg_iou")
    return out


# ---- open-vocabulary test stage: the steps after the accumulation (csrc/tester.hip) ---------------------------------------
VOCAB_MAX_K = 8


def vocab_finish(pred, k=1, threshold=0.0, ignore_index=-1, inverse=None, lut=None):
    """pred (n, C) f32 -> out (m, k) int32: the k classes of every row by descending value (equal values: the lower class first);
    k == 1: ignore_index where the maximum is < threshold; lut (C + 1) int32 maps [ignore_index, class 0, ...]; inverse (m) int64
    expands out[j] = labels[inverse[j]] (engines/test.py:372-394)."""
    _req(pred, torch.float32, "pred")
    if pred.dim() != 2 or not 1 <= pred.shape[1] <= SEG_MAX_CLASSES:
        raise RuntimeError(f"vocab_finish: pred must be (n, C) with 1 <= C <= {SEG_MAX_CLASSES}")
    n, C = pred.shape
    k = int(k)
    if not 1 <= k <= min(C, VOCAB_MAX_K):
        raise RuntimeError(f"vocab_finish: 1 <= k <= min(C, {VOCAB_MAX_K})")
    m = n
    if inverse is not None:
        _req(inverse, torch.int64, "inverse")
        if inverse.dim() != 1:
            raise RuntimeError("inverse: expected a 1-d tensor")
        m = inverse.shape[0]
    if lut is not None:
        _req(lut, torch.int32, "lut", (C + 1,))
    out = torch.empty((m, k), dtype=torch.int32, device=pred.device)
    if m == 0:                    # (an empty tensor's pointer is NULL, which the entry point would read as "no inverse")
        return out
    if n == 0:
        raise RuntimeError("vocab_finish: inverse into a pred without rows")
    ws = _ws(lib().ss_vocab_finish_workspace_bytes(n, k, m), pred.device) if inverse is not None else None
    check(lib().ss_vocab_finish(_p(pred), n, C, k, float(threshold), int(ignore_index), _p(inverse), m, _p(lut), _p(out), _p(ws),
                                ws.numel() if ws is not None else 0, _stream()), "ss_vocab_finish")
    return out


def cluster_vote(pred, instance_dense, num_instances, num_classes, ignore_index):
    """pred (m) int32 in {ignore_index} U [0, C), instance_dense (m) int32 in [0, num_instances) or < 0 -> out (m) int32: every
    row of an instance takes the instance's most frequent pred (equal counts: the smallest value; utils/misc.py:98-125)."""
    m = pred.shape[0]
    _req(pred, torch.int32, "pred", (m,))
    _req(instance_dense, torch.int32, "instance_dense", (m,))
    C, ni = int(num_classes), int(num_instances)
    if not 1 <= C <= SEG_MAX_CLASSES or ni < 0:
        raise RuntimeError(f"cluster_vote: 1 <= num_classes <= {SEG_MAX_CLASSES}, num_instances >= 0")
    out = torch.empty(m, dtype=torch.int32, device=pred.device)
    ws = _ws(lib().ss_cluster_vote_workspace_bytes(ni, C), pred.device)
    check(lib().ss_cluster_vote(_p(pred), _p(instance_dense), m, ni, C, int(ignore_index), _p(out), _p(ws), ws.numel(), _stream()),
          "ss_cluster_vote")
    return out


# ---- rows ------------------------------------------------------------------------------------
def gather_rows(src, idx, out=None):
    """out[i] = src[idx[i]] (zero row where idx < 0).  src (m, C)."""
    _req(src, None, "src"); _req(idx, torch.int32, "idx")
    n = idx.numel()
    if src.dim() != 2:
        raise RuntimeError("src must be (rows, C)")
    rb = src.shape[1] * src.element_size()
    if out is None:
        out = torch.empty((n, src.shape[1]), dtype=src.dtype, device=src.device)
    else:
        _req(out, src.dtype, "out", (n, src.shape[1]))
    check(lib().ss_gather_rows(_p(src), _p(idx), _p(out), n, rb, _stream()), "ss_gather_rows")
    return out


def scatter_rows(src, idx, dst):
    """dst[idx[i]] = src[i] for idx[i] >= 0 (idx unique)."""
    _req(src, None, "src"); _req(idx, torch.int32, "idx", (src.shape[0],)); _req(dst, src.dtype, "dst")
    if dst.shape[1] != src.shape[1]:
        raise RuntimeError("row width mismatch")
    rb = src.shape[1] * src.element_size()
    check(lib().ss_scatter_rows(_p(src), _p(idx), _p(dst), src.shape[0], rb, _stream()), "ss_scatter_rows")
    return dst


def gather_add_rows(a, b, idx):
    n, C = a.shape
    _req(a, None, "a"); _req(b, a.dtype, "b"); _req(idx, torch.int32, "idx", (n,))
    if b.shape[1] != C:
        raise RuntimeError("channel mismatch")
    out = torch.empty_like(a)
    check(lib().ss_gather_add_rows(_p(a), _p(b), _p(idx), _p(out), n, C, dtype_code(a), _stream()), "ss_gather_add_rows")
    return out


# ---- per-sample Gaussian augmentations (csrc/augment.hip) -----------------------------------
def _hf(values, count, name):
    """A few host floats that travel as kernel arguments -> ctypes float array (None stays NULL)."""
    if values is None:
        return None
    v = [float(x) for x in values]
    if len(v) != count:
        raise RuntimeError(f"{name}: expected {count} values, got {len(v)}")
    return (ctypes.c_float * count)(*v)


def _rows3(t, name, cols=3):
    _req(t, torch.float32, name)
    if t.dim() != 2 or t.shape[1] != cols:
        raise RuntimeError(f"{name}: expected (n, {cols}), got {tuple(t.shape)}")
    return t


def aug_bbox(x, affine=None):
    """(6,) f32 device tensor {min xyz, max xyz} of x (n, 3), or of A x + b for affine = 12 host floats (A row-major, then b)."""
    _rows3(x, "x")
    n = x.shape[0]
    if n < 1:
        raise RuntimeError("aug_bbox: empty input")
    part = torch.empty((lib().ss_aug_bbox_blocks(n), 6), dtype=torch.float32, device=x.device)
    out = torch.empty(6, dtype=torch.float32, device=x.device)
    check(lib().ss_aug_bbox(_p(x), n, _hf(affine, 12, "affine"), _p(part), _p(out), _stream()), "ss_aug_bbox")
    return out


def aug_gaussians_(coord=None, quat=None, scale=None, normal=None, affine=None, rquat=None, flip=0, scale_mul=None, lin=None,
                   jitter=None, noise=None, seed=0):
    """The fused rigid pass, in place (see include/scenesplat_hip.h).  jitter = (sigma, clip) or None; noise (n, 3) replays
    recorded N(0,1) draws, otherwise the kernel draws them from `seed`."""
    n = None
    for t, name, cols in ((coord, "coord", 3), (quat, "quat", 4), (scale, "scale", 3), (normal, "normal", 3), (noise, "noise", 3)):
        if t is None:
            continue
        _rows3(t, name, cols)
        if n is not None and t.shape[0] != n:
            raise RuntimeError(f"{name}: {t.shape[0]} rows, expected {n}")
        n = t.shape[0]
    if n is None:
        return
    sigma, clip = (0.0, 0.0) if jitter is None else (float(jitter[0]), float(jitter[1]))
    check(lib().ss_aug_gaussians(_p(coord), _p(quat), _p(scale), _p(normal), n, _hf(affine, 12, "affine"), _hf(rquat, 4, "rquat"),
                                 int(flip), _hf(scale_mul, 3, "scale_mul"), _hf(lin, 9, "lin"), int(jitter is not None), sigma, clip,
                                 _p(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "ss_aug_gaussians")


def aug_elastic_(coord, noise, origin, granularity, magnitude):
    """coord += trilinear(noise (d0, d1, d2, 3), coord) * magnitude, in place; node i at origin + i * granularity."""
    _rows3(coord, "coord"); _req(noise, torch.float32, "noise")
    if noise.dim() != 4 or noise.shape[3] != 3:
        raise RuntimeError(f"noise: expected (d0, d1, d2, 3), got {tuple(noise.shape)}")
    d0, d1, d2 = noise.shape[:3]
    check(lib().ss_aug_elastic(_p(coord), coord.shape[0], _p(noise), d0, d1, d2, _hf(origin, 3, "origin"), float(granularity),
                               float(magnitude), _stream()), "ss_aug_elastic")


AUG_COLOR_CONTRAST, AUG_COLOR_TRANSLATE, AUG_COLOR_JITTER = 1, 2, 4


def aug_color_(color, flags=0, lo=None, hi=None, blend=0.0, tr=None, jitter_std=0.0, noise=None, seed=0, normalize=False):
    """The colour steps on color (n, 3), 0..255, in place: contrast blend, translation + clip, jitter + clip, c / 127.5 - 1."""
    _rows3(color, "color")
    if noise is not None:
        _rows3(noise, "noise")
        if noise.shape[0] != color.shape[0]:
            raise RuntimeError("noise: row count differs from color")
    check(lib().ss_aug_color(_p(color), color.shape[0], int(flags), _hf(lo, 3, "lo"), _hf(hi, 3, "hi"), float(blend),
                             _hf(tr, 3, "tr"), float(jitter_std), _p(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(normalize)),
                             _stream()), "ss_aug_color")


def _hd(values, count, name):
    """A few host doubles that travel as kernel arguments -> ctypes double array (None stays NULL)."""
    if values is None:
        return None
    v = [float(x) for x in values]
    if len(v) != count:
        raise RuntimeError(f"{name}: expected {count} values, got {len(v)}")
    return (ctypes.c_double * count)(*v)


def aug_hsv_(color, hue_val, sat_ratio):
    """HueSaturationTranslation's pass on color (n, 3), 0..255, in place: the reference's fp64 HSV round trip, truncated to integers."""
    _rows3(color, "color")
    check(lib().ss_aug_hsv(_p(color), color.shape[0], _hd((hue_val, sat_ratio), 2, "hue_sat"), _stream()), "ss_aug_hsv")
    return color


def aug_moments(x, affine=None):
    """(4,) f64 device tensor {sum x, sum y, sum z, max squared norm} of x (n, 3) f32, or of A x + b for affine = 12 host doubles."""
    _rows3(x, "x")
    n = x.shape[0]
    if n < 1:
        raise RuntimeError("aug_moments: empty input")
    part = torch.empty((lib().ss_aug_moments_blocks(n), 4), dtype=torch.float64, device=x.device)
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    check(lib().ss_aug_moments(_p(x), n, _hd(affine, 12, "affine"), _p(part), _p(out), _stream()), "ss_aug_moments")
    return out


INSTANCE_MAX_VACANCY = 16


def instance_boxes(coord, segment, order, idx_ptr, K, vacancy=()):
    """-> bbox (K, 8) f32, centroid (K, 3) f32 of the K leading runs of the CSR (order, idx_ptr); see include/scenesplat_hip.h."""
    _rows3(coord, "coord")
    n, K = coord.shape[0], int(K)
    _req(segment, torch.int64, "segment", (n,)); _req(order, torch.int32, "order"); _req(idx_ptr, torch.int32, "idx_ptr")
    if K < 0 or (K > 0 and (idx_ptr.numel() < K + 1 or order.numel() > n)):
        raise RuntimeError("instance_boxes: idx_ptr shorter than K + 1, or order longer than coord")
    vac = [int(v) for v in vacancy]
    if len(vac) > INSTANCE_MAX_VACANCY:
        raise RuntimeError(f"instance_boxes: at most {INSTANCE_MAX_VACANCY} non-negative ignore indices, got {len(vac)}")
    bbox = torch.empty((K, 8), dtype=torch.float32, device=coord.device)
    centroid = torch.empty((K, 3), dtype=torch.float32, device=coord.device)
    check(lib().ss_instance_boxes(_p(coord), _p(segment), _p(order), _p(idx_ptr), K, (ctypes.c_int64 * len(vac))(*vac) if vac else None,
                                  len(vac), _p(bbox), _p(centroid), _stream()), "ss_instance_boxes")
    return bbox, centroid


def instance_scatter_(instance, cluster, K, centroid, ignore_index):
    """instance (n,) int32 / int64 <- dense id per row, in place; -> instance_centroid (n, 3) f32.  Rows of a run >= K: ignore_index."""
    _req(instance, None, "instance")
    if instance.dim() != 1 or instance.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"instance: expected (n,) int32 / int64, got {tuple(instance.shape)} {instance.dtype}")
    n, K = instance.shape[0], int(K)
    if K > 0:
        _req(cluster, torch.int32, "cluster", (n,)); _req(centroid, torch.float32, "centroid", (K, 3))
    out = torch.empty((n, 3), dtype=torch.float32, device=instance.device)
    check(lib().ss_instance_scatter(_p(cluster) if K > 0 else None, n, K, _p(centroid) if K > 0 else None, _p(instance),
                                    int(instance.dtype == torch.int64), int(ignore_index), _p(out), _stream()), "ss_instance_scatter")
    return out


# ---- the SSL view generator's colour chain and sparse voxel blur (csrc/ssl_views.hip) --------
CHAIN_BRIGHTNESS, CHAIN_CONTRAST, CHAIN_SATURATION, CHAIN_HUE, CHAIN_GRAY = 1, 2, 3, 4, 5
CHAIN_MAX_STEPS = 8


def color_chain_(color, steps):
    """steps = [(code, factor), ...] (at most 8) on color (n, 3), 0..255, in place and in ONE pass, plus one reduction pass per
    contrast step (its mean gray stays on the device).  See include/scenesplat_hip.h for the formulas."""
    _rows3(color, "color")
    steps = [(int(c), float(f)) for c, f in steps]
    if len(steps) > CHAIN_MAX_STEPS:
        raise RuntimeError(f"color_chain_: at most {CHAIN_MAX_STEPS} steps, got {len(steps)}")
    n = color.shape[0]
    if not steps or n == 0:
        return color
    part = means = None
    if any(c == CHAIN_CONTRAST for c, _ in steps):
        part = torch.empty(lib().ss_color_chain_blocks(n), dtype=torch.float32, device=color.device)
        means = torch.empty(CHAIN_MAX_STEPS, dtype=torch.float32, device=color.device)
    codes = (ctypes.c_int * len(steps))(*[c for c, _ in steps])
    check(lib().ss_color_chain(_p(color), n, len(steps), codes, _hf([f for _, f in steps], len(steps), "factors"), _p(part), _p(means),
                               _stream()), "ss_color_chain")
    return color


def voxel_blur_(grid_coord, mask, color, sigma, opacity=None, scale=None, quat=None, normal=None, normalize_quat=False):
    """GSGaussianBlurVoxelOpc's blur over the occupied voxels only, in place on the rows where mask (n,) bool is set (None: all):
    color and the optional opacity (n, 1) / scale / quat / normal become the Gaussian-weighted mean over the masked voxels of
    their (2r+1)^3 neighbourhood; normalize_quat then divides EVERY row of quat by its norm.  grid_coord (n, 3) int32 with unique
    rows.  -> the device int32 status word (0 = done; 1 = an axis spans 2^21 cells or more and nothing was blurred); reading it
    is a sync the caller may or may not want."""
    _req(grid_coord, torch.int32, "grid_coord")
    n = grid_coord.shape[0]
    if grid_coord.dim() != 2 or grid_coord.shape[1] != 3:
        raise RuntimeError(f"grid_coord: expected (n, 3), got {tuple(grid_coord.shape)}")
    _rows3(color, "color")
    for t, name, cols in ((opacity, "opacity", 1), (scale, "scale", 3), (quat, "quat", 4), (normal, "normal", 3)):
        if t is not None:
            _req(t, torch.float32, name)
            if t.numel() != n * cols or (t.dim() == 2 and t.shape[1] != cols):
                raise RuntimeError(f"{name}: expected (n, {cols}) with n = {n}, got {tuple(t.shape)}")
    if color.shape[0] != n:
        raise RuntimeError(f"color: {color.shape[0]} rows, grid_coord has {n}")
    if mask is not None:
        _req(mask, None, "mask", (n,))
        if mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError(f"mask: expected bool or uint8, got {mask.dtype}")
    nbytes = lib().ss_voxel_blur_workspace_bytes(n)
    ws = _ws(nbytes, grid_coord.device)
    check(lib().ss_voxel_blur(_p(grid_coord), _p(mask), n, _p(color), _p(opacity), _p(scale), _p(quat), _p(normal),
                              int(bool(normalize_quat)), float(sigma), _p(ws), ws.numel(), _stream()), "ss_voxel_blur")
    return ws[24:28].view(torch.int32)


def voxel_pick_labelled(order, idx_ptr, n_cells, label=None, ignore_index=-1):
    """chosen (n_cells,) int32: per cell of the CSR (order, idx_ptr) that pool_partition wrote, the first member whose label (int64,
    per row) is not ignore_index; the first member when the cell has none or label is None."""
    n_cells = int(n_cells)
    _req(order, torch.int32, "order"); _req(idx_ptr, torch.int32, "idx_ptr")
    if n_cells < 0 or idx_ptr.numel() < n_cells + 1:
        raise RuntimeError("idx_ptr shorter than n_cells + 1")
    if label is not None:
        _req(label, torch.int64, "label")
        if label.dim() != 1 or label.shape[0] < order.numel():
            raise RuntimeError(f"label: expected one int64 per row of order ({order.numel()}), got {tuple(label.shape)}")
    chosen = torch.empty(n_cells, dtype=torch.int32, device=order.device)
    check(lib().ss_voxel_pick_labelled(_p(order), _p(idx_ptr), n_cells, _p(label), int(ignore_index), _p(chosen), _stream()),
          "ss_voxel_pick_labelled")
    return chosen


def segment_reduce(src, indices, idx_ptr, n_seg, mean):
    _req(src, None, "src"); _req(idx_ptr, torch.int32, "idx_ptr")
    if indices is not None:
        _req(indices, torch.int32, "indices")
    if idx_ptr.numel() < n_seg + 1:
        raise RuntimeError("idx_ptr shorter than n_seg+1")
    C = src.shape[1]
    out = torch.empty((n_seg, C), dtype=src.dtype, device=src.device)
    check(lib().ss_segment_reduce(_p(src), _p(indices), _p(idx_ptr), _p(out), n_seg, C, dtype_code(src), int(mean),
                                  _stream()), "ss_segment_reduce")
    return out


def segment_minmax(src, indices, idx_ptr, n_seg, is_max):
    """-> (out (n_seg,C), arg (n_seg,C) int32 source rows)"""
    _req(src, None, "src"); _req(idx_ptr, torch.int32, "idx_ptr")
    if indices is not None:
        _req(indices, torch.int32, "indices")
    if idx_ptr.numel() < n_seg + 1:
        raise RuntimeError("idx_ptr shorter than n_seg+1")
    C = src.shape[1]
    out = torch.empty((n_seg, C), dtype=src.dtype, device=src.device)
    arg = torch.empty((n_seg, C), dtype=torch.int32, device=src.device)
    check(lib().ss_segment_minmax(_p(src), _p(indices), _p(idx_ptr), _p(out), _p(arg), n_seg, C, dtype_code(src), int(is_max),
                                  _stream()), "ss_segment_minmax")
    return out, arg


def segment_minmax_bwd(dout, arg, n_src):
    _req(dout, None, "dout"); _req(arg, torch.int32, "arg", tuple(dout.shape))
    n_seg, C = dout.shape
    dsrc = torch.zeros((n_src, C), dtype=dout.dtype, device=dout.device)
    check(lib().ss_segment_minmax_bwd(_p(dout), _p(arg), _p(dsrc), n_seg, C, dtype_code(dout), _stream()), "ss_segment_minmax_bwd")
    return dsrc


def segment_bcast(dout, cluster, idx_ptr, mean):
    _req(dout, None, "dout"); _req(cluster, torch.int32, "cluster"); _req(idx_ptr, torch.int32, "idx_ptr")
    n, C = cluster.numel(), dout.shape[1]
    dsrc = torch.empty((n, C), dtype=dout.dtype, device=dout.device)
    check(lib().ss_segment_bcast(_p(dout), _p(cluster), _p(idx_ptr), _p(dsrc), n, C, dtype_code(dout), int(mean),
                                 _stream()), "ss_segment_bcast")
    return dsrc


# ---- attention -------------------------------------------------------------------------------
def window_attn_fwd(qkv, win, num_heads, scale, impl):
    n, C3 = qkv.shape
    C = C3 // 3
    _req(qkv, None, "qkv")
    if n != win.n:
        raise RuntimeError(f"qkv rows {n} != window index rows {win.n}")
    out = torch.empty((n, C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((win.n_pad, num_heads), dtype=torch.float32, device=qkv.device)
    check(lib().ss_window_attn_fwd(_p(qkv), _p(win.gidx), _p(win.sidx), _p(win.win_start), win.num_windows,
                                   win.max_window, n, win.n_pad, C, num_heads, float(scale), dtype_code(qkv), int(impl),
                                   _p(out), _p(lse), _stream()), "ss_window_attn_fwd")
    return out, lse


def window_attn_bwd(qkv, out, dout, lse, win, num_heads, scale, impl):
    n, C3 = qkv.shape
    C = C3 // 3
    _req(qkv, None, "qkv"); _req(out, qkv.dtype, "out", (n, C)); _req(dout, qkv.dtype, "dout", (n, C))
    _req(lse, torch.float32, "lse", (win.n_pad, num_heads))
    dqkv = torch.empty_like(qkv)
    nb = lib().ss_window_attn_bwd_workspace_bytes(n, win.n_pad, C, num_heads, dtype_code(qkv))
    ws = _ws(nb, qkv.device)
    check(lib().ss_window_attn_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(win.gidx), _p(win.sidx), _p(win.win_start),
                                   win.num_windows, win.max_window, n, win.n_pad, C, num_heads, float(scale),
                                   dtype_code(qkv), int(impl), _p(dqkv), _p(ws), ws.numel(), _stream()),
          "ss_window_attn_bwd")
    return dqkv


# ---- window attention with relative position encoding (csrc/attention.hip; kernels: attention_rpe.hip, attention_simt.hip) ----
def _req_rpe(qkv, win, num_heads, grid_coord, table, pos_bnd):
    n, C3 = qkv.shape
    _req(qkv, None, "qkv")
    if n != win.n:
        raise RuntimeError(f"qkv rows {n} != window index rows {win.n}")
    pos_bnd = int(pos_bnd)
    _req(grid_coord, torch.int32, "grid_coord", (n, 3))
    _req(table, torch.float32, "table", (3 * (2 * pos_bnd + 1), num_heads))
    return n, C3 // 3, pos_bnd


def window_attn_rpe_fwd(qkv, win, grid_coord, table, pos_bnd, num_heads, scale, impl):
    """window_attn_fwd with the RPE bias table[clamp(g_i - g_j) + pos_bnd] (three axes) added to every score."""
    n, C, pos_bnd = _req_rpe(qkv, win, num_heads, grid_coord, table, pos_bnd)
    out = torch.empty((n, C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((win.n_pad, num_heads), dtype=torch.float32, device=qkv.device)
    check(lib().ss_window_attn_rpe_fwd(_p(qkv), _p(win.gidx), _p(win.sidx), _p(win.win_start), win.num_windows,
                                       win.max_window, n, win.n_pad, C, num_heads, float(scale), dtype_code(qkv), int(impl),
                                       _p(grid_coord), _p(table), pos_bnd, _p(out), _p(lse), _stream()),
          "ss_window_attn_rpe_fwd")
    return out, lse


def window_attn_rpe_bwd_workspace_bytes(qkv, win, num_heads, pos_bnd):
    n, C3 = qkv.shape
    return lib().ss_window_attn_rpe_bwd_workspace_bytes(n, win.n_pad, C3 // 3, num_heads, dtype_code(qkv), win.num_windows,
                                                        win.max_window, int(pos_bnd))


def window_attn_rpe_bwd(qkv, out, dout, lse, win, grid_coord, table, pos_bnd, num_heads, scale, impl, workspace=None):
    """-> (dqkv, dtable fp32).  `workspace`: optional uint8 buffer of window_attn_rpe_bwd_workspace_bytes (any content)."""
    n, C, pos_bnd = _req_rpe(qkv, win, num_heads, grid_coord, table, pos_bnd)
    _req(out, qkv.dtype, "out", (n, C)); _req(dout, qkv.dtype, "dout", (n, C))
    _req(lse, torch.float32, "lse", (win.n_pad, num_heads))
    dqkv = torch.empty_like(qkv)
    dtable = torch.empty_like(table)
    nb = window_attn_rpe_bwd_workspace_bytes(qkv, win, num_heads, pos_bnd)
    ws = _ws(nb, qkv.device) if workspace is None else _req(workspace, torch.uint8, "workspace")
    check(lib().ss_window_attn_rpe_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(win.gidx), _p(win.sidx), _p(win.win_start),
                                       win.num_windows, win.max_window, n, win.n_pad, C, num_heads, float(scale),
                                       dtype_code(qkv), int(impl), _p(grid_coord), _p(table), pos_bnd, _p(dqkv), _p(dtable),
                                       _p(ws), ws.numel(), _stream()), "ss_window_attn_rpe_bwd")
    return dqkv, dtable


# ---- head-major window attention (csrc/attention_hm.hip, round 3)------------------------------------------------------
LOG2E = 1.4426950408889634


def headmajor_eligible(k):
    """The projection can write the head-major layout from its own epilogue (gemm8.hip) when k is a multiple of 64."""
    return k >= 64 and k % 64 == 0


def linear_fwd_headmajor(x, win, w, bias, num_heads, sec0_scale):
    """hm (sections, H, n_pad, D) bf16 = head-major, window-ordered x[gidx] @ w.T + bias; section 0 times sec0_scale (fp32,
    before the one bf16 rounding).  x (n, k) bf16, w (sections * C, k) bf16, bias (sections * C) f32 or None."""
    n, k = x.shape
    nout = w.shape[0]
    _req(x, torch.bfloat16, "x"); _req(w, torch.bfloat16, "weight", (nout, k))
    if bias is not None:
        _req(bias, torch.float32, "bias", (nout,))
    if n != win.n:
        raise RuntimeError(f"x rows {n} != window index rows {win.n}")
    C = k
    if nout % C:
        raise RuntimeError("output width must be a multiple of the channel count")
    hm = torch.empty((nout // C, num_heads, win.n_pad, C // num_heads), dtype=torch.bfloat16, device=x.device)
    check(lib().ss_linear_fwd_headmajor(_p(x), _p(win.gidx), _p(w), _p(bias), _p(hm), win.n_pad, k, nout, C, C // num_heads,
                                        float(sec0_scale), _stream()), "ss_linear_fwd_headmajor")
    return hm


def headmajor_pack(src, win, num_heads, sections, sec0_scale):
    """hm (sections, H, n_pad, D) bf16 from an (n, sections * C) projection (fp32 or bf16) in memory row order."""
    n, w = src.shape
    _req(src, None, "src")
    C = w // sections
    hm = torch.empty((sections, num_heads, win.n_pad, C // num_heads), dtype=torch.bfloat16, device=src.device)
    check(lib().ss_headmajor_pack(_p(src), dtype_code(src), _p(win.gidx), _p(hm), win.n_pad, C, num_heads, sections,
                                  float(sec0_scale), _stream()), "ss_headmajor_pack")
    return hm


def window_attn_hm_fwd(hm, win, num_heads):
    _req(hm, torch.bfloat16, "hm")
    sections, H, n_pad, D = hm.shape
    if sections != 3 or H != num_heads or n_pad != win.n_pad:
        raise RuntimeError(f"hm shape {tuple(hm.shape)} does not match the window index (n_pad {win.n_pad}, heads {num_heads})")
    C = H * D
    out = torch.empty((win.n, C), dtype=torch.bfloat16, device=hm.device)
    nlse2 = torch.empty((H, n_pad), dtype=torch.float32, device=hm.device)
    check(lib().ss_window_attn_hm_fwd(_p(hm), _p(win.sidx), _p(win.win_start), win.num_windows, win.max_window, win.n, n_pad, C,
                                      H, _p(out), _p(nlse2), _stream()), "ss_window_attn_hm_fwd")
    return out, nlse2


def window_attn_hm_bwd(hm, out, dout, nlse2, win, num_heads, scale):
    sections, H, n_pad, D = hm.shape
    C = H * D
    _req(out, torch.bfloat16, "out", (win.n, C)); _req(dout, torch.bfloat16, "dout", (win.n, C))
    _req(nlse2, torch.float32, "nlse2", (H, n_pad))
    dqkv = torch.empty((win.n, 3 * C), dtype=torch.bfloat16, device=hm.device)
    nb = lib().ss_window_attn_hm_bwd_workspace_bytes(win.n, n_pad, C, H)
    ws = _ws(nb, hm.device)
    check(lib().ss_window_attn_hm_bwd(_p(hm), _p(out), _p(dout), _p(nlse2), _p(win.gidx), _p(win.sidx), _p(win.win_start),
                                      win.num_windows, win.max_window, win.n, n_pad, C, H, float(scale), _p(dqkv), _p(ws),
                                      ws.numel(), _stream()), "ss_window_attn_hm_bwd")
    return dqkv


def stream_capture_status(stream=None):
    """0 = not capturing, 1 = capturing, 2 = the capture was invalidated (it must be abandoned, never ended), -1 = unknown."""
    st = stream if stream is not None else torch.cuda.current_stream()
    return int(lib().ss_stream_capture_status(ctypes.c_void_p(st.cuda_stream)))


def gelu(x, dy=None):
    """Exact-erf GELU on the HIP kernel: gelu(x), or dy * gelu'(x) when dy is given.  x (any shape) bf16 | f32, contiguous."""
    _req(x, None, "x")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"gelu: float32 / bfloat16 only, got {x.dtype}")
    if dy is not None:
        _req(dy, x.dtype, "dy", x.shape)
    out = torch.empty_like(x)
    check(lib().ss_gelu(_p(x), _p(dy), _p(out), x.numel(), dtype_code(x), _stream()), "ss_gelu")
    return out


def row_keep_scales(keep, seed=None):
    """keep (n) f32 in (0, 1] -> (n) f32 of Bernoulli(keep) / keep, one Philox draw per row.  seed: (1,) int64 DEVICE tensor; None draws
    it from torch's generator of the device (graph-safe: a captured call gets a fresh seed on every replay)."""
    _req(keep, torch.float32, "keep")
    if seed is None:
        seed = torch.randint(-(1 << 62), 1 << 62, (1,), dtype=torch.int64, device=keep.device)
    _req(seed, torch.int64, "seed", (1,))
    out = torch.empty_like(keep)
    check(lib().ss_row_keep_scales(_p(seed), _p(keep), _p(out), keep.numel(), _stream()), "ss_row_keep_scales")
    return out


def stream_capture_id(stream=None):
    """> 0: identity of the capture the stream is recording into; 0: not capturing."""
    st = stream if stream is not None else torch.cuda.current_stream()
    return int(lib().ss_stream_capture_id(ctypes.c_void_p(st.cuda_stream)))


def cast_bf16_group(srcs, dsts):
    """ONE launch: dst (bf16) = src (fp32) for every pair of equally shaped contiguous tensors (the weight shadows)."""
    if not srcs:
        return
    dev = srcs[0].device
    per = lib().ss_cast_bf16_group_elems_per_workgroup()
    desc = np.zeros((len(srcs), 3), dtype=np.int64)
    for j, (s, d) in enumerate(zip(srcs, dsts)):
        if s.dtype != torch.float32 or d.dtype != torch.bfloat16 or s.numel() != d.numel() or not (s.is_contiguous() and d.is_contiguous()):
            raise RuntimeError("cast_bf16_group: contiguous fp32 -> bf16 pairs of equal size")
        desc[j] = (s.data_ptr(), d.data_ptr(), s.numel())
    grouped.launch("ss_cast_bf16_group", desc, grouped.starts(_div_up(desc[:, 2], per)), dev)


# ---- scene ingest: every asset of a packed scene arena -> its output tensor in one grouped launch (csrc/ingest.hip) ----------------
INGEST_CODES = {"float64": 0, "float32": 1, "float16": 2, "uint8": 3, "int8": 4, "int16": 5, "int32": 6, "int64": 7, "bool": 8}
INGEST_HAS_LO, INGEST_HAS_HI, INGEST_PICK = 1, 2, 4
INGEST_ALIGN = 256          # arena offsets: an asset that needs no conversion is handed out as a view of the arena
_INGEST_INT = ("uint8", "int8", "int16", "int32", "int64", "bool")


def ingest_pair_on_device(src, dst):
    """Does the kernel convert numpy dtype `src` to `dst` itself?  (f64 -> f16 would round twice on the way through f32, and a
    float -> int / bool cast has numpy's own corner cases: those are converted on the host before packing.)"""
    if src not in INGEST_CODES or dst not in INGEST_CODES:
        return False
    return src == dst or dst == "float32" or (dst == "float16" and src == "float32") or (dst in ("int32", "bool") and src in _INGEST_INT)


def ingest_plan(arrays, rules):
    """The launch of one scene as a pure host function.  arrays: {stored name: ndarray}, in packing order.  rules: {stored name:
    dict(name=output key, dtype=target numpy dtype name | None (as stored), lo=, hi= (clip bounds of an f32 target), shape="keep" |
    "flat" | "col1" (n, 1) | "column" ([:, column]) | "column_or_flat" (the column of a 2-d array, else flattened), column=0)}; a
    name without a rule is passed through as stored.
    -> (desc (k, 8) int64: the rows of ss_ingest_group with word 0 = the BYTE OFFSET of the asset in the arena and word 1 = 0 (the
        caller adds the arena's address and fills in the outputs'),
        offsets {stored name: byte offset, a multiple of INGEST_ALIGN; "" : the arena's size},
        specs [dict(stored, name, dtype, shape, alias (the arena's bytes ARE the output), array (what to pack))], one per row,
        fallback [stored names converted with numpy on the host])."""
    desc = np.zeros((len(arrays), 8), dtype=np.int64)
    offsets, specs, fallback, off = {}, [], [], 0
    for j, (stored, arr) in enumerate(arrays.items()):
        rule = rules.get(stored, {})
        arr = np.asarray(arr)
        if arr.dtype.byteorder == ">" or not arr.flags.c_contiguous:
            arr = np.ascontiguousarray(arr.astype(arr.dtype.newbyteorder("=")))
        src = arr.dtype.name
        dst = rule.get("dtype") or src
        lo, hi = rule.get("lo"), rule.get("hi")
        if (lo is not None or hi is not None) and dst != "float32":
            raise ValueError(f"ingest_plan: '{stored}': a clip needs a float32 target")
        if dst not in INGEST_CODES:
            raise TypeError(f"ingest_plan: '{stored}': dtype {dst} has no device form")
        if not ingest_pair_on_device(src, dst):
            with np.errstate(over="ignore", invalid="ignore"):
                arr = arr.astype(dst)                  # numpy's own conversion; the device pair becomes dst -> dst
            fallback.append(stored)
            src = dst
        shape_rule = rule.get("shape", "keep")
        flags = (INGEST_HAS_LO if lo is not None else 0) | (INGEST_HAS_HI if hi is not None else 0)
        stride = col = 0
        if shape_rule == "column_or_flat":
            shape_rule = "column" if arr.ndim == 2 else "flat"
        if shape_rule == "column":
            if arr.ndim != 2:
                raise IndexError(f"ingest_plan: '{stored}': [:, {rule.get('column', 0)}] of a {arr.ndim}-d array")
            stride, col = arr.shape[1], int(rule.get("column", 0)) % max(arr.shape[1], 1)
            shape, flags = (arr.shape[0],), flags | INGEST_PICK
        elif shape_rule == "flat":
            shape = (arr.size,)
        elif shape_rule == "col1":
            shape = (arr.size, 1)
        elif shape_rule == "keep":
            shape = tuple(arr.shape)
        else:
            raise ValueError(f"ingest_plan: shape rule '{shape_rule}'")
        n_out = int(np.prod(shape, dtype=np.int64))
        desc[j] = (off, 0, n_out, INGEST_CODES[src] | (INGEST_CODES[dst] << 8) | (flags << 16), stride, col,
                   int(np.float32(0.0 if lo is None else lo).view(np.uint32)), int(np.float32(0.0 if hi is None else hi).view(np.uint32)))
        offsets[stored] = off
        specs.append(dict(stored=stored, name=rule.get("name", stored), dtype=dst, shape=shape, alias=(src == dst and flags == 0), array=arr))
        off = _div_up(off + arr.nbytes, INGEST_ALIGN) * INGEST_ALIGN
    offsets[""] = off
    return desc, offsets, specs, fallback


def ingest_group(desc, dev):
    """ONE launch of ss_ingest_group over the rows of `desc` ((k, 8) int64 with real device addresses in words 0 and 1)."""
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    if desc.ndim != 2 or desc.shape[1] != 8:
        raise RuntimeError("ingest_group: desc must be (k, 8) int64")
    if desc.shape[0] == 0:
        return
    names = {v: k for k, v in INGEST_CODES.items()}
    for word, n_out, flags in zip(desc[:, 3].tolist(), desc[:, 2].tolist(), (desc[:, 3] >> 16).tolist()):
        s, d = names.get(word & 0xff), names.get((word >> 8) & 0xff)
        if s is None or d is None or not ingest_pair_on_device(s, d):
            raise RuntimeError(f"ingest_group: no device conversion {s} -> {d} (convert on the host before packing)")
        if n_out < 0 or ((flags & (INGEST_HAS_LO | INGEST_HAS_HI)) and d != "float32"):
            raise RuntimeError("ingest_group: negative size, or a clip on a target that is not float32")
    if ((desc[:, 2] > 0) & ((desc[:, 0] == 0) | (desc[:, 1] == 0))).any():
        raise RuntimeError("ingest_group: null pointer in a non-empty problem")
    per = lib().ss_ingest_group_elems_per_workgroup()
    grouped.launch("ss_ingest_group", desc, grouped.starts(_div_up(desc[:, 2], per)), dev)


# ---- optimizer step: global gradient norm + grouped AdamW update (csrc/optim.hip) ----------------------------------------------
_NORM_PARTIALS = {}    # device -> fp64 partial sums of the norm kernel, one per workgroup (grown on demand, reused every step)


def _norm_partials(dev, n):
    buf = _NORM_PARTIALS.get(dev)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(int(n), 1024), dtype=torch.float64, device=dev)
        _NORM_PARTIALS[dev] = buf
    return buf


def _optim_starts(numels):
    """numels: the descriptor column of element counts"""
    return grouped.starts(_div_up(numels, lib().ss_optim_group_elems_per_workgroup()))


def grad_norm_group(grads, max_norm, record=None):
    """-> record (2,) fp32 on the device: [total_norm, coef] with total_norm the 2-norm over ALL of `grads` and
    coef = min(1, max_norm / (total_norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s arithmetic.  Two launches, no host read;
    the gradients are only read.  `record`: an existing (2,) fp32 tensor to write into."""
    if record is not None:
        dev = _req(record, torch.float32, "record", (2,)).device
    else:
        dev = _req(grads[0], None, "grads[0]").device if len(grads) else torch.device("cuda", torch.cuda.current_device())
        record = torch.empty(2, dtype=torch.float32, device=dev)
    for j, g in enumerate(grads):
        _req_dense_f32(g, None, dev, f"grads[{j}]")
    grads = [g for g in grads if g.numel()]                  # (an empty tensor adds nothing and owns no workgroup)
    desc = np.empty((len(grads), 3), dtype=np.int64)
    desc[:, 0], desc[:, 1] = [g.data_ptr() for g in grads], [g.numel() for g in grads]
    desc[:, 2] = (desc[:, 0] & 15) == 0                      # bit 0: 16-byte lanes
    starts = _optim_starts(desc[:, 1])
    partials = _norm_partials(dev, starts[-1])
    if grads:
        grouped.launch("ss_grad_sqnorm_group", desc, starts, dev, _p(partials))
    check(lib().ss_grad_norm_finish(_p(partials), starts[-1], float(max_norm), _p(record), _stream()), "ss_grad_norm_finish")
    return record


def adamw_group(rows, record=None):
    """ONE launch: the AdamW update of every row (p, g, m, v, scalars) with scalars = (1 - lr*wd, 1 - beta1, beta2, 1 - beta2,
    sqrt(1 - beta2^t), eps, lr / (1 - beta1^t)) computed by the caller in double.  p, m, v are updated in place, g is only read;
    `record` (from grad_norm_group) scales g by its clip coefficient on the fly, None means no clipping."""
    if not len(rows):
        return
    dev = _req(rows[0][0], torch.float32, "rows[0].p").device
    if record is not None and _req(record, torch.float32, "record", (2,)).device != dev:
        raise RuntimeError("record: must live on the parameters' device")
    for j, (p, g, m, v, s) in enumerate(rows):
        for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
            _req_dense_f32(t, p.numel(), dev, f"rows[{j}].{nm}")
        if len(s) != 7:
            raise RuntimeError(f"rows[{j}]: 7 scalars per row")
    rows = [r for r in rows if r[0].numel()]
    if not rows:
        return
    desc = np.zeros((len(rows), 10), dtype=np.int64)
    for k in range(4):
        desc[:, k] = [r[k].data_ptr() for r in rows]
    desc[:, 4] = [r[0].numel() for r in rows]
    desc[:, 5] = ((desc[:, 0] | desc[:, 1] | desc[:, 2] | desc[:, 3]) & 15) == 0        # bit 0: 16-byte lanes
    desc[:, 6:].view(np.float32)[:, :7] = np.asarray([r[4] for r in rows], dtype=np.float64)   # fp32 over the last four words
    grouped.launch("ss_adamw_group", desc, _optim_starts(desc[:, 4]), dev, _p(record))


# ---- PDNorm prompt modulation of all PDNorm layers of a model: one grouped launch each way (csrc/pdnorm.hip) --------------------
PDNORM_WORDS = 14


class PDNormTable:
    """Host side of the descriptor table of a group of PDNorm layers under ONE condition: the columns that do not change from call
    to call (C, W, b, gamma, beta), built once and reused while the parameters stay where they are (`current`)."""

    def __init__(self, rows, context_channels):
        if not rows:
            raise RuntimeError("pdnorm: an empty group has no table")
        self.cc = int(context_channels)
        self.dev = _req(rows[0][0], torch.float32, "rows[0].W").device
        self.widths = []
        for j, (w, b, g, be) in enumerate(rows):
            if w.dim() != 2 or w.shape[0] % 2 or w.shape[1] != self.cc:
                raise RuntimeError(f"rows[{j}].W: expected (2C, {self.cc}), got {tuple(w.shape)}")
            c = w.shape[0] // 2
            _req_dense_f32(w, 2 * c * self.cc, self.dev, f"rows[{j}].W")
            _req_dense_f32(b, 2 * c, self.dev, f"rows[{j}].b")
            for t, nm in ((g, "gamma"), (be, "beta")):
                if t is not None:
                    _req_dense_f32(t, c, self.dev, f"rows[{j}].{nm}")
            self.widths.append(c)
        per = lib().ss_pdnorm_channels_per_workgroup()
        self.starts = grouped.starts(_div_up(c, per) for c in self.widths)
        self.sig = self.signature(rows)
        self.desc = np.zeros((len(rows), PDNORM_WORDS), dtype=np.int64)
        self.desc[:, 0] = self.widths
        self.desc[:, 1:5] = np.asarray(self.sig, dtype=np.int64).reshape(len(rows), 4)
        self.off = np.concatenate([[0], np.cumsum(self.widths)]).astype(np.int64)          # channel offsets of the layers
        self.w_off = np.concatenate([[0], np.cumsum([2 * c * self.cc for c in self.widths])]).astype(np.int64)
        self.vec4 = int(self.cc % 4 == 0 and not np.any(self.desc[:, 1] & 15))
        self.affine = [(g is not None, be is not None) for _, _, g, be in rows]

    @staticmethod
    def signature(rows):
        return tuple(t.data_ptr() if t is not None else 0 for r in rows for t in r)

    def current(self, rows):
        return self.signature(rows) == self.sig


def _pdnorm_context(context, tab):
    _req(context, torch.float32, "context")
    if context.numel() != tab.cc or context.device != tab.dev:
        raise RuntimeError(f"context: expected {tab.cc} values on {tab.dev} (one prompt per batch)")
    return context


def pdnorm_mod_fwd(context, tab):
    """-> (gamma_eff list, beta_eff list, ops): the folded affine pair of every layer of the table and 1 + scale (all channels of all
    layers in one tensor, for the backward).  ONE launch; the outputs are separate views of one allocation."""
    _pdnorm_context(context, tab)
    total = int(tab.off[-1])
    out = torch.empty(3 * total, dtype=torch.float32, device=tab.dev)
    desc = tab.desc.copy()
    base = out.data_ptr()
    desc[:, 5] = base + 4 * tab.off[:-1]
    desc[:, 6] = base + 4 * (total + tab.off[:-1])
    desc[:, 7] = base + 4 * (2 * total + tab.off[:-1])
    vec4 = int(tab.vec4 and context.data_ptr() % 16 == 0)
    grouped.launch("ss_pdnorm_mod_fwd", desc, tab.starts, tab.dev, _p(context), tab.cc, vec4)
    o = [int(x) for x in tab.off]
    geff = [out[o[l]:o[l + 1]] for l in range(len(tab.widths))]
    beff = [out[total + o[l]:total + o[l + 1]] for l in range(len(tab.widths))]
    return geff, beff, out[2 * total:]


def pdnorm_mod_bwd(context, tab, ops, dgeff, dbeff, split_row=0):
    """Backward of pdnorm_mod_fwd from the gradients the norm kernels returned for gamma_eff / beta_eff (None: that norm sent none).
    -> (dcontext (context's shape), dW list, db list, dgamma list, dbeta list); dgamma / dbeta are None for affine-free rows.
    ONE grouped launch plus the fixed-order finish of dcontext.  split_row: the rows below it and from it on contribute to dcontext
    as two launches over the two parts would (bit for bit): the unsplit form of a backward that may also run in two calls."""
    _pdnorm_context(context, tab)
    n = len(tab.widths)
    total = int(tab.off[-1])
    _req_dense_f32(ops, total, tab.dev, "ops")
    for l in range(n):
        for t, nm in ((dgeff[l], "dgamma_eff"), (dbeff[l], "dbeta_eff")):
            if t is not None:
                _req_dense_f32(t, tab.widths[l], tab.dev, f"{nm}[{l}]")
    wtot = int(tab.w_off[-1])
    out = torch.empty(wtot + 4 * total, dtype=torch.float32, device=tab.dev)      # dW | db (2 per channel) | dgamma | dbeta
    partials = torch.empty(tab.starts[-1] * tab.cc, dtype=torch.float32, device=tab.dev)
    dcontext = torch.empty_like(context)
    desc = tab.desc.copy()
    base = out.data_ptr()
    desc[:, 7] = ops.data_ptr() + 4 * tab.off[:-1]
    desc[:, 8] = [t.data_ptr() if t is not None else 0 for t in dgeff]
    desc[:, 9] = [t.data_ptr() if t is not None else 0 for t in dbeff]
    desc[:, 10] = base + 4 * tab.w_off[:-1]
    desc[:, 11] = base + 4 * (wtot + 2 * tab.off[:-1])
    desc[:, 12] = [base + 4 * (wtot + 2 * total + int(tab.off[l])) if tab.affine[l][0] else 0 for l in range(n)]
    desc[:, 13] = [base + 4 * (wtot + 3 * total + int(tab.off[l])) if tab.affine[l][1] else 0 for l in range(n)]
    vec4 = int(tab.vec4 and context.data_ptr() % 16 == 0 and base % 16 == 0)
    grouped.launch("ss_pdnorm_mod_bwd", desc, tab.starts, tab.dev, _p(context), tab.cc, vec4, int(tab.starts[split_row]), _p(partials), _p(dcontext))
    o, wo = [int(x) for x in tab.off], [int(x) for x in tab.w_off]
    dW = [out[wo[l]:wo[l + 1]].view(2 * tab.widths[l], tab.cc) for l in range(n)]
    db = [out[wtot + 2 * o[l]:wtot + 2 * o[l + 1]] for l in range(n)]
    dg = [out[wtot + 2 * total + o[l]:wtot + 2 * total + o[l + 1]] if tab.affine[l][0] else None for l in range(n)]
    dbt = [out[wtot + 3 * total + o[l]:wtot + 3 * total + o[l + 1]] if tab.affine[l][1] else None for l in range(n)]
    return dcontext, dW, db, dg, dbt


# ---- SimDINO pretraining model: patch masks, mask token, grouped EMA (csrc/ssl_model.hip) ------------------------------------------
def _mask_offset(offset, n):
    _req(offset, torch.int32, "offset")
    B = offset.numel()
    if B < 1 or B > lib().ss_mask_max_samples():
        raise RuntimeError(f"mask generator: 1 .. {lib().ss_mask_max_samples()} samples per batch, got {B}")
    return B


def mask_patches(grid_coord, offset, mask_grid_size):
    """Step 1 of the patch mask generator, on the device.  grid_coord (n,3) int32, offset (B) int32 (inclusive row ends).
    -> patch_id (n) int32: rank of the row's mask cell floor(grid_coord / mask_grid_size) among the occupied cells of its sample (x
    fastest, then y, then z); patch_start (B+1) int32; counts (B+1) int32 = the B patch counts followed by a status word that is non-zero
    when a cell left the 17 bits per axis the sort key has (the caller reads counts on the host and must check it)."""
    n = grid_coord.shape[0]
    _req(grid_coord, torch.int32, "grid_coord", (n, 3))
    B = _mask_offset(offset, n)
    dev = grid_coord.device
    counts = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    patch_start = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    patch_id = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return patch_id, patch_start, counts
    keys = torch.empty((1, n), dtype=torch.int64, device=dev)
    check(lib().ss_mask_keys(_p(grid_coord), _p(offset), B, n, float(mask_grid_size), _p(keys), _p(counts[B:]), _stream()), "ss_mask_keys")
    order, _, _ = argsort_i64(keys, lib().ss_mask_key_bits(), want_inverse=False, want_sorted=False)
    cluster, _, _, n_out = pool_partition(keys[0], order[0], 0)
    check(lib().ss_mask_patches(_p(cluster), _p(order), _p(offset), B, n, _p(n_out), _p(patch_start), _p(counts), _p(patch_id), _stream()),
          "ss_mask_patches")
    return patch_id, patch_start, counts


def mask_select(selected, patch_id, patch_start, offset, sample_weight, n):
    """Step 2.  selected: one byte per patch (all samples, in patch_start order), or per row when patch_id is None (`splats`);
    sample_weight (B) fp16.  -> mask (n) bool, index (n capacity) int32 ascending masked rows, weight (n capacity) fp16,
    count (1) int32 on the device."""
    _req(selected, torch.uint8, "selected"); _req(sample_weight, torch.float16, "sample_weight", (offset.numel(),))
    B = _mask_offset(offset, n)
    dev = offset.device
    if patch_id is not None:
        _req(patch_id, torch.int32, "patch_id", (n,)); _req(patch_start, torch.int32, "patch_start", (B + 1,))
    elif selected.numel() != n:
        raise RuntimeError("selected: one byte per row without patch ids")
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    weight = torch.empty(n, dtype=torch.float16, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    blocks = torch.empty(lib().ss_mask_select_blocks(n), dtype=torch.int32, device=dev)
    check(lib().ss_mask_select(_p(selected), _p(patch_id), _p(patch_start), _p(offset), B, n, _p(sample_weight), _p(mask), _p(index),
                               _p(weight), _p(count), _p(blocks), _stream()), "ss_mask_select")
    return mask, index, weight, count


def _mask_rows(mask, n):
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return _req(m, torch.uint8, "mask", (n,))


def mask_token_fwd(x, mask, token):
    """out[i] = token where mask[i] else x[i].  x (n, C) fp32 / bf16, mask (n) bool, token (C) fp32."""
    n, C = x.shape
    _req(x, None, "x"); _req(token, torch.float32, "token")
    if token.numel() != C:
        raise RuntimeError("token: one value per channel")
    out = torch.empty_like(x)
    check(lib().ss_mask_token_fwd(_p(x), dtype_code(x), _p(_mask_rows(mask, n)), _p(token), n, C, _p(out), _stream()), "ss_mask_token_fwd")
    return out


def mask_token_bwd(g, mask):
    """-> dx (n, C) = g with the masked rows zeroed, dtoken (C) fp32 = column sums of the masked rows (fixed order: reproducible)."""
    n, C = g.shape
    _req(g, None, "g")
    if C > 256:
        raise RuntimeError("mask token: at most 256 channels")
    dx = torch.empty_like(g)
    dtoken = torch.empty(C, dtype=torch.float32, device=g.device)
    partial = torch.empty((lib().ss_mask_token_bwd_blocks(n), C), dtype=torch.float32, device=g.device)
    check(lib().ss_mask_token_bwd(_p(g), dtype_code(g), _p(_mask_rows(mask, n)), n, C, _p(dx), _p(partial), _p(dtoken), _stream()),
          "ss_mask_token_bwd")
    return dx, dtoken


def ema_group(teacher, student, m, cache=None):
    """ONE launch: t = m * t + (1 - m) * s for every pair, in place.  alpha = 1 - m is formed in double and rounded to fp32 once, as
    torch._foreach_add_(alpha=1 - m) does.  The caller bumps the version counters of `teacher` (the kernel writes through raw pointers).
    cache: a dict the caller keeps between calls; while every tensor stays where it was (same data pointers) the checked and uploaded
    descriptor table is reused, and a call is the pointer comparison plus the launch."""
    if len(teacher) != len(student):
        raise RuntimeError("ema_group: one student tensor per teacher tensor")
    if not len(teacher):
        return
    m = float(m)
    key = tuple(t.data_ptr() for t in teacher) + tuple(s.data_ptr() for s in student)
    if cache is not None and cache.get("key") == key:
        grouped.relaunch("ss_ema_group", *cache["launch"], m, 1.0 - m)
        return
    dev = _req(teacher[0], torch.float32, "teacher[0]").device
    for j, (t, s) in enumerate(zip(teacher, student)):
        _req_dense_f32(t, None, dev, f"teacher[{j}]"); _req_dense_f32(s, t.numel(), dev, f"student[{j}]")
    pairs = [(t, s) for t, s in zip(teacher, student) if t.numel()]
    if not pairs:
        return
    desc = np.zeros((len(pairs), 4), dtype=np.int64)
    desc[:, 0], desc[:, 1] = [t.data_ptr() for t, _ in pairs], [s.data_ptr() for _, s in pairs]
    desc[:, 2] = [t.numel() for t, _ in pairs]
    desc[:, 3] = ((desc[:, 0] | desc[:, 1]) & 15) == 0
    starts = _optim_starts(desc[:, 2])
    tables = grouped.launch("ss_ema_group", desc, starts, dev, m, 1.0 - m)
    if cache is not None and not torch.cuda.is_current_stream_capturing():
        cache["key"], cache["launch"] = key, (tables, starts[-1])


# ---- scene chunking (csrc/chunking.hip; the steps of sampling_chunking_data_gs.py::chunking_scene) ---------------------------------
CHUNK_DTYPES = {torch.float16: _C["SS_CHUNK_F16"], torch.float32: _C["SS_CHUNK_F32"]}


def chunk_extent(x, idx=None):
    """(6,) f32 {min xyz, max xyz} of the rows x[idx] (idx int32; None: every row) of x (n, 3) f32; deterministic, NaN skipped."""
    _rows3(x, "x")
    if idx is not None:
        _req(idx, torch.int32, "idx")
    m = x.shape[0] if idx is None else idx.numel()
    if m < 1:
        raise ValueError("chunk_extent: no rows")
    partials = torch.empty(lib().ss_chunk_extent_blocks(m) * 6, dtype=torch.float32, device=x.device)
    out = torch.empty(6, dtype=torch.float32, device=x.device)
    check(lib().ss_chunk_extent(_p(x), _p(idx), m, _p(partials), _p(out), _stream()), "ss_chunk_extent")
    return out


def chunk_recentre(coord, ext6):
    """coord - ext6[:3] per column, one rounded fp32 subtraction (ext6 stays on the device)"""
    _rows3(coord, "coord"); _req(ext6, torch.float32, "ext6", (6,))
    out = torch.empty_like(coord)
    check(lib().ss_chunk_recentre(_p(coord), _p(ext6), coord.shape[0], _p(out), _stream()), "ss_chunk_recentre")
    return out


def chunk_lang_normalize_(feat, valid):
    """feat[valid != 0] /= its row norm, in place.  feat (n, width) fp16 | fp32; valid (n) uint8."""
    _req(feat, None, "lang_feat")
    if feat.dim() != 2 or feat.dtype not in CHUNK_DTYPES:
        raise RuntimeError(f"lang_feat: expected (n, width) float16 | float32, got {tuple(feat.shape)} {feat.dtype}")
    _req(valid, torch.uint8, "valid", (feat.shape[0],))
    if feat.shape[1] < 1:
        return feat
    check(lib().ss_chunk_lang_normalize(_p(feat), CHUNK_DTYPES[feat.dtype], _p(valid), feat.shape[0], feat.shape[1], _stream()),
          "ss_chunk_lang_normalize")
    return feat


def chunk_cell_keys(rec, grid_size, bits, status):
    """int64 cell keys of floor(rec / grid_size) (fp32 IEEE division) packed with bits = (x, y, z) bits; status: (1,) int32, zeroed by
    the caller, set when a cell does not fit.  More than 63 bits in all: NativeError."""
    _rows3(rec, "rec"); _req(status, torch.int32, "status")
    keys = torch.empty(rec.shape[0], dtype=torch.int64, device=rec.device)
    check(lib().ss_chunk_cell_keys(_p(rec), rec.shape[0], float(grid_size), int(bits[0]), int(bits[1]), int(bits[2]), _p(keys), _p(status),
                                   _stream()), "ss_chunk_cell_keys")
    return keys


def chunk_cell_pick(order, idx_ptr, n_cells, valid=None, seed=0):
    """Per cell of the CSR (order, idx_ptr) over a stable argsort: (first (n_cells,) int64 = the smallest row, pick (n_cells,) int32 =
    that row, or with `valid` (n) uint8 the cell's valid row number Philox(seed, first) mod n_valid when it has one)."""
    _req(order, torch.int32, "order"); _req(idx_ptr, torch.int32, "idx_ptr")
    if valid is not None:
        _req(valid, torch.uint8, "valid", (order.numel(),))
    if idx_ptr.numel() < n_cells + 1:
        raise RuntimeError("idx_ptr shorter than n_cells + 1")
    first = torch.empty(n_cells, dtype=torch.int64, device=order.device)
    pick = torch.empty(n_cells, dtype=torch.int32, device=order.device)
    check(lib().ss_chunk_cell_pick(_p(order), _p(idx_ptr), n_cells, _p(valid), int(seed) & (2 ** 64 - 1), _p(first), _p(pick), _stream()),
          "ss_chunk_cell_pick")
    return first, pick


def chunk_membership(rec, pick, bounds, nx, ny, slots, status):
    """Membership of the rows rec[pick] (pick None: every row) in the nx * ny chunks of `bounds` (fp64 {lo_x, hi_x, lo_y, hi_y}).
    -> (slot_keys (m, slots) int64, counts (nx * ny) int32); status (1,) int32, caller-zeroed, set when a row needed more slots."""
    _rows3(rec, "rec"); _req(bounds, torch.float64, "bounds", (2 * nx + 2 * ny,)); _req(status, torch.int32, "status")
    if pick is not None:
        _req(pick, torch.int32, "pick")
    m = rec.shape[0] if pick is None else pick.numel()
    if m * slots >= 2 ** 31:
        raise RuntimeError(f"chunk_membership: {m} rows x {slots} slots do not fit the int32 sort order")
    slot_keys = torch.empty((m, slots), dtype=torch.int64, device=rec.device)
    counts = torch.zeros(nx * ny, dtype=torch.int32, device=rec.device)
    check(lib().ss_chunk_membership(_p(rec), _p(pick), m, _p(bounds), int(nx), int(ny), int(slots), _p(slot_keys), _p(counts), _p(status),
                                    _stream()), "ss_chunk_membership")
    return slot_keys, counts


def chunk_offsets(counts):
    """(nchunk + 1,) int64 exclusive running sum of counts (nchunk,) int32"""
    _req(counts, torch.int32, "counts")
    offsets = torch.empty(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    check(lib().ss_chunk_offsets(_p(counts), counts.numel(), _p(offsets), _stream()), "ss_chunk_offsets")
    return offsets


def chunk_slot_rows(slot_order, total, slots):
    """rows (total,) int32 = slot_order[:total] // slots"""
    _req(slot_order, torch.int32, "slot_order")
    if total > slot_order.numel():
        raise RuntimeError("chunk_slot_rows: total exceeds the sorted slots")
    rows = torch.empty(total, dtype=torch.int32, device=slot_order.device)
    check(lib().ss_chunk_slot_rows(_p(slot_order), int(total), int(slots), _p(rows), _stream()), "ss_chunk_slot_rows")
    return rows


def chunk_gather_group(desc, dev):
    """ONE launch of ss_chunk_gather_group over the rows of `desc` ((k, 8) int64: {src, dst, idx, n_rows, row_bytes, pick | 0, src_rows,
    pick_rows}, real device addresses)."""
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    if desc.ndim != 2 or desc.shape[1] != 8:
        raise RuntimeError("chunk_gather_group: desc must be (k, 8) int64")
    if desc.shape[0] == 0:
        return
    if (desc[:, 3] < 0).any() or (desc[:, 4] < 1).any() or (desc[:, 4] >= 2 ** 31).any() or (desc[:, 6] < 0).any() or (desc[:, 7] < 0).any():
        raise RuntimeError("chunk_gather_group: negative size, or row_bytes outside [1, 2^31)")
    if ((desc[:, 3] > 0) & ((desc[:, 0] == 0) | (desc[:, 1] == 0) | (desc[:, 2] == 0))).any():
        raise RuntimeError("chunk_gather_group: null pointer in a non-empty problem")
    per = np.array([lib().ss_chunk_gather_rows_per_workgroup(int(rb)) for rb in desc[:, 4]], dtype=np.int64)
    grouped.launch("ss_chunk_gather_group", desc, grouped.starts(_div_up(desc[:, 3], per)), dev)


# ---- 3DGS checkpoint decode (csrc/ply.hip) ---------------------------------------------------------------------------------------------
def ply_decode(records, n, stride, offsets, n_scale, n_rot, coord, color, opacity, scale, quat, row=0):
    """ONE launch of ss_ply_decode: the first n records (stride bytes apart) of `records` (device uint8, 4-byte aligned) -> rows
    row .. row + n of coord (N, 3) f32, color (N, 3) u8, opacity (N,) f32, scale (N, n_scale) f32, quat (N, n_rot) f32.  offsets: the
    7 + n_scale + n_rot byte offsets of x, y, z, f_dc_0..2, opacity, scale_*, rot_* inside a record (host integers)."""
    n, stride, row, n_scale, n_rot = int(n), int(stride), int(row), int(n_scale), int(n_rot)
    _req(records, torch.uint8, "records")
    offsets = [int(o) for o in offsets]
    if not (1 <= n_scale <= 4 and 1 <= n_rot <= 4) or len(offsets) != 7 + n_scale + n_rot:
        raise RuntimeError(f"ply_decode: n_scale / n_rot in 1..4 and 7 + n_scale + n_rot offsets expected, got {n_scale}, {n_rot}, {len(offsets)}")
    if stride < 4 or stride % 4 or any(o < 0 or o % 4 or o + 4 > stride for o in offsets):
        raise RuntimeError("ply_decode: the stride and every offset must be multiples of 4, and offset + 4 <= stride")
    if n < 0 or row < 0 or records.numel() < n * stride or records.data_ptr() % 4:
        raise RuntimeError("ply_decode: records must hold n whole records and start 4-byte aligned")
    N = coord.shape[0] if isinstance(coord, torch.Tensor) and coord.dim() == 2 else -1
    if row + n > N:
        raise RuntimeError(f"ply_decode: rows {row}..{row + n} do not fit outputs of {N} rows")
    _req(coord, torch.float32, "coord", (N, 3)); _req(color, torch.uint8, "color", (N, 3)); _req(opacity, torch.float32, "opacity", (N,))
    _req(scale, torch.float32, "scale", (N, n_scale)); _req(quat, torch.float32, "quat", (N, n_rot))
    if n == 0:
        return

    def at(t, width):
        return ctypes.c_void_p(t.data_ptr() + row * width * t.element_size())

    check(lib().ss_ply_decode(_p(records), n, stride, (ctypes.c_int32 * len(offsets))(*offsets), n_scale, n_rot, at(coord, 3), at(color, 3),
                              at(opacity, 1), at(scale, n_scale), at(quat, n_rot), _stream()), "ss_ply_decode")


# ---- ScanNet mesh converter (csrc/mesh.hip) ----------------------------------------------------------------------------------------------
MESH_FORMS = {"pc": _C["SS_MESH_FORM_PC"], "gs": _C["SS_MESH_FORM_GS"]}
MESH_FACE_BYTES = 13
MESH_BAD_COUNT, MESH_BAD_INDEX = 1, 2        # the bits of the status word


def _mesh_records(records, start, nbytes, name):
    """address of byte `start` of `records` (device uint8); the kernels read the aligned words that cover [start, start + nbytes), which
    torch's allocations (sized in multiples of 512 bytes, 256-byte aligned) always hold"""
    _req(records, torch.uint8, "records")
    if start < 0 or nbytes < 0 or start + nbytes > records.numel():
        raise RuntimeError(f"{name}: bytes {start}..{start + nbytes} do not lie inside records of {records.numel()} bytes")
    return ctypes.c_void_p(records.data_ptr() + start)


def mesh_decode_vertices(records, n, stride, offsets, coord, color, row=0, start=0):
    """ONE launch of ss_mesh_decode_vertices: n records, stride bytes apart, from byte `start` of `records` (device uint8; any alignment)
    -> rows row .. row + n of coord (N, 3) f32 and color (N, 3) u8.  offsets: byte offsets of x, y, z (float32, multiples of 4) and of
    red, green, blue (uchar) inside a record."""
    n, stride, row, start = int(n), int(stride), int(row), int(start)
    offsets = [int(o) for o in offsets]
    if len(offsets) != 6 or stride < 15 or any(o < 0 or o % 4 or o + 4 > stride for o in offsets[:3]) or any(not 0 <= o < stride for o in offsets[3:]):
        raise RuntimeError("mesh_decode_vertices: six offsets inside the record expected, x / y / z at multiples of 4")
    if n < 0 or row < 0:
        raise RuntimeError("mesh_decode_vertices: negative count or row")
    src = _mesh_records(records, start, n * stride, "mesh_decode_vertices")
    N = coord.shape[0] if isinstance(coord, torch.Tensor) and coord.dim() == 2 else -1
    if row + n > N:
        raise RuntimeError(f"mesh_decode_vertices: rows {row}..{row + n} do not fit outputs of {N} rows")
    _req(coord, torch.float32, "coord", (N, 3)); _req(color, torch.uint8, "color", (N, 3))
    if n == 0:
        return
    check(lib().ss_mesh_decode_vertices(src, n, stride, (ctypes.c_int32 * 6)(*offsets), ctypes.c_void_p(coord.data_ptr() + row * 12),
                                        ctypes.c_void_p(color.data_ptr() + row * 3), _stream()), "ss_mesh_decode_vertices")


def mesh_decode_faces(records, n_faces, n_vertices, faces, status, row=0, start=0):
    """ONE launch of ss_mesh_decode_faces: n_faces records of 13 bytes from byte `start` of `records` (device uint8; any alignment) ->
    rows row .. row + n_faces of faces (F, 3) int32.  status (1,) int32, zeroed by the caller: mesh_check_status reads it."""
    n_faces, n_vertices, row, start = int(n_faces), int(n_vertices), int(row), int(start)
    if n_faces < 0 or row < 0 or not 0 <= n_vertices < 2 ** 31:
        raise RuntimeError("mesh_decode_faces: negative count or row, or more than 2^31 - 1 vertices")
    src = _mesh_records(records, start, n_faces * MESH_FACE_BYTES, "mesh_decode_faces")
    F = faces.shape[0] if isinstance(faces, torch.Tensor) and faces.dim() == 2 else -1
    if row + n_faces > F:
        raise RuntimeError(f"mesh_decode_faces: rows {row}..{row + n_faces} do not fit faces of {F} rows")
    _req(faces, torch.int32, "faces", (F, 3)); _req(status, torch.int32, "status", (1,))
    if n_faces == 0:
        return
    check(lib().ss_mesh_decode_faces(src, n_faces, n_vertices, ctypes.c_void_p(faces.data_ptr() + row * 12), _p(status), _stream()),
          "ss_mesh_decode_faces")


def mesh_check_status(status, what):
    """reads the status word once (a synchronisation); ValueError names what the kernels met"""
    bits = int(status.item())
    if bits & MESH_BAD_COUNT:
        raise ValueError(f"{what}: a face with a vertex count other than 3 (only triangle meshes have a device form)")
    if bits & MESH_BAD_INDEX:
        raise ValueError(f"{what}: a face names a vertex outside [0, number of vertices)")


def _mesh_incidence(faces, n):
    """the 3F corner entries faces[face][corner] (entry p = 3 * face + corner) under a stable argsort by vertex, with the run boundaries
    of equal vertices: -> (order, idx_ptr, head, n_runs).  Every index must lie inside [0, n): the keys of the sort are non-negative."""
    keys = faces.view(1, -1).to(torch.int64)
    order, _, _ = argsort_i64(keys, max(1, (n - 1).bit_length()), want_inverse=False, want_sorted=False)
    _, idx_ptr, head, n_runs = pool_partition(keys.view(-1), order.view(-1), 0)
    return order, idx_ptr, head, n_runs


def mesh_vertex_normals(coord, faces, form):
    """coord (n, 3) f32, faces (F, 3) int32 -> normal (n, 3) f32, `vertex_normal` of preprocess_scannet.py (form 'pc') or
    preprocess_scannet_gs.py (form 'gs') bit for bit: ss_mesh_face_terms, the stable argsort of the 3F corner entries by vertex,
    ss_pool_partition's run boundaries, ss_mesh_vertex_normals.  ValueError: a face index outside [0, n)."""
    if form not in MESH_FORMS:
        raise ValueError(f"mesh_vertex_normals: form must be 'pc' or 'gs', got {form!r}")
    n = coord.shape[0] if isinstance(coord, torch.Tensor) and coord.dim() == 2 else -1
    F = faces.shape[0] if isinstance(faces, torch.Tensor) and faces.dim() == 2 else -1
    _req(coord, torch.float32, "coord", (n, 3)); _req(faces, torch.int32, "faces", (F, 3))
    if n >= 2 ** 31 or 3 * F >= 2 ** 31:
        raise RuntimeError("mesh_vertex_normals: more than 2^31 - 1 vertices or corner entries")
    dev = coord.device
    normal = torch.zeros((n, 3), dtype=torch.float32, device=dev)          # a vertex in no face keeps 0 / length = 0
    if F == 0:
        return normal
    if n == 0:
        raise ValueError("mesh_vertex_normals: faces over an empty vertex list")
    code = MESH_FORMS[form]
    terms = torch.empty((F, 3), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().ss_mesh_face_terms(_p(coord), _p(faces), F, n, code, _p(terms), _p(status), _stream()), "ss_mesh_face_terms")
    mesh_check_status(status, "mesh_vertex_normals")                       # (before the sort: its keys must be non-negative)
    order, idx_ptr, head, n_runs = _mesh_incidence(faces, n)
    check(lib().ss_mesh_vertex_normals(_p(terms), _p(faces), _p(order), _p(idx_ptr), _p(head), _p(n_runs), F, n, code, _p(normal),
                                       _stream()), "ss_mesh_vertex_normals")
    return normal


def mesh_labels(seg_indices, seg_to_group, table20, table200, table_instance, dtype, src=None):
    """ONE launch of ss_mesh_labels -> (segment20, segment200, instance) of `dtype` (torch.int16 or torch.int64), one row per row of
    `src` (int32 rows of seg_indices; None: one per entry of seg_indices).  Every table is int32 on the device."""
    _req(seg_indices, torch.int32, "seg_indices"); _req(seg_to_group, torch.int32, "seg_to_group")
    G = table20.numel() if isinstance(table20, torch.Tensor) else -1
    for name, t in (("table20", table20), ("table200", table200), ("table_instance", table_instance)):
        _req(t, torch.int32, name, (G,))
    if dtype not in (torch.int16, torch.int64):
        raise RuntimeError(f"mesh_labels: int16 or int64 outputs, got {dtype}")
    if src is not None:
        _req(src, torch.int32, "src")
    n = seg_indices.numel() if src is None else src.numel()
    outs = [torch.empty(n, dtype=dtype, device=seg_indices.device) for _ in range(3)]
    if n:
        check(lib().ss_mesh_labels(_p(seg_indices), seg_indices.numel(), _p(src), _p(seg_to_group), seg_to_group.numel(), _p(table20),
                                   _p(table200), _p(table_instance), G, n, 2 if dtype == torch.int16 else 8, _p(outs[0]), _p(outs[1]),
                                   _p(outs[2]), _stream()), "ss_mesh_labels")
    return tuple(outs)


# ---- ScanNet++ converter (csrc/scannetpp.hip) --------------------------------------------------------------------------------------------
def mesh_vertex_normals_o3d(coord, faces):
    """coord (n, 3) f32, faces (F, 3) int32 -> normal (n, 3) f32 in Open3D's definition (`compute_vertex_normals(normalized=True)`):
    ss_mesh_face_cross_f64, the stable argsort of the 3F corner entries by vertex, ss_pool_partition's run boundaries,
    ss_mesh_vertex_normals_f64.  ValueError: a face index outside [0, n)."""
    n = coord.shape[0] if isinstance(coord, torch.Tensor) and coord.dim() == 2 else -1
    F = faces.shape[0] if isinstance(faces, torch.Tensor) and faces.dim() == 2 else -1
    _req(coord, torch.float32, "coord", (n, 3)); _req(faces, torch.int32, "faces", (F, 3))
    if n >= 2 ** 31 or 3 * F >= 2 ** 31:
        raise RuntimeError("mesh_vertex_normals_o3d: more than 2^31 - 1 vertices or corner entries")
    dev = coord.device
    normal = torch.zeros((n, 3), dtype=torch.float32, device=dev)          # a vertex in no face keeps its zero sum
    if F == 0:
        return normal
    if n == 0:
        raise ValueError("mesh_vertex_normals_o3d: faces over an empty vertex list")
    cross = torch.empty((F, 3), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().ss_mesh_face_cross_f64(_p(coord), _p(faces), F, n, _p(cross), _p(status), _stream()), "ss_mesh_face_cross_f64")
    mesh_check_status(status, "mesh_vertex_normals_o3d")                   # (before the sort: its keys must be non-negative)
    order, idx_ptr, head, n_runs = _mesh_incidence(faces, n)
    check(lib().ss_mesh_vertex_normals_f64(_p(cross), _p(faces), _p(order), _p(idx_ptr), _p(head), _p(n_runs), F, n, _p(normal), _stream()),
          "ss_mesh_vertex_normals_f64")
    return normal


def spp_segment_hist(seg_indices, n_segments):
    """ONE launch of ss_spp_segment_hist: seg_indices (n,) int32 -> count (n_segments,) int32 of the ids inside [0, n_segments)"""
    _req(seg_indices, torch.int32, "seg_indices")
    n_segments = int(n_segments)
    if seg_indices.dim() != 1 or seg_indices.numel() >= 2 ** 31 or n_segments < 0:
        raise RuntimeError("spp_segment_hist: seg_indices must be (n,) with n < 2^31, n_segments >= 0")
    count = torch.zeros(n_segments, dtype=torch.int32, device=seg_indices.device)
    check(lib().ss_spp_segment_hist(_p(seg_indices), seg_indices.numel(), n_segments, _p(count), _stream()), "ss_spp_segment_hist")
    return count


def spp_group_sizes(first3, count, n_groups):
    """ONE launch of ss_spp_group_sizes: first3 (S, 3) int32, count (S,) int32 -> size (n_groups,) int32"""
    S = count.numel() if isinstance(count, torch.Tensor) else -1
    _req(first3, torch.int32, "first3", (S, 3)); _req(count, torch.int32, "count", (S,))
    n_groups = int(n_groups)
    if not 0 <= n_groups < 2 ** 31:
        raise RuntimeError("spp_group_sizes: n_groups outside [0, 2^31)")
    size = torch.zeros(n_groups, dtype=torch.int32, device=count.device)
    check(lib().ss_spp_group_sizes(_p(first3), _p(count), S, n_groups, _p(size), _stream()), "ss_spp_group_sizes")
    return size


def spp_labels(seg_indices, first3, table_label, table_object, size, src=None, empty=-1):
    """ONE launch of ss_spp_labels -> (segment, instance) (n, 3) int16, one row per row of `src` (int32 rows of seg_indices; None: one
    per entry of seg_indices).  Every table is int32 on the device; size = spp_group_sizes(...)."""
    _req(seg_indices, torch.int32, "seg_indices")
    S = first3.shape[0] if isinstance(first3, torch.Tensor) and first3.dim() == 2 else -1
    _req(first3, torch.int32, "first3", (S, 3))
    G = table_label.numel() if isinstance(table_label, torch.Tensor) else -1
    for name, t in (("table_label", table_label), ("table_object", table_object), ("size", size)):
        _req(t, torch.int32, name, (G,))
    if src is not None:
        _req(src, torch.int32, "src")
    if not -2 ** 15 <= int(empty) < 2 ** 15:
        raise RuntimeError(f"spp_labels: the empty value {empty} does not fit int16")
    n = seg_indices.numel() if src is None else src.numel()
    outs = [torch.empty((n, 3), dtype=torch.int16, device=seg_indices.device) for _ in range(2)]
    if n:
        check(lib().ss_spp_labels(_p(seg_indices), seg_indices.numel(), _p(src), _p(first3), S, _p(table_label), _p(table_object), _p(size), G,
                                  n, int(empty), _p(outs[0]), _p(outs[1]), _stream()), "ss_spp_labels")
    return tuple(outs)


# ---- labelled point cloud of a batch of chunks (csrc/pc_attach.hip) ---------------------------------------------------------------------
def pc_mark(pc, q, q_offset, idx, dist_limit):
    """ss_pc_mark: pc (M, 3) f32, q (m, 3) f32, q_offset (nc + 1) int32, idx (m, k) int32 (-1 = unfilled), dist_limit: a Python float
    (fp64).  -> (bitmap (nc, ceil(M / 32)) int32 words, nearest (m,) int32, status (1,) int32: 1 when an idx >= M was met)."""
    _rows3(pc, "pc"); _rows3(q, "q"); _req(q_offset, torch.int32, "q_offset"); _req(idx, torch.int32, "idx")
    M, m, nc = pc.shape[0], q.shape[0], q_offset.numel() - 1
    if idx.dim() != 2 or idx.shape[0] != m or idx.shape[1] < 1:
        raise RuntimeError(f"idx: expected (m = {m}, k >= 1), got {tuple(idx.shape)}")
    if M < 1 or nc < 1:
        raise RuntimeError("pc_mark: an empty cloud, or no chunk")
    bitmap = torch.empty((nc, lib().ss_pc_bitmap_words(M)), dtype=torch.int32, device=pc.device)
    nearest = torch.empty(m, dtype=torch.int32, device=pc.device)
    status = torch.empty(1, dtype=torch.int32, device=pc.device)
    limit = ctypes.c_double(float(dist_limit))
    check(lib().ss_pc_mark(_p(pc), M, _p(q), m, _p(q_offset), nc, _p(idx), idx.shape[1], ctypes.addressof(limit), _p(bitmap), _p(nearest),
                           _p(status), _stream()), "ss_pc_mark")
    return bitmap, nearest, status


def pc_compact_scan(bitmap, M):
    """ss_pc_compact_scan -> (tile_base: the scan the emit pass reads, counts (nc,) int32: the distinct rows of every chunk)"""
    _req(bitmap, torch.int32, "bitmap", (bitmap.shape[0], lib().ss_pc_bitmap_words(M)))
    nc = bitmap.shape[0]
    tile_base = torch.empty(2 * lib().ss_pc_compact_tiles(M, nc) + 1, dtype=torch.int32, device=bitmap.device)
    counts = torch.empty(nc, dtype=torch.int32, device=bitmap.device)
    check(lib().ss_pc_compact_scan(_p(bitmap), M, nc, _p(tile_base), _p(counts), _stream()), "ss_pc_compact_scan")
    return tile_base, counts


def pc_compact(bitmap, M, tile_base, total):
    """ss_pc_compact -> rows (total,) int32: the ascending cloud rows of chunk 0, then of chunk 1, ...; total = counts.sum()"""
    _req(bitmap, torch.int32, "bitmap", (bitmap.shape[0], lib().ss_pc_bitmap_words(M)))
    _req(tile_base, torch.int32, "tile_base", (2 * lib().ss_pc_compact_tiles(M, bitmap.shape[0]) + 1,))
    rows = torch.empty(int(total), dtype=torch.int32, device=bitmap.device)
    check(lib().ss_pc_compact(_p(bitmap), M, bitmap.shape[0], _p(tile_base), _p(rows), int(total), _stream()), "ss_pc_compact")
    return rows


# ---- minimal oriented bounding box (csrc/obb.hip) ----------------------------------------------------------------------------------------
def obb_extremes(points, dirs):
    """ss_obb_extremes: points (N, 3) f32, dirs (K, 3) f64 -> (rows_max, rows_min) (K,) int32: per direction the row of the largest and
    of the smallest projection (equal values: the lower row)"""
    _rows3(points, "points"); _req(dirs, torch.float64, "dirs")
    N, K = points.shape[0], dirs.shape[0]
    if dirs.dim() != 2 or dirs.shape[1] != 3 or N < 1 or K < 1:
        raise RuntimeError(f"obb_extremes: expected dirs (K >= 1, 3) and N >= 1, got {tuple(dirs.shape)}, N = {N}")
    rows = torch.empty((2, K), dtype=torch.int32, device=points.device)
    ws = _ws(lib().ss_obb_extremes_workspace_bytes(N, K), points.device)
    check(lib().ss_obb_extremes(_p(points), N, _p(dirs), K, _p(rows[0]), _p(rows[1]), _p(ws), ws.numel(), _stream()), "ss_obb_extremes")
    return rows[0], rows[1]


def obb_filter(points, planes, tol):
    """ss_obb_filter: points (N, 3) f32, planes (F, 4) f64, tol: a Python float -> bitmap (1, ceil(N / 32)) int32 words of the rows that
    are not below every plane by more than tol"""
    _rows3(points, "points"); _req(planes, torch.float64, "planes")
    N = points.shape[0]
    if planes.dim() != 2 or planes.shape[1] != 4 or planes.shape[0] < 1 or N < 1:
        raise RuntimeError(f"obb_filter: expected planes (F >= 1, 4) and N >= 1, got {tuple(planes.shape)}, N = {N}")
    bitmap = torch.empty((1, lib().ss_pc_bitmap_words(N)), dtype=torch.int32, device=points.device)
    h_tol = ctypes.c_double(float(tol))
    check(lib().ss_obb_filter(_p(points), N, _p(planes), planes.shape[0], ctypes.addressof(h_tol), _p(bitmap), _stream()), "ss_obb_filter")
    return bitmap


def obb_search(verts, tris):
    """ss_obb_search: verts (H, 3) f64, tris (T, 3) int32 rows of verts -> (volumes (3 T,) f64, best_index (1,) int32, box (15,) f64)"""
    _req(verts, torch.float64, "verts"); _req(tris, torch.int32, "tris")
    if verts.dim() != 2 or verts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 3 or verts.shape[0] < 1 or tris.shape[0] < 1:
        raise RuntimeError(f"obb_search: expected verts (H >= 1, 3) and tris (T >= 1, 3), got {tuple(verts.shape)}, {tuple(tris.shape)}")
    T = tris.shape[0]
    volumes = torch.empty(3 * T, dtype=torch.float64, device=verts.device)
    best = torch.empty(1, dtype=torch.int32, device=verts.device)
    box = torch.empty(15, dtype=torch.float64, device=verts.device)
    check(lib().ss_obb_search(_p(verts), verts.shape[0], _p(tris), T, _p(volumes), _p(best), _p(box), _stream()), "ss_obb_search")
    return volumes, best, box


def obb_within(points, box15):
    """ss_obb_within: points (M >= 1, 3) f32, box15: 15 host doubles (center, R row-major, extent) -> bitmap (1, ceil(M / 32)) int32"""
    _rows3(points, "points")
    M = points.shape[0]
    h_box = (ctypes.c_double * 15)(*[float(v) for v in box15])
    bitmap = torch.empty((1, lib().ss_pc_bitmap_words(M)), dtype=torch.int32, device=points.device)
    check(lib().ss_obb_within(_p(points), M, ctypes.addressof(h_box), _p(bitmap), _stream()), "ss_obb_within")
    return bitmap


def bitmap_rows(bitmap, n):
    """the ascending rows of the set bits of a (1, ceil(n / 32)) bitmap: ss_pc_compact_scan, ONE count read, ss_pc_compact"""
    tile_base, counts = pc_compact_scan(bitmap, n)
    return pc_compact(bitmap, n, tile_base, int(counts.cpu()[0]))


# ---- PCA colours of a feature matrix (csrc/feature_pca.hip) --------------------------------------------------------
PCA_MAX_DIM, PCA_GRAM_CHAIN, PCA_GRAM_ROWS = _C["SS_PCA_MAX_DIM"], _C["SS_PCA_GRAM_CHAIN"], _C["SS_PCA_GRAM_ROWS"]
PCA_GRAM_SHARE_MIN, PCA_PROJECT_ROWS = _C["SS_PCA_GRAM_SHARE_MIN"], _C["SS_PCA_PROJECT_ROWS"]
_PCA_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: _C["SS_DTYPE_F16"]}


def _pca_x(x, shift=None):
    _req(x, None, "features")
    if x.dim() != 2 or x.dtype not in _PCA_DTYPES or x.shape[0] < 1 or not 1 <= x.shape[1] <= PCA_MAX_DIM:
        raise RuntimeError(f"features: expected (N >= 1, 1 <= D <= {PCA_MAX_DIM}) float32 / float16 / bfloat16, got "
                           f"{tuple(x.shape)} {x.dtype}")
    if shift is not None:
        _req(shift, torch.float32, "shift", (x.shape[1],))
    return x.shape[0], x.shape[1], _PCA_DTYPES[x.dtype]


def _pca_ws(workspace, nbytes, device):
    if workspace is None:
        return _ws(nbytes, device)
    _req(workspace, torch.uint8, "workspace")
    return workspace


def pca_col_sums(x, shift=None, workspace=None):
    """ss_pca_col_sums: x (N, D) f32 / f16 / bf16, shift (D,) f32 or None -> (D,) f64 sums of (double)x - (double)shift"""
    N, D, dt = _pca_x(x, shift)
    sums = torch.empty(D, dtype=torch.float64, device=x.device)
    ws = _pca_ws(workspace, lib().ss_pca_col_sums_workspace_bytes(N, D), x.device)
    check(lib().ss_pca_col_sums(_p(x), dt, N, D, _p(shift), _p(sums), _p(ws), ws.numel(), _stream()), "ss_pca_col_sums")
    return sums


def pca_gram_workspace_bytes(N, D):
    return int(lib().ss_pca_gram_workspace_bytes(N, D))


def pca_gram_share_rows(N, D):
    """the rows one workgroup of ss_pca_gram takes at this shape (a multiple of PCA_GRAM_CHAIN, at least PCA_GRAM_SHARE_MIN)"""
    return int(lib().ss_pca_gram_share_rows(N, D))


def pca_gram(x, shift=None, workspace=None):
    """ss_pca_gram: -> (D, D) f64 = (x - shift)^T (x - shift), both triangles; workspace: a uint8 tensor of
    pca_gram_workspace_bytes(N, D) bytes (None: allocated here)"""
    N, D, dt = _pca_x(x, shift)
    gram = torch.empty((D, D), dtype=torch.float64, device=x.device)
    ws = _pca_ws(workspace, pca_gram_workspace_bytes(N, D), x.device)
    check(lib().ss_pca_gram(_p(x), dt, N, D, _p(shift), _p(gram), _p(ws), ws.numel(), _stream()), "ss_pca_gram")
    return gram


def pca_project(x, comp, shift=None, off=None, workspace=None):
    """ss_pca_project: comp (k, D) f32, off (k,) f32 or None -> (y (N, k) f32 = (x - shift) comp^T - off, extremes (2, k) f32: the minima
    and the maxima of y)"""
    N, D, dt = _pca_x(x, shift)
    _req(comp, torch.float32, "comp")
    if comp.dim() != 2 or comp.shape[1] != D or not 1 <= comp.shape[0] <= min(3, D):
        raise RuntimeError(f"pca_project: expected comp (1 <= k <= min(3, D), {D}), got {tuple(comp.shape)}")
    k = comp.shape[0]
    if off is not None:
        _req(off, torch.float32, "off", (k,))
    y = torch.empty((N, k), dtype=torch.float32, device=x.device)
    ext = torch.empty((2, k), dtype=torch.float32, device=x.device)
    ws = _pca_ws(workspace, lib().ss_pca_project_workspace_bytes(N), x.device)
    check(lib().ss_pca_project(_p(x), dt, N, D, _p(shift), _p(comp), _p(off), k, _p(y), _p(ext), _p(ws), ws.numel(), _stream()),
          "ss_pca_project")
    return y, ext


def pca_colors(y, extremes):
    """ss_pca_colors: y (N, k) f32, extremes (2, k) f32 -> (N, 3) f32 colours"""
    _req(y, torch.float32, "y")
    if y.dim() != 2 or y.shape[0] < 1 or not 1 <= y.shape[1] <= 3:
        raise RuntimeError(f"pca_colors: expected y (N >= 1, 1..3), got {tuple(y.shape)}")
    _req(extremes, torch.float32, "extremes", (2, y.shape[1]))
    colors = torch.empty((y.shape[0], 3), dtype=torch.float32, device=y.device)
    check(lib().ss_pca_colors(_p(y), _p(extremes), y.shape[0], y.shape[1], _p(colors), _stream()), "ss_pca_colors")
    return colors


# ---- text queries on scene features (csrc/text_query.hip) ------------------------------------------------------------
QUERY_MAX_DIM, QUERY_MAX_QUERIES = _C["SS_QUERY_MAX_DIM"], _C["SS_QUERY_MAX_QUERIES"]
QUERY_ROWS, QUERY_SELECT_ROWS = _C["SS_QUERY_ROWS"], _C["SS_QUERY_SELECT_ROWS"]


def query_scores_workspace_bytes(N, Q):
    return int(lib().ss_query_scores_workspace_bytes(N, Q))


def query_scores(x, t_hat, valid=None, workspace=None):
    """ss_query_scores: x (N, D) f32 / f16 / bf16, t_hat (Q, D) f32 unit rows, valid (N,) uint8 / bool or None -> (scores (Q, N) f32:
    cosine scores, -inf in dead rows; stats (Q, 3) f64 = {live rows, sum s, sum s^2}); workspace: a uint8 tensor of
    query_scores_workspace_bytes(N, Q) bytes (None: allocated here)"""
    _req(x, None, "features"); _req(t_hat, torch.float32, "t_hat")
    if x.dim() != 2 or x.dtype not in _PCA_DTYPES or x.shape[0] < 1 or not 1 <= x.shape[1] <= QUERY_MAX_DIM:
        raise RuntimeError(f"features: expected (N >= 1, 1 <= D <= {QUERY_MAX_DIM}) float32 / float16 / bfloat16, got "
                           f"{tuple(x.shape)} {x.dtype}")
    N, D = x.shape
    if t_hat.dim() != 2 or t_hat.shape[1] != D or not 1 <= t_hat.shape[0] <= QUERY_MAX_QUERIES:
        raise RuntimeError(f"t_hat: expected (1 <= Q <= {QUERY_MAX_QUERIES}, {D}), got {tuple(t_hat.shape)}")
    Q = t_hat.shape[0]
    if valid is not None:
        _req(valid, None, "valid", (N,))
        if valid.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError(f"valid: expected uint8 or bool, got {valid.dtype}")
    scores = torch.empty((Q, N), dtype=torch.float32, device=x.device)
    stats = torch.empty((Q, 3), dtype=torch.float64, device=x.device)
    ws = _pca_ws(workspace, query_scores_workspace_bytes(N, Q), x.device)
    check(lib().ss_query_scores(_p(x), _PCA_DTYPES[x.dtype], N, D, _p(t_hat), Q, _p(valid), _p(scores), _p(stats), _p(ws), ws.numel(),
                                _stream()), "ss_query_scores")
    return scores, stats


def query_select_workspace_bytes(N, Q):
    return int(lib().ss_query_select_workspace_bytes(N, Q))


def query_select(scores, tau, m, workspace=None):
    """ss_query_select: scores (Q, N) f32 as query_scores writes them; tau: Q host floats (rounded to fp32; -inf: no threshold); m: Q
    host ints (negative: no cap) -> (bitmap (Q, ceil(N / 32)) int32 words, tau_out (Q,) f32, counts (Q,) int32)"""
    _req(scores, torch.float32, "scores")
    if scores.dim() != 2 or scores.shape[1] < 1 or not 1 <= scores.shape[0] <= QUERY_MAX_QUERIES:
        raise RuntimeError(f"scores: expected (1 <= Q <= {QUERY_MAX_QUERIES}, N >= 1), got {tuple(scores.shape)}")
    Q, N = scores.shape
    tau = np.ascontiguousarray(np.asarray(tau, dtype=np.float32).reshape(-1))
    m = np.ascontiguousarray(np.clip(np.asarray(m, dtype=np.int64).reshape(-1), -1, 2 ** 31 - 1).astype(np.int32))
    if tau.shape[0] != Q or m.shape[0] != Q:
        raise RuntimeError(f"query_select: expected {Q} thresholds and caps, got {tau.shape[0]} and {m.shape[0]}")
    bitmap = torch.empty((Q, lib().ss_pc_bitmap_words(N)), dtype=torch.int32, device=scores.device)
    tau_out = torch.empty(Q, dtype=torch.float32, device=scores.device)
    counts = torch.empty(Q, dtype=torch.int32, device=scores.device)
    ws = _pca_ws(workspace, query_select_workspace_bytes(N, Q), scores.device)
    check(lib().ss_query_select(_p(scores), N, Q, tau.ctypes.data, m.ctypes.data, _p(bitmap), _p(tau_out), _p(counts), _p(ws), ws.numel(),
                                _stream()), "ss_query_select")
    return bitmap, tau_out, counts


def query_best(scores, bitmap):
    """ss_query_best: -> best (N,) int32: the selecting query of highest score per row (the lowest q among equals), -1 when none"""
    _req(scores, torch.float32, "scores")
    Q, N = scores.shape
    _req(bitmap, torch.int32, "bitmap", (Q, lib().ss_pc_bitmap_words(N)))
    best = torch.empty(N, dtype=torch.int32, device=scores.device)
    check(lib().ss_query_best(_p(scores), _p(bitmap), N, Q, _p(best), _stream()), "ss_query_best")
    return best


# ---- headless Gaussian-splat rendering (csrc/splat.hip) ---------------------------------------------------------------
SPLAT_TILE, SPLAT_BATCH, SPLAT_MAX_DIM = _C["SS_SPLAT_TILE"], _C["SS_SPLAT_BATCH"], _C["SS_SPLAT_MAX_DIM"]
SPLAT_CAMERA_WORDS, SPLAT_SCAN_ROWS = _C["SS_SPLAT_CAMERA_WORDS"], _C["SS_SPLAT_SCAN_ROWS"]
SPLAT_MODES = {"gaussians": _C["SS_SPLAT_MODE_GAUSSIANS"], "pointcloud": _C["SS_SPLAT_MODE_POINTCLOUD"]}
SPLAT_MAX_PAIRS = 2 ** 31 - 1          # the largest count ss_argsort_i64 takes


def _splat_camera(camera):
    """the packed camera block: SPLAT_CAMERA_WORDS 32-bit words in a contiguous host array -> (block, width, height)"""
    cam = np.ascontiguousarray(camera)
    if cam.dtype.itemsize != 4 or cam.size != SPLAT_CAMERA_WORDS:
        raise RuntimeError(f"camera: expected a packed block of {SPLAT_CAMERA_WORDS} 32-bit words, got {cam.dtype} x {cam.size}")
    w, h = (int(v) for v in cam.reshape(-1).view(np.int32)[19:21])
    if not (1 <= w <= SPLAT_MAX_DIM and 1 <= h <= SPLAT_MAX_DIM):
        raise RuntimeError(f"camera: width and height must be in 1..{SPLAT_MAX_DIM}, got {w} x {h}")
    return cam, w, h


def splat_project(coord, scale, quat, opacity, color, camera, mode="gaussians", scale_modifier=1.0, point_size=2.0):
    """ss_splat_project: coord (N, 3), scale (N, 3), quat (N, 4), opacity (N,), color (N, 3), all f32; camera: the packed host block ->
    dict(mean2d (N, 2) f32, conic_opacity (N, 4) f32, depth (N,) f32, rect (N, 4) int32, radius (N,) int32, tiles_touched (N,) int32)"""
    _req(coord, torch.float32, "coord")
    if coord.dim() != 2 or coord.shape[1] != 3 or coord.shape[0] < 1:
        raise RuntimeError(f"coord: expected (N >= 1, 3), got {tuple(coord.shape)}")
    N, dev = coord.shape[0], coord.device
    _req(scale, torch.float32, "scale", (N, 3)); _req(quat, torch.float32, "quat", (N, 4))
    _req(opacity, torch.float32, "opacity", (N,)); _req(color, torch.float32, "color", (N, 3))
    if mode not in SPLAT_MODES:
        raise RuntimeError(f"mode must be one of {tuple(SPLAT_MODES)}, got {mode!r}")
    cam, _, _ = _splat_camera(camera)
    out = dict(mean2d=torch.empty((N, 2), dtype=torch.float32, device=dev), conic_opacity=torch.empty((N, 4), dtype=torch.float32, device=dev),
               depth=torch.empty(N, dtype=torch.float32, device=dev), rect=torch.empty((N, 4), dtype=torch.int32, device=dev),
               radius=torch.empty(N, dtype=torch.int32, device=dev), tiles_touched=torch.empty(N, dtype=torch.int32, device=dev))
    check(lib().ss_splat_project(_p(coord), _p(scale), _p(quat), _p(opacity), _p(color), N, cam.ctypes.data, SPLAT_MODES[mode],
                                 float(scale_modifier), float(point_size), _p(out["mean2d"]), _p(out["conic_opacity"]), _p(out["depth"]),
                                 _p(out["rect"]), _p(out["radius"]), _p(out["tiles_touched"]), _stream()), "ss_splat_project")
    return out


def splat_offsets_workspace_bytes(N):
    return int(lib().ss_splat_offsets_workspace_bytes(N))


def splat_offsets(tiles_touched, workspace=None):
    """ss_splat_offsets: tiles_touched (N,) int32 -> (offsets (N,) int64: its exclusive running sum, totals (2,) int64 = {P, visible rows});
    workspace: a uint8 tensor of splat_offsets_workspace_bytes(N) bytes (None: allocated here)"""
    _req(tiles_touched, torch.int32, "tiles_touched")
    if tiles_touched.dim() != 1 or tiles_touched.shape[0] < 1:
        raise RuntimeError(f"tiles_touched: expected (N >= 1,), got {tuple(tiles_touched.shape)}")
    N, dev = tiles_touched.shape[0], tiles_touched.device
    offsets = torch.empty(N, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    ws = _ws(splat_offsets_workspace_bytes(N), dev) if workspace is None else _req(workspace, torch.uint8, "workspace")
    check(lib().ss_splat_offsets(_p(tiles_touched), N, _p(offsets), _p(totals), _p(ws), ws.numel(), _stream()), "ss_splat_offsets")
    return offsets, totals


def splat_keys(depth, rect, tiles_touched, offsets, P, tiles_x, tiles_y):
    """ss_splat_keys: -> (keys (P,) int64 = (tile << 32) | bits(depth), rows (P,) int32)"""
    _req(depth, torch.float32, "depth")
    N, dev = depth.shape[0], depth.device
    _req(rect, torch.int32, "rect", (N, 4)); _req(tiles_touched, torch.int32, "tiles_touched", (N,))
    _req(offsets, torch.int64, "offsets", (N,))
    P = int(P)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    rows = torch.empty(P, dtype=torch.int32, device=dev)
    check(lib().ss_splat_keys(_p(depth), _p(rect), _p(tiles_touched), _p(offsets), N, P, int(tiles_x), int(tiles_y), _p(keys), _p(rows),
                              _stream()), "ss_splat_keys")
    return keys, rows


def splat_ranges(sorted_keys, order, rows, num_tiles):
    """ss_splat_ranges: sorted_keys (P,) int64 and order (P,) int32 as argsort_i64 wrote them, rows (P,) int32 -> (ranges (num_tiles, 2)
    int32, sorted_rows (P,) int32 = rows[order])"""
    _req(sorted_keys, torch.int64, "sorted_keys")
    P, dev = sorted_keys.numel(), sorted_keys.device
    _req(order, torch.int32, "order"); _req(rows, torch.int32, "rows", (P,))
    if order.numel() != P:
        raise RuntimeError(f"order: expected {P} entries, got {order.numel()}")
    ranges = torch.empty((int(num_tiles), 2), dtype=torch.int32, device=dev)
    sorted_rows = torch.empty(P, dtype=torch.int32, device=dev)
    check(lib().ss_splat_ranges(_p(sorted_keys), _p(order), _p(rows), P, int(num_tiles), _p(ranges), _p(sorted_rows), _stream()),
          "ss_splat_ranges")
    return ranges, sorted_rows


def splat_composite(mean2d, conic_opacity, color, depth, ranges, sorted_rows, width, height, background, out=None):
    """ss_splat_composite: -> (image (H, W, 3) f32, alpha (H, W) f32, depth (H, W) f32); background: 3 host floats; out: the three
    tensors to write (None: allocated here)"""
    _req(mean2d, torch.float32, "mean2d")
    N, dev = mean2d.shape[0], mean2d.device
    _req(mean2d, torch.float32, "mean2d", (N, 2)); _req(conic_opacity, torch.float32, "conic_opacity", (N, 4))
    _req(color, torch.float32, "color", (N, 3)); _req(depth, torch.float32, "depth", (N,))
    width, height = int(width), int(height)
    tiles = _div_up(width, SPLAT_TILE) * _div_up(height, SPLAT_TILE)
    _req(ranges, torch.int32, "ranges", (tiles, 2)); _req(sorted_rows, torch.int32, "sorted_rows")
    P = sorted_rows.numel()
    bg = np.ascontiguousarray(np.asarray(background, dtype=np.float32).reshape(-1))
    if bg.shape[0] != 3:
        raise RuntimeError(f"background: expected 3 values, got {bg.shape[0]}")
    if out is None:
        out = (torch.empty((height, width, 3), dtype=torch.float32, device=dev), torch.empty((height, width), dtype=torch.float32, device=dev),
               torch.empty((height, width), dtype=torch.float32, device=dev))
    image, alpha, zmap = out
    _req(image, torch.float32, "image", (height, width, 3)); _req(alpha, torch.float32, "alpha", (height, width))
    _req(zmap, torch.float32, "depth image", (height, width))
    check(lib().ss_splat_composite(_p(mean2d), _p(conic_opacity), _p(color), _p(depth), _p(ranges), _p(sorted_rows), N, P, width, height,
                                   bg.ctypes.data, _p(image), _p(alpha), _p(zmap), _stream()), "ss_splat_composite")
    return image, alpha, zmap
