"""CPU: the C-ABI library builds/loads and exports every symbol include/scenesplat_hip.h declares
(no compute calls without a GPU); host-side pure logic; the argument contract of the packed-layout attention entry points
on the paths that return before any launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "scenesplat_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
        assert s in _lib.PROTOTYPES, f"{s} has no ctypes prototype"
    for s in _lib.PROTOTYPES:
        assert s in syms, f"{s} bound in _lib.py but not declared in the header"
    assert lib.ss_version() >= 100


# ---- the ctypes prototypes and the constants are parsed from the header (scenesplat_amd._lib.parse_header) ----
SYNTHETIC_HEADER = """
/* a comment that names ss_in_comment(int a, double b); and must not count */
#ifndef X_H
#define X_H
#define SS_LIMIT 8
enum { SS_A = 0, SS_B = 1,
       SS_C = -2 };
int ss_three_lines(const void* a, int64_t n,
                   float scale,
                   ss_stream_t stream);
int ss_none(void);
int ss_out(int nwords, const uint32_t* mask, void** stream_out);
int ss_bytes(const unsigned char* mask, const int* orders, uint64_t seed, int32_t ignore, size_t bytes);
unsigned long long ss_id(ss_stream_t stream);
size_t ss_size(int64_t n, int num);
#endif
"""


def test_header_parser_on_synthetic_text():
    from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_ulonglong, c_void_p
    from scenesplat_amd._lib import parse_header
    protos, consts = parse_header(SYNTHETIC_HEADER)
    assert protos == {
        "ss_three_lines": (c_int, [c_void_p, c_int64, c_float, c_void_p]),
        "ss_none": (c_int, []),
        "ss_out": (c_int, [c_int, c_void_p, c_void_p]),
        "ss_bytes": (c_int, [c_void_p, c_void_p, c_uint64, c_int32, c_size_t]),
        "ss_id": (c_ulonglong, [c_void_p]),
        "ss_size": (c_size_t, [c_int64, c_int]),
    }
    assert consts == {"SS_LIMIT": 8, "SS_A": 0, "SS_B": 1, "SS_C": -2}


@pytest.mark.parametrize("text", [
    "int ss_bad(double x);",                                # a type outside the map
    "int ss_bad(int a, short);",
    "double ss_bad(int a);",
    "int ss_good(void);\nint ss_bad(int a,\n",              # no closing `);`: the name census disagrees with the parsed set
    "int ss_bad(int a,\nint ss_good(void);",
])
def test_header_parser_is_strict(text):
    from scenesplat_amd._lib import parse_header
    with pytest.raises(ValueError, match="ss_bad"):
        parse_header(text)


def test_prototypes_of_the_real_header():
    from ctypes import c_float as f, c_int as i, c_int32, c_int64 as i64, c_size_t, c_uint64, c_ulonglong, c_void_p as p
    from scenesplat_amd._lib import PROTOTYPES
    assert len(PROTOTYPES) == len(header_symbols())
    assert PROTOTYPES["ss_knn_grid_query"] == (i, [i, i, p, p, p, p, i, f, f, f, f, i, i, i, i64, p, p, p, p])
    assert PROTOTYPES["ss_aug_gaussians"] == (i, [p, p, p, p, i64, p, p, i, p, p, i, f, f, p, c_uint64, p])
    assert PROTOTYPES["ss_vocab_finish"] == (i, [p, i64, i, i, f, c_int32, p, i64, p, p, p, c_size_t, p])
    assert PROTOTYPES["ss_stream_capture_id"] == (c_ulonglong, [p])
    assert PROTOTYPES["ss_subm_rulebook_table_size"] == (i64, [i64])
    assert PROTOTYPES["ss_argsort_workspace_bytes"] == (c_size_t, [i64, i])
    assert PROTOTYPES["ss_block_tail_fwd"] == (i, [p, p, p, p, p, p, p, p, p, p, i, p, p, f, p, p, p, p, p, p, p, p, i64, i, p])
    assert len(PROTOTYPES["ss_block_tail_fwd"][1]) == 25


def test_loaded_functions_carry_the_parsed_prototypes(attn_lib):
    from scenesplat_amd._lib import PROTOTYPES
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(attn_lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_constants_come_from_the_header():
    from scenesplat_amd import _lib, native
    expect = dict(SS_OK=0, SS_ERR_ARG=1, SS_ERR_LAUNCH=2, SS_ERR_WORKSPACE=3, SS_DTYPE_F32=0, SS_DTYPE_BF16=1, SS_ATTN_SIMT=0,
                  SS_ATTN_MFMA=1, SS_ORDER_Z=0, SS_ORDER_Z_TRANS=1, SS_ORDER_HILBERT=2, SS_ORDER_HILBERT_TRANS=3, SS_MAX_ORDERS=8)
    assert {k: _lib.CONSTANTS[k] for k in expect} == expect
    assert _lib._STATUS == {1: "bad argument", 2: "kernel launch failed", 3: "workspace too small"}
    assert (native.F32, native.BF16, native.ATTN_SIMT, native.ATTN_MFMA) == (0, 1, 0, 1)
    assert native.ORDER_IDS == {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}


def test_ops_refuse_cpu_tensors():
    import torch
    from scenesplat_amd import native as nv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.gather_rows(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32))
    from scenesplat_amd.pointcept_api import MODELS
    m = MODELS.build(dict(type="PT-v3m1", in_channels=4, enc_depths=(1, 1), enc_channels=(8, 16), enc_num_head=(1, 1),
                          enc_patch_size=(16, 16), stride=(2,), dec_depths=(1,), dec_channels=(8,), dec_num_head=(1,),
                          dec_patch_size=(16,)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(dict(feat=torch.zeros(8, 4), grid_coord=torch.zeros(8, 3, dtype=torch.long), offset=torch.tensor([8])))


def test_window_layout_matches_oracle_padding():
    import numpy as np
    from oracle import serialization as oser
    from scenesplat_amd.plan import window_layout
    for offs, K in [([10, 13, 19], 4), ([1500], 1024), ([2048, 2049], 1024), ([7, 71, 271], 64), ([100, 101], 128)]:
        counts = np.diff(np.array([0] + offs)).tolist()
        off_pad, win = window_layout(counts, K)
        pad, unpad, cu = oser.padding(offs, K)
        assert win == cu.tolist()
        assert off_pad[-1] == len(pad)


def test_state_dict_contract():
    """393 tensors / 91.71 M parameters, keys == the reference's."""
    from oracle import ptv3 as optv3
    from scenesplat_amd.pointcept_api import MODELS
    cfg = dict(optv3.DEFAULT_CFG)
    m = MODELS.build(dict(type="PT-v3m1", **cfg))
    sd = m.state_dict()
    ref = optv3.init_state_dict(cfg)   # key set pinned by a strict load into the reference (make_golden.py)
    assert len(sd) == 393 and set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k].shape) for k in sd)
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - 91.71) < 0.01


def test_registry_build_contract():
    from scenesplat_amd.pointcept_api import LOSSES, MODELS
    assert {"PT-v3m1", "LangPretrainer"} <= set(MODELS.module_dict)
    assert {"CosineSimilarity", "L2Loss", "AggregatedContrastiveLoss"} <= set(LOSSES.module_dict)
    with pytest.raises(KeyError):
        MODELS.build(dict(type="nope"))
    with pytest.raises(TypeError, match="PointTransformerV3"):
        MODELS.build(dict(type="PT-v3m1", bogus=1))


def test_bfs_cluster_host_function_matches_oracle():
    """pointgroup bfs_cluster is a HOST function of the C-ABI (as in the reference): testable without a GPU."""
    import numpy as np
    import torch
    from oracle import pointops as opo
    from scenesplat_amd import pointops as po
    g = np.random.default_rng(0)
    xyz = g.random((300, 3), dtype=np.float32)
    ridx, rsl = opo.ballquery_batch_p(xyz, np.zeros(300, int), np.array([0, 300]), 0.15)
    lab = (xyz[:, 0] > 0.5).astype(np.int32)
    ci, co = po.bfs_cluster(torch.as_tensor(lab), torch.as_tensor(ridx), torch.as_tensor(rsl), 5)
    ri, ro = opo.bfs_cluster(lab, ridx, rsl, 5)
    assert np.array_equal(ci.numpy(), ri) and np.array_equal(co.numpy(), ro) and len(ro) > 2


# ---- argument contract of the six packed-layout attention entry points (every call returns before a launch: no GPU) ----
SS_OK, SS_ERR_ARG, SS_ERR_WORKSPACE = 0, 1, 3
SS_F32, SS_BF16 = 0, 1
ATTN_ARGS = dict(num_windows=4, max_window=40, n=150, n_pad=160, channels=64, num_heads=2, dtype=SS_BF16, impl=0, pos_bnd=12,
                 workspace_bytes=1 << 30)
BAD_ARGS = [dict(channels=66, num_heads=4), dict(n_pad=149), dict(dtype=2), dict(dtype=-1), dict(num_windows=-1)]
BAD_RPE_ARGS = [dict(pos_bnd=-1), dict(pos_bnd=65)]


def attn_call(lib, name, **over):
    """one of the four launching entry points with null buffers (never dereferenced on the paths under test)"""
    a = dict(ATTN_ARGS, **over)
    head = [a["num_windows"], a["max_window"], a["n"], a["n_pad"], a["channels"], a["num_heads"], 0.125, a["dtype"], a["impl"]]
    rpe = [None, None, a["pos_bnd"]]
    if name == "ss_window_attn_fwd":
        return lib.ss_window_attn_fwd(None, None, None, None, *head, None, None, None)
    if name == "ss_window_attn_rpe_fwd":
        return lib.ss_window_attn_rpe_fwd(None, None, None, None, *head, *rpe, None, None, None)
    if name == "ss_window_attn_bwd":
        return lib.ss_window_attn_bwd(None, None, None, None, None, None, None, *head, None, None, a["workspace_bytes"], None)
    assert name == "ss_window_attn_rpe_bwd"
    return lib.ss_window_attn_rpe_bwd(None, None, None, None, None, None, None, *head, *rpe, None, None, None,
                                      a["workspace_bytes"], None)


def al256(x):
    return (x + 255) & ~255


def plain_workspace(n, n_pad, channels, num_heads, dtype):
    """delta (n_pad, H) f32 | dK/dV of the borrowed slots (n_pad - n, 2C) in the element type; each part 256-byte aligned"""
    return al256(n_pad * num_heads * 4) + al256((n_pad - n) * 2 * channels * (4 if dtype == SS_F32 else 2))


def rpe_workspace(n, n_pad, channels, num_heads, dtype, num_windows, max_window, pos_bnd):
    """the plain layout | dT slabs ((window, 128-query chunk), H, 3 * (2 * pos_bnd + 1)) f32"""
    chunks = (max_window + 127) // 128
    return plain_workspace(n, n_pad, channels, num_heads, dtype) + al256(num_windows * chunks * num_heads * 3 * (2 * pos_bnd + 1) * 4)


ATTN_LAUNCHING = ["ss_window_attn_fwd", "ss_window_attn_bwd", "ss_window_attn_rpe_fwd", "ss_window_attn_rpe_bwd"]


@pytest.fixture(scope="module")
def attn_lib():
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("name", ATTN_LAUNCHING)
def test_attention_entry_points_refuse_bad_arguments(attn_lib, name):
    bad = BAD_ARGS + (BAD_RPE_ARGS if "rpe" in name else [])
    for over in bad:
        assert attn_call(attn_lib, name, **over) == SS_ERR_ARG, (name, over)
        if name.endswith("bwd"):      # the argument error wins over a workspace that is too small as well
            assert attn_call(attn_lib, name, workspace_bytes=0, **over) == SS_ERR_ARG, (name, over)
    if name == "ss_window_attn_rpe_fwd":      # the ends of the accepted pos_bnd range pass the check
        for pb in (0, 64):
            assert attn_call(attn_lib, name, pos_bnd=pb, num_windows=0) == SS_OK


def test_attention_backward_refuses_a_short_workspace(attn_lib):
    a = ATTN_ARGS
    need = attn_lib.ss_window_attn_bwd_workspace_bytes(a["n"], a["n_pad"], a["channels"], a["num_heads"], a["dtype"])
    assert attn_call(attn_lib, "ss_window_attn_bwd", workspace_bytes=need - 1) == SS_ERR_WORKSPACE
    need = attn_lib.ss_window_attn_rpe_bwd_workspace_bytes(a["n"], a["n_pad"], a["channels"], a["num_heads"], a["dtype"],
                                                           a["num_windows"], a["max_window"], a["pos_bnd"])
    assert attn_call(attn_lib, "ss_window_attn_rpe_bwd", workspace_bytes=need - 1) == SS_ERR_WORKSPACE
    for pb in (0, 64):
        need = attn_lib.ss_window_attn_rpe_bwd_workspace_bytes(a["n"], a["n_pad"], a["channels"], a["num_heads"], a["dtype"],
                                                               a["num_windows"], a["max_window"], pb)
        assert attn_call(attn_lib, "ss_window_attn_rpe_bwd", pos_bnd=pb, workspace_bytes=need - 1) == SS_ERR_WORKSPACE


def test_attention_without_windows_is_a_no_op(attn_lib):
    assert attn_call(attn_lib, "ss_window_attn_fwd", num_windows=0) == SS_OK
    need = attn_lib.ss_window_attn_bwd_workspace_bytes(150, 160, 64, 2, SS_BF16)
    assert attn_call(attn_lib, "ss_window_attn_bwd", num_windows=0, workspace_bytes=need) == SS_OK
    assert attn_call(attn_lib, "ss_window_attn_bwd", num_windows=0, workspace_bytes=need - 1) == SS_ERR_WORKSPACE


@pytest.mark.parametrize("n,n_pad,channels,num_heads,dtype,num_windows,max_window,pos_bnd", [
    (360, 400, 64, 2, SS_BF16, 10, 40, 12),          # borrowed slots, a window shorter than one query chunk
    (1000, 1000, 96, 2, SS_F32, 1, 1000, 31),        # n_pad == n: no borrowed part; 1000 = 7 chunks of 128 + 104
    (5000, 5120, 192, 4, SS_BF16, 5, 1024, 64),      # the largest pos_bnd
])
def test_attention_workspace_sizes_follow_the_stated_layout(attn_lib, n, n_pad, channels, num_heads, dtype, num_windows,
                                                            max_window, pos_bnd):
    assert attn_lib.ss_window_attn_bwd_workspace_bytes(n, n_pad, channels, num_heads, dtype) == \
        plain_workspace(n, n_pad, channels, num_heads, dtype)
    assert attn_lib.ss_window_attn_rpe_bwd_workspace_bytes(n, n_pad, channels, num_heads, dtype, num_windows, max_window,
                                                           pos_bnd) == \
        rpe_workspace(n, n_pad, channels, num_heads, dtype, num_windows, max_window, pos_bnd)
