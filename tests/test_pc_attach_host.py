"""The labelled point cloud of chunk folders without a GPU: the exports, the name helpers, the command line and the scene-level copy
of pointcept_api/pc_labels.py, the margins of the recorded reference (tests/golden/pc_attach.npz) that make a selection by fp32
distances agree with cKDTree's, the numpy statement of tests/pc_attach_cases.py against that recording, the declared entry points,
the batching rule, and the errors raised before the device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pc_attach_cases as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = pa.load_golden()


def test_exports():
    import scenesplat_amd.pointcept_api as api
    from scenesplat_amd.pointcept_api import pc_labels
    assert api.slice_point_cloud is pc_labels.slice_point_cloud and api.attach_point_cloud is pc_labels.attach_point_cloud
    assert api.pc_labels is pc_labels and callable(pc_labels.main)


def test_name_helpers():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    assert pl.is_chunk_subdir("val_grid1.0cm_chunk6x6_stride3x3") and pl.is_chunk_subdir("train_chunk6x6_stride3x3")
    assert not pl.is_chunk_subdir("val") and not pl.is_chunk_subdir("train_grid1.0cm_chunk6x6_stride3x3_filtered")
    assert [pl.split_from_subdir(s + "_grid1.0cm_chunk6x6_stride3x3") for s in ("train", "val", "test")] == ["train", "val", "test"]
    with pytest.raises(ValueError, match="split"):
        pl.split_from_subdir("grid1.0cm_chunk6x6")
    assert pl.scene_and_chunk("scene0011_00_12") == ("scene0011_00", "12")
    assert pl.scene_and_chunk("17DRP5sb8fy_region_3_0") == ("17DRP5sb8fy_region_3", "0")


def test_chunk_dirs_are_grouped_by_scene_in_chunk_order(tmp_path):
    from scenesplat_amd.pointcept_api import pc_labels as pl
    for d in ("b_x_10", "b_x_2", "a_0", "b_x_0"):
        os.makedirs(tmp_path / d)
    (tmp_path / "notes.txt").write_text("not a directory")
    got = pl.chunk_dirs_by_scene(str(tmp_path))
    assert list(got) == ["a", "b_x"]
    assert [os.path.basename(p) for p in got["b_x"]] == ["b_x_0", "b_x_2", "b_x_10"]


def test_argument_parser():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    cfg = pl.build_parser().parse_args(["--gs_root", "g", "--pc_root", "p"])
    assert (cfg.gs_root, cfg.pc_root, cfg.k_neighbors, cfg.dist_limit, cfg.write_semseg_label, cfg.no_scene_level) == ("g", "p", 16, 0.25, False, False)
    cfg = pl.build_parser().parse_args(["--gs_root", "g", "--pc_root", "p", "--k_neighbors", "8", "--dist_limit", "0.1",
                                        "--write_semseg_label", "--no_scene_level"])
    assert (cfg.k_neighbors, cfg.dist_limit, cfg.write_semseg_label, cfg.no_scene_level) == (8, 0.1, True, True)
    with pytest.raises(SystemExit):
        pl.build_parser().parse_args(["--gs_root", "g"])


def test_scene_level_copy(tmp_path, capsys):
    """coord / segment* / instance are copied under their pc_ names; an existing pc_coord / pc_segment* stays, pc_instance is copied
    again; a scene without an original is reported and skipped; only the named splits are visited; no GPU is needed without chunks"""
    from scenesplat_amd.pointcept_api import pc_labels as pl
    gs_root, pc_root, _ = pa.write_layout(str(tmp_path), FX, chunk_split="val_plain")       # ("val_plain": no chunked split)
    os.makedirs(os.path.join(gs_root, "val", "scene_b_00"))                                 # no original
    os.makedirs(os.path.join(gs_root, "train", pa.SCENE))                                   # a split that is not copied into
    os.makedirs(os.path.join(pc_root, "train", pa.SCENE))
    np.save(os.path.join(pc_root, "train", pa.SCENE, "coord.npy"), FX["pc/coord"])
    scene_dir = os.path.join(gs_root, "val", pa.SCENE)
    kept = np.arange(6, dtype=np.int16)
    np.save(os.path.join(scene_dir, "pc_segment20.npy"), kept)
    np.save(os.path.join(scene_dir, "pc_instance.npy"), kept)
    assert pl.attach_point_cloud(gs_root, pc_root) == {}
    assert "scene_b_00" in capsys.readouterr().err
    pa.same(np.load(os.path.join(scene_dir, "pc_coord.npy")), FX["pc/coord"])
    pa.same(np.load(os.path.join(scene_dir, "pc_segment_nyu_160.npy")), FX["pc/segment_nyu_160"])
    pa.same(np.load(os.path.join(scene_dir, "pc_segment20.npy")), kept)                     # not overwritten
    pa.same(np.load(os.path.join(scene_dir, "pc_instance.npy")), FX["pc/instance"])         # overwritten, as in the reference
    assert sorted(os.listdir(os.path.join(gs_root, "val", "scene_b_00"))) == [] and os.listdir(os.path.join(gs_root, "train", pa.SCENE)) == []
    # scene_level=() copies nothing; ("train",) reaches the train split
    os.remove(os.path.join(scene_dir, "pc_coord.npy"))
    pl.attach_point_cloud(gs_root, pc_root, scene_level=())
    assert not os.path.exists(os.path.join(scene_dir, "pc_coord.npy"))
    assert pl.copy_scene_level(gs_root, pc_root, ("train",)) == [os.path.join(gs_root, "train", pa.SCENE)]
    assert os.listdir(os.path.join(gs_root, "train", pa.SCENE)) == ["pc_coord.npy"]


def test_golden_margins_and_contents():
    """the two margins the generator asserts, again: the 16th and 17th (and 1st and 2nd) neighbour distances differ by more than 1e-5
    relative, and none of the 16 lies within 1e-5 of the limit; and the comparisons are not empty"""
    meta, cloud = FX["meta"], FX["pc/coord"]
    assert (meta["k"], meta["dist_limit"]) == (16, 0.25) and cloud.shape == (5000, 3) and cloud.dtype == np.float32
    assert FX["pc/segment20"].dtype == np.int16 and (FX["pc/segment20"] == -1).any() and FX["pc/segment_nyu_160"].dtype == np.int32
    over = []
    for i in range(3):
        chunk = FX[f"chunk{i}/coord"]
        assert chunk.shape == (700, 3) and chunk.dtype == np.float32
        d = np.sort(pa.distances(chunk, cloud), axis=1)[:, :17]
        assert pa.margins_hold(d, 16, 0.25)
        over.append(d[:, :16] > 0.25)
        assert FX[f"chunk{i}/pc_coord"].shape[0] == meta["kept"][i] > 0
    assert np.concatenate(over).mean() > 0.05 and (cloud.max(0) <= 2.0).all() and FX["chunk2/coord"][:, 0].max() > 2.25
    assert any((FX[f"chunk{i}/label_segment_nyu_160"] == -1).any() for i in range(3))


@pytest.mark.parametrize("i", range(3))
def test_numpy_statement_reproduces_the_reference(i):
    """tests/pc_attach_cases.py::slice_reference (the oracle of the GPU tests' other cases) against what the reference returned"""
    assets = {s: FX["pc/" + s] for s in pa.SEGMENTS}
    rows, coord, segs, nearest = pa.slice_reference(FX[f"chunk{i}/coord"], FX["pc/coord"], assets)
    pa.same(coord, FX[f"chunk{i}/pc_coord"])
    for s in pa.SEGMENTS:
        pa.same(segs[s], FX[f"chunk{i}/pc_{s}"], s)
        pa.same(pa.nearest_labels(assets[s], nearest), FX[f"chunk{i}/label_{s}"], s)


def test_header_declares_the_entry_points():
    from scenesplat_amd import _lib
    txt = open(os.path.join(ROOT, "include", "scenesplat_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = dict(ss_pc_mark=(i, [p, i64, p, i64, p, i, p, i, p, p, p, p, p]), ss_pc_compact_scan=(i, [p, i64, i, p, p, p]),
                ss_pc_compact=(i, [p, i64, i, p, p, i64, p]), ss_pc_bitmap_words=(i64, [i64]), ss_pc_compact_tiles=(i64, [i64, i]))
    for name, proto in want.items():
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert _lib.PROTOTYPES[name] == proto, name


def test_entry_points_refuse_bad_sizes_before_any_launch():
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert [lib.ss_pc_bitmap_words(m) for m in (1, 31, 32, 33, 65)] == [1, 1, 1, 2, 3]
    assert lib.ss_pc_compact_tiles(1, 1) == 1 and lib.ss_pc_compact_tiles(32 * 1024 + 1, 3) == 6
    limit = ctypes.c_double(0.25)
    err = _lib.CONSTANTS["SS_ERR_ARG"]
    assert lib.ss_pc_mark(None, 0, None, 0, None, 1, None, 16, ctypes.addressof(limit), None, None, None, None) == err      # M = 0
    assert lib.ss_pc_mark(None, 8, None, 0, None, 0, None, 16, ctypes.addressof(limit), None, None, None, None) == err      # no chunk
    assert lib.ss_pc_compact_scan(None, 8, 1, None, None, None) == err and lib.ss_pc_compact(None, 8, 1, None, None, -1, None) == err
    assert lib.ss_pc_compact_scan(1, 1 << 30, 64, 1, 1, None) == err                                                        # rows past int32


def test_batches_respect_the_budget():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    assets = [("pc_coord", 0, np.dtype(np.float32), (3,), 12), ("segment20", 0, np.dtype(np.int16), (), 2)]
    rows = [700, 0, 700, 300]
    one = pl.chunk_batches(rows, 5000, 16, assets, (), 1 << 30)
    assert one == [[0, 1, 2, 3]]
    # per chunk: the bitmap (157 words), idx and dist (8 k), q and nearest (16) per Gaussian, the staging blocks in 64-byte steps
    cost = [157 * 4 + r * (8 * 16 + 16) + sum(-(-min(5000, r * 16) * a[4] // 64) * 64 for a in assets) for r in rows]
    assert pl.chunk_batches(rows, 5000, 16, assets, (), max(cost)) == [[0], [1], [2], [3]]
    assert pl.chunk_batches(rows, 5000, 16, assets, (), cost[0] + cost[1] + cost[2]) == [[0, 1, 2], [3]]
    with pytest.raises(ValueError, match="workspace_bytes"):
        pl.chunk_batches(rows, 5000, 16, assets, (), max(cost) - 1)


def test_inputs_are_checked_before_the_device_is_touched():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    cloud, chunk = FX["pc/coord"], FX["chunk0/coord"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl.slice_point_cloud([torch.from_numpy(chunk)], cloud, {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl.slice_point_cloud([chunk], torch.from_numpy(cloud), {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl.slice_point_cloud([chunk], cloud, {"segment20": torch.from_numpy(FX["pc/segment20"])})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl.slice_point_cloud([chunk], cloud, {}, device="cpu")
    with pytest.raises(ValueError, match="float32"):
        pl.slice_point_cloud([chunk.astype(np.float64)], cloud, {})
    with pytest.raises(ValueError, match="leading dimension"):
        pl.slice_point_cloud([chunk], cloud, {"segment20": FX["pc/segment20"][:-1]})
    with pytest.raises(ValueError, match="signed integer"):
        pl.slice_point_cloud([chunk], cloud, {"w": np.zeros(5000, np.float32)}, nearest_assets=("w",))
    with pytest.raises(ValueError, match="not among"):
        pl.slice_point_cloud([chunk], cloud, {}, nearest_assets=("segment20",))
    with pytest.raises(ValueError, match="no rows"):
        pl.slice_point_cloud([chunk], cloud[:0], {})
