"""GPU: the labelled point cloud of chunk folders (scenesplat_amd/pointcept_api/pc_labels.py over csrc/pc_attach.hip).  Every
comparison is exact: dtype, shape and bytes.

 1. the recorded reference (tests/golden/pc_attach.npz): three chunks in one batch, and attach_point_cloud over the same data as folders
 2. bitmap word edges: M in {1, 31, 32, 33, 65}, M < k, and -1 padded idx slots, against the numpy statement of tests/pc_attach_cases.py
 3. an empty chunk between two others      4. contention: 4,096 Gaussians on one spot      5. the limit on a lattice, ties, nextafter
 6. brute and grid search                  7. one chunk per batch = one batch              8. nearest labels
 9. two runs are byte-equal               10. chunk_split -> attach_point_cloud -> a dataset's pc_coord / pc_segment"""
import os

import numpy as np
import pytest
import torch

import chunking_cases as cc
import pc_attach_cases as pa

pytestmark = pytest.mark.gpu
FX = pa.load_golden()
CLOUD_ASSETS = {s: FX["pc/" + s] for s in pa.SEGMENTS + ("instance",)}


def run(chunks, cloud, assets, **kw):
    from scenesplat_amd.pointcept_api import slice_point_cloud
    return slice_point_cloud(chunks, cloud, assets, **kw)


def check_against_statement(chunks, cloud, assets, got, labels=None, k=16, limit=0.25, need_margins=True):
    slices, got_labels = got
    assert len(slices) == len(chunks) == len(got_labels)
    for c, chunk in enumerate(chunks):
        rows, coord, segs, nearest = pa.slice_reference(chunk, cloud, assets, k, limit, need_margins)
        pa.same(slices[c][0], coord, ("pc_coord", c))
        assert list(slices[c][1]) == list(assets)
        for n in assets:
            pa.same(slices[c][1][n], segs[n], (n, c))
        assert list(got_labels[c]) == list(labels or ())
        for n in labels or ():
            pa.same(got_labels[c][n], pa.nearest_labels(assets[n], nearest), ("label", n, c))


def cloud_and_assets(M, seed, box=1.0):
    g = np.random.default_rng(seed)
    cloud = (g.random((M, 3)) * box).astype(np.float32)
    assets = dict(segment20=g.integers(-1, 20, M).astype(np.int16), segment_nyu_160=g.integers(0, 160, M).astype(np.int32),
                  color=g.integers(0, 256, (M, 3)).astype(np.uint8), instance=g.integers(-1, 9, M).astype(np.int64))
    return g, cloud, assets


# ---- 1. the recorded reference ----------------------------------------------------------------------------------------------------------------
def test_golden_three_chunks_in_one_batch():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    chunks = [FX[f"chunk{i}/coord"] for i in range(3)]
    slices, labels = run(chunks, FX["pc/coord"], CLOUD_ASSETS, nearest_assets=pa.SEGMENTS)
    rows_bytes = [("pc_coord", 0, np.dtype(np.float32), (3,), 12)] + [(n, 0, a.dtype, a.shape[1:], a.itemsize) for n, a in CLOUD_ASSETS.items()]
    assert pl.chunk_batches([700] * 3, 5000, 16, rows_bytes, pa.SEGMENTS, 1 << 30) == [[0, 1, 2]]
    for i in range(3):
        pa.same(slices[i][0], FX[f"chunk{i}/pc_coord"], i)
        for s in pa.SEGMENTS:
            pa.same(slices[i][1][s], FX[f"chunk{i}/pc_{s}"], (i, s))
            pa.same(labels[i][s], FX[f"chunk{i}/label_{s}"], (i, s))
        # instance is not among the reference's slices; it follows the same rows: those whose coordinates came out
        rows = pa.slice_reference(chunks[i], FX["pc/coord"], {})[0]
        pa.same(slices[i][1]["instance"], FX["pc/instance"][rows], i)


def test_golden_as_folders(tmp_path):
    from scenesplat_amd.pointcept_api import attach_point_cloud
    gs_root, pc_root, dirs = pa.write_layout(str(tmp_path), FX)
    os.makedirs(os.path.join(gs_root, pa.CHUNK_SPLIT, "scene_gone_0"))                      # its original is missing: skipped
    np.save(os.path.join(gs_root, pa.CHUNK_SPLIT, "scene_gone_0", "coord.npy"), FX["chunk0/coord"])
    os.makedirs(os.path.join(gs_root, pa.CHUNK_SPLIT + "_filtered", pa.SCENE + "_0"))       # a filtered copy: not visited
    done = attach_point_cloud(gs_root, pc_root)
    assert done == {pa.SCENE: dirs}
    for i, d in enumerate(dirs):
        assert sorted(os.listdir(d)) == ["coord.npy", "pc_coord.npy", "pc_segment20.npy", "pc_segment_nyu_160.npy"]
        pa.same(np.load(os.path.join(d, "pc_coord.npy")), FX[f"chunk{i}/pc_coord"], i)
        for s in pa.SEGMENTS:
            pa.same(np.load(os.path.join(d, f"pc_{s}.npy")), FX[f"chunk{i}/pc_{s}"], (i, s))
    assert os.listdir(os.path.join(gs_root, pa.CHUNK_SPLIT, "scene_gone_0")) == ["coord.npy"]
    assert os.listdir(os.path.join(gs_root, pa.CHUNK_SPLIT + "_filtered", pa.SCENE + "_0")) == []
    # the scene-level copy ran for the val split
    pa.same(np.load(os.path.join(gs_root, "val", pa.SCENE, "pc_instance.npy")), FX["pc/instance"])
    pa.same(np.load(os.path.join(gs_root, "val", pa.SCENE, "pc_segment20.npy")), FX["pc/segment20"])


# ---- 2. word edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 31, 32, 33, 65])
def test_bitmap_word_edges(M):
    """one chunk of 40 Gaussians; M = 1 and 5 are below k = 16 (k becomes M).  The box is small enough that the last rows are hit
    (the partial word's top bits) and large enough that some neighbours lie beyond the limit."""
    g, cloud, assets = cloud_and_assets(M, 100 + M, box=0.6)
    chunk = (g.random((40, 3)) * 0.9).astype(np.float32)
    got = run([chunk], cloud, assets, nearest_assets=("segment20",))
    check_against_statement([chunk], cloud, assets, got, labels=("segment20",))
    rows = pa.slice_reference(chunk, cloud, {})[0]
    assert rows[-1] == M - 1, "the draw should reach the last row of the cloud (the top bit of the partial last word)"


def test_padded_idx_slots_are_ignored_and_large_ones_flagged():
    """the kernels themselves with M = 5 < k = 16: -1 in the unfilled slots; a row index >= M raises the status and is not followed"""
    from scenesplat_amd import native as nv
    cloud = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.125, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [1, 0, 0.125], [5, 5, 5]], np.float32)
    idx = np.full((3, 16), -1, np.int32)
    idx[0, :5] = [0, 4, 1, 2, 3]
    idx[1, :5] = [1, 4, 0, 3, 2]
    idx[2, :5] = [1, 2, 3, 0, 4]
    dv = lambda a: torch.from_numpy(a).cuda()
    q_offset = dv(np.array([0, 2, 3], np.int32))
    bitmap, nearest, status = nv.pc_mark(dv(cloud), dv(q), q_offset, dv(idx), 0.25)
    tile_base, counts = nv.pc_compact_scan(bitmap, 5)
    assert status.item() == 0 and counts.tolist() == [3, 0] and nearest.tolist() == [0, 1, -1]
    assert bitmap.tolist() == [[0b10011], [0]]
    assert nv.pc_compact(bitmap, 5, tile_base, 3).tolist() == [0, 1, 4]
    # stray bits of a partial last word (rows >= M) are neither counted nor emitted
    bitmap[1, 0] = -1
    tile_base, counts = nv.pc_compact_scan(bitmap, 5)
    assert counts.tolist() == [3, 5] and nv.pc_compact(bitmap, 5, tile_base, 8).tolist() == [0, 1, 4, 0, 1, 2, 3, 4]
    idx[2, 3] = 5
    bitmap, nearest, status = nv.pc_mark(dv(cloud), dv(q), q_offset, dv(idx), 0.25)
    assert status.item() == 1 and bitmap.tolist() == [[0b10011], [0]]


# ---- 3. an empty chunk ---------------------------------------------------------------------------------------------------------------------------
def test_empty_chunk_between_two_others():
    g, cloud, assets = cloud_and_assets(3000, 12)
    near_a, near_b = (g.random((200, 3)) * 0.5).astype(np.float32), (0.5 + g.random((150, 3)) * 0.5).astype(np.float32)
    far = (g.random((120, 3)) + np.float32([3, 3, 3])).astype(np.float32)                   # nothing within 25 cm
    chunks = [near_a, far, near_b, np.empty((0, 3), np.float32)]                            # (and a chunk without Gaussians)
    got = run(chunks, cloud, assets, nearest_assets=("segment_nyu_160",))
    check_against_statement(chunks, cloud, assets, got, labels=("segment_nyu_160",))
    slices, labels = got
    for c in (1, 3):
        pa.same(slices[c][0], np.empty((0, 3), np.float32))
        for n, a in assets.items():
            pa.same(slices[c][1][n], np.empty((0,) + a.shape[1:], a.dtype), n)
    pa.same(labels[1]["segment_nyu_160"], np.full(120, -1, np.int32))
    pa.same(labels[3]["segment_nyu_160"], np.empty(0, np.int32))
    assert slices[0][0].shape[0] > 100 and slices[2][0].shape[0] > 100


# ---- 4. contention ------------------------------------------------------------------------------------------------------------------------------
def test_contention_on_two_words():
    """4,096 Gaussians on one spot, M = 64: every lane of the mark kernel hits the same two words; each of the 16 nearest once"""
    g, cloud, assets = cloud_and_assets(64, 11, box=0.25)
    chunk = np.tile(np.float32([[0.125, 0.125, 0.125]]), (4096, 1))
    got = run([chunk], cloud, assets, nearest_assets=("segment20",))
    rows = pa.slice_reference(chunk[:1], cloud, {})[0]
    assert len(rows) == 16 and (rows < 32).any() and (rows >= 32).any()
    pa.same(got[0][0][0], cloud[rows])
    for n, a in assets.items():
        pa.same(got[0][0][1][n], a[rows], n)
    assert got[1][0]["segment20"].shape == (4096,) and len(set(got[1][0]["segment20"].tolist())) == 1


# ---- 5. the limit ---------------------------------------------------------------------------------------------------------------------------------
def lattice_case():
    """multiples of 1 / 8: every difference, square and sum is exact in fp32 and fp64, so distances tie exactly.  Query 0 at the origin
    has 6 cloud points at exactly 0.25 (rows 1..6), one at 0.125 and, later in the table, duplicates of nearer spots."""
    cloud = np.float32([[0, 0, 0.125], [0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25],
                        [0.25, 0.125, 0], [0.375, 0, 0], [0, 0, 0.125], [0.25, 0, 0], [2, 2, 2], [2, 2, 2.25], [2.125, 2, 2]])
    chunk = np.float32([[0, 0, 0], [2, 2, 2]])
    assets = dict(segment_nyu_160=np.arange(100, 100 + len(cloud), dtype=np.int32))
    return cloud, chunk, assets


def test_limit_is_inclusive_and_ties_go_to_the_smaller_row():
    cloud, chunk, assets = lattice_case()
    got = run([chunk], cloud, assets, nearest_assets=("segment_nyu_160",))
    check_against_statement([chunk], cloud, assets, got, labels=("segment_nyu_160",), need_margins=False)
    rows = pa.slice_reference(chunk, cloud, {}, need_margins=False)[0]
    assert rows.tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13]                     # the points at exactly 0.25 are kept
    assert got[1][0]["segment_nyu_160"].tolist() == [100, 111]                           # rows 0 and 9 tie at 0.125: the smaller one
    # k = 3: query 0 takes rows 0, 9 (0.125) and of the seven at 0.25 the smallest, row 1; query 1 takes 11, 13, 12
    got3 = run([chunk], cloud, assets, k_neighbors=3)
    check_against_statement([chunk], cloud, assets, got3, k=3, need_margins=False)
    assert got3[0][0][1]["segment_nyu_160"].tolist() == [100, 101, 109, 111, 112, 113]


def test_limit_one_ulp_below_drops_the_points_at_the_limit():
    cloud, chunk, assets = lattice_case()
    limit = float(np.nextafter(0.25, 0))
    got = run([chunk], cloud, assets, dist_limit=limit, nearest_assets=("segment_nyu_160",))
    check_against_statement([chunk], cloud, assets, got, labels=("segment_nyu_160",), limit=limit, need_margins=False)
    assert got[0][0][1]["segment_nyu_160"].tolist() == [100, 109, 111, 113]


# ---- 6. brute and grid search ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,seed", [(4000, 22), (4200, 21)])        # (seeds whose draws have no near-tie: slice_reference asserts it)
def test_both_search_paths(M, seed):
    from scenesplat_amd import pointops
    assert M < pointops.KNN_GRID_MIN_POINTS or M - 200 < pointops.KNN_GRID_MIN_POINTS <= M
    g, cloud, assets = cloud_and_assets(M, seed, box=2.0)
    chunks = [(g.random((300, 3)) * np.float32([1.2, 2, 2])).astype(np.float32), (g.random((260, 3)) * 2 + np.float32([1, 0, 0])).astype(np.float32)]
    got = run(chunks, cloud, assets, nearest_assets=("segment20",))
    check_against_statement(chunks, cloud, assets, got, labels=("segment20",))
    assert (got[1][1]["segment20"] == -1).any() and got[0][1][0].shape[0] > 500


# ---- 7. batching, 9. reproducibility -------------------------------------------------------------------------------------------------------------
def test_one_chunk_per_batch_equals_one_batch_and_runs_repeat():
    from scenesplat_amd.pointcept_api import pc_labels as pl
    chunks = [FX[f"chunk{i}/coord"] for i in range(3)]
    kw = dict(nearest_assets=pa.SEGMENTS)
    one = run(chunks, FX["pc/coord"], CLOUD_ASSETS, **kw)
    again = run(chunks, FX["pc/coord"], CLOUD_ASSETS, **kw)
    assets = [("pc_coord", 0, np.dtype(np.float32), (3,), 12)] + [(n, 0, a.dtype, a.shape[1:], a.itemsize) for n, a in CLOUD_ASSETS.items()]
    small = 400 * 1024
    assert pl.chunk_batches([700] * 3, 5000, 16, assets, pa.SEGMENTS, small) == [[0], [1], [2]]
    split = run(chunks, FX["pc/coord"], CLOUD_ASSETS, workspace_bytes=small, **kw)
    dev_in = run([torch.from_numpy(c).cuda() for c in chunks], torch.from_numpy(FX["pc/coord"]).cuda(),
                 {n: torch.from_numpy(a).cuda() for n, a in CLOUD_ASSETS.items()}, **kw)     # device tensors in: the same arrays out
    for other in (again, split, dev_in):
        for c in range(3):
            pa.same(other[0][c][0], one[0][c][0], c)
            for n in CLOUD_ASSETS:
                pa.same(other[0][c][1][n], one[0][c][1][n], (c, n))
            for n in pa.SEGMENTS:
                pa.same(other[1][c][n], one[1][c][n], (c, n))


# ---- 8. nearest labels ----------------------------------------------------------------------------------------------------------------------------
def test_nearest_labels_and_write_semseg_label(tmp_path):
    from scenesplat_amd.pointcept_api import attach_point_cloud
    gs_root, pc_root, dirs = pa.write_layout(str(tmp_path), FX)
    done = attach_point_cloud(gs_root, pc_root, write_semseg_label=True, scene_level=())
    assert done == {pa.SCENE: dirs}
    for i, d in enumerate(dirs):
        # only the nyu segment is written as a per-Gaussian label, in its stored dtype, -1 beyond the limit
        assert sorted(os.listdir(d)) == ["coord.npy", "pc_coord.npy", "pc_segment20.npy", "pc_segment_nyu_160.npy", "segment_nyu_160.npy"]
        lab = np.load(os.path.join(d, "segment_nyu_160.npy"))
        pa.same(lab, FX[f"chunk{i}/label_segment_nyu_160"], i)
        d0 = pa.distances(FX[f"chunk{i}/coord"], FX["pc/coord"]).min(axis=1)
        assert lab.dtype == np.int32 and ((lab == -1) == (d0 > 0.25)).all()
    assert (np.load(os.path.join(dirs[2], "segment_nyu_160.npy")) == -1).sum() > 50
    assert not os.path.exists(os.path.join(gs_root, "val", pa.SCENE, "pc_coord.npy"))       # scene_level=()
    # int16 labels keep their dtype too
    labels = run([FX["chunk2/coord"]], FX["pc/coord"], CLOUD_ASSETS, nearest_assets=("segment20",))[1]
    pa.same(labels[0]["segment20"], FX["chunk2/label_segment20"])


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------------------------
def test_chunk_split_then_attach_then_dataset(tmp_path):
    from scenesplat_amd.pointcept_api import attach_point_cloud, build_dataset, chunk_split
    gs_root, pc_root, name = str(tmp_path / "gs"), str(tmp_path / "pc"), "scene0007_00"
    arrays = cc.scene(30000, 5, lang=16)
    arrays["segment20"] = arrays.pop("segment").astype(np.int64).reshape(-1, 1)
    arrays["quat"] = np.tile(np.float32([1, 0, 0, 0]), (30000, 1))
    arrays["scale"] = np.full((30000, 3), 0.01, np.float32)
    cc.write_scene(gs_root, arrays, split="val", name=name)
    g = np.random.default_rng(9)
    lo, hi = arrays["coord"].min(0), arrays["coord"].max(0)
    cloud = (lo + g.random((20000, 3)) * (hi - lo)).astype(np.float32)
    seg = g.integers(-1, 20, 20000).astype(np.int16)
    cc.write_scene(pc_root, dict(coord=cloud, segment20=seg), split="val", name=name)
    done = chunk_split(gs_root, "val", chunk_range=(2, 2), chunk_stride=(1, 1), chunk_minimum_size=2000)
    split = "val_chunk2x2_stride1x1"
    assert len(done[name]) >= 4
    written = attach_point_cloud(gs_root, pc_root)
    assert written == {name: done[name]}
    ds = build_dataset(dict(type="ScanNetGSDataset", split=split, data_root=gs_root, is_train=False, prefetch=False))
    assert "pc_segment20" in ds.EVAL_PC_ASSETS and len(ds) == len(done[name])
    for i in (0, len(ds) - 1):
        sample, path = ds.get_data(i), ds.data_list[i]
        pc_coord, pc_seg = np.load(os.path.join(path, "pc_coord.npy")), np.load(os.path.join(path, "pc_segment20.npy"))
        assert sample["pc_coord"].is_cuda and pc_coord.shape[0] > 1000 and pc_seg.shape == (pc_coord.shape[0],) and pc_seg.dtype == np.int16
        pa.same(sample["pc_coord"].cpu().numpy(), pc_coord)
        pa.same(sample["pc_segment"].cpu().numpy(), pc_seg.astype(np.int32))
    ds.stager.close()
    pa.same(np.load(os.path.join(gs_root, "val", name, "pc_coord.npy")), cloud)              # and the scene-level copy
