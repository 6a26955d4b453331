"""The oriented-box pruning on the GPU (csrc/obb.hip, scenesplat_amd/pointcept_api/oriented_box.py) against the recorded restatement
(tests/golden/oriented_box.npz, written with Qhull and numpy): the hull filter never loses a hull vertex, the search gives every
candidate volume and the recorded box, ties go to the lowest candidate, membership equals the recorded masks at the wave and tile
edges, and the three converters with `prune_box=0.25` write exactly the rows of the unpruned folders that lie inside the box."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import obb_cases as oc
import scannet_mesh_cases as mc
import scannetpp_cases as sc
from test_scannet_mesh_host import CATEGORIES, CELLS, IDS20, IDS200, OUTSIDE

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = oc.load_golden()


def _ob():
    from scenesplat_amd.pointcept_api import oriented_box
    return oriented_box


def _nv():
    from scenesplat_amd import native
    return native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_rows(rows, want):
    assert rows.dtype == torch.int32 and rows.is_cuda and rows.dim() == 1
    assert np.array_equal(rows.cpu().numpy(), want.astype(np.int32))


# ---- extremes and filter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [5, 13])                                # 125 points: one tile; 2,197: three tiles, the last one partial
def test_extremes_take_the_lower_row_of_equal_projections(side):
    """an integer lattice and integer directions: every projection is exact, most extremes are shared by many rows"""
    g = np.arange(side, dtype=np.float32)
    points = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    dirs = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (1, 1, 0), (1, -1, 0), (0, 1, -1), (1, 1, 1), (2, -1, 3)], dtype=np.float64)
    proj = points.astype(np.float64) @ dirs.T
    rows_max, rows_min = _nv().obb_extremes(_dev(points), _dev(dirs))
    assert np.array_equal(rows_max.cpu().numpy(), proj.argmax(axis=0)) and np.array_equal(rows_min.cpu().numpy(), proj.argmin(axis=0))
    again = _nv().obb_extremes(_dev(points), _dev(dirs))
    assert torch.equal(again[0], rows_max) and torch.equal(again[1], rows_min)


@pytest.mark.parametrize("case", list(oc.CASES))
def test_filter_keeps_every_hull_vertex(case):
    points = GOLD[f"{case}.points"]
    rows = _ob().hull_candidates(points, filter_above=0, device=DEV)
    got = rows.cpu().numpy()
    assert rows.dtype == torch.int32 and np.all(np.diff(got) > 0) and (got.size == 0 or (got[0] >= 0 and got[-1] < len(points)))
    assert np.isin(np.unique(GOLD[f"{case}.tris"]), got).all()
    if case == "room5000":
        assert got.size < len(points) // 2, got.size                    # the filter thins a room
    if len(points) <= 4096:                                             # at or below the default threshold nothing is filtered
        assert_rows(_ob().hull_candidates(points, device=DEV), np.arange(len(points)))


def test_filter_keeps_rows_it_cannot_compare():
    points = GOLD["room5000.points"].copy()
    points[[7, 4000]] = np.nan
    assert np.isin([7, 4000], _ob().hull_candidates(points, filter_above=0, device=DEV).cpu().numpy()).all()


# ---- search ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.GENERAL)
def test_search_gives_every_volume_and_the_recorded_box(case):
    verts, tris, _ = oc.hull_vertices(GOLD[f"{case}.points"], GOLD[f"{case}.tris"])
    volumes, best, box = _nv().obb_search(_dev(verts), _dev(tris))
    want = GOLD[f"{case}.volumes"]
    got = volumes.cpu().numpy()
    assert got.shape == want.shape == (3 * len(tris),) and np.isfinite(want).all()
    rel = np.abs(got - want) / want
    print(f"{case}: {len(verts)} vertices, {len(tris)} triangles, largest relative volume error {rel.max():.3g}")
    assert rel.max() <= 1e-12
    assert int(best.cpu()) == int(GOLD[f"{case}.best"])
    assert np.abs(box.cpu().numpy() - GOLD[f"{case}.box"]).max() <= 1e-9


@pytest.mark.parametrize("slanted_first", [True, False])
def test_search_breaks_ties_by_the_lowest_candidate(slanted_first):
    """`tet` rescaled to the unit corner tetrahedron: all nine frames on the three axis faces give volume exactly 1, the three on the
    slanted face 1 - 2^-52 (1 in exact arithmetic): the least volume is shared by three candidates, and the lowest of them wins
    wherever the slanted face stands in the list"""
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.float64)
    axis_faces, slanted = [(0, 2, 1), (0, 1, 3), (0, 3, 2)], [(1, 2, 3)]
    tris = np.array(slanted + axis_faces if slanted_first else axis_faces + slanted, dtype=np.int32)
    want_best, want_box, want = oc.restated_box(verts, tris)
    volumes, best, box = _nv().obb_search(_dev(verts), _dev(tris))
    got = volumes.cpu().numpy()
    assert np.array_equal(got, want) and (got == 1.0).sum() == 9 and abs(got.min() - 1.0) <= 2.0 ** -52
    shared = np.flatnonzero(got == got.min())
    assert shared.size == 3 and int(best.cpu()) == want_best == int(shared[0]) == (0 if slanted_first else 9)
    assert np.array_equal(box.cpu().numpy(), want_box)


def test_search_over_more_vertices_than_one_lds_chunk():
    """1,500 vertices: a full chunk of 1,024 and a partial one; the triangles need not be a hull for the volumes to be defined"""
    rng = np.random.default_rng(17)
    verts = rng.standard_normal((1500, 3)) * np.array([3.0, 2.0, 1.0])
    tris = np.stack([rng.choice(1500, 3, replace=False) for _ in range(43)]).astype(np.int32)       # 129 candidates: three waves, one partial
    want_best, want_box, want = oc.restated_box(verts, tris)
    volumes, best, box = _nv().obb_search(_dev(verts), _dev(tris))
    assert np.abs(volumes.cpu().numpy() - want).max() <= 1e-12 * want.max()
    assert int(best.cpu()) == want_best and np.abs(box.cpu().numpy() - want_box).max() <= 1e-9


def test_filter_merges_the_chunks_of_a_long_plane_table():
    """2,500 planes: 2,048 that every point lies far below, then the six faces of the unit cube among more of the same: what a row keeps
    is decided in the second chunk and must survive the merge with the first"""
    rng = np.random.default_rng(19)
    points = (rng.random((1000, 3)) * 1.2 - 0.1).astype(np.float32)      # around [0, 1]^3: about 42 % outside
    far = np.tile(np.array([[1.0, 0.0, 0.0, -1e6]]), (2500, 1))
    cube = np.array([(1, 0, 0, -1), (-1, 0, 0, 0), (0, 1, 0, -1), (0, -1, 0, 0), (0, 0, 1, -1), (0, 0, -1, 0)], dtype=np.float64)
    planes = far.copy()
    planes[2100:2106] = cube
    tol = 1e-9
    want = ((points.astype(np.float64) @ planes[:, :3].T + planes[:, 3]) >= -tol).any(axis=1)
    assert 0 < want.sum() < want.size
    rows = _nv().bitmap_rows(_nv().obb_filter(_dev(points), _dev(planes), tol), len(points))
    assert_rows(rows, np.flatnonzero(want))
    assert_rows(_nv().bitmap_rows(_nv().obb_filter(_dev(points), _dev(far), tol), len(points)), np.arange(0))


def test_search_gives_a_triangle_without_area_no_volume():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0)], dtype=np.float64)
    tris = np.array([(0, 1, 4), (0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3), (0, 1, 9)], dtype=np.int32)   # collinear; a row out of range
    volumes, best, box = _nv().obb_search(_dev(verts), _dev(tris))
    got = volumes.cpu().numpy()
    assert np.isnan(got[0:3]).all() and np.isnan(got[15:18]).all() and np.isfinite(got[3:15]).all()
    assert 3 <= int(best.cpu()) < 15
    volumes, best, box = _nv().obb_search(_dev(verts), _dev(tris[:1]))
    assert int(best.cpu()) == -1 and np.isnan(volumes.cpu().numpy()).all()


# ---- the box end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_above", [0, 4096])
@pytest.mark.parametrize("case", oc.GENERAL)
def test_minimal_oriented_box_gives_the_recorded_box(case, filter_above):
    box = _ob().minimal_oriented_box(GOLD[f"{case}.points"], device=DEV, filter_above=filter_above)
    want = GOLD[f"{case}.box"]
    err = np.abs(box.as15() - want).max()
    print(f"{case}, filter_above={filter_above}: largest difference to the recorded box {err:.3g}")
    assert err <= 1e-9
    assert box.volume == pytest.approx(np.nanmin(GOLD[f"{case}.volumes"]), rel=1e-12)


@pytest.mark.parametrize("filter_above", [0, 4096])
@pytest.mark.parametrize("case", oc.LATTICE)
def test_minimal_oriented_box_of_a_lattice(case, filter_above):
    points = GOLD[f"{case}.points"]
    box = _ob().minimal_oriented_box(_dev(points), filter_above=filter_above)
    print(f"{case}, filter_above={filter_above}: volume {box.volume!r}")
    assert abs(box.volume - oc.LATTICE_VOLUME) <= 1e-5 * oc.LATTICE_VOLUME
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    assert box.enlarged(1e-6 * extent).contains(points).all()


def test_minimal_oriented_box_refuses_a_flat_cloud():
    rng = np.random.default_rng(3)
    flat = rng.random((6000, 3)).astype(np.float32)
    flat[:, 1] = 0.5
    for filter_above in (0, 4096, 10000):
        with pytest.raises(ValueError, match="span no volume"):
            _ob().minimal_oriented_box(flat, device=DEV, filter_above=filter_above)


# ---- membership ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", oc.PREFIXES)
def test_points_within_box_equals_the_recorded_mask(m):
    ob = _ob()
    for case in oc.CASES:
        box = GOLD[f"{case}.box"]
        big = ob.OrientedBox(box[0:3], box[3:12], box[12:15]).enlarged(oc.MARGIN)
        rows = ob.points_within_box(big, GOLD[f"{case}.queries"][:m], device=DEV)
        assert_rows(rows, np.flatnonzero(GOLD[f"{case}.mask"][:m]))


def test_points_within_box_all_inside_and_all_outside():
    ob, case = _ob(), "box300"
    box, q, mask = GOLD[f"{case}.box"], GOLD[f"{case}.queries"], GOLD[f"{case}.mask"]
    big = ob.OrientedBox(box[0:3], box[3:12], box[12:15]).enlarged(oc.MARGIN)
    assert_rows(ob.points_within_box(big, _dev(q[mask])), np.arange(int(mask.sum())))
    assert_rows(ob.points_within_box(big, _dev(q[~mask])), np.arange(0))
    aligned = ob.OrientedBox([1.0, 2.0, 3.0], np.eye(3), [2.0, 4.0, 8.0])
    on_face = np.array([(2.0, 2.0, 3.0), (0.0, 4.0, 7.0), (2.0000002, 2.0, 3.0), (1.0, 2.0, np.nan)], dtype=np.float32)
    assert_rows(ob.points_within_box(aligned, on_face, device=DEV), np.array([0, 1]))               # inclusive; NaN is outside


# ---- the converters ------------------------------------------------------------------------------------------------------------------------
def restated_mask(cloud, coord, margin=oc.MARGIN):
    """the membership of coord in the restated box of cloud: the package's hull (tests/test_oriented_box_host.py holds it to Qhull's),
    then steps 2-6 in numpy"""
    tris = _ob().convex_hull(cloud.astype(np.float64))
    verts, local, _ = oc.hull_vertices(cloud, tris)
    _, box, _ = oc.restated_box(verts, local)
    return oc.inside(box, coord, margin)


def spread_gaussians(cloud, n, seed):
    """a checkpoint whose centres spread to 1.5 x the scan's extent and, the test scans being under a metre, 50 cm more on every side:
    a bare 1.5 x would lie inside the 25 cm margin"""
    rng = np.random.default_rng(seed)
    lo, hi = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)
    half = 0.75 * (hi - lo) + 0.5
    arr = np.zeros(n, dtype=np.dtype([(name, "<f4") for name, _ in mc.GS_PROPS]))
    for name, _ in mc.GS_PROPS:
        arr[name] = rng.standard_normal(n).astype(np.float32)
    xyz = ((lo + hi) * 0.5 + (rng.random((n, 3)) * 2.0 - 1.0) * half).astype(np.float32)
    for a, name in enumerate("xyz"):
        arr[name] = xyz[:, a]
    return arr, xyz


def features_valid_inside(mask, seed):
    """(n, 8) float32 features: none outside the box, four in five inside: under half of the file, over half of the kept rows"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((mask.size, 8)).astype(np.float32)
    f[~mask | (rng.random(mask.size) < 0.2)] = 0
    return f


def _folder(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def assert_pruned_folder(pruned, full, mask, what, extra=()):
    kept = int(mask.sum())
    assert 0 < kept < mask.size, (what, kept, mask.size)
    assert sorted(pruned) == sorted(list(full) + list(extra)), (what, sorted(pruned), sorted(full))
    for name, a in full.items():
        want = a[mask]                                                   # boolean indexing keeps the file order
        assert pruned[name].dtype == want.dtype and pruned[name].shape == want.shape, (what, name, pruned[name].shape, want.shape)
        assert pruned[name].tobytes() == want.tobytes(), (what, name)


def test_preprocess_scannet_gs_prunes_by_the_box(tmp_path, capsys):
    from scenesplat_amd.pointcept_api import scannet_mesh
    root = tmp_path / "raw"
    for k, (scene_id, case) in enumerate(mc.SCENES.items()):
        mc.write_scene(str(root), scene_id, case, CATEGORIES, OUTSIDE, with_labels=k == 0, subdir="scans" if k == 0 else "scans_test", pad=k)
    (tmp_path / "train.txt").write_text("scene0000_00\n")
    (tmp_path / "val.txt").write_text("scene0500_00\n")
    common = dict(labels_tsv=mc.write_tsv(tmp_path / "labels.tsv", CELLS), class_ids20=IDS20, class_ids200=IDS200,
                  train_list=tmp_path / "train.txt", val_list=tmp_path / "val.txt")
    gs_root, feat_root, masks = tmp_path / "gs", tmp_path / "feat", OrderedDict()
    for k, (scene_id, case) in enumerate(mc.SCENES.items()):
        cloud = mc.mesh(case)["coord"]
        arr, xyz = spread_gaussians(cloud, 900 + 333 * k, 71 + k)
        masks[scene_id] = restated_mask(cloud, xyz)
        mc.write_file(str(gs_root / scene_id / "ckpts" / "point_cloud_30000.ply"), mc.gaussian_ply_bytes(arr))
        os.makedirs(feat_root / scene_id)
        torch.save((torch.from_numpy(features_valid_inside(masks[scene_id], 81 + k)), None), feat_root / scene_id / "langfeat.pth")
    args = (str(root), str(gs_root))
    full = scannet_mesh.preprocess_scannet_gs(args[0], str(tmp_path / "full"), args[1], feat_root=str(feat_root), device=DEV, **common)
    capsys.readouterr()
    pruned = scannet_mesh.preprocess_scannet_gs(args[0], str(tmp_path / "pruned"), args[1], feat_root=str(feat_root), device=DEV,
                                                prune_box=0.25, **common)
    said = capsys.readouterr().out
    assert len(full) == len(pruned) == 2
    for (scene_id, mask), f, p in zip(masks.items(), full, pruned):
        got = _folder(p)
        assert "lang_feat" in got and "valid_feat_mask" in got and "normal" in got
        assert_pruned_folder(got, _folder(f), mask, scene_id)
        assert f"Pruned {int((~mask).sum())} gaussians by init bounding box." in said


@pytest.fixture(scope="module")
def scannetpp_tree(tmp_path_factory):
    from scenesplat_amd.pointcept_api import scannetpp_mesh
    tmp = tmp_path_factory.mktemp("obb_scannetpp")
    root, pc_root, gs_root, feat_root = tmp / "raw", tmp / "pc", tmp / "gs", tmp / "feat"
    sc.write_tree(root)
    scannetpp_mesh.preprocess_scannetpp(str(root), str(pc_root), device=DEV)
    masks = OrderedDict()
    for k, (name, (split, case)) in enumerate(sc.SCENES.items()):
        cloud = np.load(pc_root / split / name / "coord.npy")
        arr, xyz = spread_gaussians(cloud, 800 + 257 * k, 91 + k)
        masks[name] = restated_mask(cloud, xyz)
        mc.write_file(str(gs_root / "run_a" / ("scannetpp_" + name) / "ckpts" / "point_cloud_30000.ply"), mc.gaussian_ply_bytes(arr))
        os.makedirs(feat_root / name)
        torch.save((torch.from_numpy(features_valid_inside(masks[name], 95 + k)), None), feat_root / name / "langfeat.pth")
    return dict(tmp=tmp, common=(str(root), str(gs_root), str(pc_root)), feat_root=feat_root, pc_root=pc_root, masks=masks)


def test_preprocess_scannetpp_gs_prunes_by_the_box(scannetpp_tree, capsys):
    from scenesplat_amd.pointcept_api import scannetpp_mesh
    t = scannetpp_tree
    full, skipped_full = scannetpp_mesh.preprocess_scannetpp_gs(*t["common"], str(t["tmp"] / "full"), feat_root=str(t["feat_root"]), device=DEV)
    capsys.readouterr()
    pruned, skipped = scannetpp_mesh.preprocess_scannetpp_gs(*t["common"], str(t["tmp"] / "pruned"), feat_root=str(t["feat_root"]), device=DEV,
                                                             prune_box=0.25)
    said = capsys.readouterr().out
    assert len(full) == len(pruned) == len(sc.SCENES)
    # under half of every file holds a feature, over half of the kept rows: the rule looks at the kept rows
    assert skipped_full == list(sc.SCENES) and skipped == []
    feats = {name: torch.load(t["feat_root"] / name / "langfeat.pth")[0].to(torch.float16).numpy() for name in sc.SCENES}
    for (name, mask), f, p in zip(t["masks"].items(), full, pruned):
        got, whole = _folder(p), _folder(f)
        assert "lang_feat" not in whole
        whole["lang_feat"] = feats[name]
        whole["valid_feat_mask"] = np.any(feats[name] != 0.0, axis=1).astype(int)
        assert_pruned_folder(got, whole, mask, name)
        assert f"Pruned {int((~mask).sum())} gaussians by init bounding box." in said
    # feat_only never prunes, as in the reference
    only, _ = scannetpp_mesh.preprocess_scannetpp_gs(*t["common"], str(t["tmp"] / "featonly"), feat_root=str(t["feat_root"]), feat_only=True,
                                                     device=DEV, prune_box=0.25)
    assert only == []                                                    # (every file is under half valid)


def test_preprocess_gs_prunes_by_the_box_of_pc_dir(scannetpp_tree, tmp_path, capsys):
    from scenesplat_amd.pointcept_api import gaussian_ply
    t = scannetpp_tree
    name, (split, case) = list(sc.SCENES.items())[0]
    pc_dir = t["pc_root"] / split / name                                 # coord, normal, segment, instance of a labelled scene
    mask = t["masks"][name]
    ply = next((t["tmp"] / "gs").rglob(f"*{name}/ckpts/point_cloud_30000.ply"))
    feat = tmp_path / "feat.npy"
    np.save(feat, features_valid_inside(mask, 99))
    full = gaussian_ply.preprocess_gs(ply, tmp_path / "full", pc_dir=str(pc_dir), feat=str(feat), device=DEV)
    capsys.readouterr()
    pruned = gaussian_ply.preprocess_gs(ply, tmp_path / "pruned", pc_dir=str(pc_dir), feat=str(feat), device=DEV, prune_box=0.25)
    assert f"Pruned {int((~mask).sum())} gaussians by init bounding box." in capsys.readouterr().out
    got = _folder(pruned[0])
    assert {"lang_feat", "valid_feat_mask", "normal", "segment", "instance"} <= set(got)
    assert_pruned_folder(got, _folder(full[0]), mask, name)
    # a cloud without a volume has no box: the checkpoint is skipped
    flat = tmp_path / "flat"
    os.makedirs(flat)
    cloud = np.load(pc_dir / "coord.npy")
    cloud[:, 2] = 1.0
    np.save(flat / "coord.npy", cloud)
    assert gaussian_ply.preprocess_gs(ply, tmp_path / "none", pc_dir=str(flat), device=DEV, prune_box=0.25) == []
    assert "span no volume" in capsys.readouterr().out
