"""CPU: the host half of the oriented-box pruning (scenesplat_amd/pointcept_api/oriented_box.py): the numpy hull against Qhull's recorded
triangle sets, OrientedBox against the recorded membership masks, the refusals, and the `prune_box` keyword / `--prune_box` flag of the
three converters.  The kernels are tested in tests/test_hip_oriented_box.py."""
import inspect

import numpy as np
import pytest

import obb_cases as oc


@pytest.fixture(scope="module")
def golden():
    return oc.load_golden()


@pytest.mark.parametrize("case", oc.GENERAL)
def test_convex_hull_returns_qhulls_triangle_set(golden, case):
    from scenesplat_amd.pointcept_api.oriented_box import convex_hull
    points = golden[f"{case}.points"].astype(np.float64)
    tris = convex_hull(points)
    assert tris.dtype == np.int32 and tris.ndim == 2 and tris.shape[1] == 3
    assert oc.triangle_set(tris) == oc.triangle_set(golden[f"{case}.tris"])
    # every triangle is counter-clockwise seen from outside: no point lies above its plane
    a, b, c = points[tris[:, 0]], points[tris[:, 1]], points[tris[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert ((points @ n.T) - (n * a).sum(axis=1)).max() <= 1e-9


@pytest.mark.parametrize("case", oc.LATTICE)
def test_convex_hull_of_a_lattice_bounds_it(golden, case):
    """coplanar points: the triangle set is not unique, the body is"""
    from scenesplat_amd.pointcept_api.oriented_box import convex_hull
    points = golden[f"{case}.points"].astype(np.float64)
    tris = convex_hull(points)
    a, b, c = points[tris[:, 0]], points[tris[:, 1]], points[tris[:, 2]]
    volume = np.einsum("ij,ij->i", a - points.mean(axis=0), np.cross(b - points.mean(axis=0), c - points.mean(axis=0))).sum() / 6.0
    assert abs(volume - oc.LATTICE_VOLUME) <= 1e-5 * oc.LATTICE_VOLUME


@pytest.mark.parametrize("case", list(oc.CASES))
def test_contains_equals_the_recorded_masks(golden, case):
    from scenesplat_amd.pointcept_api.oriented_box import OrientedBox
    box = golden[f"{case}.box"]
    ob = OrientedBox(box[0:3], box[3:12], box[12:15])
    assert ob.R.shape == (3, 3) and ob.center.dtype == ob.R.dtype == ob.extent.dtype == np.float64
    assert np.array_equal(ob.enlarged(oc.MARGIN).contains(golden[f"{case}.queries"]), golden[f"{case}.mask"])
    assert ob.enlarged(1e-6).contains(golden[f"{case}.points"]).all()
    assert ob.volume == pytest.approx(np.nanmin(golden[f"{case}.volumes"]), rel=1e-15)
    assert ob.contains(np.empty((0, 3), np.float32)).shape == (0,)


def test_enlarged_changes_only_the_extent(golden):
    from scenesplat_amd.pointcept_api.oriented_box import OrientedBox
    box = golden["box300.box"]
    ob = OrientedBox(box[0:3], box[3:12], box[12:15])
    big = ob.enlarged(0.25)
    assert np.array_equal(big.center, ob.center) and np.array_equal(big.R, ob.R)
    assert np.array_equal(big.extent, ob.extent + 0.5)
    assert np.array_equal(ob.extent, box[12:15]) and big is not ob                               # the original is untouched
    assert np.array_equal(big.as15()[:12], box[:12])


def test_hull_refuses_too_few_points_and_flat_clouds():
    from scenesplat_amd.pointcept_api.oriented_box import convex_hull, minimal_oriented_box
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="fewer than 4 points"):
        convex_hull(rng.random((3, 3)))
    with pytest.raises(ValueError, match="fewer than 4 points"):
        minimal_oriented_box(rng.random((3, 3)).astype(np.float32), device="cuda")               # (refused before the device is touched)
    flat = rng.random((50, 3))
    flat[:, 2] = 0.25
    with pytest.raises(ValueError, match="span no volume"):
        convex_hull(flat)
    line = np.outer(np.arange(10.0), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="span no volume"):
        convex_hull(line)
    with pytest.raises(ValueError, match="span no volume"):
        convex_hull(np.ones((10, 3)))
    with pytest.raises(ValueError, match="not finite"):
        convex_hull(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan]]))


def test_points_are_checked_before_the_device():
    from scenesplat_amd.pointcept_api.oriented_box import minimal_oriented_box
    with pytest.raises(ValueError, match=r"\(n, 3\) float32"):
        minimal_oriented_box(np.zeros((10, 3), dtype=np.float64), device="cuda")
    with pytest.raises(ValueError, match=r"\(n, 3\) float32"):
        minimal_oriented_box(np.zeros((10, 2), dtype=np.float32), device="cuda")


def test_exports():
    import scenesplat_amd.pointcept_api as api
    from scenesplat_amd.pointcept_api import oriented_box
    assert api.OrientedBox is oriented_box.OrientedBox
    assert api.minimal_oriented_box is oriented_box.minimal_oriented_box
    assert api.points_within_box is oriented_box.points_within_box
    src = inspect.getsource(oriented_box)
    for banned in ("scipy", "sklearn", "open3d"):
        assert f"import {banned}" not in src and f"from {banned}" not in src


def test_prune_box_keyword_and_flag():
    from scenesplat_amd.pointcept_api import gaussian_ply, scannet_mesh, scannetpp_mesh
    for fn in (gaussian_ply.preprocess_gs, scannet_mesh.preprocess_scannet_gs, scannetpp_mesh.preprocess_scannetpp_gs):
        assert inspect.signature(fn).parameters["prune_box"].default is None
    required = {gaussian_ply: ["--input", "i", "--output", "o"],
                scannet_mesh: ["--dataset_root", "d", "--output_root", "o", "--labels_tsv", "l", "--class_ids20", "a", "--class_ids200", "b",
                               "--train_list", "t", "--val_list", "v"],
                scannetpp_mesh: ["--dataset_root", "d", "--output_root", "o"]}
    for module, argv in required.items():
        parser = module.build_parser()
        assert parser.parse_args(argv).prune_box is None
        assert parser.parse_args(argv + ["--prune_box"]).prune_box == 0.25
        assert parser.parse_args(argv + ["--prune_box", "0.1"]).prune_box == 0.1


def test_prune_box_needs_a_point_cloud(tmp_path):
    from scenesplat_amd.pointcept_api.gaussian_ply import preprocess_gs
    with pytest.raises(ValueError, match="prune_box needs pc_dir"):
        preprocess_gs(tmp_path, tmp_path / "out", prune_box=0.25)


def test_without_prune_box_the_box_code_is_never_entered(tmp_path, monkeypatch):
    """prune_box=None: preprocess_gs runs as before.  load_gaussian_ply is replaced by host arrays (no GPU here), the box functions by
    trip wires."""
    import torch
    from scenesplat_amd.pointcept_api import gaussian_ply, oriented_box

    def trip(*a, **k):
        raise AssertionError("the oriented-box code was entered without prune_box")

    for name in ("minimal_oriented_box", "points_within_box", "hull_candidates", "convex_hull"):
        monkeypatch.setattr(oriented_box, name, trip)
    monkeypatch.setattr(gaussian_ply, "prune_gaussians", trip)
    rng = np.random.default_rng(5)
    fake = {"coord": torch.from_numpy(rng.random((9, 3)).astype(np.float32)), "color": torch.zeros((9, 3), dtype=torch.uint8),
            "opacity": torch.ones(9), "scale": torch.ones((9, 3)), "quat": torch.ones((9, 4))}
    monkeypatch.setattr(gaussian_ply, "load_gaussian_ply", lambda path, device=None: fake)
    (tmp_path / "a.ply").write_bytes(b"ply\n")
    done = gaussian_ply.preprocess_gs(tmp_path / "a.ply", tmp_path / "out")
    assert done == [str(tmp_path / "out")]
    assert np.array_equal(np.load(tmp_path / "out" / "coord.npy"), fake["coord"].numpy())
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["color.npy", "coord.npy", "opacity.npy", "quat.npy", "scale.npy"]
