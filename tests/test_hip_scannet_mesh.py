"""The ScanNet converter on the GPU (csrc/mesh.hip, scenesplat_amd/pointcept_api/scannet_mesh.py) against the recorded reference
(tests/golden/scannet_mesh.npz): the decode byte for byte, the vertex normals of both scripts bit for bit, the label arrays with their
dtypes, the refusals the kernels raise, and both end-to-end functions over a temporary two-scene tree."""
import os

import numpy as np
import pytest
import torch

import scannet_mesh_cases as mc
from test_scannet_mesh_host import CATEGORIES, CELLS, GOLD, IDS20, IDS200, OUTSIDE

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sm():
    from scenesplat_amd.pointcept_api import scannet_mesh
    return scannet_mesh


def assert_bytes(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:4].tolist())


def assert_mesh(out, case, what):
    assert list(out) == ["coord", "color", "faces"]
    for a in ("coord", "color", "faces"):
        assert_bytes(out[a], GOLD[f"{case}/{a}"], (what, a))


def _write(tmp_path, data, name="mesh.ply"):
    path = tmp_path / name
    path.write_bytes(data)
    return path


def test_tile_is_the_one_the_cases_assume():
    from scenesplat_amd import native
    assert native.lib().ss_mesh_decode_rows_per_workgroup() == mc.ROWS_PER_WORKGROUP


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(mc.MESHES))
def test_load_equals_the_recording(tmp_path, case):
    assert_mesh(_sm().load_ply_mesh(_write(tmp_path, mc.ply_bytes(case)), DEV), case, case)


@pytest.mark.parametrize("case", ["scan", "extra"])
def test_every_alignment_of_the_face_block(tmp_path, case):
    sm = _sm()
    seen = set()
    for pad in mc.pads_for_alignments(case):
        path = _write(tmp_path, mc.ply_bytes(case, pad))
        seen.add(sm.read_mesh_header(path).face_offset % 4)
        assert_mesh(sm.load_ply_mesh(path, DEV), case, (case, pad))
        assert_mesh(sm.load_ply_mesh(path, DEV, staging_bytes=1000), case, (case, pad, "pieces"))     # splits inside both blocks
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("case", ["scan", "extra", "n257"])
def test_decode_where_the_records_lie(case):
    """the whole file on the device: both blocks decoded in place, at every alignment, and in two pieces at a row offset"""
    from scenesplat_amd import native
    m, spec = mc.mesh(case), mc.MESHES[case]
    n, F = len(m["coord"]), len(m["faces"])
    stride = mc.vertex_records(case, m).dtype.itemsize
    for pad in mc.pads_for_alignments(case):
        data = mc.ply_bytes(case, pad, m)
        head = len(data) - n * stride - 13 * F
        buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
        coord = torch.full((n, 3), -7.0, dtype=torch.float32, device=DEV)
        color = torch.full((n, 3), 9, dtype=torch.uint8, device=DEV)
        faces = torch.full((F, 3), -5, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        cut_v, cut_f = n // 3, F // 2 + 1
        native.mesh_decode_vertices(buf, cut_v, stride, [0, 4, 8, 12, 13, 14], coord, color, row=0, start=head)
        native.mesh_decode_vertices(buf, n - cut_v, stride, [0, 4, 8, 12, 13, 14], coord, color, row=cut_v, start=head + cut_v * stride)
        native.mesh_decode_faces(buf, cut_f, n, faces, status, row=0, start=head + n * stride)
        native.mesh_decode_faces(buf, F - cut_f, n, faces, status, row=cut_f, start=head + n * stride + 13 * cut_f)
        native.mesh_check_status(status, case)
        assert_mesh(dict(coord=coord, color=color, faces=faces), case, (case, pad))


def test_wide_records_are_read_where_they_lie(tmp_path):
    """a stride beyond the LDS tile (200 bytes), colours away from the coordinates: against the inputs"""
    rng = np.random.default_rng(5)
    props = [("x", "float"), ("y", "float"), ("z", "float")] + [(f"e{i}", "float") for i in range(46)] + [("blue", "uchar"), ("red", "uchar"),
                                                                                                      ("green", "uchar"), ("alpha", "uchar")]
    n = 600
    arr = np.zeros(n, dtype=np.dtype([(name, "<" + mc.NP_TYPES[t]) for name, t in props]))
    assert arr.dtype.itemsize == 200
    for name in "xyz":
        arr[name] = rng.uniform(0, 8, n).astype(np.float32)
    for name in ("red", "green", "blue"):
        arr[name] = rng.integers(0, 256, n)
    faces = rng.integers(0, n, (300, 3))
    for pad in (0, 1, 2, 3):
        data = mc.header_bytes(n, len(faces), props, pad=pad) + arr.tobytes() + mc.face_bytes(faces)
        out = _sm().load_ply_mesh(_write(tmp_path, data), DEV, staging_bytes=200 * 260)
        assert_bytes(out["coord"], np.stack([arr["x"], arr["y"], arr["z"]], 1), ("wide", pad))
        assert_bytes(out["color"], np.stack([arr["red"], arr["green"], arr["blue"]], 1), ("wide", pad))
        assert_bytes(out["faces"], faces.astype(np.int32), ("wide", pad))


def test_non_triangles_and_indices_out_of_range_are_refused(tmp_path):
    sm = _sm()
    m = mc.mesh("n257")
    n, F = len(m["coord"]), len(m["faces"])
    head = mc.header_bytes(n, F, mc.SCANNET_PROPS) + mc.vertex_records("n257", m).tobytes()
    counts = np.full(F, 3)
    counts[F - 1] = 4
    with pytest.raises(ValueError, match="vertex count other than 3"):
        sm.load_ply_mesh(_write(tmp_path, head + mc.face_bytes(m["faces"], counts=counts)), DEV)
    for bad in (n, -1, 2 ** 31 - 1):
        faces = m["faces"].copy()
        faces[100, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            sm.load_ply_mesh(_write(tmp_path, head + mc.face_bytes(faces)), DEV, staging_bytes=2000)
        with pytest.raises(ValueError, match="outside"):
            sm.mesh_vertex_normals(torch.from_numpy(m["coord"]).to(DEV), torch.from_numpy(faces.astype(np.int32)).to(DEV))
    sm.load_ply_mesh(_write(tmp_path, head + mc.face_bytes(m["faces"])), DEV)


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(mc.MESHES))
@pytest.mark.parametrize("form", ["pc", "gs"])
def test_normals_are_bit_equal(case, form):
    coord, faces = torch.from_numpy(GOLD[f"{case}/coord"]).to(DEV), torch.from_numpy(GOLD[f"{case}/faces"]).to(DEV)
    got = _sm().mesh_vertex_normals(coord, faces, form)
    assert_bytes(got, GOLD[f"{case}/normal_{form}"], (case, form))
    assert_bytes(_sm().mesh_vertex_normals(coord, faces, form), GOLD[f"{case}/normal_{form}"], (case, form, "again"))


def test_normals_of_a_dense_random_mesh_equal_the_restatement():
    """random triangles over few vertices: long runs in every block, faces that repeat vertices"""
    rng = np.random.default_rng(3)
    coord = (rng.uniform(0, 0.05, (700, 3)) + rng.uniform(0, 8, 3)).astype(np.float32)
    faces = rng.integers(0, 700, (6000, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]
    for form in ("pc", "gs"):
        got = _sm().mesh_vertex_normals(torch.from_numpy(coord).to(DEV), torch.from_numpy(faces).to(DEV), form)
        assert_bytes(got, mc.normals_restated(coord, faces, form), form)


def test_normals_refuse_a_form_they_do_not_know():
    with pytest.raises(ValueError, match="'pc' or 'gs'"):
        _sm().mesh_vertex_normals(torch.zeros((3, 3), device=DEV), torch.zeros((1, 3), dtype=torch.int32, device=DEV), "open3d")


# ---- labels ------------------------------------------------------------------------------------------------------------------------------
def _tables(tmp_path):
    return _sm().scannet_label_tables(mc.write_tsv(tmp_path / "labels.tsv", CELLS), IDS20, IDS200)


@pytest.mark.parametrize("case", mc.LABELLED)
def test_labels_equal_the_recording(tmp_path, case):
    sm = _sm()
    seg_indices, groups = mc.labels(case, CATEGORIES, OUTSIDE)
    g = sm.group_tables(groups, _tables(tmp_path))
    for name, got in zip(("segment20", "segment200", "instance"), sm.mesh_labels(seg_indices, g, torch.int64, DEV)):
        assert_bytes(got, GOLD[f"{case}/pc/{name}"], (case, name))
    nearest = torch.from_numpy(GOLD[f"{case}/gs/nearest"].astype(np.int32)).to(DEV)
    for name, got in zip(("segment20", "segment200", "instance"), sm.mesh_labels(seg_indices, g, torch.int16, DEV, src=nearest)):
        assert GOLD[f"{case}/gs/{name}"].dtype == np.int16
        assert_bytes(got, GOLD[f"{case}/gs/{name}"], (case, "gs", name))


def test_labels_read_out_of_range_as_none(tmp_path):
    sm = _sm()
    g = sm.group_tables([dict(id=5, segments=[2], label="chair")], _tables(tmp_path))
    src = torch.tensor([0, 1, 2, 3, -1, 7], dtype=torch.int32, device=DEV)
    s20, s200, inst = sm.mesh_labels([2, -3, 2 ** 31 - 1, 2], g, torch.int16, DEV, src=src)
    assert inst.tolist() == [5, -1, -1, 5, -1, -1] and s20.tolist() == [IDS20.index(5), -1, -1, IDS20.index(5), -1, -1]
    assert s200.dtype == torch.int16 and s200.tolist()[0] == IDS200.index(2)
    empty = sm.group_tables([], _tables(tmp_path))
    assert [t.tolist() for t in sm.mesh_labels([1, 2], empty, torch.int64, DEV)] == [[-1, -1]] * 3


# ---- nearest vertex and the end-to-end functions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(mc.GS_CASES))
def test_nearest_vertex_equals_the_kd_tree(case):
    from scenesplat_amd.pointcept_api.gaussian_ply import _nearest_rows
    gs = mc.gaussians(case)
    coord = torch.from_numpy(np.stack([gs["x"], gs["y"], gs["z"]], -1)).to(DEV)
    idx, m = _nearest_rows(coord, torch.from_numpy(GOLD[f"{case}/coord"]).to(DEV))
    assert m == len(GOLD[f"{case}/coord"])
    assert_bytes(idx.to(torch.int64), GOLD[f"{case}/gs/nearest"], case)


def _tree(tmp_path):
    """two scenes: SCENES[0] in the train list, SCENES[1] in no list (so `test`); a third folder whose mesh does not parse"""
    root = tmp_path / "raw"
    for k, (scene_id, case) in enumerate(mc.SCENES.items()):
        mc.write_scene(str(root), scene_id, case, CATEGORIES, OUTSIDE, with_labels=k == 0, subdir="scans" if k == 0 else "scans_test", pad=k)
    mc.write_file(str(root / "scans" / "scene0002_00" / "scene0002_00_vh_clean_2.ply"), b"not a ply file\n")
    (tmp_path / "train.txt").write_text("scene0000_00\nscene0002_00\nscene9999_00\n")
    (tmp_path / "val.txt").write_text("scene0500_00\n")
    return root, dict(labels_tsv=mc.write_tsv(tmp_path / "labels.tsv", CELLS), class_ids20=IDS20, class_ids200=IDS200,
                      train_list=tmp_path / "train.txt", val_list=tmp_path / "val.txt")


def _folder(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_preprocess_scannet_end_to_end(tmp_path, capsys):
    root, common = _tree(tmp_path)
    out = tmp_path / "out"
    (train_id, train_case), (test_id, test_case) = mc.SCENES.items()
    written = _sm().preprocess_scannet(str(root), str(out), device=DEV, **common)
    assert written == [str(out / "train" / train_id), str(out / "test" / test_id)]
    assert "scene0002_00" in capsys.readouterr().out and not (out / "train" / "scene0002_00").exists()
    got = _folder(out / "train" / train_id)
    assert sorted(got) == ["color", "coord", "instance", "normal", "segment20", "segment200"]
    for name, a in got.items():
        assert_bytes(a, GOLD[f"{train_case}/pc/{name}"], (train_id, name))
    got = _folder(out / "test" / test_id)
    assert sorted(got) == ["color", "coord", "normal"]                   # a test scene gets no label files
    for name, key in (("coord", "coord"), ("color", "color"), ("normal", "normal_pc")):
        assert_bytes(got[name], GOLD[f"{test_case}/{key}"], (test_id, name))
    written = _sm().preprocess_scannet(str(root), str(tmp_path / "plain"), parse_normals=False, device=DEV, **common)
    assert sorted(os.listdir(written[0])) == ["color.npy", "coord.npy", "instance.npy", "segment20.npy", "segment200.npy"]


def test_preprocess_scannet_gs_end_to_end(tmp_path):
    root, common = _tree(tmp_path)
    out, gs_root, feat_root = tmp_path / "out", tmp_path / "gs", tmp_path / "feat"
    inputs = {}
    for scene_id, case in mc.SCENES.items():
        inputs[scene_id] = mc.gaussians(case)
        mc.write_file(str(gs_root / scene_id / "ckpts" / "point_cloud_30000.ply"), mc.gaussian_ply_bytes(inputs[scene_id]))
        os.makedirs(feat_root / scene_id)
        torch.save((torch.from_numpy(mc.features(case)), None), feat_root / scene_id / "langfeat.pth")
    (train_id, train_case), (test_id, test_case) = mc.SCENES.items()
    written = _sm().preprocess_scannet_gs(str(root), str(out), str(gs_root), feat_root=str(feat_root), feat_only=True, device=DEV, **common)
    assert written == [str(out / "train" / train_id), str(out / "test" / test_id)]      # (scene0002_00 has no checkpoint: skipped)
    assert not (out / "train" / "scene0002_00").exists()
    shapes = dict(coord=(3,), color=(3,), opacity=(), scale=(3,), quat=(4,))
    for scene_id, case, split in ((train_id, train_case, "train"), (test_id, test_case, "test")):
        got = _folder(out / split / scene_id)
        labels = ["instance", "segment20", "segment200"] if split == "train" else []
        assert sorted(got) == sorted(["color", "coord", "lang_feat", "normal", "opacity", "quat", "scale", "valid_feat_mask"] + labels)
        n = len(inputs[scene_id])
        for name, trailing in shapes.items():
            assert got[name].shape == (n,) + trailing and got[name].dtype == (np.uint8 if name == "color" else np.float32), name
        assert_bytes(got["coord"], np.stack([inputs[scene_id][k] for k in "xyz"], -1), (scene_id, "coord"))
        for name in ["normal", "lang_feat", "valid_feat_mask"] + labels:
            assert_bytes(got[name], GOLD[f"{case}/gs/{name}"], (scene_id, name))
    written = _sm().preprocess_scannet_gs(str(root), str(tmp_path / "nofeat"), str(gs_root), feat_root=str(feat_root), skip_feat=True, device=DEV, **common)
    assert "lang_feat.npy" not in os.listdir(written[0]) and "valid_feat_mask.npy" not in os.listdir(written[0])
