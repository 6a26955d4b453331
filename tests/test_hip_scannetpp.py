"""The ScanNet++ converter on the GPU (csrc/scannetpp.hip, scenesplat_amd/pointcept_api/scannetpp_mesh.py) against the recorded reference
(tests/golden/scannetpp.npz): the 15-byte vertex layout through the shared decode byte for byte, the normals in Open3D's definition bit
for bit, the top-3 label arrays the reference's loop wrote byte for byte (per vertex and through `src`), both end-to-end functions over a
temporary three-scene tree, and the chain down to a `ScanNetPPGSDataset` validation loader."""
import os

import numpy as np
import pytest
import torch

import scannet_mesh_cases as mc
import scannetpp_cases as sc
from test_scannetpp_host import GOLD, NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sp():
    from scenesplat_amd.pointcept_api import scannetpp_mesh
    return scannetpp_mesh


def assert_bytes(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:4].tolist())


def assert_mesh(out, m, what):
    assert list(out) == ["coord", "color", "faces"]
    assert_bytes(out["coord"], m["coord"], (what, "coord"))
    assert_bytes(out["color"], m["color"], (what, "color"))                # (Open3D's c / 255.0 * 255 gives the file's bytes back)
    assert_bytes(out["faces"], m["faces"].astype(np.int32), (what, "faces"))


def _write(tmp_path, data, name="mesh.ply"):
    path = tmp_path / name
    path.write_bytes(data)
    return path


def _groups(case):
    seg_indices, groups = sc.annotation(case, NAMES)
    return seg_indices, _sp().first_groups(groups, {name: k for k, name in enumerate(NAMES)})


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.MESHES)
def test_the_15_byte_layout_loads_at_every_alignment(tmp_path, case):
    sp, m = _sp(), sc.mesh(case)
    seen = set()
    for pad in sc.pads_for_alignments(case):
        path = _write(tmp_path, sc.ply_bytes(case, pad, m))
        seen.add(sp.read_mesh_header(path).face_offset % 4)
        assert_mesh(sp.load_ply_mesh(path, DEV), m, (case, pad))
        assert_mesh(sp.load_ply_mesh(path, DEV, staging_bytes=1000), m, (case, pad, "pieces"))       # splits inside both blocks
    assert seen == {0, 1, 2, 3}


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.MESHES)
def test_normals_are_bit_equal(case):
    m = sc.mesh(case)
    coord, faces = torch.from_numpy(m["coord"]).to(DEV), torch.from_numpy(m["faces"].astype(np.int32)).to(DEV)
    assert_bytes(_sp().mesh_vertex_normals_o3d(coord, faces), GOLD[f"{case}/normal"], case)
    assert_bytes(_sp().mesh_vertex_normals_o3d(coord, faces), GOLD[f"{case}/normal"], (case, "again"))


def test_normals_of_a_dense_random_mesh_equal_the_restatement():
    """random triangles over few vertices: long runs in every block, faces that repeat vertices, sums that nearly cancel"""
    rng = np.random.default_rng(3)
    coord = (rng.uniform(0, 0.05, (700, 3)) + rng.uniform(0, 8, 3)).astype(np.float32)
    faces = rng.integers(0, 700, (6000, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]
    got = _sp().mesh_vertex_normals_o3d(torch.from_numpy(coord).to(DEV), torch.from_numpy(faces).to(DEV))
    assert_bytes(got, sc.normals_o3d_restated(coord, faces), "dense")


def test_normals_refuse_an_index_out_of_range():
    m = sc.mesh("n257")
    for bad in (len(m["coord"]), -1, 2 ** 31 - 1):
        faces = m["faces"].astype(np.int32)
        faces[100, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            _sp().mesh_vertex_normals_o3d(torch.from_numpy(m["coord"]).to(DEV), torch.from_numpy(faces).to(DEV))


# ---- labels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sc.ANNOS))
def test_labels_equal_the_recording(case):
    seg_indices, g = _groups(case)
    segment, instance = _sp().multilabels(seg_indices, g, DEV)
    assert_bytes(segment, GOLD[f"{case}/segment"], (case, "segment"))
    assert_bytes(instance, GOLD[f"{case}/instance"], (case, "instance"))
    odd = len(seg_indices) - 1 if len(seg_indices) % 2 == 0 else len(seg_indices) - 2       # the other parity: the last lane holds one row
    segment, instance = _sp().multilabels(seg_indices[:odd], g, DEV)
    want = sc.labels_restated(seg_indices[:odd], g)
    assert_bytes(segment, want[0], (case, "segment", "cut")); assert_bytes(instance, want[1], (case, "instance", "cut"))


def test_labels_through_src_equal_the_recording():
    """the GS form: one row per Gaussian, the labels of its nearest vertex"""
    seg_indices, g = _groups("scan")
    nearest = torch.from_numpy(GOLD["scan/gs/nearest"].astype(np.int32)).to(DEV)
    segment, instance = _sp().multilabels(seg_indices, g, DEV, src=nearest)
    assert_bytes(segment, GOLD["scan/gs/segment"], "segment"); assert_bytes(instance, GOLD["scan/gs/instance"], "instance")
    segment, instance = _sp().multilabels(seg_indices, g, DEV, src=nearest[:333])
    assert_bytes(segment, GOLD["scan/gs/segment"][:333], "segment 333"); assert_bytes(instance, GOLD["scan/gs/instance"][:333], "instance 333")


def test_kernels_one_by_one():
    from scenesplat_amd import native
    seg_indices, g = _groups("rich")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    seg, first3 = up(seg_indices), up(g["first3"])
    S, G = len(g["first3"]), len(g["table_label"])
    count = native.spp_segment_hist(seg, S)
    want = np.bincount(np.asarray(seg_indices)[np.asarray(seg_indices) < S], minlength=S).astype(np.int32)
    assert_bytes(count, want, "count")
    assert want.max() > 1024                                             # one counter takes more than a thousand adds
    size = native.spp_group_sizes(first3, count, G)
    want_size = np.zeros(G, dtype=np.int32)
    for k in range(3):
        np.add.at(want_size, g["first3"][g["first3"][:, k] >= 0, k], want[g["first3"][:, k] >= 0])
    assert_bytes(size, want_size, "size")
    assert native.spp_segment_hist(seg, 0).shape == (0,) and native.spp_group_sizes(first3[:0], count[:0], 0).shape == (0,)


def test_labels_read_out_of_range_as_none():
    sp = _sp()
    g = sp.first_groups([dict(objectId=5, segments=[2], label="chair"), dict(objectId=9, segments=[2, 6], label="table")], {"chair": 4, "table": 7})
    src = torch.tensor([0, 1, 2, 3, -1, 7, 4], dtype=torch.int32, device=DEV)
    segment, instance = sp.multilabels([2, 3, 2 ** 31 - 1, 2, 6], g, DEV, src=src)
    assert instance.tolist() == [[5, 9, -1], [-1, -1, -1], [-1, -1, -1], [5, 9, -1], [-1, -1, -1], [-1, -1, -1], [9, -1, -1]]
    assert segment.tolist()[0] == [4, 7, -1] and segment.tolist()[6] == [7, -1, -1] and segment.dtype == torch.int16
    g["first3"][2, 1] = 5                                                # a slot beyond the tables: the row holds nothing
    assert sp.multilabels([2, 6], g, DEV)[1].tolist() == [[-1, -1, -1], [9, -1, -1]]
    g = sp.first_groups([dict(objectId=5, segments=[2], label="chair")], {"chair": 4}, ignore_index=-100)
    assert sp.multilabels([2, 1], g, DEV)[0].tolist() == [[4, -100, -100], [-100, -100, -100]]
    empty = sp.first_groups([], {})
    assert [t.tolist() for t in sp.multilabels([1, 2, 3], empty, DEV)] == [[[-1, -1, -1]] * 3] * 2
    assert [tuple(t.shape) for t in sp.multilabels([], empty, DEV)] == [(0, 3), (0, 3)]


# ---- the end-to-end functions --------------------------------------------------------------------------------------------------------------
def _folder(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the raw download of three scenes, its point-cloud folders (written once, shared), checkpoints and features"""
    tmp = tmp_path_factory.mktemp("scannetpp")
    root, pc_root, gs_root, feat_root = tmp / "raw", tmp / "pc", tmp / "gs", tmp / "feat"
    sc.write_tree(root)
    written = _sp().preprocess_scannetpp(str(root), str(pc_root), device=DEV)
    inputs = {}
    for name, (split, case) in sc.SCENES.items():
        inputs[name] = sc.gaussians(case)
        mc.write_file(str(gs_root / "run_a" / ("scannetpp_" + name) / "ckpts" / "point_cloud_30000.ply"), mc.gaussian_ply_bytes(inputs[name]))
        os.makedirs(feat_root / name)
        torch.save((torch.from_numpy(sc.features(case)), None), feat_root / name / "langfeat.pth")
    return dict(root=root, pc_root=pc_root, gs_root=gs_root, feat_root=feat_root, written=written, inputs=inputs, tmp=tmp)


def test_preprocess_scannetpp_end_to_end(tree, capsys):
    pc_root = tree["pc_root"]
    assert tree["written"] == [str(pc_root / split / name) for name, (split, _) in sc.SCENES.items()]
    assert not (pc_root / "train" / sc.UNREADABLE).exists() and not (pc_root / "train" / "0000000000").exists()
    for name, (split, case) in sc.SCENES.items():
        got, m = _folder(pc_root / split / name), sc.mesh(case)
        assert sorted(got) == (["color", "coord", "normal"] if split == "test" else ["color", "coord", "instance", "normal", "segment"])
        assert_bytes(got["coord"], m["coord"], (name, "coord")); assert_bytes(got["color"], m["color"], (name, "color"))
        assert_bytes(got["normal"], GOLD[f"{case}/normal"], (name, "normal"))
        if split != "test":
            assert_bytes(got["segment"], GOLD[f"{case}/segment"], (name, "segment"))
            assert_bytes(got["instance"], GOLD[f"{case}/instance"], (name, "instance"))
    # the scenes that cannot be read are reported; a list of scenes narrows the run
    only = _sp().preprocess_scannetpp(str(tree["root"]), str(tree["tmp"] / "only"), scenes=[sc.UNREADABLE, list(sc.SCENES)[1]], device=DEV)
    assert only == [str(tree["tmp"] / "only" / "val" / list(sc.SCENES)[1])]
    assert sc.UNREADABLE in capsys.readouterr().out


def test_preprocess_scannetpp_gs_end_to_end(tree):
    sp, out = _sp(), tree["tmp"] / "out"
    common = (str(tree["root"]), str(tree["gs_root"]), str(tree["pc_root"]))
    written, skipped = sp.preprocess_scannetpp_gs(*common, str(out), feat_root=str(tree["feat_root"]), device=DEV)
    assert written == [str(out / split / name) for name, (split, _) in sc.SCENES.items()]
    assert skipped == [name for name, (_, case) in sc.SCENES.items() if bool(GOLD[f"{case}/gs/too_few"])] and len(skipped) == 1
    shapes = dict(coord=(3,), color=(3,), opacity=(), scale=(3,), quat=(4,))
    for name, (split, case) in sc.SCENES.items():
        got = _folder(out / split / name)
        labels = ["instance", "segment"] if split != "test" else []
        feats = [] if name in skipped else ["lang_feat", "valid_feat_mask"]     # under half valid: no feature files
        assert sorted(got) == sorted(["color", "coord", "normal", "opacity", "quat", "scale"] + labels + feats)
        n = len(tree["inputs"][name])
        for a, trailing in shapes.items():
            assert got[a].shape == (n,) + trailing and got[a].dtype == (np.uint8 if a == "color" else np.float32), a
        assert_bytes(got["coord"], np.stack([tree["inputs"][name][k] for k in "xyz"], -1), (name, "coord"))
        for a in ["normal"] + labels + feats:
            assert_bytes(got[a], GOLD[f"{case}/gs/{a}"], (name, a))
    train = list(sc.SCENES)[0]
    written, skipped = sp.preprocess_scannetpp_gs(*common, str(tree["tmp"] / "nofeat"), feat_root=str(tree["feat_root"]), skip_feat=True,
                                                  scenes_list=[train], device=DEV)
    assert skipped == [] and sorted(os.listdir(written[0])) == sorted(a + ".npy" for a in ("color", "coord", "normal", "opacity", "quat", "scale",
                                                                                          "instance", "segment"))
    written, skipped = sp.preprocess_scannetpp_gs(*common, str(tree["tmp"] / "featonly"), feat_root=str(tree["feat_root"]), feat_only=True,
                                                  device=DEV)
    assert len(skipped) == 1 and [os.path.basename(w) for w in written] == [n for n in sc.SCENES if n not in skipped]
    for w in written:
        assert sorted(os.listdir(w)) == ["lang_feat.npy", "valid_feat_mask.npy"]
    assert_bytes(np.load(os.path.join(written[0], "lang_feat.npy")), GOLD["scan/gs/lang_feat"], "feat_only")


def test_chain_down_to_the_validation_loader(tmp_path):
    """raw scan -> point-cloud folder -> GS folder -> chunks -> the cloud attached -> ScanNetPPGSDataset behind build_val_loader"""
    from scenesplat_amd.pointcept_api import attach_point_cloud, build_val_loader, chunk_split
    sp, name = _sp(), "0a5c013435"
    root, pc_root, gs_root = tmp_path / "raw", str(tmp_path / "pc"), str(tmp_path / "gs")
    sc.write_scans(root, name, "val", "scan", anno_case="scan")
    sc.write_meta(root, dict(train=[], val=[name], test=[]))
    mc.write_file(str(tmp_path / "ckpt" / name / "ckpts" / "point_cloud_30000.ply"), mc.gaussian_ply_bytes(sc.gaussians("scan")))
    assert len(sp.preprocess_scannetpp(str(root), pc_root, device=DEV)) == 1
    written, _ = sp.preprocess_scannetpp_gs(str(root), str(tmp_path / "ckpt"), pc_root, gs_root, device=DEV)
    assert written == [os.path.join(gs_root, "val", name)]
    done = chunk_split(gs_root, "val", chunk_range=(0.4, 0.3), chunk_stride=(0.2, 0.15), chunk_minimum_size=20)
    assert len(done[name]) >= 2
    assert attach_point_cloud(gs_root, pc_root) == {name: done[name]}
    split = os.path.basename(os.path.dirname(done[name][0]))
    loader = build_val_loader(dict(data=dict(val=dict(type="ScanNetPPGSDataset", split=split, data_root=gs_root, is_train=False, prefetch=False)),
                                   batch_size_val_per_gpu=1))
    ds = loader.dataset
    assert len(loader) == len(ds) == len(done[name])
    some = False
    for i in range(len(ds)):
        sample, path = ds.get_data(i), ds.data_list[i]
        segment, pc_segment = np.load(os.path.join(path, "segment.npy")), np.load(os.path.join(path, "pc_segment.npy"))
        assert segment.dtype == pc_segment.dtype == np.int16 and segment.shape[1:] == pc_segment.shape[1:] == (3,)
        assert_bytes(sample["segment"], segment[:, 0].astype(np.int32), (i, "segment"))
        assert_bytes(sample["pc_segment"], pc_segment[:, 0].astype(np.int32), (i, "pc_segment"))
        assert_bytes(sample["pc_coord"], np.load(os.path.join(path, "pc_coord.npy")), (i, "pc_coord"))
        some = some or bool((segment[:, 0] >= 0).any() and (segment[:, 1] >= 0).any())
    assert some
    ds.stager.close()
