"""The ScanNet++ converter without a GPU: the exports, the 15-byte vertex layout through the shared header parser, the class list against
the recorded one, `first_groups` plus the numpy statement of the per-row rule (tests/scannetpp_cases.py) against the arrays the
reference's own loop wrote, the numpy restatement of the normals against the recorded ones, the refusals, and the command line."""
import ctypes

import numpy as np
import pytest

import scannet_mesh_cases as mc
import scannetpp_cases as sc

GOLD = sc.load_golden()
NAMES = sc.class_names()


def _sp():
    from scenesplat_amd.pointcept_api import scannetpp_mesh
    return scannetpp_mesh


def _class2idx():
    return {name: k for k, name in enumerate(NAMES)}


def _write(tmp_path, data, name="mesh.ply"):
    path = tmp_path / name
    path.write_bytes(data)
    return path


def test_exports():
    import scenesplat_amd.pointcept_api as api
    from scenesplat_amd import native
    sp = _sp()
    for name in ("scannetpp_classes", "first_groups", "mesh_vertex_normals_o3d", "multilabels", "preprocess_scannetpp", "preprocess_scannetpp_gs"):
        assert getattr(api, name) is getattr(sp, name)
    assert api.scannetpp_mesh is sp
    assert callable(sp.main) and callable(sp.build_parser)
    for name in ("mesh_vertex_normals_o3d", "spp_segment_hist", "spp_group_sizes", "spp_labels"):
        assert callable(getattr(native, name))


def test_c_entries_are_declared():
    from scenesplat_amd import _lib
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.PROTOTYPES["ss_mesh_face_cross_f64"] == (i, [p, p, i64, i64, p, p, p])
    assert _lib.PROTOTYPES["ss_mesh_vertex_normals_f64"] == (i, [p] * 6 + [i64, i64, p, p])
    assert _lib.PROTOTYPES["ss_spp_segment_hist"] == (i, [p, i64, i64, p, p])
    assert _lib.PROTOTYPES["ss_spp_group_sizes"] == (i, [p, p, i64, i, p, p])
    assert _lib.PROTOTYPES["ss_spp_labels"] == (i, [p, i64, p, p, i64, p, p, p, i, i64, i, p, p, p])


def test_fixture_holds_every_case():
    for case in sc.MESHES:
        m = sc.mesh(case)
        assert GOLD[f"{case}/normal"].dtype == np.float32 and GOLD[f"{case}/normal"].shape == (len(m["coord"]), 3)
    for case in sc.ANNOS:
        for a in ("segment", "instance"):
            assert GOLD[f"{case}/{a}"].dtype == np.int16 and GOLD[f"{case}/{a}"].shape == (sc.anno_vertices(case), 3)
    assert ((GOLD["rich/segment"] >= 0).sum(1) == 3).any() and (GOLD["extra/segment"] == -1).all()
    assert bool(GOLD["extra/gs/too_few"]) and not bool(GOLD["scan/gs/too_few"]) and "n257/gs/segment" not in GOLD


# ---- the mesh ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.MESHES)
def test_header_of_the_15_byte_layout(tmp_path, case, monkeypatch):
    from scenesplat_amd.pointcept_api import scannet_mesh
    sp = _sp()

    def refuse(device):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(scannet_mesh, "_device", refuse)
    m = sc.mesh(case)
    seen = set()
    for pad in [0] + sc.pads_for_alignments(case):
        data = sc.ply_bytes(case, pad, m)
        h = sp.read_mesh_header(_write(tmp_path, data))
        head = len(mc.header_bytes(len(m["coord"]), len(m["faces"]), sc.SPP_PROPS, sc.INDEX[case], pad))
        assert (h.n_vertices, h.vertex_stride, h.vertex_offset, h.n_faces) == (len(m["coord"]), 15, head, len(m["faces"]))
        assert h.face_offset == head + 15 * len(m["coord"]) and h.face_offset + 13 * h.n_faces == len(data) and h.index_type == sc.INDEX[case]
        assert sp.mesh_columns(h) == [0, 4, 8, 12, 13, 14]
        seen.add(h.face_offset % 4)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("case", sc.MESHES)
def test_restated_normals_equal_the_recording(case):
    m = sc.mesh(case)
    got = sc.normals_o3d_restated(m["coord"], m["faces"])
    want = GOLD[f"{case}/normal"]
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    if len(m["faces"]):                                                  # neither ScanNet form, nor an fp32 walk, gives these normals
        for form in ("pc", "gs"):
            assert (mc.normals_restated(m["coord"], m["faces"], form).view(np.uint32) != want.view(np.uint32)).any()
        assert (sc.normals_o3d_restated(m["coord"], m["faces"], np.float32).view(np.uint32) != want.view(np.uint32)).any()


def test_the_cancelling_vertex_needs_fp64():
    m = sc.mesh("cancel")
    v = m["special"]["cancel_vertex"]
    walk32 = sc.normals_o3d_restated(m["coord"], m["faces"], np.float32)
    assert (walk32[v].view(np.uint32) != GOLD["cancel/normal"][v].view(np.uint32)).any()
    assert abs(np.linalg.norm(GOLD["cancel/normal"][v].astype(np.float64)) - 1) < 1e-6


# ---- the label tables ----------------------------------------------------------------------------------------------------------------------
def test_classes_equal_the_recording():
    names, class2idx = _sp().scannetpp_classes(sc.TOP100)
    assert names.tolist() == GOLD["classes"].tolist() and len(names) == 100
    assert class2idx == {str(n): k for k, n in enumerate(GOLD["classes"])}
    assert any(" " in n for n in names)                                  # the dummy delimiter keeps a name of several words whole


@pytest.mark.parametrize("case", list(sc.ANNOS))
def test_first_groups_reproduce_the_recorded_labels(case):
    """first_groups, then the rule the kernel applies stated in numpy: equal to what the reference's sequential loop wrote"""
    seg_indices, groups = sc.annotation(case, NAMES)
    g = _sp().first_groups(groups, _class2idx())
    assert g["first3"].dtype == g["table_label"].dtype == g["table_object"].dtype == np.int32
    assert g["first3"].shape == ((max(max(x["segments"]) for x in groups) + 1 if groups else 0), 3) and len(g["table_label"]) == len(groups)
    segment, instance = sc.labels_restated(seg_indices, g)
    assert segment.tobytes() == GOLD[f"{case}/segment"].tobytes() and instance.tobytes() == GOLD[f"{case}/instance"].tobytes()
    if groups:
        ids = sc.segment_ids(case)
        filled = lambda name: int((g["first3"][ids[name]] >= 0).sum())
        assert [filled(n) for n in ("none", "one", "two", "three", "five", "ignored_between", "repeated")] == [0, 1, 2, 3, 3, 2, 2]
        assert ids["beyond"] >= len(g["first3"]) and (g["first3"][ids["absent"]] >= 0).sum() == 1
        slots = g["first3"][ids["ignored_between"]]
        assert slots[1] == slots[0] + 2                                  # the ignored group between them took no slot


def test_first_groups_through_src():
    seg_indices, groups = sc.annotation("scan", NAMES)
    g = _sp().first_groups(groups, _class2idx())
    nearest = GOLD["scan/gs/nearest"]
    segment, instance = sc.labels_restated(seg_indices, g, src=nearest)
    assert segment.tobytes() == GOLD["scan/gs/segment"].tobytes() and instance.tobytes() == GOLD["scan/gs/instance"].tobytes()


def test_first_groups_small_cases_and_refusals():
    sp = _sp()
    c2i = {"chair": 4, "table": 7}
    groups = [dict(objectId=5, segments=[3, 3, 9], label="chair"), dict(objectId=6, segments=[9], label="lamp"),
              dict(objectId=-7, segments=[9, 1], label="table"), dict(objectId=8, segments=[], label="chair")]
    g = sp.first_groups(groups, c2i)
    assert g["first3"].tolist()[3] == [0, -1, -1] and g["first3"].tolist()[9] == [0, 2, -1] and g["first3"].tolist()[1] == [2, -1, -1]
    assert g["first3"].shape == (10, 3) and g["table_label"].tolist() == [4, -1, 7, 4] and g["table_object"].tolist() == [5, -1, -7, 8]
    # an ignore_index that is a class index: that class takes no slot, as `label_index == ignore_index` skips it in the reference
    g = sp.first_groups(groups, c2i, ignore_index=4)
    assert g["first3"].tolist()[9] == [2, -1, -1] and g["first3"].tolist()[3] == [-1, -1, -1] and g["ignore_index"] == 4
    empty = sp.first_groups([], c2i)
    assert empty["first3"].shape == (0, 3) and empty["table_label"].shape == (0,)
    with pytest.raises(ValueError, match="negative segment"):
        sp.first_groups([dict(objectId=1, segments=[2, -4], label="chair")], c2i)
    with pytest.raises(ValueError, match="outside int16"):
        sp.first_groups([dict(objectId=40000, segments=[2], label="chair")], c2i)
    sp.first_groups([dict(objectId=40000, segments=[-2], label="lamp")], c2i)      # an ignored group reaches no output: not looked at


# ---- no device ------------------------------------------------------------------------------------------------------------------------------
def test_cpu_device_is_refused(tmp_path):
    import torch
    sp = _sp()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.mesh_vertex_normals_o3d(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32))
    g = sp.first_groups([], {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.multilabels([1, 2], g, "cpu")
    with pytest.raises(ValueError, match="segIndices outside"):
        sp.multilabels([1, -2], g, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.preprocess_scannetpp(str(tmp_path), str(tmp_path / "out"), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.preprocess_scannetpp_gs(str(tmp_path), str(tmp_path), str(tmp_path), str(tmp_path / "out"), device="cpu")


def test_split_lists(tmp_path):
    sp = _sp()
    sc.write_meta(tmp_path, dict(train=["b1", "a1"], val=["c1"], test=[]))
    assert sp._scenes_and_splits(tmp_path) == [("b1", "train"), ("a1", "train"), ("c1", "val")]      # (an empty test list)
    assert sp._scenes_and_splits(tmp_path, scenes=["c1", "a1", "zz"]) == [("a1", "train"), ("c1", "val")]
    (tmp_path / "some.txt").write_text("b1\n")
    assert sp._scenes_and_splits(tmp_path, scenes=tmp_path / "some.txt") == [("b1", "train")]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_command_line(monkeypatch):
    sp = _sp()
    base = ["--dataset_root", "raw", "--output_root", "out"]
    cfg = sp.build_parser().parse_args(base)
    assert (cfg.gs_root, cfg.pc_root, cfg.feat_root, cfg.skip_feat, cfg.feat_only, cfg.ignore_index, cfg.scenes_list) == (None, None, None, False, False, -1, None)
    assert sp.build_parser().parse_args(base + ["--num_workers", "8", "--ignore_index", "255"]).ignore_index == 255
    with pytest.raises(SystemExit):
        sp.build_parser().parse_args(base[2:])
    calls = []
    monkeypatch.setattr(sp, "preprocess_scannetpp", lambda *a, **k: calls.append(("pc", a, k)) or ["x"])
    monkeypatch.setattr(sp, "preprocess_scannetpp_gs", lambda *a, **k: calls.append(("gs", a, k)) or ([], ["s"]))
    assert sp.main(base + ["--scenes_list", "some.txt"]) == 0
    assert sp.main(base + ["--gs_root", "gs", "--pc_root", "pc", "--feat_root", "feat", "--skip_feat", "--feat_only"]) == 1
    with pytest.raises(SystemExit):
        sp.main(base + ["--gs_root", "gs"])                              # the GS form reads the point-cloud folders
    (kind0, a0, k0), (kind1, a1, k1) = calls
    assert kind0 == "pc" and a0 == ("raw", "out") and k0 == dict(ignore_index=-1, scenes="some.txt")
    assert kind1 == "gs" and a1 == ("raw", "gs", "pc", "out")
    assert k1 == dict(feat_root="feat", feat_only=True, skip_feat=True, scenes_list=None)
