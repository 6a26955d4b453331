"""The 3DGS checkpoint reader without a GPU: the exports, the header parser and the column choice of pointcept_api/gaussian_ply.py on
synthetic headers, every error raised before the device is touched, the output-directory rule and the command line against the
recorded reference, and the numpy restatement of tests/ply_cases.py against the same recording."""
import os

import numpy as np
import pytest

import ply_cases as pc

GOLD = pc.load_golden()
STD = pc.standard_properties()


def _gp():
    from scenesplat_amd.pointcept_api import gaussian_ply
    return gaussian_ply


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to choose a device fails the test"""
    gp = _gp()

    def refuse(device):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(gp, "_device", refuse)
    return gp


def _write(tmp_path, data, name="scene.ply"):
    path = tmp_path / name
    path.write_bytes(data)
    return path


def _offsets(props):
    off, out = 0, {}
    for name, t in props:
        out[name] = off
        off += np.dtype(pc.NP_TYPES[t]).itemsize
    return out, off


def test_exports():
    import scenesplat_amd.pointcept_api as api
    from scenesplat_amd import native
    gp = _gp()
    for name in ("read_ply_header", "load_gaussian_ply", "transfer_labels", "preprocess_gs"):
        assert getattr(api, name) is getattr(gp, name)
    assert api.gaussian_ply is gp
    assert callable(gp.main) and callable(gp.build_parser) and callable(native.ply_decode)


def test_c_entry_is_declared():
    from scenesplat_amd import _lib
    import ctypes
    res, args = _lib.PROTOTYPES["ss_ply_decode"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    assert _lib.PROTOTYPES["ss_ply_decode_rows_per_workgroup"] == (ctypes.c_int, [])


def test_fixture_holds_every_case():
    assert list(GOLD["layouts"]) == list(pc.LAYOUTS) and list(GOLD["transfer"]) == list(pc.TRANSFER)
    total = 0
    for case, spec in pc.LAYOUTS.items():
        g = GOLD["layouts"][case]
        assert len(g["records"]) == spec["n"] and g["records"].tobytes() == pc.records(case).tobytes()     # the inputs are reproducible
        total += spec["n"]
    assert 1000 <= total <= 5000
    assert sorted(r["records"].dtype.itemsize for r in GOLD["layouts"].values()) == [64, 68, 68, 80, 248, 540]
    for case, spec in pc.TRANSFER.items():
        assert list(GOLD["transfer"][case]) == list(spec["assets"])


# ---- the header parser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pc.LAYOUTS))
def test_header_of_every_layout(tmp_path, case):
    gp = _gp()
    props, arr = pc.LAYOUTS[case]["props"], GOLD["layouts"][case]["records"]
    data = pc.ply_bytes(arr, props)
    h = gp.read_ply_header(_write(tmp_path, data))
    want, stride = _offsets(props)
    assert h.count == len(arr) and h.stride == stride == arr.dtype.itemsize
    assert h.data_offset == len(data) - arr.nbytes
    assert list(h.properties) == [name for name, _ in props]
    for name, t in props:
        assert h.properties[name] == (np.dtype("<" + pc.NP_TYPES[t]), want[name])
    offsets, n_scale, n_rot = gp.gaussian_columns(h)
    scale, rot = pc.gaussian_names(arr.dtype.names)
    assert (n_scale, n_rot) == (len(scale), len(rot))
    assert offsets == [want[k] for k in ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"] + scale + rot]


def test_standard_layouts_by_number():
    assert len(STD) == 62 and len(pc.standard_properties(0)) == 17
    assert _offsets(STD)[0]["opacity"] == 216 and _offsets(STD)[1] == 248          # the record needs bytes 0-36 and 216-248


def test_header_comments_crlf_face_and_both_spellings(tmp_path):
    gp = _gp()
    props = [("x", "float32"), ("y", "float"), ("z", "float32"), ("a", "char"), ("b", "int8"), ("c", "uchar"), ("d", "uint8"), ("e", "short"),
             ("f", "int16"), ("g", "ushort"), ("h", "uint16"), ("i", "int"), ("j", "int32"), ("k", "uint"), ("l", "uint32"), ("m", "double"),
             ("n", "float64")]
    arr = np.zeros(5, dtype=pc.record_dtype(props))
    plain = gp.read_ply_header(_write(tmp_path, pc.ply_bytes(arr, props), "plain.ply"))
    assert plain.stride == 3 * 4 + 4 * 1 + 4 * 2 + 4 * 4 + 2 * 8 == arr.dtype.itemsize
    assert [plain.properties[k][0].str for k in "abcdefghijklmn"] == ["|i1", "|i1", "|u1", "|u1", "<i2", "<i2", "<u2", "<u2", "<i4", "<i4",
                                                                      "<u4", "<u4", "<f8", "<f8"]
    data = pc.ply_bytes(arr, props, comments=("one", "element face 9 is only a comment"), crlf=True, face=True)
    assert b"\r\nend_header\r\n" in data
    h = gp.read_ply_header(_write(tmp_path, data, "crlf.ply"))
    assert (h.count, h.stride, list(h.properties)) == (5, plain.stride, list(plain.properties))
    assert data[h.data_offset:h.data_offset + arr.nbytes] == arr.tobytes()
    obj = data.replace(b"comment one", b"obj_info x")
    assert gp.read_ply_header(_write(tmp_path, obj, "obj.ply")).data_offset == h.data_offset - 1
    odd = pc.ply_bytes(arr, props, pad_to_odd=True)
    assert gp.read_ply_header(_write(tmp_path, odd, "odd.ply")).data_offset % 2 == 1


def _header(lines, payload=b""):
    return ("\n".join(lines) + "\n").encode() + payload


HEAD = ["ply", "format binary_little_endian 1.0"]
BAD_HEADERS = {
    "magic": (_header(["plx"] + HEAD[1:] + ["element vertex 0", "end_header"]), "magic"),
    "ascii": (_header(["ply", "format ascii 1.0", "element vertex 0", "property float x", "end_header"]), "ascii"),
    "big_endian": (_header(["ply", "format binary_big_endian 1.0", "element vertex 0", "property float x", "end_header"]), "binary_big_endian"),
    "face_first": (_header(HEAD + ["element face 0", "property list uchar int vertex_indices", "element vertex 0", "property float x",
                                   "end_header"]), "first element"),
    "list_in_vertex": (_header(HEAD + ["element vertex 0", "property float x", "property list uchar float weights", "end_header"]), "list"),
    "unknown_type": (_header(HEAD + ["element vertex 0", "property half x", "end_header"]), "half"),
    "short_file": (_header(HEAD + ["element vertex 3", "property float x", "property float y", "end_header"], b"\0" * 23), "shorter"),
}


@pytest.mark.parametrize("case", list(BAD_HEADERS))
def test_header_refusals_name_the_cause(tmp_path, no_device, case):
    data, word = BAD_HEADERS[case]
    path = _write(tmp_path, data)
    with pytest.raises(ValueError, match=word):
        no_device.read_ply_header(path)
    with pytest.raises(ValueError, match=word):
        no_device.load_gaussian_ply(path)


def test_short_file_by_one_byte(tmp_path):
    gp = _gp()
    arr, props = GOLD["layouts"]["sh0_17"]["records"], pc.LAYOUTS["sh0_17"]["props"]
    data = pc.ply_bytes(arr, props)
    assert gp.read_ply_header(_write(tmp_path, data, "whole.ply")).count == len(arr)
    with pytest.raises(ValueError, match="shorter"):
        gp.read_ply_header(_write(tmp_path, data[:-1], "cut.ply"))


# ---- the column choice ---------------------------------------------------------------------------------------------------------------------
def _file_with(tmp_path, props, n=2):
    return _write(tmp_path, pc.ply_bytes(np.zeros(n, dtype=pc.record_dtype(props)), props))


@pytest.mark.parametrize("missing", ["x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"])
def test_missing_property_is_a_keyerror(tmp_path, no_device, missing):
    path = _file_with(tmp_path, [p for p in pc.standard_properties(0) if p[0] != missing])
    with pytest.raises(KeyError, match=missing):
        no_device.load_gaussian_ply(path)


@pytest.mark.parametrize("kind, count", [("scale", 0), ("scale", 5), ("rot", 0), ("rot", 5)])
def test_scale_and_rot_counts(tmp_path, no_device, kind, count):
    props = pc.standard_properties(0, n_scale=count if kind == "scale" else 3, n_rot=count if kind == "rot" else 4)
    with pytest.raises(ValueError, match="1 to 4"):
        no_device.load_gaussian_ply(_file_with(tmp_path, props))


def test_no_device_form(tmp_path, no_device):
    std = pc.standard_properties(0)
    as_double = [(n, "double" if n == "opacity" else t) for n, t in std]
    with pytest.raises(ValueError, match="no device form.*opacity.*float64"):
        no_device.load_gaussian_ply(_file_with(tmp_path, as_double))
    shifted = [("flag", "uchar")] + std                                   # every offset 1 mod 4, stride 69
    with pytest.raises(ValueError, match="no device form"):
        no_device.load_gaussian_ply(_file_with(tmp_path, shifted))
    odd_stride = std + [("flag", "uchar"), ("flag2", "uchar")]            # offsets fine, stride 70
    with pytest.raises(ValueError, match="no device form.*stride 70"):
        no_device.load_gaussian_ply(_file_with(tmp_path, odd_stride))
    unused_double = std[:3] + [("t", "double")] + std[3:]                 # a double nobody needs is fine
    gp = _gp()
    offsets, n_scale, n_rot = gp.gaussian_columns(gp.read_ply_header(_file_with(tmp_path, unused_double)))
    assert offsets[:4] == [0, 4, 8, 32] and (n_scale, n_rot) == (3, 4)


def test_columns_are_sorted_by_numeric_suffix(tmp_path):
    gp = _gp()
    props = pc._f(["rot_3", "scale_1", "x", "rot_0", "y", "scale_0", "z", "rot_2", "f_dc_2", "f_dc_0", "opacity", "f_dc_1", "rot_1"])
    off, _ = _offsets(props)
    offsets, n_scale, n_rot = gp.gaussian_columns(gp.read_ply_header(_file_with(tmp_path, props)))
    names = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "rot_0", "rot_1", "rot_2", "rot_3"]
    assert offsets == [off[k] for k in names] and (n_scale, n_rot) == (2, 4)


def test_cpu_device_is_refused(tmp_path):
    gp = _gp()
    path = _write(tmp_path, pc.ply_bytes(GOLD["layouts"]["scale2"]["records"], pc.LAYOUTS["scale2"]["props"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gp.load_gaussian_ply(path, device="cpu")


def test_empty_cloud_is_refused():
    import torch
    gp = _gp()
    with pytest.raises(ValueError, match="point cloud is empty"):           # (checked before coord's device is looked at)
        gp.transfer_labels(torch.zeros((4, 3)), np.zeros((0, 3), dtype=np.float32), {})
    with pytest.raises(ValueError, match=r"pc_coord must be \(m, 3\)"):
        gp.transfer_labels(torch.zeros((4, 3)), np.zeros((5, 2), dtype=np.float32), {})


# ---- the output-directory rule and the command line ----------------------------------------------------------------------------------------
def test_output_directory_rule(tmp_path):
    gp = _gp()
    src = pc.write_dir_tree(str(tmp_path / "in"))
    out = tmp_path / "out"

    def rel(pairs):
        return sorted(os.path.relpath(d, out).replace(os.sep, "/") for _, d in pairs)

    single = gp.collect_ply_files(os.path.join(src, "a.ply"), out)
    assert [(str(f), str(d)) for f, d in single] == [(os.path.join(src, "a.ply"), str(out))]
    assert rel(single) == GOLD["dirs"]["single"]
    # the recording lists the directories that received a scene; "broken.ply" is found by both and written by neither
    flat, deep = gp.collect_ply_files(src, out), gp.collect_ply_files(src, out, recursive=True)
    assert [d for d in rel(flat) if d != "broken"] == GOLD["dirs"]["flat"] and "broken" in rel(flat)
    assert [d for d in rel(deep) if d != "broken"] == GOLD["dirs"]["deep"]
    assert [os.path.relpath(f, src).replace(os.sep, "/") for f, _ in deep] == sorted(pc.DIR_TREE)
    with pytest.raises(ValueError, match="neither a .ply file nor a directory"):
        gp.collect_ply_files(tmp_path / "nothing_here", out)
    (tmp_path / "notes.txt").write_text("x")
    with pytest.raises(ValueError, match="neither a .ply file nor a directory"):
        gp.collect_ply_files(tmp_path / "notes.txt", out)


def test_unparsable_file_is_skipped_before_the_device(tmp_path, no_device, capsys):
    bad = _write(tmp_path, b"not a ply file\n", "broken.ply")
    assert no_device.preprocess_gs(bad, tmp_path / "out") == []
    assert "skipped, it could not be read" in capsys.readouterr().out and not (tmp_path / "out").exists()
    (tmp_path / "empty").mkdir()
    assert no_device.preprocess_gs(tmp_path / "empty", tmp_path / "out") == []


def test_command_line_parser():
    gp = _gp()
    cfg = gp.build_parser().parse_args(["--input", "a.ply", "--output", "out"])
    assert (cfg.input, cfg.output, cfg.recursive, cfg.pc_dir, cfg.feat) == ("a.ply", "out", False, None, None)
    cfg = gp.build_parser().parse_args(["--input", "in", "--output", "out", "--recursive", "--pc_dir", "pc", "--feat", "langfeat.pth"])
    assert (cfg.recursive, cfg.pc_dir, cfg.feat) == (True, "pc", "langfeat.pth")
    with pytest.raises(SystemExit):
        gp.build_parser().parse_args(["--input", "in"])


def test_feature_files(tmp_path):
    import torch
    gp = _gp()
    lang = GOLD["lang"]
    torch.save((torch.from_numpy(lang["features"]), None), tmp_path / "langfeat.pth")
    np.save(tmp_path / "feat.npy", lang["features"])
    for name in ("langfeat.pth", "feat.npy"):
        got = gp._load_features(tmp_path / name)
        assert got.dtype == np.float16 and got.tobytes() == lang["lang_feat"].tobytes()
        mask = np.any(got != 0.0, axis=1).astype(np.int64)
        assert mask.dtype == lang["valid_feat_mask"].dtype and mask.tobytes() == lang["valid_feat_mask"].tobytes()


# ---- the restatement against the recording -------------------------------------------------------------------------------------------------
def recording_error():
    """E per array: the recording's own largest distance, in fp32 ulp, from the fp64 value, over the whole fixture"""
    worst = dict(scale=0.0, opacity=0.0)
    for g in GOLD["layouts"].values():
        mine = pc.decode_reference(g["records"])
        for a in worst:
            worst[a] = max(worst[a], float(pc.ulp_error(g["out"][a], mine[a + "64"]).max()))
    return worst


@pytest.mark.parametrize("case", list(pc.LAYOUTS))
def test_restatement_against_the_recording(case):
    g = GOLD["layouts"][case]
    mine, E = pc.decode_reference(g["records"]), recording_error()
    for a in ("coord", "color", "quat"):
        assert mine[a].dtype == g["out"][a].dtype and mine[a].shape == g["out"][a].shape
        assert mine[a].tobytes() == g["out"][a].tobytes(), a
    for a in ("scale", "opacity"):
        rec = g["out"][a]
        assert mine[a].dtype == rec.dtype and mine[a].shape == rec.shape
        assert pc.ulp_error(mine[a], mine[a + "64"]).max() <= 0.5                       # one rounding
        print(f"{case} {a}: E = {E[a]:.3f} ulp, restatement vs recording {pc.ulp_error(mine[a], rec.astype(np.float64)).max():.3f} ulp")
        # both lie around the fp64 value, in units of its fp32 spacing: at most E + 1 apart
        assert (np.abs(mine[a].astype(np.float64) - rec.astype(np.float64)) <= (E[a] + 1) * np.spacing(np.abs(mine[a])).astype(np.float64)).all()
    assert 0.5 < E["scale"] < 8 and 0.5 < E["opacity"] < 8                              # numpy's fp32 exp is close, and not correctly rounded


def test_special_rows_of_the_recording():
    for case, g in GOLD["layouts"].items():
        out, rec = g["out"], g["records"]
        assert (out["quat"][0] == 0).all() and rec["rot_1"][0] != 0 and (out["quat"][1] == 0).all()
        assert rec["rot_0"][2] < 0 < out["quat"][2, 0]
        assert out["color"][3].tolist() == [0, 255, 127]
        assert out["opacity"][4] == 1.0 and 0 < out["opacity"][5] < 1e-12
        assert np.allclose(np.linalg.norm(out["quat"][2:].astype(np.float64), axis=1), 1.0, atol=1e-6)
