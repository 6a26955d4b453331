"""The 3DGS checkpoint reader on the GPU (csrc/ply.hip, scenesplat_amd/pointcept_api/gaussian_ply.py) against the recorded reference
(tests/golden/gaussian_ply.npz) and the numpy restatement of tests/ply_cases.py.

coord / color / quat are compared byte for byte.  scale / opacity: within 1 fp32 ulp of the fp64 value (one rounding of an fp64 result
that is good to 1 fp64 ulp), and within E + 1 ulp of the recording, E being the recording's own largest distance from the fp64 value
(computed from the fixture in test_gaussian_ply_host.recording_error; numpy's fp32 exp is not correctly rounded).

A logit or log of -100: the fp64 expression rounds to the fp32 denormal 3.8e-44, not to 0 (numpy's fp32 exp(-100) is a denormal as
well); the tests assert that value, exact zeros at -1000, and inf / 1 at +100."""
import os

import numpy as np
import pytest
import torch

import ply_cases as pc
from test_gaussian_ply_host import GOLD, recording_error

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARRAYS = ("coord", "color", "opacity", "scale", "quat")
SH0 = pc.standard_properties(0)


def _gp():
    from scenesplat_amd.pointcept_api import gaussian_ply
    return gaussian_ply


def rows_per_workgroup():
    from scenesplat_amd import native
    return native.lib().ss_ply_decode_rows_per_workgroup()


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:4].tolist())


def assert_decode(got, arr, what, recording=None):
    """got: host arrays of a decode of `arr`.  Bytes against the restatement (and the recording); the ulp bounds of the docstring."""
    mine = pc.decode_reference(arr)
    assert list(got) == list(ARRAYS)
    for a in ("coord", "color", "quat"):
        assert_bytes(got[a], mine[a], (what, a))
        if recording is not None:
            assert_bytes(got[a], recording[a], (what, a, "recording"))
    for a in ("scale", "opacity"):
        assert got[a].dtype == np.float32 and got[a].shape == mine[a].shape, (what, a, got[a].shape)
        err = pc.ulp_error(got[a], mine[a + "64"])
        print(f"{what} {a}: {err.max(initial=0.0):.3f} ulp from the fp64 value")
        assert err.max(initial=0.0) <= 1.0, (what, a, err.max(initial=0.0))
        if recording is not None:
            E = recording_error()[a]
            unit = np.spacing(np.abs(mine[a])).astype(np.float64)
            apart = np.abs(got[a].astype(np.float64) - recording[a].astype(np.float64)) / unit
            print(f"{what} {a}: {apart.max(initial=0.0):.3f} ulp from the recording (E = {E:.3f})")
            assert apart.max(initial=0.0) <= E + 1, (what, a, apart.max(initial=0.0), E)


def load(tmp_path, arr, props, name="scene.ply", staging_bytes=256 << 20, **kw):
    path = pc.write_ply(os.path.join(str(tmp_path), name), arr, props, **kw)
    out = _gp().load_gaussian_ply(path, DEV, staging_bytes=staging_bytes)
    for k, v in out.items():
        assert v.is_cuda and v.is_contiguous(), k
    return host(out)


# ---- 1. against the recording ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pc.LAYOUTS))
def test_decode_against_the_recording(case, tmp_path):
    g = GOLD["layouts"][case]
    got = load(tmp_path, g["records"], pc.LAYOUTS[case]["props"], comments=("fixture",))
    assert_decode(got, g["records"], case, recording=g["out"])


# ---- 2. row-count edges against the restatement -------------------------------------------------------------------------------------------
def edge_sizes():
    R = rows_per_workgroup()
    return [0, 1, 63, 64, 65, R - 1, R, R + 1, 3 * R + 7]


@pytest.mark.parametrize("props", [pc.standard_properties(), SH0, pc.LAYOUTS["wide540"]["props"]], ids=["stride248", "stride68", "stride540"])
def test_row_count_edges(props, tmp_path):
    for n in edge_sizes():
        arr = pc.synthetic(n, props, seed=100 + n)
        got = load(tmp_path, arr, props, name=f"n{n}.ply")
        assert got["coord"].shape == (n, 3) and got["opacity"].shape == (n,) and got["scale"].shape == (n, 3) and got["quat"].shape == (n, 4)
        assert_decode(got, arr, f"n={n}")


@pytest.mark.parametrize("props, per", [(pc.standard_properties(), 150), (SH0, 37), (pc.standard_properties(), 1)], ids=["248x150", "68x37", "248x1"])
def test_pieces_with_a_short_last_one(props, per, tmp_path):
    stride = pc.record_dtype(props).itemsize
    n = 3 * per + max(1, per // 3) if per > 1 else 5
    arr = pc.synthetic(n, props, seed=7)
    got = load(tmp_path, arr, props, staging_bytes=per * stride + stride // 2)     # (not a whole number of records: rounded down)
    assert_decode(got, arr, f"{n} rows in pieces of {per}")
    if per == 1:
        assert_decode(load(tmp_path, arr, props, staging_bytes=1), arr, "staging_bytes below one record")


@pytest.mark.parametrize("props", [pc.standard_properties(), SH0], ids=["stride248", "stride68"])
@pytest.mark.parametrize("skip", [0, 1, 2, 3, 4])
def test_tile_starts_aligned_and_not(props, skip):
    """the records tensor starts `skip` records into an aligned buffer: 248 * skip is 0 or 8 mod 16, 68 * skip is 0, 4, 8 or 12 mod 16"""
    from scenesplat_amd import native as nv
    R, stride = rows_per_workgroup(), pc.record_dtype(props).itemsize
    n = 2 * R + 9
    arr = pc.synthetic(n + skip, props, seed=11 + skip)
    buf = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[skip * stride:]
    assert view.data_ptr() % 16 == (skip * stride) % 16
    scale_names, rot_names = pc.gaussian_names(arr.dtype.names)
    offsets = [arr.dtype.fields[k][1] for k in ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"] + scale_names + rot_names]
    n_scale, n_rot = len(scale_names), len(rot_names)
    pad = 5                                                               # rows around the written ones keep their fill
    out = dict(coord=torch.full((n + 2 * pad, 3), -7.0, device=DEV), color=torch.full((n + 2 * pad, 3), 9, dtype=torch.uint8, device=DEV),
               opacity=torch.full((n + 2 * pad,), -7.0, device=DEV), scale=torch.full((n + 2 * pad, 3), -7.0, device=DEV),
               quat=torch.full((n + 2 * pad, 4), -7.0, device=DEV))
    nv.ply_decode(view, n, stride, offsets, n_scale, n_rot, out["coord"], out["color"], out["opacity"], out["scale"], out["quat"], row=pad)
    got = host(out)
    for k, v in got.items():
        fill = 9 if k == "color" else -7.0
        assert (v[:pad] == fill).all() and (v[pad + n:] == fill).all(), k
    assert_decode({k: np.ascontiguousarray(got[k][pad:pad + n]) for k in ARRAYS}, arr[skip:], f"skip={skip}")


def test_vertex_block_at_an_odd_file_offset(tmp_path):
    arr = pc.synthetic(200, pc.standard_properties(), seed=3)
    path = pc.write_ply(os.path.join(str(tmp_path), "odd.ply"), arr, pc.standard_properties(), pad_to_odd=True, crlf=True, face=True)
    assert _gp().read_ply_header(path).data_offset % 2 == 1
    assert_decode(host(_gp().load_gaussian_ply(path, DEV)), arr, "odd offset")


def test_c_entry_refuses_bad_arguments():
    import ctypes
    from scenesplat_amd import native as nv, _lib
    lib, bad = nv.lib(), _lib.CONSTANTS["SS_ERR_ARG"]
    buf = torch.zeros(68 * 4, dtype=torch.uint8, device=DEV)
    out = torch.zeros(64, dtype=torch.float32, device=DEV)
    p, o = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def call(n=4, stride=68, offs=tuple(range(0, 56, 4)), n_scale=3, n_rot=4, rec=p):
        return lib.ss_ply_decode(rec, n, stride, (ctypes.c_int32 * 15)(*offs), n_scale, n_rot, o, o, o, o, o, None)
    assert call(n=0) == 0 and call(n=0, rec=None) == 0
    assert call(stride=70) == bad and call(stride=0) == bad
    assert call(offs=(2,) + tuple(range(4, 56, 4))) == bad and call(offs=tuple(range(0, 52, 4)) + (68,)) == bad and call(offs=(-4,) + tuple(range(4, 56, 4))) == bad
    assert call(n_scale=0) == bad and call(n_scale=5) == bad and call(n_rot=0) == bad and call(n_rot=5) == bad and call(n=-1) == bad
    assert call(rec=ctypes.c_void_p(buf.data_ptr() + 2)) == bad
    torch.cuda.synchronize()
    assert (out == 0).all()
    with pytest.raises(RuntimeError, match="multiples of 4"):
        f3, u3, f4 = out[:3].view(1, 3), buf[:3].view(1, 3), out[:4].view(1, 4)
        nv.ply_decode(buf, 1, 66, list(range(0, 56, 4)), 3, 4, f3, u3, out[:1], f3, f4)


# ---- 3. values ----------------------------------------------------------------------------------------------------------------------------
def test_quaternion_rules(tmp_path):
    arr = pc.synthetic(16, SH0, seed=5)
    arr["rot_0"][0], arr["rot_1"][0], arr["rot_2"][0], arr["rot_3"][0] = 0.0, 0.5, -0.25, 2.0           # rot_0 == 0, the rest set
    for k in ("rot_0", "rot_1", "rot_2", "rot_3"):
        arr[k][1] = 0.0                                                                                # all zero
    arr["rot_0"][2], arr["rot_1"][2] = -0.5, 0.25                                                      # negative real part
    arr["rot_2"][3] = np.nan                                                                           # a NaN component
    arr["rot_0"][4] = -0.0
    arr["rot_0"][5], arr["rot_1"][5], arr["rot_2"][5], arr["rot_3"][5] = 1e-30, 1e-30, 0.0, 0.0        # squares underflow: norm 0 + 1e-9
    arr["rot_0"][6], arr["rot_1"][6] = 3e19, 3e19                                                      # squares overflow: q / inf
    got = load(tmp_path, arr, SH0)
    q = got["quat"]
    assert (q[0] == 0).all() and (q[1] == 0).all()
    assert q[2, 0] > 0 and q[2, 1] < 0
    assert np.isnan(q[3]).all()
    assert (q[4] == 0).all()
    assert q[5, 0] > 0 and (q[6] == 0).all()
    mine = pc.decode_reference(arr)
    keep = np.arange(len(arr)) != 3                                                                    # (NaN payloads are not compared)
    assert_bytes(q[keep], mine["quat"][keep], "quat")
    assert np.isnan(mine["quat"][3]).all()
    for a in ("coord", "color"):
        assert_bytes(got[a], mine[a], a)


def test_colour_clip_bounds_and_integer_landings(tmp_path):
    f32 = np.float32
    c0 = f32(pc.C0)
    # f_dc at which clip((f * c0) + 0.5) * 255 lands on and just under an integer k: the fp32 neighbours t of k / 255, and for each the
    # fp32 neighbours of the f_dc that solves (f * c0) + 0.5 = t
    vals = []
    for k in (1, 2, 100, 127, 128, 200, 254, 255):
        seen = set()
        for j in range(-4, 5):
            t = f32(k / 255.0)
            for _ in range(abs(j)):
                t = np.nextafter(t, f32(np.inf if j > 0 else -np.inf), dtype=f32)
            f = f32((float(t) - 0.5) / pc.C0)
            for i in range(-2, 3):
                g = f
                for _ in range(abs(i)):
                    g = np.nextafter(g, f32(np.inf if i > 0 else -np.inf), dtype=f32)
                seen.add(int(f32(min(max(f32(f32(g * c0) + f32(0.5)), f32(0)), f32(1)) * f32(255))))
                vals.append(g)
        assert {k - 1, k} <= seen, (k, seen)                             # both sides of the landing are among the inputs
    lo, hi = f32(-0.5 / pc.C0), f32(0.5 / pc.C0)
    for b in (lo, hi):
        vals += [np.nextafter(b, f32(-np.inf), dtype=f32), b, np.nextafter(b, f32(np.inf), dtype=f32)]
    vals += [f32(-1e30), f32(1e30), f32(-np.inf), f32(np.inf), f32(0.0), f32(-0.0), f32(1e-45), f32(-1.7724538), f32(1.7724539)]
    vals = np.asarray(vals, dtype=f32)
    n = len(vals)
    arr = pc.synthetic(n, SH0, seed=8)
    arr["f_dc_0"], arr["f_dc_1"], arr["f_dc_2"] = vals, vals[::-1], np.roll(vals, 7)
    got = load(tmp_path, arr, SH0)
    mine = pc.decode_reference(arr)
    assert_bytes(got["color"], mine["color"], "color")
    col = got["color"][:, 0]
    assert col[vals <= lo].max() == 0 and col[vals >= hi].min() == 255 and set(np.unique(col)) >= {0, 1, 127, 128, 254, 255}


def test_exp_and_sigmoid_limits(tmp_path):
    props = pc.standard_properties(0, n_scale=2)
    logits = np.array([100.0, -100.0, 1000.0, -1000.0, np.nan, np.inf, -np.inf, 0.0, 88.0, 89.0, -87.0, -104.0, 17.0, -17.0], dtype=np.float32)
    arr = pc.synthetic(len(logits), props, seed=9)
    arr["opacity"], arr["scale_0"], arr["scale_1"] = logits, logits, logits[::-1]
    got = load(tmp_path, arr, props)
    assert got["scale"].shape == (len(logits), 2) and got["quat"].shape == (len(logits), 4)           # two scale columns give (n, 2)
    s, o = got["scale"][:, 0], got["opacity"]
    tiny = np.float32(np.exp(-100.0))                                      # 3.8e-44: a denormal, what the fp64 expression rounds to
    assert 0 < tiny < np.finfo(np.float32).tiny
    assert s[0] == np.inf and s[2] == np.inf and s[5] == np.inf and s[3] == 0 and s[6] == 0 and s[7] == 1 and np.isnan(s[4])
    assert s[1] == tiny
    assert o[0] == 1 and o[2] == 1 and o[5] == 1 and o[3] == 0 and o[6] == 0 and o[7] == 0.5 and np.isnan(o[4])
    assert o[1] == np.float32(1.0 / (1.0 + np.exp(100.0))) and o[1] == tiny
    assert np.isfinite(s[8]) and s[9] == np.inf                            # the fp32 overflow threshold of exp lies between 88 and 89
    assert_bytes(got["scale"][:, 1], got["scale"][::-1, 0].copy(), "scale_1")
    mine = pc.decode_reference(arr)
    for a in ("scale", "opacity"):
        assert pc.ulp_error(got[a], mine[a + "64"]).max() <= 1.0, a


# ---- 4. label transfer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pc.TRANSFER))
def test_transfer_labels_against_the_kd_tree(case):
    gp, spec = _gp(), pc.TRANSFER[case]
    coord = torch.from_numpy(GOLD["layouts"][spec["layout"]]["out"]["coord"]).to(DEV)
    cloud, assets = pc.cloud(spec["cloud"]), pc.cloud_assets(case, spec)
    from scenesplat_amd import pointops
    assert (len(cloud) >= pointops.KNN_GRID_MIN_POINTS) == (spec["cloud"] == "fine")                 # both searches are covered
    got = gp.transfer_labels(coord, cloud, assets)
    assert list(got) == list(assets)
    for a, want in GOLD["transfer"][case].items():
        assert got[a].is_cuda
        assert_bytes(got[a].cpu().numpy(), want, (case, a))                # every row, dtype and squeezed shape included
    as_tensors = gp.transfer_labels(coord, torch.from_numpy(cloud).to(DEV), {a: torch.from_numpy(v).to(DEV) for a, v in assets.items()})
    for a, want in GOLD["transfer"][case].items():
        assert_bytes(as_tensors[a].cpu().numpy(), want, (case, a, "tensors"))


@pytest.mark.parametrize("case", list(pc.TRANSFER))
def test_transfer_assets_of_odd_row_widths(case):
    """rows of 1, 3 and 5 bytes (ss_gather_rows has no byte lane: these take the grouped gather) beside even ones, against the rows
    the recorded KD-tree choice selects: the chosen row numbers are checked against the case's recorded float normals first"""
    gp, spec = _gp(), pc.TRANSFER[case]
    coord = torch.from_numpy(GOLD["layouts"][spec["layout"]]["out"]["coord"]).to(DEV)
    cloud, recorded = pc.cloud(spec["cloud"]), pc.cloud_assets(case, spec)
    m = len(cloud)
    rng = np.random.default_rng(5)
    assets = dict(row=np.arange(m, dtype=np.int32), u8=rng.integers(0, 256, m).astype(np.uint8), i8=rng.integers(-128, 128, m).astype(np.int8),
                  flag=rng.random(m) < 0.5, rgb=rng.integers(0, 256, (m, 3)).astype(np.uint8), five=rng.integers(0, 256, (m, 5)).astype(np.uint8),
                  pair=rng.integers(0, 256, (m, 2)).astype(np.uint8), cube=rng.integers(0, 256, (m, 3, 3)).astype(np.uint8))
    got = {a: v.cpu().numpy() for a, v in gp.transfer_labels(coord, cloud, assets).items()}
    rows = got["row"]
    want_normal = GOLD["transfer"][case]["normal"]                        # float rows of the recording pin the choice, row by row
    assert_bytes(recorded["normal"][rows], want_normal, "the chosen rows")
    for a, v in assets.items():
        assert_bytes(got[a], v[rows], (case, a))
    as_tensors = gp.transfer_labels(coord, cloud, {a: torch.from_numpy(assets[a]).to(DEV) for a in ("u8", "flag", "rgb")})
    for a in ("u8", "flag", "rgb"):
        assert_bytes(as_tensors[a].cpu().numpy(), assets[a][rows], (case, a, "tensor"))


def test_transfer_tie_goes_to_the_lower_row():
    gp = _gp()
    cloud = np.array([[5, 5, 5], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, 0]], dtype=np.float32)
    coord = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.75, 0.0]], device=DEV)
    got = gp.transfer_labels(coord, cloud, dict(segment=np.arange(10, 16, dtype=np.int16), pair=np.arange(12, dtype=np.uint8).reshape(6, 2)))
    assert got["segment"].cpu().tolist() == [11, 11, 13] and got["segment"].dtype == torch.int16
    assert got["pair"].cpu().tolist() == [[2, 3], [2, 3], [6, 7]]
    empty = gp.transfer_labels(coord[:0], cloud, dict(segment=np.arange(6, dtype=np.int64)))
    assert tuple(empty["segment"].shape) == (0,) and empty["segment"].dtype == torch.int64
    with pytest.raises(ValueError, match="empty"):
        gp.transfer_labels(coord, cloud[:0], {})
    with pytest.raises(ValueError, match="rows"):
        gp.transfer_labels(coord, cloud, dict(segment=np.arange(5)))


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------------------------
def _round_trip_inputs(tmp_path):
    rt = pc.ROUND_TRIP
    spec = pc.TRANSFER[rt["transfer"]]
    g = GOLD["layouts"][rt["layout"]]
    ply = pc.write_ply(os.path.join(str(tmp_path), "ckpt", "point_cloud.ply"), g["records"], pc.LAYOUTS[rt["layout"]]["props"])
    pc_dir = os.path.join(str(tmp_path), "pc")
    os.makedirs(pc_dir, exist_ok=True)
    np.save(os.path.join(pc_dir, "coord.npy"), pc.cloud(spec["cloud"]))
    for a, v in pc.cloud_assets(rt["transfer"], spec).items():
        np.save(os.path.join(pc_dir, a + ".npy"), v)
    feat = os.path.join(str(tmp_path), "langfeat.pth")
    torch.save((torch.from_numpy(GOLD["lang"]["features"]), torch.zeros(1)), feat)
    return ply, pc_dir, feat


def test_round_trip_into_dataset_and_chunking(tmp_path, capsys):
    from scenesplat_amd.pointcept_api import build_dataset, chunk_scene, preprocess_gs
    rt = pc.ROUND_TRIP
    g = GOLD["layouts"][rt["layout"]]
    ply, pc_dir, feat = _round_trip_inputs(tmp_path)
    root = os.path.join(str(tmp_path), "data")
    scene = os.path.join(root, "train", "scene0000_00")
    assert preprocess_gs(ply, scene, pc_dir=pc_dir, feat=feat) == [scene]
    assert sorted(os.listdir(scene)) == GOLD["files"]
    saved = {f[:-4]: np.load(os.path.join(scene, f)) for f in GOLD["files"]}
    assert_decode({a: saved[a] for a in ARRAYS}, g["records"], "round trip", recording=g["out"])
    for a, want in GOLD["transfer"][rt["transfer"]].items():
        assert_bytes(saved[a], want, a)
    assert_bytes(saved["lang_feat"], GOLD["lang"]["lang_feat"], "lang_feat")
    assert_bytes(saved["valid_feat_mask"], GOLD["lang"]["valid_feat_mask"], "valid_feat_mask")
    # a second run writes the same bytes
    again = os.path.join(str(tmp_path), "again")
    assert preprocess_gs(ply, again, pc_dir=pc_dir, feat=feat) == [again]
    for f in GOLD["files"]:
        with open(os.path.join(scene, f), "rb") as a, open(os.path.join(again, f), "rb") as b:
            assert a.read() == b.read(), f
    # the folder feeds the dataset ...
    ds = build_dataset(dict(type="GenericGSDataset", split="train", data_root=root))
    assert len(ds) == 1
    d = ds.get_data(0)
    assert d["name"] == "scene0000_00" and tuple(d["coord"].shape) == (len(g["records"]), 3) and d["coord"].is_cuda
    assert_bytes(d["coord"].cpu().numpy(), g["out"]["coord"], "dataset coord")
    assert d["segment"].cpu().numpy().tolist() == GOLD["transfer"][rt["transfer"]]["segment"].astype(np.int32).tolist()
    if hasattr(ds, "stager"):
        ds.stager.close()
    # ... and the chunker
    dirs = chunk_scene("scene0000_00", root, os.path.join(str(tmp_path), "chunks"), "train", None, chunk_range=(3, 3), chunk_stride=(3, 3),
                       chunk_minimum_size=1)
    assert len(dirs) >= 2
    assert sum(len(np.load(os.path.join(d, "coord.npy"))) for d in dirs) <= len(g["records"])
    assert sorted(os.listdir(dirs[0])) == GOLD["files"]
    # a row-count mismatch of the features is an error, not a skip
    np.save(os.path.join(str(tmp_path), "short.npy"), GOLD["lang"]["features"][:-1])
    with pytest.raises(ValueError, match="feature rows"):
        preprocess_gs(ply, os.path.join(str(tmp_path), "bad"), feat=os.path.join(str(tmp_path), "short.npy"))


def test_directory_mode_and_command_line(tmp_path, capsys):
    gp = _gp()
    src = pc.write_dir_tree(os.path.join(str(tmp_path), "in"))
    flat, deep = os.path.join(str(tmp_path), "flat"), os.path.join(str(tmp_path), "deep")
    written = gp.preprocess_gs(src, flat)
    assert pc.scene_dirs(flat) == GOLD["dirs"]["flat"] == sorted(os.path.relpath(d, flat) for d in written)
    assert "skipped, it could not be read" in capsys.readouterr().out                     # broken.ply is reported and skipped
    assert gp.main(["--input", src, "--output", deep, "--recursive"]) == 0
    assert pc.scene_dirs(deep) == GOLD["dirs"]["deep"]
    want = pc.decode_reference(pc.records(pc.DIR_CASE))
    got = np.load(os.path.join(deep, "sub", "deep", "d", "scale.npy"))
    assert got.shape == (pc.LAYOUTS[pc.DIR_CASE]["n"], 2) and pc.ulp_error(got, want["scale64"]).max() <= 1.0
    assert_bytes(np.load(os.path.join(deep, "sub", "c", "quat.npy")), want["quat"], "quat")
