"""Generator of tests/golden/gaussian_ply.npz: the 3DGS checkpoint reader against the reference's OWN scripts/preprocess_gs.py.

    python tests/golden/make_golden_gaussian_ply.py <path of the reference tree>

For every case of tests/ply_cases.py::LAYOUTS the record array is written as a .ply into a temporary folder, the reference's
scripts/preprocess_gs.py (imported by path) reads it with `read_gaussian_attributes` and writes it with `process_ply_file`, and the
file records the input records (as bytes) and the five arrays.  `plyfile` is not installed (nor `open3d` / `h5py`, which the HoliCity
script imports): objects of this file stand in for it and for `tqdm` (`PlyData.read` parses the header and views the vertex block
through a numpy structured dtype, which is what plyfile does).
For the TRANSFER cases it records what `sklearn.neighbors.KDTree(pc_coord).query(coord, k=1)` selects, the call of
pointcept/datasets/preprocessing/holicity/preprocess_holicity_gs.py, applied to the cloud's assets with that script's squeeze; for the
round trip the `lang_feat` / `valid_feat_mask` pair by that script's two statements.  The output-directory rule is recorded by running
the reference's command line (single file, directory, --recursive) over tests/ply_cases.py::DIR_TREE.  Only data is written.

Keys: `index` (JSON), `<layout>/records` (n, stride) uint8, `<layout>/out/<asset>`, `<transfer>/gs/<asset>`, `lang/features`,
`lang/lang_feat`, `lang/valid_feat_mask`.

Asserted here, so that no test hides behind it: process_ply_file's files equal read_gaussian_attributes' arrays; no NaN in f_dc; in
every transfer case the squared distances to the nearest and second-nearest cloud point differ by a relative 1e-4 or more for every
Gaussian, and the fp64 brute-force choice equals the KD-tree's; the special rows (rot_0 == 0, zero quaternion, negative rot_0, both
clip bounds) are in the inputs and behave as documented.  It prints E, the recording's largest distance from the fp64 value of
exp / the sigmoid: the figure quoted in profiles/ply_ingest.md."""
import contextlib
import importlib.util
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ply_cases as pc  # noqa: E402


# ---- stand-ins for the imports the reference needs and this machine lacks --------------------------------------------------------------
class _Property:
    def __init__(self, name):
        self.name = name


class _Element:
    def __init__(self, data):
        self.data = data
        self.properties = [_Property(n) for n in data.dtype.names]

    def __getitem__(self, name):
        return self.data[name]


class PlyData:
    def __init__(self, elements):
        self.elements = elements

    def __getitem__(self, name):
        return self.elements[name]

    @staticmethod
    def read(path):
        with open(path, "rb") as f:
            raw = f.read()
        end = raw.index(b"end_header")
        start = raw.index(b"\n", end) + 1
        lines = [ln.strip().split() for ln in raw[:end].decode("ascii").splitlines()]
        if lines[0] != ["ply"] or ["format", "binary_little_endian", "1.0"] not in lines:
            raise ValueError("not a binary little-endian PLY")
        fields, count, element = [], None, None
        for words in lines:
            if words and words[0] == "element":
                element = words[1]
                if element == "vertex":
                    count = int(words[2])
            elif words and words[0] == "property" and element == "vertex":
                fields.append((words[2], "<" + pc.NP_TYPES[words[1]]))
        return PlyData({"vertex": _Element(np.frombuffer(raw, dtype=np.dtype(fields), count=count, offset=start))})


def install_stand_ins():
    plyfile = types.ModuleType("plyfile")
    plyfile.PlyData = PlyData
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, *a, **k: it
    sys.modules.setdefault("plyfile", plyfile)
    sys.modules.setdefault("tqdm", tqdm)


def reference_path(ref_root):
    return os.path.join(ref_root, "scripts", "preprocess_gs.py")


def reference_module(ref_root):
    spec = importlib.util.spec_from_file_location("ref_preprocess_gs", reference_path(ref_root))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_command_line(ref_root, argv):
    old = sys.argv
    sys.argv = [reference_path(ref_root)] + argv
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            runpy.run_path(reference_path(ref_root), run_name="__main__")
    finally:
        sys.argv = old


def main():
    from sklearn.neighbors import KDTree
    import torch

    ref_root = sys.argv[1]
    install_stand_ins()
    ref = reference_module(ref_root)
    arrays, index = {}, dict(layouts=[], transfer={}, files=None, dirs={})
    worst = dict(scale=0.0, opacity=0.0)
    differ = dict(scale=[0, 0], opacity=[0, 0])
    outs, recs = {}, {}
    for case, spec in pc.LAYOUTS.items():
        arr = pc.records(case)
        recs[case] = arr
        for a in range(3):
            assert not np.isnan(arr[f"f_dc_{a}"]).any(), case
        with tempfile.TemporaryDirectory() as tmp:
            path = pc.write_ply(os.path.join(tmp, "point_cloud.ply"), arr, spec["props"], comments=("made for the fixture",))
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                got = ref.read_gaussian_attributes(ref.IO.get(path)["vertex"])
                assert ref.process_ply_file(path, os.path.join(tmp, "out")) is True
            files = sorted(os.listdir(os.path.join(tmp, "out")))
            assert files == sorted(a + ".npy" for a in got), files
            for a in got:
                saved = np.load(os.path.join(tmp, "out", a + ".npy"))
                assert saved.dtype == got[a].dtype and saved.shape == got[a].shape and saved.tobytes() == got[a].tobytes(), (case, a)
        mine = pc.decode_reference(arr)
        for a in ("coord", "color", "quat"):
            assert got[a].dtype == mine[a].dtype and got[a].shape == mine[a].shape and got[a].tobytes() == mine[a].tobytes(), (case, a)
        for a in ("scale", "opacity"):
            err = pc.ulp_error(got[a], mine[a + "64"])
            worst[a] = max(worst[a], float(err.max()))
            differ[a][0] += int((got[a] != mine[a]).sum())
            differ[a][1] += got[a].size
        # the special rows
        assert (got["quat"][0] == 0).all() and (arr["rot_1"][0] != 0), case
        assert (got["quat"][1] == 0).all(), case
        assert got["quat"][2, 0] > 0 and arr["rot_0"][2] < 0, case
        assert got["color"][3].tolist() == [0, 255, 127], (case, got["color"][3])
        assert (got["color"] == 0).any() and (got["color"] == 255).any(), case
        outs[case] = got
        arrays[f"{case}/records"] = np.ascontiguousarray(arr).view(np.uint8).reshape(len(arr), arr.dtype.itemsize)
        for a, v in got.items():
            arrays[f"{case}/out/{a}"] = v
        index["layouts"].append(case)
        print(f"{case}: {len(arr)} records of {arr.dtype.itemsize} bytes, scale {got['scale'].shape}, quat {got['quat'].shape}")

    for case, spec in pc.TRANSFER.items():
        coord = outs[spec["layout"]]["coord"]
        cloud = pc.cloud(spec["cloud"])
        assets = pc.cloud_assets(case, spec)
        _, indices = KDTree(cloud).query(coord, k=1)
        brute, gap = pc.two_nearest(coord, cloud)
        assert gap.min() >= 1e-4, (case, gap.min())
        assert (brute == indices[:, 0]).all(), case
        assert len(np.unique(indices[:, 0])) > len(coord) // 4, case
        index["transfer"][case] = list(assets)
        for a, v in assets.items():
            if a == "segment" and v.ndim == 2 and v.shape[1] == 1:
                v = v.squeeze(1)
            arrays[f"{case}/gs/{a}"] = v[indices[:, 0]]
        print(f"{case}: cloud of {len(cloud)} points, smallest relative gap {gap.min():.2e}")

    rt = pc.ROUND_TRIP
    n = pc.LAYOUTS[rt["layout"]]["n"]
    rng = np.random.default_rng(rt["feat_seed"])
    features = rng.standard_normal((n, rt["feat_width"])).astype(np.float32)
    features[rng.random(n) < 0.3] = 0
    features[5] = 0
    features[6] = 0
    features[6, 3] = 1e-9                                                # non-zero in fp32, zero in fp16: the mask is taken after the cast
    gs_feat_np = torch.from_numpy(features).to(torch.float16).numpy()
    valid_feat_mask = np.any(gs_feat_np != 0.0, axis=1).astype(int)
    assert valid_feat_mask[6] == 0 and 0 < valid_feat_mask.sum() < n
    arrays["lang/features"], arrays["lang/lang_feat"], arrays["lang/valid_feat_mask"] = features, gs_feat_np, valid_feat_mask
    index["files"] = sorted([a + ".npy" for a in ("coord", "color", "opacity", "scale", "quat", "lang_feat", "valid_feat_mask")]
                            + [a + ".npy" for a in pc.TRANSFER[rt["transfer"]]["assets"]])

    with tempfile.TemporaryDirectory() as tmp:
        src = pc.write_dir_tree(os.path.join(tmp, "in"))
        with np.errstate(all="ignore"):
            run_command_line(ref_root, ["--input", os.path.join(src, "a.ply"), "--output", os.path.join(tmp, "single")])
            run_command_line(ref_root, ["--input", src, "--output", os.path.join(tmp, "flat")])
            run_command_line(ref_root, ["--input", src, "--output", os.path.join(tmp, "deep"), "--recursive"])
        for mode in ("single", "flat", "deep"):
            index["dirs"][mode] = pc.scene_dirs(os.path.join(tmp, mode))
    assert index["dirs"] == dict(single=["."], flat=["a", "b"], deep=["a", "b", "sub/c", "sub/deep/d"]), index["dirs"]

    arrays["index"] = np.asarray(json.dumps(index))
    np.savez_compressed(pc.GOLDEN, **arrays)
    print(f"{pc.GOLDEN}: {os.path.getsize(pc.GOLDEN)} bytes")
    for a in ("scale", "opacity"):
        print(f"numpy fp32 {a} vs fp64 rounded once: E = {worst[a]:.3f} fp32 ulp, {100 * differ[a][0] / differ[a][1]:.1f} % of the values differ")


if __name__ == "__main__":
    main()
