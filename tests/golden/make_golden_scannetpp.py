"""Generator of tests/golden/scannetpp.npz: the ScanNet++ converter against the reference's OWN
pointcept/datasets/preprocessing/scannetpp/preprocess_scannetpp.py, and of tests/golden/scannetpp_top100.txt, a copy of the class list
`metadata/semantic_benchmark/top100.txt` beside that script (a list of names).

    python tests/golden/make_golden_scannetpp.py <path of the reference tree>

`preprocess_scannetpp.py` is imported by path and its `parse_scene` is run on every case.  `open3d` is not installed: an object of this
file stands in for it.  `read_triangle_mesh` parses the .ply as Open3D does (vertices as doubles, colours as c / 255.0), and
`compute_vertex_normals(normalized=True)` is tests/scannetpp_cases.py::normals_o3d_restated, an fp64 numpy restatement of the
definition Open3D implements (unnormalised face cross products added per vertex in face order, once per corner; a division by the norm
where it is above zero).  THE RECORDED NORMALS ARE THEREFORE HELD TO THAT STATED DEFINITION, NOT TO OPEN3D'S BINARY.  The label arrays
are what the reference's own loop wrote, byte for byte.  Only data is written.

Recorded: `classes` (the names as the reference's np.loadtxt call reads them); per mesh case `<case>/normal` (coord, color and faces
are those of the case, asserted equal to what `parse_scene` wrote); per annotation case `<anno>/segment`, `<anno>/instance` ((n, 3)
int16, from a train scene); per GS case what `sklearn.neighbors.KDTree(pc_coord).query(coord, k=1)` selects and the rows of the
reference-written normal / segment / instance it gathers, `lang_feat` and `valid_feat_mask` as preprocess_scannetpp_gs.py makes them.
That script needs plyfile, h5py and open3d's oriented box; its `read_gaussian_attribute` is imported (with stand-ins) only to count how
many quaternion and colour values differ from the fp32 decode this package shares with the other converters (printed; quoted in
profiles/scannetpp.md).

Asserted here, so that no test hides behind the fixture: `(c / 255.0 * 255).astype(uint8)` gives every byte value back; both ScanNet
normal forms differ from the new definition in at least one row of every case with faces, and the fp32 walk of the new definition
differs at the `cancel` vertex; every annotation case listed at scannetpp_cases.annotation is present and behaves as documented; every
Gaussian's nearest and second-nearest squared distances differ by a relative 1e-4 or more and the fp64 brute-force choice equals the
KD-tree's; a test scene gets no label files."""
import contextlib
import io
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ply_cases  # noqa: E402
import scannet_mesh_cases as mc  # noqa: E402
import scannetpp_cases as sc  # noqa: E402
from make_golden_scannet_mesh import PlyData, same  # noqa: E402  (the plyfile stand-in)


# ---- the stand-in for open3d -----------------------------------------------------------------------------------------------------------
class _TriangleMesh:
    def __init__(self, vertices, colors, triangles):
        self.vertices, self.vertex_colors, self.triangles, self.vertex_normals = vertices, colors, triangles, None

    def compute_vertex_normals(self, normalized=True):
        assert normalized
        self.vertex_normals = sc.normals_o3d_restated(self.vertices.astype(np.float32), self.triangles).astype(np.float64)


def _read_triangle_mesh(path):
    ply = PlyData.read(path)
    v = ply["vertex"].data
    vertices = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64)
    colors = np.stack([v["red"], v["green"], v["blue"]], 1) / 255.0
    return _TriangleMesh(vertices, colors, np.asarray(ply["face"].data["vertex_indices"]).astype(np.int64).reshape(-1, 3))


class _Vertex:
    """what read_gaussian_attribute asks of a plyfile element"""

    def __init__(self, arr):
        self.arr = arr
        self.properties = [types.SimpleNamespace(name=n) for n in arr.dtype.names]

    def __getitem__(self, name):
        return self.arr[name]


def install_stand_ins():
    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(read_triangle_mesh=_read_triangle_mesh)
    sys.modules["open3d"] = o3d
    plyfile = types.ModuleType("plyfile")
    plyfile.PlyData = PlyData
    sys.modules.setdefault("plyfile", plyfile)
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))


def reference_module(ref_root, name):
    folder = os.path.join(ref_root, "pointcept", "datasets", "preprocessing", "scannetpp")
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, folder


def _parse(ref, root, out, name, split, label_mapping, class2idx):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        ref.parse_scene(name, split, root, out, label_mapping, class2idx, -1)
    d = os.path.join(out, split, name)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def check_annotation(case, seg_indices, groups, class2idx, segment, instance):
    """the cases scannetpp_cases.annotation promises, read off the reference's arrays"""
    seg, ids = np.asarray(seg_indices), sc.segment_ids(case)
    rows = lambda name: segment[seg == ids[name]]
    labels = lambda name: (rows(name) >= 0).sum(1)
    valid = [class2idx.get(g["label"], -1) != -1 for g in groups]
    in_valid = lambda name: sum(ids[name] in g["segments"] for g, ok in zip(groups, valid) if ok)
    assert 55 <= len(groups) <= 70 and not all(valid)
    for name, k in (("none", 0), ("one", 1), ("two", 2), ("three", 3), ("five", 5), ("ignored_between", 2), ("repeated", 2), ("beyond", 0)):
        assert in_valid(name) == k and len(rows(name)) and (labels(name) == min(k, 3)).all(), (case, name)
    between = [k for k, g in enumerate(groups) if ids["ignored_between"] in g["segments"]]
    assert [valid[k] for k in between] == [True, False, True]
    assert any(g["segments"].count(ids["repeated"]) == 2 for g in groups)
    assert not (seg == ids["absent"]).any() and any(ids["absent"] in g["segments"] and len(g["segments"]) > 1 for g in groups)
    assert any(g["segments"] == [ids["absent_alone"]] for g in groups)
    assert ids["beyond"] > max(max(g["segments"]) for g in groups)
    # `full`: the fourth group of `five` lists nothing else, so its objectId reaches no row
    full = [g for g in groups if g["segments"] == [ids["five"]]][2]
    assert not (instance == full["objectId"]).any()
    obj = lambda name, k: [g["objectId"] for g, ok in zip(groups, valid) if ok and ids[name] in g["segments"]][k]
    inst = lambda name: instance[seg == ids[name]]
    # equal sizes: the first wins.  tie: slots 0 and 1 equal, no swap; tie_later: slots 1 and 2 equal and smaller, slot 1 goes first
    assert (inst("tie") == [obj("tie", 0), obj("tie", 1), -1]).all()
    assert (inst("tie_later") == [obj("tie_later", 1), obj("tie_later", 0), obj("tie_later", 2)]).all()
    assert (inst("repeated") == [obj("repeated", 0), obj("repeated", 1), -1]).all()     # a repeat counted twice would swap
    assert (inst("pos0") == [obj("pos0", 0), obj("pos0", 1), -1]).all()
    assert (inst("pos1") == [obj("pos1", 1), obj("pos1", 0), -1]).all()
    assert (inst("pos2") == [obj("pos2", 2), obj("pos2", 1), obj("pos2", 0)]).all()
    # naive: its second group also lists `five`, whose vertices had no free slot left: counted, they would keep column 0
    assert (inst("naive") == [obj("naive", 1), obj("naive", 0), -1]).all()
    mate, n_naive, n_five = (seg == ids["naive_mate"]).sum(), (seg == ids["naive"]).sum(), (seg == ids["five"]).sum()
    assert n_naive < n_naive + mate < n_naive + n_five
    if case == "rich":
        assert (seg == ids["big"]).sum() > 1024
    assert (instance[:, 0] >= 0).sum() > 0 and (segment[:, 2] >= 0).any() and (segment == -1).all(1).any()


def main():
    import pandas as pd
    from sklearn.neighbors import KDTree
    import torch

    ref_root = sys.argv[1]
    install_stand_ins()
    ref, folder = reference_module(ref_root, "preprocess_scannetpp")
    gs_ref, _ = reference_module(ref_root, "preprocess_scannetpp_gs")
    shutil.copyfile(os.path.join(folder, "metadata", "semantic_benchmark", "top100.txt"), sc.TOP100)
    names = np.loadtxt(sc.TOP100, dtype=str, delimiter=".")              # the reference's call
    class2idx = {class_name: idx for (idx, class_name) in enumerate(names)}
    label_mapping = ref.filter_map_classes(pd.read_csv(os.path.join(folder, "metadata", "semantic_benchmark", "map_benchmark.csv")),
                                           count_thresh=0, count_type="count", mapping_type="semantic")
    assert len(names) == 100 and sc.IGNORED_LABEL not in class2idx and any(" " in n for n in names)
    every = np.arange(256, dtype=np.uint8)
    assert ((every / 255.0 * 255).astype(np.uint8) == every).all()      # Open3D's colours give the file's bytes back
    arrays = {"classes": np.asarray(names, dtype=str)}
    written = {}

    with tempfile.TemporaryDirectory() as tmp:
        root, out = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        # ---- meshes: each as a test scene, and as a train scene where an annotation goes with it -----------------------------------------
        for case in sc.MESHES:
            m = sc.mesh(case)
            sc.write_scans(root, "mesh_" + case, "test", case)
            got = _parse(ref, root, out, "mesh_" + case, "test", label_mapping, class2idx)
            assert sorted(got) == ["color", "coord", "normal"], (case, sorted(got))       # a test scene gets no label files
            assert same(got["coord"], m["coord"]) and same(got["color"], m["color"]) and got["normal"].dtype == np.float32
            arrays[f"{case}/normal"] = got["normal"]
            differ32 = 0
            if len(m["faces"]):
                for form in ("pc", "gs"):
                    old = mc.normals_restated(m["coord"], m["faces"], form)
                    assert (old.view(np.uint32) != got["normal"].view(np.uint32)).any(), (case, form)
                walk32 = sc.normals_o3d_restated(m["coord"], m["faces"], np.float32)
                differ32 = int((walk32.view(np.uint32) != got["normal"].view(np.uint32)).any(1).sum())
            sp = m["special"]
            if "lonely_vertex" in sp:
                assert (got["normal"][sp["lonely_vertex"]] == 0).all() and (got["normal"][sp["collinear_vertex"]] == 0).all()
            if "cancel_vertex" in sp:
                v = sp["cancel_vertex"]
                assert (walk32[v].view(np.uint32) != got["normal"][v].view(np.uint32)).any()
                print(f"cancel vertex: fp64 {got['normal'][v]}, fp32 walk {walk32[v]}")
            print(f"{case}: {len(m['coord'])} vertices, {len(m['faces'])} faces; an fp32 walk differs in {differ32} rows")
            written[case] = got

        # ---- annotations -----------------------------------------------------------------------------------------------------------------
        for case in sc.ANNOS:
            n = sc.anno_vertices(case)
            name = "anno_" + case
            seg_indices, groups = sc.annotation(case, names)
            if case in sc.MESHES:
                sc.write_scans(root, name, "train", case, anno_case=case)
            else:                                                        # vertices alone: the label loop does not look at the mesh
                rng = np.random.default_rng(5)
                arr = sc.vertex_records(dict(coord=rng.uniform(0, 8, (n, 3)).astype(np.float32), color=rng.integers(0, 256, (n, 3))))
                d = sc.write_scans(root, name, "train", "single", anno_case=case)
                mc.write_file(os.path.join(d, "mesh_aligned_0.05.ply"), mc.header_bytes(n, 0, sc.SPP_PROPS) + arr.tobytes())
            got = _parse(ref, root, out, name, "train", label_mapping, class2idx)
            assert sorted(got) == ["color", "coord", "instance", "normal", "segment"]
            for a in ("segment", "instance"):
                assert got[a].dtype == np.int16 and got[a].shape == (n, 3)
                arrays[f"{case}/{a}"] = got[a]
            if groups:
                check_annotation(case, seg_indices, groups, class2idx, got["segment"], got["instance"])
            else:
                assert (got["segment"] == -1).all() and (got["instance"] == -1).all()
            if case in sc.MESHES:
                assert same(got["normal"], arrays[f"{case}/normal"])
            written["anno_" + case] = got
            print(f"{case}: {n} vertices, {len(groups)} groups, rows with 0/1/2/3 labels: "
                  f"{[int(((got['segment'] >= 0).sum(1) == k).sum()) for k in range(4)]}")

        # ---- Gaussians -------------------------------------------------------------------------------------------------------------------
        diff_quat = diff_color = total = far = 0
        for case in sc.GS_CASES:
            gs = sc.gaussians(case)
            pc = written["anno_" + case] if "anno_" + case in written else written[case]
            coord = np.stack([gs["x"], gs["y"], gs["z"]], -1).astype(np.float32)
            _, nn_idx = KDTree(pc["coord"]).query(coord, k=1)
            nn_idx = nn_idx[:, 0]
            brute, gap = mc.two_nearest(coord, pc["coord"])
            assert gap.min() >= 1e-4 and (brute == nn_idx).all(), (case, gap.min())
            arrays[f"{case}/gs/nearest"] = nn_idx.astype(np.int64)
            arrays[f"{case}/gs/normal"] = pc["normal"][nn_idx[:, None]][:, 0]
            if "segment" in pc:
                arrays[f"{case}/gs/segment"] = pc["segment"][nn_idx[:, None]][:, 0]
                arrays[f"{case}/gs/instance"] = pc["instance"][nn_idx[:, None]][:, 0]
            f16 = torch.from_numpy(sc.features(case)).to(torch.float16).numpy()
            valid = np.any(f16 != 0.0, axis=1).astype(int)
            arrays[f"{case}/gs/lang_feat"], arrays[f"{case}/gs/valid_feat_mask"] = f16, valid
            arrays[f"{case}/gs/too_few"] = np.asarray(bool(valid.sum() / valid.size < 0.5))
            with np.errstate(all="ignore"):
                theirs = gs_ref.read_gaussian_attribute(_Vertex(gs))
            ours = ply_cases.decode_reference(gs)
            diff_quat += int((theirs["quat"].astype(np.float32) != ours["quat"]).sum())
            far = max(far, int(np.abs(theirs["quat"].astype(np.float32).view(np.int32).astype(np.int64) - ours["quat"].view(np.int32)).max()))
            diff_color += int((theirs["color"].astype(np.uint8) != ours["color"]).sum())
            total += len(gs)
            assert same(theirs["coord"].astype(np.float32), ours["coord"])
            print(f"{case}: {len(gs)} Gaussians, smallest relative gap {gap.min():.2e}, {len(np.unique(nn_idx))} distinct vertices, "
                  f"valid features {valid.mean():.2f}")
        assert bool(arrays["extra/gs/too_few"]) and not bool(arrays["scan/gs/too_few"])
        print(f"checkpoint decode against preprocess_scannetpp_gs.py over {total} Gaussians: {diff_quat} of {4 * total} quaternion values (by at most "
              f"{far} fp32 steps) and {diff_color} of {3 * total} colour bytes differ")

    arrays = {k: np.ascontiguousarray(v) if v.ndim else v for k, v in arrays.items()}
    np.savez_compressed(sc.GOLDEN, **arrays)
    print(f"{sc.GOLDEN}: {os.path.getsize(sc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
