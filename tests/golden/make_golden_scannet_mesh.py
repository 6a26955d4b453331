"""Generator of tests/golden/scannet_mesh.npz: the ScanNet converter against the reference's OWN
pointcept/datasets/preprocessing/scannet/preprocess_scannet.py and preprocess_scannet_gs.py.

    python tests/golden/make_golden_scannet_mesh.py <path of the reference tree>

Both scripts are imported by path.  `plyfile` and `open3d` are not installed: objects of this file stand in for them (`PlyData.read`
parses the header and views the vertex and face blocks through numpy structured dtypes, which is what plyfile does; open3d is only
imported, the oriented-box pruning is not recorded).  Only data is written.

For every case of tests/scannet_mesh_cases.py::MESHES: `read_plymesh`'s vertices[:, :3] (as float32), colours and faces, and
`vertex_normal` of each script (`<case>/coord|color|faces|normal_pc|normal_gs`; the F = 0 case goes around `np.stack`, which refuses an
empty list).  For the LABELLED cases the files the point-cloud script's `handle_process` writes for a train scene
(`<case>/pc/<asset>`), and for the GS cases what `sklearn.neighbors.KDTree(mesh).query(coord, k=1)` selects, the gathered normals and
the arrays of the GS script's label loop run with its own `point_indices_from_group` (`<case>/gs/nearest|normal|segment20|...`).
The label table: `tsv/cells` = the columns raw_category, id, nyu40id of the reference's tsv as the file holds them, followed by rows
added here (a repeated raw_category with other ids, and raw categories pandas reads as missing); `tsv/queries` and `tsv/pairs` = what
`point_indices_from_group` returns for every raw_category of that file and for a label it does not hold; `ids20`, `ids200` = the two
valid-id lists.

Asserted here, so that no test hides behind the fixture: every Gaussian's nearest and second-nearest squared distances differ by a
relative 1e-4 or more and the fp64 brute-force choice equals the KD-tree's; the PC and GS normals differ in at least one row; both
scripts map every label alike; the special inputs of the cases are present and behave as documented."""
import contextlib
import csv
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import scannet_mesh_cases as mc  # noqa: E402

NP_TYPES = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8"}
EXTRA_ROWS = [("chair", "777", "33"), ("NA", "3", "2"), ("null", "3", "2"), ("", "3", "2"), ("n/a", "5", "8")]


# ---- stand-ins for the imports the reference needs and this machine lacks --------------------------------------------------------------
class _Element:
    def __init__(self, data):
        self.data = data
        self.count = len(data)

    def __getitem__(self, name):
        return self.data[name]


class PlyData:
    def __init__(self, elements):
        self._elements = elements
        self.elements = list(elements.values())

    def __getitem__(self, name):
        return self._elements[name]

    @staticmethod
    def read(f):
        raw = f.read() if hasattr(f, "read") else open(f, "rb").read()
        end = raw.index(b"end_header")
        start = raw.index(b"\n", end) + 1
        lines = [ln.strip().split() for ln in raw[:end].decode("ascii").splitlines()]
        assert lines[0] == ["ply"] and ["format", "binary_little_endian", "1.0"] in lines
        elements, current = [], None
        for words in lines:
            if words and words[0] == "element":
                current = (words[1], int(words[2]), [])
                elements.append(current)
            elif words and words[0] == "property":
                if words[1] == "list":
                    assert words[2] == "uchar"
                    current[2].extend([("_count_" + words[4], "u1"), (words[4], "<" + NP_TYPES[words[3]], (3,))])
                else:
                    current[2].append((words[2], "<" + NP_TYPES[words[1]]))
        out = {}
        for name, count, fields in elements:
            data = np.frombuffer(raw, dtype=np.dtype(fields), count=count, offset=start)
            start += data.nbytes
            out[name] = _Element(data)
        return PlyData(out)


def install_stand_ins():
    plyfile = types.ModuleType("plyfile")
    plyfile.PlyData = PlyData
    sys.modules.setdefault("plyfile", plyfile)
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))


def reference_module(ref_root, name):
    folder = os.path.join(ref_root, "pointcept", "datasets", "preprocessing", "scannet")
    if folder not in sys.path:
        sys.path.insert(0, folder)                                       # `from meta_data.scannet200_constants import ...`
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, folder


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    import pandas as pd
    from sklearn.neighbors import KDTree

    ref_root = sys.argv[1]
    install_stand_ins()
    pc_ref, folder = reference_module(ref_root, "preprocess_scannet")
    gs_ref, _ = reference_module(ref_root, "preprocess_scannet_gs")
    arrays = {}

    with tempfile.TemporaryDirectory() as tmp:
        # ---- the label table -------------------------------------------------------------------------------------------------------------
        with open(os.path.join(folder, "meta_data", "scannetv2-labels.combined.tsv"), newline="", encoding="utf-8") as f:
            rows = list(csv.reader(f, delimiter="\t"))
        names = rows[0]
        col = [names.index(c) for c in ("raw_category", "id", "nyu40id")]
        cells = [tuple(r[c] for c in col) for r in rows[1:] if r] + EXTRA_ROWS
        tsv = mc.write_tsv(os.path.join(tmp, "labels.tsv"), cells)
        labels_pd = pd.read_csv(tsv, sep="\t", header=0)                 # as both scripts read it
        real_pd = pd.read_csv(os.path.join(folder, "meta_data", "scannetv2-labels.combined.tsv"), sep="\t", header=0)
        ids20, ids200 = list(pc_ref.CLASS_IDS20), list(pc_ref.CLASS_IDS200)
        queries = list(_distinct(c[0] for c in cells)) + [mc.ABSENT_LABEL]
        pairs = []
        for q in queries:
            group = dict(segments=[1], label=q)
            _, a20, a200 = pc_ref.point_indices_from_group(np.array([1]), group, labels_pd)
            _, b20, b200 = gs_ref.point_indices_from_group(np.array([1]), group, labels_pd)
            assert (a20, a200) == (b20, b200), q
            if q not in [e[0] for e in EXTRA_ROWS] and q != mc.ABSENT_LABEL:
                _, r20, r200 = pc_ref.point_indices_from_group(np.array([1]), group, real_pd)      # the rewritten file reads as the real one
                assert (a20, a200) == (r20, r200), q
            pairs.append((a20, a200))
        pairs = np.asarray(pairs, dtype=np.int64)
        by = dict(zip(queries, map(tuple, pairs)))
        assert by["NA"] == by["null"] == by[""] == by["n/a"] == by[mc.ABSENT_LABEL] == (-1, -1)
        assert by["chair"] == (ids20.index(5), ids200.index(2))         # the first row wins over the added one
        outside = [q for q in queries[:len(queries) - 1] if by[q] == (-1, -1) and q not in [e[0] for e in EXTRA_ROWS]]
        assert outside, "no label with ids outside both valid lists"
        outside_label = outside[0]
        categories = [c[0] for c in cells[:len(cells) - len(EXTRA_ROWS)]]
        arrays["tsv/cells"] = np.asarray(cells, dtype=str)
        arrays["tsv/queries"] = np.asarray(queries, dtype=str)
        arrays["tsv/pairs"] = pairs
        arrays["ids20"], arrays["ids200"] = np.asarray(ids20, dtype=np.int64), np.asarray(ids200, dtype=np.int64)
        arrays["outside_label"] = np.asarray(outside_label)
        print(f"label table: {len(cells)} rows, {len(queries)} queries, outside label '{outside_label}'")

        # ---- meshes ------------------------------------------------------------------------------------------------------------------------
        for case, spec in mc.MESHES.items():
            m = mc.mesh(case)
            scene_id = "scene_" + case
            with_labels = case in mc.LABELLED
            scene = mc.write_scene(os.path.join(tmp, case), scene_id, case, categories, outside_label, with_labels=with_labels)
            mesh_path = os.path.join(scene, f"{scene_id}_vh_clean_2.ply")
            if len(m["faces"]):
                vertices, faces = pc_ref.read_plymesh(mesh_path)
                v2, f2 = gs_ref.read_plymesh(mesh_path)
                assert same(vertices, v2) and same(faces, f2)
            else:                                                        # np.stack refuses the empty face list: around it
                import pandas
                with open(mesh_path, "rb") as f:
                    ply = PlyData.read(f)
                vertices, faces = pandas.DataFrame(ply["vertex"].data).values, np.zeros((0, 3), dtype=np.int32)
            assert vertices.dtype == np.float32, (case, vertices.dtype)  # so both scripts compute the normals in fp32
            coords = vertices[:, :3]
            arrays[f"{case}/coord"] = np.ascontiguousarray(coords.astype(np.float32))
            arrays[f"{case}/color"] = np.ascontiguousarray(vertices[:, 3:6].astype(np.uint8))
            arrays[f"{case}/faces"] = np.ascontiguousarray(faces).view(np.int32).reshape(-1, 3)
            assert same(arrays[f"{case}/coord"], m["coord"]) and same(arrays[f"{case}/color"], m["color"])
            assert (arrays[f"{case}/faces"] == m["faces"]).all()
            with np.errstate(all="ignore"):
                normal_pc = pc_ref.vertex_normal(coords, faces).astype(np.float32)
                normal_gs = gs_ref.vertex_normal(coords, faces)
            assert normal_pc.dtype == normal_gs.dtype == np.float32
            arrays[f"{case}/normal_pc"], arrays[f"{case}/normal_gs"] = normal_pc, normal_gs
            differ = int((normal_pc.view(np.uint32) != normal_gs.view(np.uint32)).any(1).sum())
            print(f"{case}: {len(coords)} vertices, {len(faces)} faces, stride {vertices.shape[1]} columns; PC and GS normals differ in {differ} rows")
            if len(faces) > 300:
                assert differ > 0, case
            sp = m["special"]
            if "lonely_vertex" in sp:
                assert not (m["faces"] == sp["lonely_vertex"]).any() and (normal_pc[sp["lonely_vertex"]] == 0).all()
                assert (m["faces"] == sp["one_face_vertex"]).sum() == 1
                assert (normal_pc[sp["collinear_vertex"]] == 0).all() and (normal_gs[sp["collinear_vertex"]] == 0).all()
                twice = ((m["faces"][:, 0] == m["faces"][:, 1]) | (m["faces"][:, 0] == m["faces"][:, 2])).sum()
                thrice = ((m["faces"][:, 0] == m["faces"][:, 1]) & (m["faces"][:, 0] == m["faces"][:, 2])).sum()
                assert twice >= 3 and thrice >= 1
                assert len(np.unique(np.sort(m["faces"], 1), axis=0)) < len(m["faces"])
            if "fan_vertex" in sp:
                assert (m["faces"] == sp["fan_vertex"]).any(1).sum() > 256
            if with_labels:
                out = os.path.join(tmp, case, "out")
                with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                    pc_ref.handle_process(scene, out, labels_pd, [scene_id], [], True)
                files = sorted(os.listdir(os.path.join(out, "train", scene_id)))
                assert files == sorted(a + ".npy" for a in ("coord", "color", "normal", "segment20", "segment200", "instance")), files
                for a in ("coord", "color", "normal", "segment20", "segment200", "instance"):
                    arrays[f"{case}/pc/{a}"] = np.load(os.path.join(out, "train", scene_id, a + ".npy"))
                assert same(arrays[f"{case}/pc/normal"], normal_pc) and same(arrays[f"{case}/pc/coord"], m["coord"])
                seg_indices, groups = mc.labels(case, categories, outside_label)
                s20 = arrays[f"{case}/pc/segment20"]
                assert s20.dtype == np.int64 and (s20 == -1).any() and (s20 >= 0).any() and len(groups) >= 40
                assert (arrays[f"{case}/pc/instance"] == 1234).any()
                shared = groups[3]["segments"][0]
                assert (arrays[f"{case}/pc/instance"][np.asarray(seg_indices) == shared] == groups[20]["id"]).all() and (np.asarray(seg_indices) == shared).any()
                out_test = os.path.join(tmp, case, "out_test")
                with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                    pc_ref.handle_process(scene, out_test, labels_pd, [], [], True)
                assert sorted(os.listdir(os.path.join(out_test, "test", scene_id))) == ["color.npy", "coord.npy", "normal.npy"]

            if case in mc.GS_CASES:
                gs = mc.gaussians(case)
                coord_gs = np.stack([gs["x"], gs["y"], gs["z"]], -1).astype(np.float32)
                _, nn_idx = KDTree(coords).query(coord_gs, k=1)
                nn_idx = nn_idx[:, 0]
                brute, gap = mc.two_nearest(coord_gs, coords)
                assert gap.min() >= 1e-4, (case, gap.min())
                assert (brute == nn_idx).all(), case
                seg_indices = np.array(seg_indices)
                seg_gs = seg_indices[nn_idx]
                s20, s200, inst = (np.full(len(gs), -1, dtype=np.int16) for _ in range(3))
                for group in groups:                                    # the loop of the GS script's handle_process
                    group_segments, l20, l200 = gs_ref.point_indices_from_group(seg_indices, group, labels_pd)
                    mask = np.isin(seg_gs, group_segments)
                    s20[mask], s200[mask], inst[mask] = l20, l200, group["id"]
                arrays[f"{case}/gs/nearest"] = nn_idx.astype(np.int64)
                arrays[f"{case}/gs/normal"] = normal_gs[nn_idx, :]
                arrays[f"{case}/gs/segment20"], arrays[f"{case}/gs/segment200"], arrays[f"{case}/gs/instance"] = s20, s200, inst
                feats = mc.features(case)
                import torch
                f16 = torch.from_numpy(feats).to(torch.float16).numpy()
                arrays[f"{case}/gs/lang_feat"] = f16
                arrays[f"{case}/gs/valid_feat_mask"] = np.any(f16 != 0.0, axis=1).astype(int)
                print(f"{case}: {len(gs)} Gaussians, smallest relative gap {gap.min():.2e}, {len(np.unique(nn_idx))} distinct vertices")

    arrays = {k: np.ascontiguousarray(v) if v.ndim else v for k, v in arrays.items()}   # (DataFrame.values is column-major; the bytes compared are row-major)
    np.savez_compressed(mc.GOLDEN, **arrays)
    print(f"{mc.GOLDEN}: {os.path.getsize(mc.GOLDEN)} bytes")


def _distinct(items):
    seen = {}
    for i in items:
        seen.setdefault(i, None)
    return seen.keys()


if __name__ == "__main__":
    main()
