"""Inputs shared by tests/test_scannet_mesh_host.py (CPU), tests/test_hip_scannet_mesh.py (GPU) and
tests/golden/make_golden_scannet_mesh.py (the fixture generator) for the ScanNet converter
(scenesplat_amd/pointcept_api/scannet_mesh.py, csrc/mesh.hip).  Nothing here touches the library under test.

Meshes: jittered 2 cm lattices at an origin inside 0..8 m (edges of 1 to 3 cm, so the `1e-8` terms of the reference matter in fp32 as they
do on a real scan), plus the special inputs listed at `mesh`.  The face order is shuffled: the order of the additions is part of the
result.  Labels: sparse segment ids over lattice patches, the groups drawn from the categories handed in (the recorded tsv column)."""
import json
import os
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scannet_mesh.npz")
SCANNET_PROPS = [("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar"), ("alpha", "uchar")]
EXTRA_PROPS = [("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar"), ("alpha", "uchar"),
               ("quality", "float"), ("flag", "uchar")]                  # 21 bytes: the face block of n records starts at n mod 4; the
                                                                         # extras follow the colours, which the reference takes by column
NP_TYPES = {"float": "f4", "uchar": "u1", "int": "i4", "uint": "u4"}
ROWS_PER_WORKGROUP = 256                                                 # the decode kernels' tile (asserted against the library on the GPU)

# name -> lattice (rows, cols), seed, props, index type, extras: fan (faces around one vertex), specials
MESHES = OrderedDict([
    ("scan", dict(grid=(30, 40), seed=11, props=SCANNET_PROPS, index="int", fan=300, specials=True)),
    ("extra", dict(grid=(15, 20), seed=12, props=EXTRA_PROPS, index="uint", fan=0, specials=True)),
    ("n257", dict(grid=(2, 128), seed=13, props=SCANNET_PROPS, index="int", fan=0, specials=False)),      # + 1 vertex: n = 257, F = 256
    ("single", dict(grid=None, seed=14, props=SCANNET_PROPS, index="int", fan=0, specials=False)),         # n = 1, F = 0
])
LABELLED = ("scan", "extra")                                             # the cases with segment and aggregation files
GS_CASES = OrderedDict([("scan", dict(n=700, seed=31)), ("extra", dict(n=300, seed=32))])
MIN_GAP = 1e-3             # relative gap of the squared distances nearest / second nearest vertex (the maker asserts 1e-4)
ABSENT_LABEL = "a label no table holds"
SCENES = OrderedDict([("scene0000_00", "scan"), ("scene0001_00", "extra")])   # the end-to-end tree: the first is a train scene, the second in no list


def mesh(case):
    """-> dict(coord (n, 3) f32, color (n, 3) u8, faces (F, 3) int64, special {name: row or face number}).  With `specials`: a vertex in
    no face, a triangle of vertices in one face each, a face naming a vertex twice, one naming it three times, three distinct collinear
    vertices, a duplicated face; with `fan`: that many faces around one vertex."""
    spec = MESHES[case]
    rng = np.random.default_rng(spec["seed"])
    origin = rng.uniform(0.5, 7.0, 3)
    special = {}
    if spec["grid"] is None:
        coord = origin[None, :].astype(np.float32)
        return dict(coord=coord, color=rng.integers(0, 256, (1, 3)).astype(np.uint8), faces=np.zeros((0, 3), dtype=np.int64), special=special)
    rows, cols = spec["grid"]
    gy, gx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    pts = np.stack([gx.reshape(-1) * 0.02, gy.reshape(-1) * 0.02, np.zeros(rows * cols)], 1)
    pts = pts + rng.uniform(-0.004, 0.004, pts.shape) + origin
    vid = lambda r, c: r * cols + c
    faces = []
    for r in range(rows - 1):
        for c in range(cols - 1):
            faces.append((vid(r, c), vid(r, c + 1), vid(r + 1, c)))
            faces.append((vid(r + 1, c), vid(r, c + 1), vid(r + 1, c + 1)))
    pts = list(pts)

    def add(p):
        pts.append(np.asarray(p, dtype=np.float64))
        return len(pts) - 1

    if case == "n257":
        extra = add(pts[cols - 1] + np.array([0.02, 0.003, 0.001]))
        faces.append((vid(0, cols - 1), extra, vid(1, cols - 1)))
        faces.append((vid(0, cols - 2), extra, vid(0, cols - 1)))
    if spec["fan"]:
        centre = origin + np.array([0.4, 0.9, 0.2])
        c = add(centre)
        special["fan_vertex"] = c
        shell = []
        for _ in range(40):
            d = rng.standard_normal(3)
            shell.append(add(centre + d / np.linalg.norm(d) * rng.uniform(0.015, 0.03)))
        made = 0
        while made < spec["fan"]:
            i, j = rng.choice(40, 2, replace=False)
            if 0.01 <= np.linalg.norm(pts[shell[i]] - pts[shell[j]]) <= 0.03:
                faces.append((c, shell[i], shell[j]))
                made += 1
    if spec["specials"]:
        base = origin + np.array([0.1, 0.8, 0.3])
        special["lonely_vertex"] = add(base)
        tri = [add(base + np.array(o)) for o in ((0.1, 0.0, 0.0), (0.12, 0.001, 0.0), (0.1, 0.02, 0.003))]
        special["one_face_vertex"] = tri[0]
        faces.append(tuple(tri))
        faces.append((vid(2, 2), vid(2, 2), vid(2, 3)))                  # names a vertex twice
        faces.append((vid(3, 3), vid(3, 3), vid(3, 3)))                  # ... three times
        faces.append((vid(4, 1), vid(4, 2), vid(4, 1)))                  # twice, first and last corner
        p = np.array([1.0, 2.0, 0.5]) + np.floor(origin)                 # exactly representable: collinear in fp32 as well
        line = [add(p + k * np.array([0.015625, 0.0, 0.0])) for k in range(3)]
        special["collinear_vertex"] = line[1]
        faces.append(tuple(line))
        faces.append(faces[7])                                           # a duplicated face
    faces = np.asarray(faces, dtype=np.int64)
    faces = faces[rng.permutation(len(faces))]
    coord = np.asarray(pts).astype(np.float32)
    return dict(coord=coord, color=rng.integers(0, 256, (len(coord), 3)).astype(np.uint8), faces=faces, special=special)


def vertex_records(case, m=None):
    """the structured vertex array of a case (every extra column holds its column number)"""
    m = mesh(case) if m is None else m
    props = MESHES[case]["props"]
    arr = np.zeros(len(m["coord"]), dtype=np.dtype([(name, "<" + NP_TYPES[t]) for name, t in props]))
    for col, (name, _) in enumerate(props):
        arr[name] = col
    for a, name in enumerate("xyz"):
        arr[name] = m["coord"][:, a]
    for a, name in enumerate(("red", "green", "blue")):
        arr[name] = m["color"][:, a]
    return arr


def face_bytes(faces, index="int", counts=None):
    """the face block: per face a uchar count and the indices"""
    faces = np.asarray(faces)
    rec = np.zeros(len(faces), dtype=np.dtype([("count", "u1"), ("vertex_indices", "<" + NP_TYPES[index], (3,))]))
    rec["count"] = 3 if counts is None else counts
    rec["vertex_indices"] = faces.astype(np.int64).astype("<" + NP_TYPES[index], casting="unsafe") if len(faces) else faces.reshape(0, 3)
    return rec.tobytes()


def header_bytes(n, n_faces, props, index="int", pad=0, fmt="binary_little_endian 1.0", face_property=None, vertex_extra=()):
    """pad: the length of a comment line's text, which moves every block by that many bytes + 9"""
    lines = ["ply", f"format {fmt}"]
    if pad:
        lines.append("comment " + "p" * pad)
    lines += [f"element vertex {n}"] + [f"property {t} {name}" for name, t in props] + list(vertex_extra)
    lines += [f"element face {n_faces}", face_property or f"property list uchar {index} vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def ply_bytes(case, pad=0, m=None):
    m = mesh(case) if m is None else m
    spec = MESHES[case]
    return (header_bytes(len(m["coord"]), len(m["faces"]), spec["props"], spec["index"], pad) + vertex_records(case, m).tobytes()
            + face_bytes(m["faces"], spec["index"]))


def pads_for_alignments(case):
    """four comment lengths that put the face block at file offsets 0, 1, 2, 3 mod 4"""
    m = mesh(case)
    found = {}
    for pad in range(1, 16):
        spec = MESHES[case]
        off = len(header_bytes(len(m["coord"]), len(m["faces"]), spec["props"], spec["index"], pad)) + vertex_records(case, m).nbytes
        found.setdefault(off % 4, pad)
    assert sorted(found) == [0, 1, 2, 3]
    return [found[k] for k in range(4)]


def write_file(path, data):
    os.makedirs(os.path.dirname(os.fspath(path)) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def labels(case, categories, outside_label):
    """-> (segIndices list, segGroups list) of a LABELLED case: sparse segment ids, 45 groups of 1 to 3 segments, one segment in two
    groups, segments (so vertices) in no group, one group labelled ABSENT_LABEL and one `outside_label` (ids outside both valid lists);
    the other labels are drawn from `categories`."""
    n = len(mesh(case)["coord"])
    rng = np.random.default_rng(MESHES[case]["seed"] + 100)
    seg_ids = np.sort(rng.choice(np.arange(3, 5000), 110, replace=False)) * 7            # sparse
    seg_indices = seg_ids[(np.arange(n) // 9) % len(seg_ids)]
    seg_indices[rng.random(n) < 0.03] = 4                                                   # a segment no group names
    groups, at = [], 0
    for g in range(45):
        k = int(rng.integers(1, 4))
        segs = [int(s) for s in seg_ids[at:at + k]]
        at += k
        label = ABSENT_LABEL if g == 5 else outside_label if g == 9 else str(categories[int(rng.integers(0, len(categories)))])
        groups.append(dict(id=g if g != 10 else 1234, objectId=g, segments=segs, label=label))
    groups[20]["segments"].append(groups[3]["segments"][0])                                # a segment in two groups: the later one wins
    return [int(s) for s in seg_indices], groups


def write_scene(root, scene_id, case, categories, outside_label, with_labels=True, subdir="scans", pad=0):
    d = os.path.join(root, subdir, scene_id)
    write_file(os.path.join(d, f"{scene_id}_vh_clean_2.ply"), ply_bytes(case, pad))
    if with_labels:
        seg_indices, groups = labels(case, categories, outside_label)
        with open(os.path.join(d, f"{scene_id}_vh_clean_2.0.010000.segs.json"), "w") as f:
            json.dump(dict(sceneId=scene_id, segIndices=seg_indices), f)
        with open(os.path.join(d, f"{scene_id}.aggregation.json"), "w") as f:
            json.dump(dict(sceneId=scene_id, segGroups=groups), f)
    return d


def write_tsv(path, cells):
    """cells: (rows, 3) strings raw_category, id, nyu40id, as the file holds them -> a tsv with the reference file's column layout"""
    names = ["id", "raw_category", "category", "count", "nyu40id", "eigen13id"]
    with open(path, "w", newline="", encoding="utf-8") as f:
        f.write("\t".join(names) + "\n")
        for raw, id200, nyu in cells:
            f.write("\t".join([str(id200), str(raw), "c", "1", str(nyu), "0"]) + "\n")
    return path


# ---- Gaussians ---------------------------------------------------------------------------------------------------------------------------
def two_nearest(coord, pc):
    """fp64 brute force: (index of the nearest point, relative gap of the squared distances nearest / second nearest)"""
    c, p = np.asarray(coord, dtype=np.float64), np.asarray(pc, dtype=np.float64)
    idx, gap = np.empty(len(c), dtype=np.int64), np.empty(len(c))
    for s in range(0, len(c), 256):
        d2 = ((c[s:s + 256, None, :] - p[None, :, :]) ** 2).sum(-1)
        part = np.argpartition(d2, 1, axis=1)[:, :2]
        a, b = np.take_along_axis(d2, part, 1).T
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        idx[s:s + 256] = np.where(a <= b, part[:, 0], part[:, 1])
        gap[s:s + 256] = (hi - lo) / np.maximum(hi, 1e-300)
    return idx, gap


GS_PROPS = [(n, "float") for n in ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1",
                                   "rot_2", "rot_3"]]


def gaussians(case):
    """the structured vertex array of a checkpoint: centres within 2 cm of the mesh's vertices, each with a clear nearest vertex"""
    spec = GS_CASES[case]
    rng = np.random.default_rng(spec["seed"])
    verts = mesh(case)["coord"]
    out = np.empty((0, 3), dtype=np.float32)
    while len(out) < spec["n"]:
        c = (verts[rng.integers(0, len(verts), 2 * spec["n"])] + rng.uniform(-0.02, 0.02, (2 * spec["n"], 3))).astype(np.float32)
        out = np.concatenate([out, c[two_nearest(c, verts)[1] >= MIN_GAP]])
    out = out[:spec["n"]]
    arr = np.zeros(spec["n"], dtype=np.dtype([(n, "<f4") for n, _ in GS_PROPS]))
    for name, _ in GS_PROPS:
        arr[name] = rng.standard_normal(spec["n"]).astype(np.float32)
    for a, name in enumerate("xyz"):
        arr[name] = out[:, a]
    return arr


def gaussian_ply_bytes(arr):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(arr)}"] + [f"property float {n}" for n in arr.dtype.names] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii") + arr.tobytes()


def features(case):
    """(n, 8) f32 language features with all-zero rows"""
    n = GS_CASES[case]["n"]
    rng = np.random.default_rng(GS_CASES[case]["seed"] + 7)
    f = rng.standard_normal((n, 8)).astype(np.float32)
    f[rng.random(n) < 0.3] = 0
    return f


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def normals_restated(coord, faces, form):
    """the device scheme in numpy: per face the term with every fp32 operation rounded on its own, per vertex the terms of its incident
    faces added in ascending face index into one fp32 accumulator per component (form 'pc': a face once per vertex; 'gs': once per
    corner).  The host tests show that it reproduces both recorded `vertex_normal`s bit for bit."""
    f32 = np.float32
    coord, faces = np.asarray(coord, dtype=f32), np.asarray(faces).astype(np.int64).reshape(-1, 3)
    eps = f32(1e-8)
    with np.errstate(all="ignore"):
        u, w = coord[faces[:, 1]] - coord[faces[:, 0]], coord[faces[:, 2]] - coord[faces[:, 0]]
        c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        r = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        if form == "pc":
            length = r + eps
            area = length * f32(0.5)
        else:
            area, length = f32(0.5) * r, np.maximum(eps, r)
        terms = (c / length[:, None]) * area[:, None]
        acc = np.zeros_like(coord)
        keys = faces.reshape(-1)
        prev = {}
        for p in np.argsort(keys, kind="stable"):
            v, f = keys[p], p // 3
            if form == "pc" and prev.get(v) == f:
                continue
            prev[v] = f
            acc[v] = acc[v] + terms[f]
        r = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        length = r + eps if form == "pc" else np.maximum(eps, r)
        return acc / length[:, None]
