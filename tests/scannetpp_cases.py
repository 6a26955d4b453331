"""Inputs shared by tests/test_scannetpp_host.py (CPU), tests/test_hip_scannetpp.py (GPU) and tests/golden/make_golden_scannetpp.py (the
fixture generator) for the ScanNet++ converter (scenesplat_amd/pointcept_api/scannetpp_mesh.py, csrc/scannetpp.hip).  Nothing here
touches the library under test.

Meshes: those of tests/scannet_mesh_cases.py, written with the 15-byte `x y z red green blue` vertex records of a ScanNet++
`mesh_aligned_0.05.ply`, plus `cancel`: a vertex whose incident cross products cancel to a residual an fp32 sum cannot hold.
Annotations: `segIndices` and `segGroups` built so that every branch of the reference's label loop is taken (the list at `annotation`).
The two restatements, of the normals and of the per-row label rule, are numpy; the host tests hold them against the fixture."""
import json
import os
from collections import OrderedDict

import numpy as np

import scannet_mesh_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scannetpp.npz")
TOP100 = os.path.join(HERE, "golden", "scannetpp_top100.txt")            # the reference's metadata/semantic_benchmark/top100.txt: a list of names
SPP_PROPS = [("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]     # 15 bytes
MESHES = list(mc.MESHES) + ["cancel"]
INDEX = dict(scan="int", extra="uint", n257="int", single="int", cancel="uint")
IGNORED_LABEL = "a label the benchmark does not list"
# annotation case -> vertex count (None: that of the mesh of the same name), seed, vertices of the big segment, whether it has groups
ANNOS = OrderedDict([("rich", dict(n=3000, seed=51, big=1100, groups=True)), ("scan", dict(n=None, seed=52, big=300, groups=True)),
                     ("extra", dict(n=None, seed=53, big=0, groups=False))])
# the end-to-end tree: scene name -> (split, mesh case); the annotation of a train / val scene is the case of the mesh's name
SCENES = OrderedDict([("0a5c013435", ("train", "scan")), ("1ada7a0617", ("val", "extra")), ("c4c04e6d6c", ("test", "n257"))])
UNREADABLE = "ffffffffff"                                                # in the train list, its mesh does not parse
GS_CASES = OrderedDict([("scan", dict(n=400, seed=61, zero=0.3)), ("extra", dict(n=250, seed=62, zero=0.7)),      # extra: under half valid
                        ("n257", dict(n=200, seed=63, zero=0.3))])
MIN_GAP = 1e-3             # relative gap of the squared distances nearest / second nearest vertex (the maker asserts 1e-4)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def mesh(case):
    """-> dict(coord (n, 3) f32, color (n, 3) u8, faces (F, 3) int64, special {name: row}).  `cancel`: the n257 mesh plus a vertex with
    two large faces of opposite orientation over nearly the same corners and a small third one: the sum of the three cross products is
    five orders below its terms."""
    if case != "cancel":
        return mc.mesh(case)
    m = mc.mesh("n257")
    rng = np.random.default_rng(71)
    c = m["coord"][0].astype(np.float64) + np.array([0.31, 0.47, 0.53])
    a, b = c + np.array([0.0203, 0.0011, 0.0007]), c + np.array([0.0013, 0.0197, -0.0009])
    extra = np.stack([c, a, b, a + np.array([0.0, 1e-6, 2e-6]), b + np.array([1.5e-6, 0.0, -1e-6]), c + np.array([0.0004, -0.0003, 0.0006])])
    n0 = len(m["coord"])
    v, va, vb, va2, vb2, vd = range(n0, n0 + 6)
    faces = np.concatenate([m["faces"], np.array([(v, va, vb), (v, vb2, va2), (v, va, vd)], dtype=np.int64)])
    faces = faces[rng.permutation(len(faces))]
    coord = np.concatenate([m["coord"], extra.astype(np.float32)])
    color = np.concatenate([m["color"], rng.integers(0, 256, (6, 3)).astype(np.uint8)])
    return dict(coord=coord, color=color, faces=faces, special=dict(cancel_vertex=v))


def vertex_records(m):
    arr = np.zeros(len(m["coord"]), dtype=np.dtype([(name, "<" + mc.NP_TYPES[t]) for name, t in SPP_PROPS]))
    for a, name in enumerate("xyz"):
        arr[name] = m["coord"][:, a]
    for a, name in enumerate(("red", "green", "blue")):
        arr[name] = m["color"][:, a]
    assert arr.dtype.itemsize == 15
    return arr


def ply_bytes(case, pad=0, m=None):
    m = mesh(case) if m is None else m
    return (mc.header_bytes(len(m["coord"]), len(m["faces"]), SPP_PROPS, INDEX[case], pad) + vertex_records(m).tobytes()
            + mc.face_bytes(m["faces"], INDEX[case]))


def pads_for_alignments(case):
    """four comment lengths that put the face block at file offsets 0, 1, 2, 3 mod 4"""
    m = mesh(case)
    found = {}
    for pad in range(1, 16):
        off = len(mc.header_bytes(len(m["coord"]), len(m["faces"]), SPP_PROPS, INDEX[case], pad)) + 15 * len(m["coord"])
        found.setdefault(off % 4, pad)
    assert sorted(found) == [0, 1, 2, 3]
    return [found[k] for k in range(4)]


def normals_o3d_restated(coord, faces, dtype=np.float64):
    """The definition `TriangleMesh::ComputeVertexNormals(normalized=True)` implements, in numpy: the vertices as `dtype`, per face the
    unnormalised cross product (v1 - v0) x (v2 - v0) with every component mul, mul, sub, per vertex the cross products of its faces
    added one after the other in face order, once per corner (`np.add.at` is sequential), z = (x^2 + y^2) + z^2 and a division by
    sqrt(z) where z > 0, then one rounding to float32.  dtype=float32 is the same walk in fp32 (what the ScanNet kernels would do)."""
    v, f = np.asarray(coord, dtype=np.float32).astype(dtype), np.asarray(faces).astype(np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        acc = np.zeros_like(v)
        np.add.at(acc, f.reshape(-1), np.repeat(c, 3, axis=0))
        z = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
        r = np.sqrt(z)
        acc = np.where((z > 0)[:, None], acc / np.where(z > 0, r, 1)[:, None], acc)
    return acc.astype(np.float32)


# ---- annotations ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_SEGMENTS = OrderedDict([   # name -> vertices; the groups that list each are built in `annotation`
    ("none", 40), ("one", 30), ("two", 25), ("three", 20), ("five", 50), ("ignored_between", 15), ("repeated", 12), ("tie", 18),
    ("tie_later", 16), ("pos0", 22), ("pos1", 24), ("pos2", 26), ("naive", 10), ("naive_mate", 20), ("beyond", 9)]
    + [(f"h{k}", 15) for k in range(1, 8)])
BULK_SEGMENTS, BULK_GROUPS = 35, 30


def anno_vertices(case):
    return ANNOS[case]["n"] if ANNOS[case]["n"] is not None else len(mesh(case)["coord"])


def segment_ids(case):
    """-> {name: segment id}: sparse ids; `absent` and `absent_alone` are ids no vertex has, `beyond` lies above every id a group lists"""
    names = list(SPECIAL_SEGMENTS) + ["big"] + [f"bulk{k}" for k in range(BULK_SEGMENTS)]
    rng = np.random.default_rng(ANNOS[case]["seed"] + 1000)
    ids = rng.choice(np.arange(1, 4000), len(names), replace=False) * 5 + 2
    out = {name: int(i) for name, i in zip(names, ids)}
    out.update(absent=30001, absent_alone=30007, beyond=40003)
    return out


def annotation(case, class_names):
    """-> (segIndices list, segGroups list).  With groups: segments in 0 (`none`), 1, 2, 3 and 5 valid groups; an ignored-label group
    between two valid ones; a segment id twice in one list; a group that lists a segment no vertex has, and one that lists nothing
    else; a group (`full`) whose only segment holds three labels already; two slots of equal size at positions 0 / 1 and at 1 / 2;
    the smallest instance at position 0, 1 and 2; `naive`: a segment whose second group also lists the full segment `five`, so that
    counting all of that group's vertices would pick the other column; `big`: one segment with more than 1,024 vertices (case rich);
    `beyond`: a segment id above every listed one; then BULK_GROUPS random groups over BULK_SEGMENTS more segments.  Without groups:
    an empty list."""
    spec, n = ANNOS[case], anno_vertices(case)
    rng = np.random.default_rng(spec["seed"])
    if not spec["groups"]:
        return [int(s) for s in (np.arange(n) // 11) * 3], []
    ids = segment_ids(case)
    counts = OrderedDict(SPECIAL_SEGMENTS)
    counts["big"] = spec["big"]
    rest = n - sum(counts.values())
    assert rest >= 4 * BULK_SEGMENTS, (case, rest)
    cuts = np.sort(rng.choice(np.arange(1, rest), BULK_SEGMENTS - 1, replace=False))
    for k, c in enumerate(np.diff(np.r_[0, cuts, rest])):
        counts[f"bulk{k}"] = int(c)
    seg_indices = np.concatenate([np.full(c, ids[name], dtype=np.int64) for name, c in counts.items()])[rng.permutation(n)]
    groups = []

    def add(names, valid=True):
        label = str(class_names[int(rng.integers(0, len(class_names)))]) if valid else IGNORED_LABEL
        groups.append(dict(id=len(groups) + 1, objectId=1000 + 3 * len(groups), segments=[ids[s] for s in names], label=label))

    add(["one"])
    add(["two"]); add(["two", "h3"])
    add(["three"]); add(["three"]); add(["three", "h4"])
    add(["five", "big"]); add(["five"]); add(["five"])
    add(["five"])                                                        # `full`: every vertex it lists holds three labels already
    add(["naive", "naive_mate"])
    add(["five", "naive"])                                               # the fifth of `five`; for `naive` its size is the 10 of `naive`
    add(["ignored_between"]); add(["ignored_between"], valid=False); add(["ignored_between"])
    add(["repeated", "repeated"]); add(["repeated"])
    add(["absent", "h7"]); add(["absent_alone"])
    add(["tie"]); add(["tie"])
    add(["tie_later", "h5"]); add(["tie_later"]); add(["tie_later"])
    add(["pos0"]); add(["pos0", "h6"])
    add(["pos1", "h1"]); add(["pos1"])
    add(["pos2", "h1", "h2"]); add(["pos2", "h1"]); add(["pos2"])
    for _ in range(BULK_GROUPS):
        add([f"bulk{k}" for k in rng.choice(BULK_SEGMENTS, int(rng.integers(1, 5)), replace=False)], valid=rng.random() > 0.15)
    return [int(s) for s in seg_indices], groups


def labels_restated(seg_indices, g, src=None):
    """the rule ss_spp_labels applies, in numpy: g = first_groups(...) -> (segment, instance) (n, 3) int16"""
    seg, f3, ignore = np.asarray(seg_indices, dtype=np.int64), g["first3"].astype(np.int64), g["ignore_index"]
    S, G = len(f3), len(g["table_label"])
    count = np.bincount(seg[(seg >= 0) & (seg < S)], minlength=S)
    size = np.zeros(G, dtype=np.int64)
    for k in range(3):
        np.add.at(size, f3[f3[:, k] >= 0, k], count[f3[:, k] >= 0])
    rows = seg if src is None else seg[np.asarray(src, dtype=np.int64)]
    inside = (rows >= 0) & (rows < S)
    slots = np.where(inside[:, None], f3[np.where(inside, rows, 0)], -1) if S else np.full((len(rows), 3), -1, dtype=np.int64)
    used = slots >= 0
    sizes = np.where(used, size[np.maximum(slots, 0)] if G else 0, np.inf)
    p = np.where(used.sum(1) > 1, np.argmin(sizes, axis=1), 0)
    outs = []
    for table in (g["table_label"], g["table_object"]):
        a = np.where(used, table[np.maximum(slots, 0)] if G else 0, ignore).astype(np.int16)
        r = np.arange(len(a))
        a[r, p], a[r, 0] = a[r, 0].copy(), a[r, p].copy()
        outs.append(a)
    return tuple(outs)


# ---- the download tree ---------------------------------------------------------------------------------------------------------------------
def class_names():
    return np.loadtxt(TOP100, dtype=str, delimiter=".")


def write_scans(root, name, split, mesh_case, anno_case=None, pad=0):
    """<root>/data|sem_test/<name>/scans/ with the mesh and, with anno_case, the two json files"""
    d = os.path.join(os.fspath(root), "sem_test" if split == "test" else "data", name, "scans")
    mc.write_file(os.path.join(d, "mesh_aligned_0.05.ply"), ply_bytes(mesh_case, pad))
    if anno_case is not None:
        seg_indices, groups = annotation(anno_case, class_names())
        with open(os.path.join(d, "segments.json"), "w") as f:
            json.dump(dict(scene_id=name, segIndices=seg_indices), f)
        with open(os.path.join(d, "segments_anno.json"), "w") as f:
            json.dump(dict(scene_id=name, segGroups=groups), f)
    return d


def write_meta(root, lists):
    """the split lists {split: [names]} and the class list"""
    root = os.fspath(root)
    for split, fname in (("train", "nvs_sem_train.txt"), ("val", "nvs_sem_val.txt"), ("test", "sem_test.txt")):
        mc.write_file(os.path.join(root, "splits", fname), "".join(s + "\n" for s in lists.get(split, [])).encode())
    with open(TOP100, "rb") as f:
        mc.write_file(os.path.join(root, "metadata", "semantic_benchmark", "top100.txt"), f.read())


def write_tree(root):
    """the three SCENES (train, val, test), a scene of the train list whose mesh does not parse and one that has no folder"""
    lists = dict(train=[], val=[], test=[])
    for k, (name, (split, case)) in enumerate(SCENES.items()):
        write_scans(root, name, split, case, anno_case=case if split != "test" else None, pad=k)
        lists[split].append(name)
    mc.write_file(os.path.join(os.fspath(root), "data", UNREADABLE, "scans", "mesh_aligned_0.05.ply"), b"not a ply file\n")
    lists["train"] += [UNREADABLE, "0000000000"]
    write_meta(root, lists)
    return root


# ---- Gaussians ---------------------------------------------------------------------------------------------------------------------------
def gaussians(case):
    """the structured vertex array of a checkpoint: centres within 2 cm of the mesh's vertices, each with a clear nearest vertex"""
    spec = GS_CASES[case]
    rng = np.random.default_rng(spec["seed"])
    verts = mesh(case)["coord"]
    out = np.empty((0, 3), dtype=np.float32)
    while len(out) < spec["n"]:
        c = (verts[rng.integers(0, len(verts), 2 * spec["n"])] + rng.uniform(-0.02, 0.02, (2 * spec["n"], 3))).astype(np.float32)
        out = np.concatenate([out, c[mc.two_nearest(c, verts)[1] >= MIN_GAP]])
    arr = np.zeros(spec["n"], dtype=np.dtype([(n, "<f4") for n, _ in mc.GS_PROPS]))
    for name, _ in mc.GS_PROPS:
        arr[name] = rng.standard_normal(spec["n"]).astype(np.float32)
    for a, name in enumerate("xyz"):
        arr[name] = out[:spec["n"], a]
    return arr


def features(case):
    """(n, 8) f32 language features; a share `zero` of the rows is all zero"""
    spec = GS_CASES[case]
    rng = np.random.default_rng(spec["seed"] + 7)
    f = rng.standard_normal((spec["n"], 8)).astype(np.float32)
    f[rng.random(spec["n"]) < spec["zero"]] = 0
    return f


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
