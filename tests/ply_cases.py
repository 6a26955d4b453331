"""Inputs and the numpy restatement shared by tests/test_gaussian_ply_host.py (CPU), tests/test_hip_gaussian_ply.py (GPU) and
tests/golden/make_golden_gaussian_ply.py (the fixture generator) for the 3DGS checkpoint reader
(scenesplat_amd/pointcept_api/gaussian_ply.py, csrc/ply.hip).  Nothing here touches the library under test.

`decode_reference` restates the decode in this project's words: coord copied; colour, quaternion in separately rounded fp32 steps in
numpy's order; exp and the sigmoid in fp64, rounded once.  The host tests show that it reproduces the recorded outputs of the reference
bit for bit for coord / color / quat, and how far the recording's fp32 exp lies from it; the GPU tests then use it at sizes and values
the fixture does not hold.

Layouts: `f_rest_*` and every extra column hold their own column number, so the fixture compresses and a wrong offset shows as a wrong
value.  The coordinates of every layout case lie clear of the Voronoi faces of both labelled clouds (TRANSFER), so that an fp32 grid
search and an fp64 KD-tree must select the same point for every row."""
import json
import os
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gaussian_ply.npz")
C0 = 0.28209479177387814
NP_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
            "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
BOX_LO, BOX_HI = np.array([-3.0, -3.0, 0.0]), np.array([3.0, 3.0, 2.0])
MIN_GAP = 1e-3             # relative gap of the squared distances to the nearest and the second nearest cloud point (the maker asserts 1e-4)


def _f(names):
    return [(n, "float") for n in names]


def standard_properties(sh_rest=45, n_scale=3, n_rot=4):
    """the vertex layout the 3DGS trainer writes: 62 float properties at SH degree 3, 17 at degree 0"""
    return _f(["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(sh_rest)] + ["opacity"]
              + [f"scale_{i}" for i in range(n_scale)] + [f"rot_{i}" for i in range(n_rot)])


def _shuffled():
    props = standard_properties(0)
    order = np.random.default_rng(77).permutation(len(props))
    return [props[i] for i in order]


# name -> dict(n, seed, props).  Strides: 248 (16-byte tiles through LDS), 68, 68, 80, 540 (no LDS tile: rows straight from memory), 64.
LAYOUTS = OrderedDict([
    ("standard62", dict(n=300, seed=1, props=standard_properties())),
    ("sh0_17", dict(n=200, seed=2, props=standard_properties(0))),
    ("shuffled", dict(n=150, seed=3, props=_shuffled())),
    ("extra_types", dict(n=150, seed=4, props=[("red", "uchar"), ("green", "uint8"), ("blue", "uchar"), ("alpha", "uchar")]
                         + standard_properties(0)[:9] + [("time", "double")] + standard_properties(0)[9:])),
    ("wide540", dict(n=150, seed=5, props=[("r", "uchar"), ("g", "uchar"), ("b", "uchar"), ("a", "uchar"), ("stamp", "float64")]
                     + standard_properties()[:54] + _f([f"extra_{i}" for i in range(70)]) + standard_properties()[54:])),
    ("scale2", dict(n=100, seed=6, props=standard_properties(0, n_scale=2))),
])

# labelled clouds: a jittered lattice over the box.  cloud "fine" is large enough for the hash-grid search, "coarse" takes the scan.
CLOUDS = OrderedDict([("fine", dict(spacing=0.25, seed=21)), ("coarse", dict(spacing=0.5, seed=22))])
# name -> the layout whose coord is labelled, the cloud, and the assets of the cloud (dtype, trailing shape)
TRANSFER = OrderedDict([
    ("fine_i16", dict(layout="standard62", cloud="fine", assets=dict(segment=("int16", ()), normal=("float32", (3,)), instance=("int64", ())))),
    ("coarse_i64_col", dict(layout="sh0_17", cloud="coarse", assets=dict(segment=("int64", (1,)), normal=("float32", (3,))))),
])
ROUND_TRIP = dict(layout="standard62", transfer="fine_i16", feat_width=8, feat_seed=31)


# ---- clouds and coordinates ------------------------------------------------------------------------------------------------------------
def cloud(name):
    """(m, 3) float32: lattice points of the box, each moved by up to 0.3 spacings per axis"""
    spec = CLOUDS[name]
    rng = np.random.default_rng(spec["seed"])
    axes = [np.arange(BOX_LO[a] + spec["spacing"] / 2, BOX_HI[a], spec["spacing"]) for a in range(3)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    pts = pts + rng.uniform(-0.3, 0.3, pts.shape) * spec["spacing"]
    return rng.permutation(pts).astype(np.float32)                       # (row order carries no geometry)


def cloud_assets(name, spec):
    """{asset: (m, ...) array} of a TRANSFER case; every row's values are its own"""
    m = cloud(spec["cloud"]).shape[0]
    rng = np.random.default_rng(1000 + len(name))
    out = OrderedDict()
    for asset, (dtype, trailing) in spec["assets"].items():
        if asset == "normal":
            out[asset] = rng.standard_normal((m,) + tuple(trailing)).astype(dtype)
        else:
            out[asset] = (rng.integers(-1, 200, (m,) + tuple(trailing)) * (1 if asset == "segment" else 1000003)).astype(dtype)
    return out


def two_nearest(coord, pc):
    """fp64 brute force: (index of the nearest cloud point, relative gap of the squared distances nearest / second nearest)"""
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


_CLOUDS = {}


def coords(rng, n):
    """n float32 points of the box with a clear nearest point in every cloud"""
    for name in CLOUDS:
        if name not in _CLOUDS:
            _CLOUDS[name] = cloud(name)
    out = np.empty((0, 3), dtype=np.float32)
    while len(out) < n:
        c = rng.uniform(BOX_LO, BOX_HI, (2 * n, 3)).astype(np.float32)
        keep = np.ones(len(c), dtype=bool)
        for pc in _CLOUDS.values():
            keep &= two_nearest(c, pc)[1] >= MIN_GAP
        out = np.concatenate([out, c[keep]])
    return out[:n]


# ---- records and files -------------------------------------------------------------------------------------------------------------------
def record_dtype(props):
    return np.dtype([(name, "<" + NP_TYPES[t]) for name, t in props])


def records(case):
    """the structured vertex array of a LAYOUTS case.  Rows 0..7 of every case: rot_0 == 0 with the other components set, an all-zero
    quaternion, a negative rot_0, f_dc far outside both clip bounds, opacity logits +-30, and scale logs -20 / 12."""
    spec = LAYOUTS[case]
    rng = np.random.default_rng(spec["seed"])
    n, props = spec["n"], spec["props"]
    arr = np.zeros(n, dtype=record_dtype(props))
    for col, (name, t) in enumerate(props):
        arr[name] = col                                                  # f_rest_*, normals and every extra column: the column number
    c = coords(rng, n)
    for a, name in enumerate("xyz"):
        arr[name] = c[:, a]
    for a in range(3):
        arr[f"f_dc_{a}"] = rng.uniform(-2.5, 2.5, n).astype(np.float32)
    arr["opacity"] = (rng.standard_normal(n) * 4).astype(np.float32)
    names = [p[0] for p in props]
    for name in names:
        if name.startswith("scale_"):
            arr[name] = rng.uniform(-8.0, 1.0, n).astype(np.float32)
        if name.startswith("rot"):
            arr[name] = rng.standard_normal(n).astype(np.float32)
    arr["rot_0"][0] = 0.0
    for name in names:
        if name.startswith("rot"):
            arr[name][1] = 0.0
    arr["rot_0"][2] = -0.75
    arr["f_dc_0"][3], arr["f_dc_1"][3], arr["f_dc_2"][3] = -40.0, 40.0, 0.0
    arr["opacity"][4], arr["opacity"][5] = 30.0, -30.0
    arr["scale_0"][6], arr["scale_0"][7] = -20.0, 12.0
    return arr


def ply_bytes(arr, props, comments=(), crlf=False, pad_to_odd=False, face=False):
    """the bytes of a binary little-endian .ply holding `arr` as its vertex element.  pad_to_odd: a comment sized so that the vertex block
    starts at an odd file offset; face: a trailing `face` element with a list property and two faces of data"""
    eol = "\r\n" if crlf else "\n"
    lines = ["ply", "format binary_little_endian 1.0"] + [f"comment {c}" for c in comments]
    body = [f"element vertex {len(arr)}"] + [f"property {t} {name}" for name, t in props]
    if face:
        body += ["element face 2", "property list uchar int vertex_indices"]
    body.append("end_header")
    if pad_to_odd:
        size = sum(len(line) + len(eol) for line in lines + body)
        fill = "comment pad"
        if (size + len(fill) + len(eol)) % 2 == 0:
            fill += "_"
        lines.append(fill)
    head = (eol.join(lines + body) + eol).encode("ascii")
    tail = b""
    if face:
        tail = b"".join(np.uint8(3).tobytes() + np.array(t, dtype="<i4").tobytes() for t in ((0, 1, 2), (1, 2, 3)))
    return head + np.ascontiguousarray(arr).tobytes() + tail


def write_ply(path, arr, props, **kw):
    os.makedirs(os.path.dirname(os.fspath(path)) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(ply_bytes(arr, props, **kw))
    return path


def synthetic(n, props, seed):
    """a record array of n rows with plausible checkpoint values (no special rows, any coordinates): the sizes the fixture does not hold"""
    rng = np.random.default_rng(seed)
    arr = np.zeros(n, dtype=record_dtype(props))
    for col, (name, t) in enumerate(props):
        if name in ("x", "y", "z"):
            arr[name] = (rng.standard_normal(n) * 3).astype(np.float32)
        elif name.startswith("f_dc_"):
            arr[name] = rng.uniform(-2.5, 2.5, n).astype(np.float32)
        elif name == "opacity":
            arr[name] = (rng.standard_normal(n) * 4).astype(np.float32)
        elif name.startswith("scale_"):
            arr[name] = rng.uniform(-8.0, 1.0, n).astype(np.float32)
        elif name.startswith("rot"):
            arr[name] = rng.standard_normal(n).astype(np.float32)
        else:
            arr[name] = col
    return arr


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def gaussian_names(names):
    scale = sorted([p for p in names if p.startswith("scale_")], key=lambda s: int(s.split("_")[-1]))
    rot = sorted([p for p in names if p.startswith("rot")], key=lambda s: int(s.split("_")[-1]))
    return scale, rot


def decode_reference(arr):
    """-> {coord, color, opacity, scale, quat, opacity64, scale64}: the decode of a structured vertex array; the *64 entries are the
    fp64 values that opacity and scale are the single roundings of"""
    f32 = np.float32
    scale_names, rot_names = gaussian_names(arr.dtype.names)
    with np.errstate(all="ignore"):
        out = OrderedDict()
        out["coord"] = np.stack([arr[k].astype(f32) for k in "xyz"], 1)
        t = np.stack([arr[f"f_dc_{a}"].astype(f32) for a in range(3)], 1) * f32(C0)
        t = np.clip(t + f32(0.5), f32(0), f32(1)) * f32(255)
        out["color"] = np.where(np.isnan(t), f32(0), t).astype(np.uint8)     # (the NaN colour is unspecified; nothing compares it)
        out["opacity64"] = 1.0 / (1.0 + np.exp(-arr["opacity"].astype(np.float64)))
        out["opacity"] = out["opacity64"].astype(f32)
        out["scale64"] = np.exp(np.stack([arr[k].astype(np.float64) for k in scale_names], 1))
        out["scale"] = out["scale64"].astype(f32)
        q = np.stack([arr[k].astype(f32) for k in rot_names], 1)
        p = q * q
        s = p[:, 0]
        for a in range(1, q.shape[1]):
            s = s + p[:, a]                                              # ((q0^2 + q1^2) + q2^2) + q3^2, each sum rounded to fp32
        quo = q / (np.sqrt(s) + f32(1e-9))[:, None]
        out["quat"] = quo * np.sign(quo[:, :1])
    assert all(out[k].dtype == f32 for k in ("coord", "opacity", "scale", "quat"))
    return out


def ulp_error(got, exact64):
    """|got - exact| in units of the fp32 spacing at exact (fp64 array of the same shape).  Where the exact value rounds to inf or is
    NaN, got must be the same (error 0) or the error is inf."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exact64.shape, (got.dtype, got.shape, exact64.shape)
    with np.errstate(all="ignore"):
        want = exact64.astype(np.float32)
        special = ~np.isfinite(want)
        same = (np.isnan(want) & np.isnan(got)) | (want == got)
        unit = np.spacing(np.abs(np.where(special, np.float32(1), want))).astype(np.float64)
        err = np.abs(got.astype(np.float64) - exact64) / unit
    return np.where(special, np.where(same, 0.0, np.inf), err)


# ---- the recorded reference ------------------------------------------------------------------------------------------------------------------
def load_golden():
    """-> dict(layouts {case: dict(records structured array, out {asset: array})}, transfer {case: {asset: array}},
    lang dict(features f32, lang_feat f16, valid_feat_mask i64), files [file names of the round-trip folder],
    dirs {mode: [relative directories holding a scene]})"""
    z = np.load(GOLDEN)
    index = json.loads(str(z["index"]))
    layouts = OrderedDict()
    for case in index["layouts"]:
        raw = z[f"{case}/records"]
        layouts[case] = dict(records=raw.reshape(-1).view(record_dtype(LAYOUTS[case]["props"])),
                             out=OrderedDict((a, z[f"{case}/out/{a}"]) for a in ("coord", "color", "opacity", "scale", "quat")))
    transfer = OrderedDict((case, OrderedDict((a, z[f"{case}/gs/{a}"]) for a in assets)) for case, assets in index["transfer"].items())
    lang = dict(features=z["lang/features"], lang_feat=z["lang/lang_feat"], valid_feat_mask=z["lang/valid_feat_mask"])
    return dict(layouts=layouts, transfer=transfer, lang=lang, files=index["files"], dirs=index["dirs"])


# the tree of the output-directory rule: relative .ply paths under the input folder ("broken.ply" does not parse)
DIR_TREE = ("a.ply", "b.ply", "sub/c.ply", "sub/deep/d.ply", "broken.ply")
DIR_CASE = "scale2"


def write_dir_tree(root):
    arr = records(DIR_CASE)
    for rel in DIR_TREE:
        path = os.path.join(root, *rel.split("/"))
        if rel == "broken.ply":
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(b"not a ply file\n")
        else:
            write_ply(path, arr, LAYOUTS[DIR_CASE]["props"])
    return root


def scene_dirs(root):
    """sorted relative directories under root that hold a coord.npy ('.' for root itself)"""
    found = []
    for d, _, files in os.walk(root):
        if "coord.npy" in files:
            found.append(os.path.relpath(d, root).replace(os.sep, "/"))
    return sorted(found)
