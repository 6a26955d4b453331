"""The clouds of the oriented-box tests (seeded generators), the numpy restatement of the definition and the
golden file tests/golden/oriented_box.npz, which tests/golden/make_golden_oriented_box.py writes with scipy's Qhull.  Neither scipy
nor Open3D is imported here."""
import os
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "oriented_box.npz")
MARGIN = 0.25                      # the reference's enlargement
N_QUERIES = 4000
ROOM = np.array([6.0, 4.0, 2.5])
MIN_VOLUME_GAP = 1e-6              # the maker asserts this relative gap between the two smallest candidate volumes
MIN_FACE_DISTANCE = 1e-8           # ... and this distance of every query point to the faces of the enlarged box
PREFIXES = (0, 1, 31, 32, 33, 255, 256, 257, 4000)

CASES = OrderedDict([
    ("tet", dict(kind="blob", n=4, seed=101)),
    ("blob64", dict(kind="blob", n=64, seed=102)),
    ("blob257", dict(kind="blob", n=257, seed=103)),
    ("box65", dict(kind="box", n=65, seed=104)),
    ("box300", dict(kind="box", n=300, seed=105)),
    ("room5000", dict(kind="room", n=5000, seed=106)),
    ("lattice_axis", dict(kind="lattice", rotate=False, seed=107)),
    ("lattice_rot", dict(kind="lattice", rotate=True, seed=108)),
])
GENERAL = tuple(c for c, spec in CASES.items() if spec["kind"] != "lattice")       # points in general position
LATTICE = tuple(c for c, spec in CASES.items() if spec["kind"] == "lattice")
LATTICE_VOLUME = 64.0


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def cloud(case):
    """-> (n, 3) float32"""
    spec = CASES[case]
    rng = np.random.default_rng(spec["seed"])
    if spec["kind"] == "blob":
        p = rng.standard_normal((spec["n"], 3)) * np.array([3.0, 1.5, 0.5])
    elif spec["kind"] == "box":
        p = (rng.random((spec["n"], 3)) - 0.5) * ROOM
    elif spec["kind"] == "room":
        p = (rng.random((spec["n"], 3)) - 0.5) * ROOM
        face = rng.integers(0, 6, spec["n"])
        axis, side = face // 2, (face % 2) * 2.0 - 1.0
        p[np.arange(spec["n"]), axis] = side * ROOM[axis] * 0.5
        p += rng.standard_normal(p.shape) * 0.01
    else:
        g = np.arange(5, dtype=np.float64)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        if not spec["rotate"]:
            return p.astype(np.float32)
    return (p @ rotation(rng).T + rng.standard_normal(3) * 2.0).astype(np.float32)


# ---- the definition in numpy: every operation on its own, in the order the kernel takes them --------------------------------------------
def _unit(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                    axis=1)


def candidate_frames(verts, tris):
    """verts (H, 3) fp64, tris (T, 3) -> a, u, v, w, each (3 T, 3): candidate 3 t + k starts at corner k of triangle t"""
    tris = np.asarray(tris).astype(np.int64)
    k = np.arange(3)
    ia, ib, ic = tris[:, k].reshape(-1), tris[:, (k + 1) % 3].reshape(-1), tris[:, (k + 2) % 3].reshape(-1)
    a = verts[ia]
    u = _unit(verts[ib] - a)
    w = _unit(_cross(u, verts[ic] - a))
    v = _unit(_cross(w, u))
    return a, u, v, w


def candidate_boxes(verts, tris):
    """-> (volumes (3 T,), lo (3 T, 3), hi (3 T, 3), frames): steps 2 and 3 over the vertices `verts` (all of them are looked at)"""
    a, u, v, w = candidate_frames(verts, tris)
    lo, hi = np.full((a.shape[0], 3), np.inf), np.full((a.shape[0], 3), -np.inf)
    for p in verts:
        d = p[None, :] - a
        for j, r in enumerate((u, v, w)):
            q = (d[:, 0] * r[:, 0] + d[:, 1] * r[:, 1]) + d[:, 2] * r[:, 2]
            lo[:, j], hi[:, j] = np.fmin(lo[:, j], q), np.fmax(hi[:, j], q)
    e = hi - lo
    framed = np.isfinite(u).all(axis=1) & np.isfinite(v).all(axis=1) & np.isfinite(w).all(axis=1)      # no frame: no volume
    return np.where(framed, (e[:, 0] * e[:, 1]) * e[:, 2], np.nan), lo, hi, (a, u, v, w)


def restated_box(verts, tris):
    """-> (best candidate, box (15,): center, R row-major with the axes as columns, extent; volumes (3 T,)).  verts: the hull's vertices
    (fp64), tris: rows of verts."""
    volumes, lo, hi, (a, u, v, w) = candidate_boxes(verts, tris)
    best = int(np.nanargmin(volumes))                                    # the first of equal volumes
    m = (lo[best] + hi[best]) * 0.5
    center = a[best] + ((u[best] * m[0] + v[best] * m[1]) + w[best] * m[2])
    R = np.stack([u[best], v[best], w[best]], axis=1)
    return best, np.concatenate([center, R.reshape(-1), hi[best] - lo[best]]), volumes


def hull_vertices(points, tris):
    """the hull's vertices and the triangles as rows of them: (verts fp64 (H, 3), tris (T, 3) int32, rows (H,) of points)"""
    rows, inverse = np.unique(np.asarray(tris).reshape(-1), return_inverse=True)
    return points[rows].astype(np.float64), inverse.reshape(-1, 3).astype(np.int32), rows


def box_coordinates(box, points):
    """(n, 3) fp64: the coordinates of points in the box's frame, relative to its centre"""
    center, R = box[0:3], box[3:12].reshape(3, 3)
    d = np.asarray(points).astype(np.float64) - center
    return np.stack([(d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k] for k in range(3)], axis=1)


def inside(box, points, margin=0.0):
    return np.all(np.abs(box_coordinates(box, points)) <= (box[12:15] + 2.0 * margin) * 0.5, axis=1)


def queries(box, seed, n=N_QUERIES, margin=MARGIN):
    """n float32 points around the box grown by margin: about 40 % inside"""
    rng = np.random.default_rng(seed + 1000)
    center, R = box[0:3], box[3:12].reshape(3, 3)
    s = (rng.random((n, 3)) * 2.0 - 1.0) * 1.35 * (box[12:15] + 2.0 * margin) * 0.5
    return (center + s @ R.T).astype(np.float32)


def triangle_set(tris):
    return set(map(tuple, np.sort(np.asarray(tris).astype(np.int64), axis=1).tolist()))


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
