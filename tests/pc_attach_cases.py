"""What tests/test_pc_attach_host.py and tests/test_hip_pc_attach.py share: the recorded reference (tests/golden/pc_attach.npz), the
fp64 brute-force statement of the slice in numpy, and the folder layout of a scene with its chunks."""
import json
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_attach.npz")
SEGMENTS = ("segment20", "segment_nyu_160")
SCENE = "scene_a_00"                                  # a scene name with underscores, as real ones have
CHUNK_SPLIT = "val_grid1.0cm_chunk6x6_stride3x3"
MARGIN = 1e-5


def load_golden():
    with np.load(GOLDEN) as z:
        fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


def distances(chunk, cloud):
    """(m, M) fp64: sqrt(dx * dx + dy * dy + dz * dz) of the fp32 coordinates, the squares added in x, y, z order"""
    q, p = np.asarray(chunk, np.float32).astype(np.float64), np.asarray(cloud, np.float32).astype(np.float64)
    dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def margins_hold(d_sorted, k, limit=None):
    """the k-th and (k + 1)-th, and the 1st and 2nd, sorted distances of every row differ by more than MARGIN relative (a selection by
    fp32 distances then equals the fp64 one); with `limit`, none of the k lies within MARGIN of it"""
    ok = True
    if d_sorted.shape[1] > k:
        ok = ok and bool(((d_sorted[:, k] - d_sorted[:, k - 1]) > MARGIN * d_sorted[:, k]).all())
    if d_sorted.shape[1] > 1:
        ok = ok and bool(((d_sorted[:, 1] - d_sorted[:, 0]) > MARGIN * d_sorted[:, 1]).all())
    if limit is not None:
        ok = ok and bool((np.abs(d_sorted[:, :k] - limit) > MARGIN).all())
    return ok


def slice_reference(chunk, cloud, assets, k=16, limit=0.25, need_margins=True):
    """The rule in numpy: per Gaussian its k nearest cloud rows (equal distances: the smaller row first), kept where the fp64
    distance is <= limit; the distinct kept rows ascending.  -> (rows, pc_coord rows, {asset: rows}, nearest (m,) rows or -1).
    need_margins: assert that no near-tie makes the fp32 selection of the code under test ambiguous (off for lattice inputs, whose
    fp32 arithmetic is exact)."""
    cloud = np.asarray(cloud, np.float32)
    k = min(k, cloud.shape[0])
    d = distances(chunk, cloud)
    order = np.argsort(d, axis=1, kind="stable")
    ds = np.take_along_axis(d, order, axis=1)
    if need_margins:
        assert margins_hold(ds, k), "the draw has a near-tie at the k-th place: choose another seed"
    keep = ds[:, :k] <= limit
    rows = np.unique(order[:, :k][keep]).astype(np.int64)
    nearest = np.where(keep[:, 0], order[:, 0], -1).astype(np.int64) if d.shape[0] else np.empty((0,), np.int64)
    return rows, cloud[rows], OrderedDict((n, np.asarray(a)[rows]) for n, a in assets.items()), nearest


def nearest_labels(asset, nearest):
    out = np.asarray(asset)[np.maximum(nearest, 0)].copy()
    out[nearest < 0] = -1
    return out


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def write_layout(root, fx, split="val", chunk_split=CHUNK_SPLIT, scene=SCENE):
    """the recorded scene as folders: <root>/pc/<split>/<scene>/{coord, segment*, instance}.npy, <root>/gs/<split>/<scene>/coord.npy and
    <root>/gs/<chunk_split>/<scene>_<i>/coord.npy.  -> (gs_root, pc_root, [chunk directories])"""
    gs_root, pc_root = os.path.join(root, "gs"), os.path.join(root, "pc")
    src = os.path.join(pc_root, split, scene)
    os.makedirs(src)
    for k in ("coord",) + SEGMENTS + ("instance",):
        np.save(os.path.join(src, k + ".npy"), fx["pc/" + k])
    os.makedirs(os.path.join(gs_root, split, scene))
    np.save(os.path.join(gs_root, split, scene, "coord.npy"), fx["chunk0/coord"])
    dirs = []
    for i in range(3):
        d = os.path.join(gs_root, chunk_split, f"{scene}_{i}")
        os.makedirs(d)
        np.save(os.path.join(d, "coord.npy"), fx[f"chunk{i}/coord"])
        dirs.append(d)
    return gs_root, pc_root, dirs
