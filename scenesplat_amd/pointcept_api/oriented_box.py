"""The minimal oriented bounding box of a scan and the Gaussians inside it: what preprocess_scannet_gs.py:233-238,311-332 and
preprocess_scannetpp_gs.py:234-267 do with Open3D's `get_minimal_oriented_bounding_box()` / `get_point_indices_within_bounding_box()`
(the box of the scan's vertices, grown by 25 cm on every side, keeps the Gaussians of a checkpoint that lie in the room).

The definition, for points (N, 3) float32 with all arithmetic in fp64:
1. H = the convex hull of the points, as triangles.
2. every triangle t and each of its three edges k is a candidate 3 t + k: corners a, b, c cyclically from corner k,
   u = unit(b - a), w = unit(u x (c - a)), v = unit(w x u), R = [u v w] as columns.
3. q = R^T (p - a) for every hull vertex p; lo / hi = per-axis min / max; extent = hi - lo; volume = extent0 * extent1 * extent2;
   center = a + R (lo + hi) / 2.
4. the box is the candidate of least volume; equal volumes go to the lowest candidate.
5. `enlarged(m)` adds 2 m to every extent.
6. p is inside when |(p - center) . R[:, k]| <= extent_k / 2 for k = 0, 1, 2 (inclusive).

ONE deliberate difference from Open3D: it tries one edge per triangle, in the vertex order Qhull happens to emit, which no other hull
code reproduces.  Here all three edges are tried: the candidate set depends on the hull alone, and the box is never larger than
Open3D's.

    points (device) -> ss_obb_extremes: rows of the largest / smallest projection along 512 directions      (csrc/obb.hip)
      -> convex_hull of those <= 1,024 points (host, numpy fp64) -> its planes -> ss_obb_filter: a row strictly inside that polytope is
         no hull vertex -> ss_pc_compact_scan / ss_pc_compact -> ss_gather_rows: the few rows that may be hull vertices
      -> convex_hull of the survivors (host) -> ss_obb_search: 3 T candidates x H hull vertices -> the box (15 doubles)
    Gaussians (device) -> ss_obb_within -> ss_pc_compact_scan / ss_pc_compact: the ascending rows inside

The hull is an incremental (quickhull) one in numpy: it sees the survivors of the filter, not the scan.  A point within 1e-12 of the
cloud's extent of the current hull is not inserted.  Points closer than 1e-9 of the extent to one plane span no volume (ValueError).
There is no CPU path for the passes over all points."""
import numpy as np
import torch

from .. import native as nv

N_DIRECTIONS = 512
HULL_TOL = 1e-12          # x the cloud's extent: a point this close to the hull is not a new vertex
FLAT_TOL = 1e-9           # x the cloud's extent: a cloud this thin spans no volume
FILTER_TOL = 1e-9         # x the cloud's extent: the filter drops a row only when it is this far below every plane
_DIRS = {}


class OrientedBox:
    """center (3,), R (3, 3) with the axes as columns, extent (3,): fp64 numpy arrays"""

    def __init__(self, center, R, extent):
        self.center = np.array(center, dtype=np.float64).reshape(3)
        self.R = np.array(R, dtype=np.float64).reshape(3, 3)
        self.extent = np.array(extent, dtype=np.float64).reshape(3)

    @property
    def volume(self):
        return float(self.extent[0] * self.extent[1] * self.extent[2])

    def enlarged(self, margin):
        """the box grown by `margin` on every side: centre and axes stay"""
        return OrientedBox(self.center, self.R, self.extent + 2.0 * float(margin))

    def contains(self, points):
        """(n,) bool for points (n, 3): step 6 of the module docstring in numpy"""
        d = np.asarray(points).astype(np.float64).reshape(-1, 3) - self.center
        q = np.stack([(d[:, 0] * self.R[0, k] + d[:, 1] * self.R[1, k]) + d[:, 2] * self.R[2, k] for k in range(3)], axis=1)
        return np.all(np.abs(q) <= self.extent * 0.5, axis=1)

    def as15(self):
        return np.concatenate([self.center, self.R.reshape(-1), self.extent])

    def __repr__(self):
        return f"OrientedBox(center={self.center.tolist()}, extent={self.extent.tolist()})"


# ---- host side: the hull of a few thousand points -------------------------------------------------------------------------------------
def _face_planes(P, tris):
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    n = np.cross(b - a, c - a)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.sqrt((n * n).sum(axis=1))[:, None]
    return n, -(n * a).sum(axis=1)


def convex_hull(points64):
    """points (n, 3) -> (T, 3) int32 rows: the triangles of the convex hull, counter-clockwise seen from outside.  Quickhull in numpy
    fp64: every face keeps the points above it, the farthest of them is inserted next, the faces it sees are replaced by the fan from
    their horizon.  ValueError: fewer than 4 points, a coordinate that is not finite, or points that span no volume."""
    P = np.ascontiguousarray(points64, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError(f"convex_hull: points must be (n, 3), got {P.shape}")
    n = P.shape[0]
    if n < 4:
        raise ValueError(f"convex_hull: fewer than 4 points ({n})")
    if not np.isfinite(P).all():
        raise ValueError("convex_hull: a coordinate is not finite")
    span = P.max(axis=0) - P.min(axis=0)
    scale = float(span.max())
    if scale == 0.0:
        raise ValueError("convex_hull: the points span no volume (they coincide)")
    tol, flat = HULL_TOL * scale, FLAT_TOL * scale
    # the first tetrahedron: the ends of the longest axis, the point farthest from their line, the point farthest from that plane
    ax = int(np.argmax(span))
    i0, i1 = int(np.argmin(P[:, ax])), int(np.argmax(P[:, ax]))
    e = P[i1] - P[i0]
    off_line = np.sqrt((np.cross(P - P[i0], e) ** 2).sum(axis=1)) / np.sqrt((e * e).sum())
    i2 = int(np.argmax(off_line))
    if off_line[i2] <= flat:
        raise ValueError("convex_hull: the points span no volume (they lie on one line)")
    nrm = np.cross(e, P[i2] - P[i0])
    nrm /= np.sqrt((nrm * nrm).sum())
    height = (P - P[i0]) @ nrm
    i3 = int(np.argmax(np.abs(height)))
    if abs(height[i3]) <= flat:
        raise ValueError("convex_hull: the points span no volume (they lie in one plane)")
    a, b, c = (i0, i2, i1) if height[i3] > 0 else (i0, i1, i2)           # i3 lies below (a, b, c)
    cap = 256
    verts, normal, offset = np.zeros((cap, 3), dtype=np.int64), np.zeros((cap, 3)), np.zeros(cap)
    alive = np.zeros(cap, dtype=bool)
    outside, todo, nf = [], [], 0

    def add_faces(tri):
        nonlocal cap, verts, normal, offset, alive, nf
        m = tri.shape[0]
        while nf + m > cap:
            cap *= 2
            verts, normal = np.resize(verts, (cap, 3)), np.resize(normal, (cap, 3))
            offset, alive = np.resize(offset, cap), np.concatenate([alive, np.zeros(cap - alive.size, dtype=bool)])
        ids = np.arange(nf, nf + m)
        verts[ids] = tri
        normal[ids], offset[ids] = _face_planes(P, tri)
        alive[ids] = True
        outside.extend([None] * m)
        nf += m
        return ids

    def assign(pts, ids):
        """every point of pts goes to the face of ids it is farthest above; a point above none of them is inside the hull for good"""
        if pts.size == 0:
            return
        D = P[pts] @ normal[ids].T + offset[ids]
        D = np.where(np.isnan(D), -np.inf, D)
        best = np.argmax(D, axis=1)
        keep = D[np.arange(pts.size), best] > tol
        for j, f in enumerate(ids):
            mine = pts[keep & (best == j)]
            if mine.size:
                outside[f] = mine
                todo.append(int(f))

    first = add_faces(np.array([(a, b, c), (b, a, i3), (c, b, i3), (a, c, i3)], dtype=np.int64))
    rest = np.ones(n, dtype=bool)
    rest[[i0, i1, i2, i3]] = False
    assign(np.flatnonzero(rest), first)
    while todo:
        f = todo.pop()
        if not alive[f] or outside[f] is None:
            continue
        pts = outside[f]
        p = int(pts[np.argmax(P[pts] @ normal[f] + offset[f])])
        vis = alive[:nf] & ((normal[:nf] @ P[p] + offset[:nf]) > tol)
        vis[f] = True
        vid = np.flatnonzero(vis)
        V = verts[vid]
        ea, eb = V.reshape(-1), V[:, [1, 2, 0]].reshape(-1)               # the directed edges a -> b of the faces p sees
        horizon = ~np.isin(eb * n + ea, ea * n + eb)                      # ... whose other side p does not see
        gathered = np.concatenate([outside[v] for v in vid if outside[v] is not None])
        alive[vid] = False
        for v in vid:
            outside[v] = None
        ids = add_faces(np.stack([ea[horizon], eb[horizon], np.full(int(horizon.sum()), p, dtype=np.int64)], axis=1))
        assign(gathered[gathered != p], ids)
    return verts[:nf][alive[:nf]].astype(np.int32)


# ---- device side -----------------------------------------------------------------------------------------------------------------------
def _points(points, device, name="points", at_least=0):
    """(n, 3) float32 numpy array or GPU tensor -> contiguous GPU tensor; every refusal that needs only the array: before the device"""
    if isinstance(points, torch.Tensor):
        if device is None and not points.is_cuda:
            raise RuntimeError(f"oriented_box: {name} must be a GPU tensor or a numpy array; there is no CPU fallback")
        t = points
    else:
        t = torch.from_numpy(np.ascontiguousarray(points))
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise ValueError(f"oriented_box: {name} must be (n, 3) float32, got {tuple(t.shape)} {t.dtype}")
    if t.shape[0] < at_least:
        raise ValueError(f"oriented_box: fewer than {at_least} points ({t.shape[0]})")
    dev = torch.device("cuda" if device is None else device) if not t.is_cuda or device is not None else t.device
    if dev.type != "cuda":
        raise RuntimeError("oriented_box: the passes over the points run on the GPU (device='cuda'); there is no CPU fallback")
    return t.to(dev).contiguous()


def directions(k=N_DIRECTIONS):
    """(k, 3) fp64 unit vectors: the axes and diagonals first (their extremes give the cloud's extent), then a Fibonacci lattice on the
    sphere.  Largest and smallest projection are both taken, so k directions look 2 k ways."""
    if k not in _DIRS:
        fixed = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)], dtype=np.float64)
        i = np.arange(k - len(fixed), dtype=np.float64) + 0.5
        z = 1.0 - 2.0 * i / (k - len(fixed))
        phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
        r = np.sqrt(1.0 - z * z)
        d = np.concatenate([fixed, np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)])
        _DIRS[k] = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return _DIRS[k]


def _all_rows(n, dev):
    return torch.arange(n, dtype=torch.int32, device=dev)


def hull_candidates(points, filter_above=4096, device=None):
    """-> the ascending rows (int32, device) of points (N, 3) float32 that may be vertices of its convex hull.  At or below filter_above
    points: all rows.  Above: the extremes along `directions()`, the hull of those, and every row that is not strictly inside it.
    The filter never removes a hull vertex; where the polytope of the extremes cannot be built it removes nothing."""
    pts = _points(points, device)
    n = pts.shape[0]
    if n <= int(filter_above) or n < 4:
        return _all_rows(n, pts.device)
    with torch.cuda.device(pts.device):
        rows_max, rows_min = nv.obb_extremes(pts, torch.from_numpy(directions()).to(pts.device))
        ext = np.unique(torch.cat([rows_max, rows_min]).cpu().numpy())
        ext = ext[ext >= 0].astype(np.int32)
        if ext.size < 4:
            return _all_rows(n, pts.device)
        corner = nv.gather_rows(pts, torch.from_numpy(ext).to(pts.device)).cpu().numpy().astype(np.float64)
        try:
            tris = convex_hull(corner)
        except ValueError:
            return _all_rows(n, pts.device)
        normal, offset = _face_planes(corner, tris)
        extent = float((corner.max(axis=0) - corner.min(axis=0)).max())
        tol = FILTER_TOL * extent
        # the planes must bound a convex body that holds its own corners: anything else filters nothing
        if not (np.isfinite(normal).all() and np.isfinite(offset).all()) or (corner @ normal.T + offset).max() > tol:
            return _all_rows(n, pts.device)
        planes = torch.from_numpy(np.ascontiguousarray(np.concatenate([normal, offset[:, None]], axis=1))).to(pts.device)
        return nv.bitmap_rows(nv.obb_filter(pts, planes, tol), n)


def minimal_oriented_box(points, device=None, filter_above=4096):
    """points (N, 3) float32 (numpy or GPU tensor) -> OrientedBox of least volume among the frames of all hull edges (module docstring).
    ValueError: fewer than 4 points, or points that span no volume."""
    pts = _points(points, device, at_least=4)
    n = pts.shape[0]
    with torch.cuda.device(pts.device):
        rows = hull_candidates(pts, filter_above)
        few = (pts if rows.numel() == n else nv.gather_rows(pts, rows)).cpu().numpy().astype(np.float64)
        tris = convex_hull(few)
        used, tris = np.unique(tris, return_inverse=True)
        verts = torch.from_numpy(np.ascontiguousarray(few[used])).to(pts.device)
        tris = torch.from_numpy(np.ascontiguousarray(tris.reshape(-1, 3).astype(np.int32))).to(pts.device)
        _, best, box = nv.obb_search(verts, tris)
        host = torch.cat([box, best.to(torch.float64)]).cpu().numpy()       # the one read
    if host[15] < 0:
        raise ValueError("minimal_oriented_box: the points span no volume")
    return OrientedBox(host[0:3], host[3:12], host[12:15])


def points_within_box(box, points, device=None):
    """-> the ascending rows (int32, device) of points (M, 3) float32 inside `box` (step 6 of the module docstring, inclusive)"""
    pts = _points(points, device)
    m = pts.shape[0]
    if m == 0:
        return torch.empty(0, dtype=torch.int32, device=pts.device)
    with torch.cuda.device(pts.device):
        return nv.bitmap_rows(nv.obb_within(pts, box.as15()), m)
