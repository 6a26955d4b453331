"""Writes tests/golden/oriented_box.npz: per cloud of tests/obb_cases.py the points, Qhull's triangles (scipy; oriented counter-clockwise
seen from outside), all 3 T candidate volumes and the winning box of the numpy restatement, 4,000 query points around the box and their
membership for the margin 0.25.  Run on the CPU:  python tests/golden/make_golden_oriented_box.py

It refuses to write unless, on the general-position clouds, the two smallest volumes are a relative 1e-6 apart and every query point
keeps 1e-8 from the faces of the enlarged box: the tests then compare every row."""
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import obb_cases as oc  # noqa: E402


def qhull_triangles(points64):
    hull = ConvexHull(points64)                                          # ('Qt' is always on: simplices are triangles)
    tris = hull.simplices.astype(np.int64)
    inner = points64[hull.vertices].mean(axis=0)
    a, b, c = points64[tris[:, 0]], points64[tris[:, 1]], points64[tris[:, 2]]
    flip = (np.cross(b - a, c - a) * (a - inner)).sum(axis=1) < 0         # the normal must point away from an inner point
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris.astype(np.int32)


def main():
    out = {}
    for case, spec in oc.CASES.items():
        points = oc.cloud(case)
        tris = qhull_triangles(points.astype(np.float64))
        verts, local, rows = oc.hull_vertices(points, tris)
        best, box, volumes = oc.restated_box(verts, local)
        order = np.sort(volumes[np.isfinite(volumes)])
        gap = (order[1] - order[0]) / order[0]
        q = oc.queries(box, spec["seed"])
        face = np.abs(np.abs(oc.box_coordinates(box, q)) - (box[12:15] + 2.0 * oc.MARGIN) * 0.5).min()
        mask = oc.inside(box, q, oc.MARGIN)
        print(f"{case}: {points.shape[0]} points, {rows.size} hull vertices, {tris.shape[0]} triangles, volume {order[0]:.9g}, "
              f"gap {gap:.3g}, least face distance {face:.3g}, {int(mask.sum())} of {q.shape[0]} queries inside")
        if case in oc.GENERAL:
            assert gap >= oc.MIN_VOLUME_GAP, (case, gap)
        assert face >= oc.MIN_FACE_DISTANCE, (case, face)
        assert 0 < mask.sum() < mask.size
        out.update({f"{case}.points": points, f"{case}.tris": tris, f"{case}.volumes": volumes, f"{case}.best": np.int32(best),
                    f"{case}.box": box, f"{case}.queries": q, f"{case}.mask": mask})
    np.savez_compressed(oc.GOLDEN, **out)
    print(f"{oc.GOLDEN}: {os.path.getsize(oc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
