#!/usr/bin/env python
"""The oriented-box pruning (`prune_box=0.25`) on two synthetic rooms: 250,000 vertices with 1,000,000 Gaussians and 1,000,000 vertices
with 4,000,000 Gaussians.  A room is a 6 x 4 x 2.5 m box, rotated, with the vertices on its six faces (1 cm noise); the Gaussians spread
to 1.5 x its extent.  Per room, in a child process of its own under a time limit (a room that fails ends the run):

  host     Qhull (scipy) on ALL vertices, the search over 3 T candidates x H hull vertices in numpy, the membership mask in numpy.
  device   pointcept_api.oriented_box: minimal_oriented_box(...).enlarged(0.25) and points_within_box, end to end from resident arrays
           to the kept rows, --repeats times after a warm-up, a host clock around work that ends in a device synchronise; then the same
           steps one by one.
  kernels  each entry point alone on resident data: --iters back-to-back launches between one HIP event pair, median of 7 windows; for
           the three passes over all rows the bytes read and written against the 8 TB/s peak.
  scene    (--room small only) preprocess_scannet_gs on a 250,000-vertex scan with a 1,000,000-Gaussian checkpoint, with prune_box=None
           (the path of the commit before the keyword existed, unchanged) and with 0.25, alternating.

The two forms must agree on the kept rows before anything is timed.  Needs a GPU: there is no CPU path.  Prints markdown tables and one
JSON line per room."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

PEAK_BYTES_PER_S = 8e12
ROOMS = dict(small=(250_000, 1_000_000), large=(1_000_000, 4_000_000))
ROOM = np.array([6.0, 4.0, 2.5])
MARGIN = 0.25


def median(v):
    return sorted(v)[len(v) // 2]


def room(n, m, seed=0):
    g = np.random.default_rng(seed)
    q, r = np.linalg.qr(g.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    p = (g.random((n, 3)) - 0.5) * ROOM
    face = g.integers(0, 6, n)
    axis, side = face // 2, (face % 2) * 2.0 - 1.0
    p[np.arange(n), axis] = side * ROOM[axis] * 0.5
    p += g.standard_normal(p.shape) * 0.01
    shift = g.standard_normal(3) * 2.0
    gs = (g.random((m, 3)) - 0.5) * ROOM * 1.5
    return (p @ q.T + shift).astype(np.float32), (gs @ q.T + shift).astype(np.float32)


def unit(x):
    return x / np.sqrt((x * x).sum(axis=1))[:, None]


def host_form(verts, gs):
    """-> (kept rows, box (center, R, extent), seconds of hull / search / mask, hull vertices)"""
    from scipy.spatial import ConvexHull
    t0 = time.perf_counter()
    p64 = verts.astype(np.float64)
    hull = ConvexHull(p64)
    t1 = time.perf_counter()
    tris, H = hull.simplices, p64[hull.vertices]
    k = np.arange(3)
    a = p64[tris[:, k].reshape(-1)]
    u = unit(p64[tris[:, (k + 1) % 3].reshape(-1)] - a)
    w = unit(np.cross(u, p64[tris[:, (k + 2) % 3].reshape(-1)] - a))
    v = unit(np.cross(w, u))
    lo, hi = [], []
    for r in (u, v, w):
        q = H @ r.T - (a * r).sum(axis=1)                                 # (H, 3 T)
        lo.append(q.min(axis=0)); hi.append(q.max(axis=0))
    lo, hi = np.stack(lo, 1), np.stack(hi, 1)
    best = int(np.argmin((hi - lo).prod(axis=1)))
    R = np.stack([u[best], v[best], w[best]], axis=1)
    center, extent = a[best] + R @ ((lo[best] + hi[best]) * 0.5), hi[best] - lo[best]
    t2 = time.perf_counter()
    rows = np.flatnonzero(np.all(np.abs((gs.astype(np.float64) - center) @ R) <= (extent + 2 * MARGIN) * 0.5, axis=1))
    t3 = time.perf_counter()
    return rows, (center, R, extent), (t1 - t0, t2 - t1, t3 - t2), hull.vertices.size


def event_windows(run, iters, windows=7):
    import torch
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            run()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / iters)
    return median(ms)


def scene_times(repeats):
    """preprocess_scannet_gs on one 250,000-vertex scene with a 1,000,000-Gaussian checkpoint: seconds without and with prune_box"""
    import bench_scannet_mesh as bsm
    from scenesplat_amd.pointcept_api import scannet_mesh as sm
    with tempfile.TemporaryDirectory() as tmp:
        folder, mesh, segs, agg, tsv, offset, n, n_faces = bsm.write_scene(tmp, 500)
        g = np.random.default_rng(1)
        names = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
        arr = np.zeros(1_000_000, dtype=np.dtype([(k, "<f4") for k in names]))
        for k in names:
            arr[k] = g.standard_normal(len(arr)).astype(np.float32)
        arr["x"], arr["y"] = g.uniform(-2.0, 13.0, len(arr)), g.uniform(-2.0, 13.0, len(arr))          # the scan spans 0.5 .. 10.5
        arr["z"] = g.uniform(0.0, 2.0, len(arr))
        ckpt = os.path.join(tmp, "gs", "scene0000_00", "ckpts")
        os.makedirs(ckpt)
        with open(os.path.join(ckpt, "point_cloud_30000.ply"), "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(arr) + "".join(f"property float {k}\n" for k in names)
                     + "end_header\n").encode() + arr.tobytes())
        lists = os.path.join(tmp, "train.txt")
        with open(lists, "w") as f:
            f.write("scene0000_00\n")
        times = {None: [], MARGIN: []}
        import contextlib
        import io
        import torch
        for rep in range(repeats + 1):
            for prune in (None, MARGIN):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()) as said:
                    done = sm.preprocess_scannet_gs(tmp, os.path.join(tmp, f"out{rep}_{prune}"), os.path.join(tmp, "gs"), tsv, bsm.IDS20, bsm.IDS200,
                                                    lists, lists, prune_box=prune)
                assert len(done) == 1, said.getvalue()
                if rep:
                    times[prune].append(time.perf_counter() - t0)
        kept = len(np.load(os.path.join(tmp, f"out1_{MARGIN}", "train", "scene0000_00", "coord.npy")))
    return median(times[None]), median(times[MARGIN]), kept


def run_room(name, repeats, iters):
    import torch
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import oriented_box as ob
    if not torch.cuda.is_available():
        raise SystemExit("bench_obb: no GPU: nothing was measured")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    n, m = ROOMS[name]
    verts, gs = room(n, m)
    host_rows, host_box, host_s, hull_vertices = host_form(verts, gs)
    print("%s: host form: hull %.3f s, search %.3f s, mask %.3f s (%d hull vertices)" % ((name,) + host_s + (hull_vertices,)), flush=True)
    verts_d, gs_d = torch.from_numpy(verts).cuda(), torch.from_numpy(gs).cuda()

    def device_form():
        box = ob.minimal_oriented_box(verts_d).enlarged(MARGIN)
        return box, ob.points_within_box(box, gs_d)

    box, rows = device_form()
    # the host form tries one edge per triangle in Qhull's order as well as all others here: the same candidate set, the same box
    assert abs(box.volume - np.prod(host_box[2] + 2 * MARGIN)) <= 1e-9 * box.volume, (box.volume, np.prod(host_box[2] + 2 * MARGIN))
    assert np.array_equal(rows.cpu().numpy(), host_rows)
    total = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, r = device_form()
        torch.cuda.synchronize()
        total.append(time.perf_counter() - t0)

    # ---- the same steps one by one ------------------------------------------------------------------------------------------------------
    stage = {}

    def lap(key, t0):
        torch.cuda.synchronize()
        stage.setdefault(key, []).append(time.perf_counter() - t0)
        return time.perf_counter()

    dirs = torch.from_numpy(ob.directions()).cuda()
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rows_max, rows_min = nv.obb_extremes(verts_d, dirs)
        ext = np.unique(torch.cat([rows_max, rows_min]).cpu().numpy()).astype(np.int32)
        corner = nv.gather_rows(verts_d, torch.from_numpy(ext).cuda()).cpu().numpy().astype(np.float64)
        t = lap("ss_obb_extremes + rows to the host", t)
        tris = ob.convex_hull(corner)
        normal, offset = ob._face_planes(corner, tris)
        t = lap("hull of the extremes (host)", t)
        planes = torch.from_numpy(np.ascontiguousarray(np.concatenate([normal, offset[:, None]], axis=1))).cuda()
        tol = ob.FILTER_TOL * float((corner.max(axis=0) - corner.min(axis=0)).max())
        survivors = nv.bitmap_rows(nv.obb_filter(verts_d, planes, tol), n)
        few = nv.gather_rows(verts_d, survivors).cpu().numpy().astype(np.float64)
        t = lap("ss_obb_filter + compaction + rows to the host", t)
        tris2 = ob.convex_hull(few)
        used, local = np.unique(tris2, return_inverse=True)
        t = lap("hull of the survivors (host)", t)
        hv, ht = torch.from_numpy(np.ascontiguousarray(few[used])).cuda(), torch.from_numpy(local.reshape(-1, 3).astype(np.int32)).cuda()
        _, best, box15 = nv.obb_search(hv, ht)
        host = torch.cat([box15, best.double()]).cpu().numpy()
        t = lap("ss_obb_search + the box to the host", t)
        big = ob.OrientedBox(host[0:3], host[3:12], host[12:15]).enlarged(MARGIN)
        kept = nv.bitmap_rows(nv.obb_within(gs_d, big.as15()), m)
        lap("ss_obb_within + compaction", t)
    assert np.array_equal(kept.cpu().numpy(), host_rows)

    # ---- the kernels alone -----------------------------------------------------------------------------------------------------------------
    kernels = {}
    kernels["ss_obb_extremes (512 directions)"] = (event_windows(lambda: nv.obb_extremes(verts_d, dirs), iters), n * 12)
    kernels[f"ss_obb_filter ({planes.shape[0]} planes)"] = (event_windows(lambda: nv.obb_filter(verts_d, planes, tol), iters), n * 12 + n // 8)
    kernels[f"ss_obb_search ({3 * ht.shape[0]} candidates x {hv.shape[0]} vertices)"] = (event_windows(lambda: nv.obb_search(hv, ht), iters), None)
    kernels["ss_obb_within"] = (event_windows(lambda: nv.obb_within(gs_d, big.as15()), iters), m * 12 + m // 8)
    bitmap = nv.obb_within(gs_d, big.as15())
    kernels["ss_pc_compact_scan + ss_pc_compact (Gaussians)"] = (event_windows(lambda: nv.bitmap_rows(bitmap, m), max(2, iters // 4)), None)

    print(f"### {name}: {n:,} vertices, {m:,} Gaussians: {ext.size} extremes, {survivors.numel()} survivors of the filter, {used.size} hull vertices, "
          f"{tris2.shape[0]} hull triangles, {kept.numel()} Gaussians kept")
    print("| form | total ms | hull | search | mask |")
    print("|---|---|---|---|---|")
    print("| host (Qhull on all vertices, numpy) | %.1f | %.1f | %.1f | %.1f |" % ((sum(host_s) * 1e3,) + tuple(s * 1e3 for s in host_s)))
    print("| device, end to end | %.1f | | | |" % (median(total) * 1e3))
    print("| device step | ms |")
    print("|---|---|")
    for k, v in stage.items():
        print("| %s | %.2f |" % (k, median(v) * 1e3))
    print("| kernel | ms | GB/s | share of 8 TB/s |")
    print("|---|---|---|---|")
    for k, (ms, nbytes) in kernels.items():
        print("| %s | %.4f | | |" % (k, ms) if nbytes is None else "| %s | %.4f | %.0f | %.3f |" % (k, ms, nbytes / ms / 1e6, nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S))
    result = dict(room=name, n=n, m=m, extremes=int(ext.size), survivors=int(survivors.numel()), hull_vertices=int(used.size),
                  kept=int(kept.numel()), host_s=dict(zip(("hull", "search", "mask"), host_s)), device_s=median(total),
                  device_step_ms={k: median(v) * 1e3 for k, v in stage.items()},
                  kernels={k: dict(ms=ms, bytes=b) for k, (ms, b) in kernels.items()})
    if name == "small":
        plain, pruned, kept_scene = scene_times(repeats)
        print("| preprocess_scannet_gs, 250,000 vertices + 1,000,000 Gaussians | s per scene |")
        print("|---|---|")
        print("| prune_box=None | %.3f |" % plain)
        print("| prune_box=0.25 (%d Gaussians kept) | %.3f |" % (kept_scene, pruned))
        result["scene_s"] = dict(plain=plain, pruned=pruned, kept=kept_scene)
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--room", choices=list(ROOMS), default=None, help="measure this room in this process (default: each room in a child process)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds a room may take")
    args = ap.parse_args()
    if args.room is not None:
        return run_room(args.room, args.repeats, args.iters)
    for name in ROOMS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--room", name, "--repeats", str(args.repeats),
               "--iters", str(args.iters)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"bench_obb: room '{name}' ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
