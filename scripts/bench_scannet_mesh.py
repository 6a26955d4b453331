#!/usr/bin/env python
"""One synthetic scan-sized ScanNet scene (default a 500 x 500 lattice: 250,000 vertices, 498,002 faces, 16-byte vertex records, 13-byte
face records, 3,000 segments in 60 annotated objects) written to a temporary folder with its two json files and read back page-cached,
converted to coord / color / normal / segment20 / segment200 / instance in two forms:

  numpy   the reference-shaped form, restated: the blocks viewed through structured dtypes (what plyfile hands out), `vertex_normal` with
          its Python loop over the faces (`nv[face[i]] += nf[i]`), one `np.isin` over all vertices per annotated object.  Timed ONCE (it
          takes seconds), split into its three parts.
  device  pointcept_api.scannet_mesh: load_ply_mesh (file -> pinned -> device, one decode launch per block), mesh_vertex_normals
          (face terms, radix argsort, partition, run walk), the json files, group_tables, mesh_labels, and the copies back to the host.
          Run --repeats times after a warm-up run, timed with a host clock around work that ends in a device synchronise; its stages
          are also timed on their own the same way.

  kernels each kernel alone on resident data: --iters back-to-back launches between one HIP event pair, median of 7 windows.  For the
          two decode kernels the bytes of RECORDS READ per second as a share of the 8 TB/s peak, at the scan's size (4 MB and 6.5 MB:
          a launch, not a bandwidth figure) and over --tile copies of the blocks (beyond the 256 MiB Infinity Cache).

The two forms are compared byte for byte before anything is timed.  Needs a GPU: there is no CPU path.  Prints markdown tables and one
JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

PEAK_BYTES_PER_S = 8e12
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
FACE = np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])
CATEGORIES = [("wall", 1, 1), ("chair", 2, 5), ("floor", 3, 2), ("table", 4, 7), ("door", 5, 8), ("couch", 6, 6), ("lamp", 35, 35), ("rod", 900, 40)]
IDS20 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
IDS200 = [1, 2, 3, 4, 5, 6, 35]


def median(v):
    return sorted(v)[len(v) // 2]


def write_scene(root, side, seed=0):
    """-> (scene folder, mesh path, segs path, aggregation path, tsv path)"""
    g = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    n = side * side
    v = np.zeros(n, dtype=VERTEX)
    jitter = g.uniform(-0.004, 0.004, (n, 3))
    v["x"], v["y"] = gx.reshape(-1) * 0.02 + jitter[:, 0] + 0.5, gy.reshape(-1) * 0.02 + jitter[:, 1] + 0.5
    v["z"] = 0.05 * np.sin(gx.reshape(-1) * 0.05) + jitter[:, 2] + 1.0
    for c in ("red", "green", "blue"):
        v[c] = g.integers(0, 256, n)
    a = (gy[:-1, :-1] * side + gx[:-1, :-1]).reshape(-1)
    tri = np.concatenate([np.stack([a, a + 1, a + side], 1), np.stack([a + side, a + 1, a + side + 1], 1)])
    f = np.zeros(len(tri), dtype=FACE)
    f["count"], f["vertex_indices"] = 3, tri[g.permutation(len(tri))]
    scene_id = "scene0000_00"
    folder = os.path.join(root, "scans", scene_id)
    os.makedirs(folder)
    mesh = os.path.join(folder, scene_id + "_vh_clean_2.ply")
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join(f"property {'float' if k in 'xyz' else 'uchar'} {k}\n" for k in VERTEX.names)
            + "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f))
    with open(mesh, "wb") as out:
        out.write(head.encode())
        out.write(v.tobytes())
        out.write(f.tobytes())
    n_seg = 3000
    patch = (gy // max(1, side // 50)) * 60 + gx // max(1, side // 60)
    seg_indices = (patch.reshape(-1) % n_seg) * 3 + 1                    # sparse ids
    groups = [dict(id=k, objectId=k, segments=[int(s) * 3 + 1 for s in range(k * 40, k * 40 + 40)], label=CATEGORIES[k % len(CATEGORIES)][0])
              for k in range(60)]                                        # segments 2400.. stay without a group
    segs, agg = os.path.join(folder, scene_id + "_vh_clean_2.0.010000.segs.json"), os.path.join(folder, scene_id + ".aggregation.json")
    with open(segs, "w") as out:
        json.dump(dict(sceneId=scene_id, segIndices=seg_indices.tolist()), out)
    with open(agg, "w") as out:
        json.dump(dict(sceneId=scene_id, segGroups=groups), out)
    tsv = os.path.join(root, "labels.tsv")
    with open(tsv, "w") as out:
        out.write("id\traw_category\tcategory\tcount\tnyu40id\n" + "".join(f"{i}\t{name}\t{name}\t1\t{nyu}\n" for name, i, nyu in CATEGORIES))
    return folder, mesh, segs, agg, tsv, len(head), n, len(f)


def numpy_form(mesh, offset, n, n_faces, segs, agg, table):
    """read_plymesh, vertex_normal and the label loop of preprocess_scannet.py; -> (arrays, seconds of read / normals / labels)"""
    t0 = time.perf_counter()
    with open(mesh, "rb") as f:
        raw = f.read()
    vertex = np.frombuffer(raw, dtype=VERTEX, count=n, offset=offset)
    faces = np.stack(np.frombuffer(raw, dtype=FACE, count=n_faces, offset=offset + n * VERTEX.itemsize)["vertex_indices"], axis=0)
    coords = np.stack([vertex["x"], vertex["y"], vertex["z"]], 1)
    out = dict(coord=coords.astype(np.float32), color=np.stack([vertex["red"], vertex["green"], vertex["blue"]], 1).astype(np.uint8))
    t1 = time.perf_counter()
    v01 = coords[faces[:, 1]] - coords[faces[:, 0]]
    v02 = coords[faces[:, 2]] - coords[faces[:, 0]]
    vec = np.cross(v01, v02)
    length = np.sqrt(np.sum(vec ** 2, axis=1, keepdims=True)) + 1.0e-8
    nf = vec / length
    area = length * 0.5
    nf = nf * area
    nv = np.zeros_like(coords)
    for i in range(faces.shape[0]):
        nv[faces[i]] += nf[i]
    length = np.sqrt(np.sum(nv ** 2, axis=1, keepdims=True)) + 1.0e-8
    out["normal"] = (nv / length).astype(np.float32)
    t2 = time.perf_counter()
    with open(segs) as f:
        seg_indices = np.array(json.load(f)["segIndices"])
    with open(agg) as f:
        seg_groups = json.load(f)["segGroups"]
    s20, s200, inst = (np.ones(n, dtype=np.int16) * -1 for _ in range(3))
    for group in seg_groups:
        id200, id20 = table.get(group["label"], (0, 0))
        l20 = IDS20.index(id20) if id20 in IDS20 else -1
        l200 = IDS200.index(id200) if id200 in IDS200 else -1
        idx = np.where(np.isin(seg_indices, np.array(group["segments"])))[0]
        s20[idx], s200[idx], inst[idx] = l20, l200, group["id"]
    out.update(segment20=s20.astype(int), segment200=s200.astype(int), instance=inst.astype(int))
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def event_windows(run, iters, windows=7):
    """median over `windows` of the average time (ms) of `iters` back-to-back calls between one HIP event pair"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", type=int, default=500, help="vertices along one side of the lattice")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tile", type=int, default=96, help="copies of the two blocks in the bandwidth run of the decode kernels")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        folder, mesh, segs, agg, tsv, offset, n, n_faces = write_scene(tmp, args.side)
        table = {name: (i, nyu) for name, i, nyu in CATEGORIES}
        ref, numpy_s = numpy_form(mesh, offset, n, n_faces, segs, agg, table)
        print("numpy form: read %.3f s, normals %.3f s, labels %.3f s" % numpy_s, flush=True)

        import torch
        from scenesplat_amd import native as nv
        from scenesplat_amd.pointcept_api import scannet_mesh as sm
        if not torch.cuda.is_available():
            raise SystemExit("bench_scannet_mesh: no GPU: nothing was measured")
        tables = sm.scannet_label_tables(tsv, IDS20, IDS200)
        stage = {}

        def device_form(clock=False):
            def lap(name, t0):
                if clock:
                    torch.cuda.synchronize()
                    stage.setdefault(name, []).append(time.perf_counter() - t0)
                return time.perf_counter()
            t = time.perf_counter()
            m = sm.load_ply_mesh(mesh, "cuda")
            t = lap("load_ply_mesh", t)
            normal = sm.mesh_vertex_normals(m["coord"], m["faces"], "pc")
            t = lap("mesh_vertex_normals", t)
            seg_indices, groups = sm._scene_labels(segs, agg, tables, n)
            t = lap("json + group_tables (host)", t)
            labels = sm.mesh_labels(seg_indices, groups, torch.int64, "cuda")
            t = lap("mesh_labels (upload + kernel)", t)
            out = dict(coord=m["coord"].cpu().numpy(), color=m["color"].cpu().numpy(), normal=normal.cpu().numpy())
            out.update((k, v.cpu().numpy()) for k, v in zip(("segment20", "segment200", "instance"), labels))
            lap("copies to the host", t)
            return out, m

        dev, m = device_form()
        for k in ("coord", "color", "normal", "segment20", "segment200", "instance"):
            assert ref[k].dtype == dev[k].dtype and ref[k].tobytes() == dev[k].tobytes(), k
        total = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_form()
            total.append(time.perf_counter() - t0)
        for _ in range(args.repeats):
            device_form(clock=True)

        # ---- the kernels alone ---------------------------------------------------------------------------------------------------------
        with open(mesh, "rb") as f:
            raw = f.read()
        vbytes, fbytes = n * VERTEX.itemsize, n_faces * FACE.itemsize
        vblock = torch.frombuffer(bytearray(raw[offset:offset + vbytes]), dtype=torch.uint8).cuda()
        fblock = torch.frombuffer(bytearray(raw[offset + vbytes:offset + vbytes + fbytes]), dtype=torch.uint8).cuda()
        coord, color, faces = m["coord"], m["color"], m["faces"]
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        offs = [0, 4, 8, 12, 13, 14]
        kernels = {}
        kernels["ss_mesh_decode_vertices"] = (event_windows(lambda: nv.mesh_decode_vertices(vblock, n, 16, offs, coord, color), args.iters), vbytes)
        kernels["ss_mesh_decode_faces"] = (event_windows(lambda: nv.mesh_decode_faces(fblock, n_faces, n, faces, status), args.iters), fbytes)
        lib, p, st = nv.lib(), nv._p, nv._stream
        terms = torch.empty((n_faces, 3), device="cuda")
        kernels["ss_mesh_face_terms"] = (event_windows(lambda: lib.ss_mesh_face_terms(p(coord), p(faces), n_faces, n, 0, p(terms), p(status), st()), args.iters), None)
        keys = faces.view(1, 3 * n_faces).to(torch.int64)
        bits = max(1, (n - 1).bit_length())
        kernels["ss_argsort_i64 (3F keys)"] = (event_windows(lambda: nv.argsort_i64(keys, bits, want_inverse=False, want_sorted=False), args.iters), None)
        order, _, _ = nv.argsort_i64(keys, bits, want_inverse=False, want_sorted=False)
        kernels["ss_pool_partition"] = (event_windows(lambda: nv.pool_partition(keys.view(-1), order.view(-1), 0), args.iters), None)
        _, idx_ptr, head, n_runs = nv.pool_partition(keys.view(-1), order.view(-1), 0)
        normal = torch.zeros((n, 3), device="cuda")
        kernels["ss_mesh_vertex_normals"] = (event_windows(lambda: lib.ss_mesh_vertex_normals(p(terms), p(faces), p(order), p(idx_ptr), p(head), p(n_runs), n_faces,
                                                                                                n, 0, p(normal), st()), args.iters), None)
        seg_indices, groups = sm._scene_labels(segs, agg, tables, n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
        lt = [up(seg_indices), up(groups["seg_to_group"]), up(groups["table20"]), up(groups["table200"]), up(groups["table_instance"])]
        kernels["ss_mesh_labels (int64)"] = (event_windows(lambda: nv.mesh_labels(*lt, torch.int64), args.iters), None)
        # beyond the Infinity Cache: the same records `tile` times over
        big_v, big_f = vblock.repeat(args.tile), fblock.repeat(args.tile)
        bc, bcol = torch.empty((args.tile * n, 3), device="cuda"), torch.empty((args.tile * n, 3), dtype=torch.uint8, device="cuda")
        bf = torch.empty((args.tile * n_faces, 3), dtype=torch.int32, device="cuda")
        it = max(2, args.iters // 4)
        kernels[f"ss_mesh_decode_vertices x{args.tile}"] = (event_windows(lambda: nv.mesh_decode_vertices(big_v, args.tile * n, 16, offs, bc, bcol), it), args.tile * vbytes)
        kernels[f"ss_mesh_decode_faces x{args.tile}"] = (event_windows(lambda: nv.mesh_decode_faces(big_f, args.tile * n_faces, n, bf, status), it), args.tile * fbytes)
        assert int(status.item()) == 0

    print("| form | total s | read / decode | normals | labels |")
    print("|---|---|---|---|---|")
    print("| numpy | %.3f | %.3f | %.3f | %.3f |" % ((sum(numpy_s),) + numpy_s))
    print("| device | %.4f | | | |" % median(total))
    print("| device stage | ms |")
    print("|---|---|")
    for k, v in stage.items():
        print("| %s | %.2f |" % (k, median(v) * 1e3))
    print("| kernel | ms | GB/s of records read | share of 8 TB/s |")
    print("|---|---|---|---|")
    for k, (ms, nbytes) in kernels.items():
        if nbytes is None:
            print("| %s | %.4f | | |" % (k, ms))
        else:
            print("| %s | %.4f | %.0f | %.3f |" % (k, ms, nbytes / ms / 1e6, nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S))
    print(json.dumps(dict(n=n, n_faces=n_faces, numpy_s=dict(zip(("read", "normals", "labels"), numpy_s)), device_s=median(total),
                          device_stage_ms={k: median(v) * 1e3 for k, v in stage.items()},
                          kernels={k: dict(ms=ms, bytes_read=b, frac_of_peak=None if b is None else b / (ms * 1e-3) / PEAK_BYTES_PER_S) for k, (ms, b) in kernels.items()},
                          speedup=sum(numpy_s) / median(total))))


if __name__ == "__main__":
    main()
