#!/usr/bin/env python
"""One synthetic scan-sized ScanNet++ scene (default a 1000 x 1000 lattice: 1,000,000 vertices, 1,996,002 faces, 15-byte vertex records,
13-byte face records, about 20,000 segments, 1,000 annotated objects that overlap) written to a temporary folder with its two json files
and read back page-cached, converted to coord / color / normal / segment / instance in two forms:

  numpy   the reference-shaped form: the blocks viewed through structured dtypes, the vertex normals in Open3D's definition as fp64
          numpy with a sequential `np.add.at` (Open3D itself is compiled code: this column says what numpy takes, not what Open3D
          takes), and the label loop of preprocess_scannetpp.py as it stands: one `np.isin` over all vertices per annotated object.
          Timed ONCE (it takes seconds), split into its three parts.
  device  pointcept_api.scannetpp_mesh: load_ply_mesh, mesh_vertex_normals_o3d (face cross products, radix argsort, partition, run
          walk in fp64), the json files, first_groups, multilabels (histogram, group sizes, rows), and the copies back to the host.
          Run --repeats times after a warm-up run, timed with a host clock around work that ends in a device synchronise; its stages
          are also timed on their own the same way.

  kernels each new kernel alone on resident data: --iters back-to-back launches between one HIP event pair, median of 7 windows, with
          the bytes the kernel has to move (stated at `kernel_bytes`) per second as a share of the 8 TB/s peak.

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
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE = np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])
CLASSES = ["wall", "ceiling", "floor", "table", "door", "ceiling lamp", "cabinet", "blinds", "curtain", "chair"]


def median(v):
    return sorted(v)[len(v) // 2]


def write_scene(root, side, n_groups, seed=0):
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
    scans = os.path.join(root, "data", "scene", "scans")
    os.makedirs(scans)
    mesh = os.path.join(scans, "mesh_aligned_0.05.ply")
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join(f"property {'float' if k in 'xyz' else 'uchar'} {k}\n" for k in VERTEX.names)
            + "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f))
    with open(mesh, "wb") as out:
        out.write(head.encode())
        out.write(v.tobytes())
        out.write(f.tobytes())
    cells = max(1, side // 141)                                          # patches of cells x cells vertices: about 20,000 segments at side 1000
    per_row = (side + cells - 1) // cells
    seg_indices = ((gy // cells) * per_row + gx // cells).reshape(-1) * 3 + 1                   # sparse ids
    n_seg = per_row * per_row
    groups = []
    for k in range(n_groups):                                            # 24 to 40 segments each, drawn anywhere: a segment meets 0 to 5 groups
        segs = g.choice(n_seg, int(g.integers(24, 41)), replace=False) * 3 + 1
        label = CLASSES[k % len(CLASSES)] if k % 9 else "object"        # every ninth label is outside the class list
        groups.append(dict(id=k + 1, objectId=k + 1, segments=[int(s) for s in segs], label=label))
    segs, anno = os.path.join(scans, "segments.json"), os.path.join(scans, "segments_anno.json")
    with open(segs, "w") as out:
        json.dump(dict(scene_id="scene", segIndices=seg_indices.tolist()), out)
    with open(anno, "w") as out:
        json.dump(dict(scene_id="scene", segGroups=groups), out)
    return mesh, segs, anno, len(head), n, len(f), n_seg


def numpy_form(mesh, offset, n, n_faces, segs, anno, class2idx, ignore_index=-1):
    """-> (arrays, seconds of read / normals / labels)"""
    t0 = time.perf_counter()
    with open(mesh, "rb") as f:
        raw = f.read()
    vertex = np.frombuffer(raw, dtype=VERTEX, count=n, offset=offset)
    faces = np.frombuffer(raw, dtype=FACE, count=n_faces, offset=offset + n * VERTEX.itemsize)["vertex_indices"].astype(np.int64)
    vertices = np.stack([vertex["x"], vertex["y"], vertex["z"]], 1).astype(np.float64)
    colors = np.stack([vertex["red"], vertex["green"], vertex["blue"]], 1) / 255.0
    out = dict(coord=vertices.astype(np.float32), color=(colors * 255).astype(np.uint8))
    t1 = time.perf_counter()
    u, w = vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]]
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    acc = np.zeros_like(vertices)
    np.add.at(acc, faces.reshape(-1), np.repeat(c, 3, axis=0))
    z = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
    acc = np.where((z > 0)[:, None], acc / np.where(z > 0, np.sqrt(z), 1)[:, None], acc)
    out["normal"] = acc.astype(np.float32)
    t2 = time.perf_counter()
    with open(segs) as f:
        seg_indices = np.array(json.load(f)["segIndices"], dtype=np.uint32)
    with open(anno) as f:
        seg_groups = json.load(f)["segGroups"]
    semantic_gt = np.ones((n, 3), dtype=np.int16) * ignore_index
    instance_gt = np.ones((n, 3), dtype=np.int16) * ignore_index
    instance_size = np.ones((n, 3), dtype=np.int16) * np.inf
    labels_used = np.zeros(n, dtype=np.int16)
    for instance in seg_groups:                                          # parse_scene's loop
        label_index = class2idx.get(instance["label"], ignore_index)
        if label_index == ignore_index:
            continue
        mask = np.isin(seg_indices, instance["segments"]) & (labels_used < 3)
        size = mask.sum()
        if size == 0:
            continue
        label_position = labels_used[mask]
        semantic_gt[mask, label_position] = label_index
        instance_gt[mask, label_position] = instance["objectId"]
        instance_size[mask, label_position] = size
        labels_used[mask] += 1
    mask = labels_used > 1
    if mask.sum() > 0:
        major = np.argmin(instance_size[mask], axis=1)
        for gt in (semantic_gt, instance_gt):
            first = gt[mask, major]
            gt[mask, major] = gt[:, 0][mask]
            gt[:, 0][mask] = first
    out.update(segment=semantic_gt, instance=instance_gt)
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def kernel_bytes(n, n_faces, n_seg_rows, n_groups):
    """the bytes each kernel has to move, from the shapes: inputs read once (a gathered row counts where it is read), outputs written once"""
    return {
        "ss_mesh_face_cross_f64": 12 * n_faces + 36 * n_faces + 24 * n_faces,        # faces, three gathered vertices, the fp64 row
        "ss_mesh_vertex_normals_f64": 4 * 3 * n_faces + 24 * 3 * n_faces + 8 * n + 12 * n,   # order, a cross row per corner, run tables, normals
        "ss_spp_segment_hist": 4 * n + 4 * n,                                        # ids, one counter update per vertex
        "ss_spp_group_sizes": 16 * n_seg_rows + 4 * n_groups,
        "ss_spp_labels": 4 * n + 12 * n + 12 * n,                                    # ids, the segment's slots, two (n, 3) int16 outputs
    }


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
    ap.add_argument("--side", type=int, default=1000, help="vertices along one side of the lattice")
    ap.add_argument("--groups", type=int, default=1000, help="annotated objects")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        mesh, segs, anno, offset, n, n_faces, n_seg = write_scene(tmp, args.side, args.groups)
        class2idx = {name: k for k, name in enumerate(CLASSES)}
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_scannetpp: no GPU: nothing was measured")
        ref, numpy_s = numpy_form(mesh, offset, n, n_faces, segs, anno, class2idx)
        print("numpy form: read %.3f s, normals %.3f s, labels %.3f s" % numpy_s, flush=True)

        from scenesplat_amd import native as nv
        from scenesplat_amd.pointcept_api import scannetpp_mesh as sp
        stage = {}

        def host_labels():
            with open(segs) as f:
                seg_indices = np.array(json.load(f)["segIndices"])
            with open(anno) as f:
                return seg_indices, sp.first_groups(json.load(f)["segGroups"], class2idx)

        def device_form(clock=False):
            def lap(name, t0):
                if clock:
                    torch.cuda.synchronize()
                    stage.setdefault(name, []).append(time.perf_counter() - t0)
                return time.perf_counter()
            t = time.perf_counter()
            m = sp.load_ply_mesh(mesh, "cuda")
            t = lap("load_ply_mesh", t)
            normal = sp.mesh_vertex_normals_o3d(m["coord"], m["faces"])
            t = lap("mesh_vertex_normals_o3d", t)
            seg_indices, groups = host_labels()
            t = lap("json + first_groups (host)", t)
            segment, instance = sp.multilabels(seg_indices, groups, "cuda")
            t = lap("multilabels (upload + 3 kernels)", t)
            out = dict(coord=m["coord"].cpu().numpy(), color=m["color"].cpu().numpy(), normal=normal.cpu().numpy(),
                       segment=segment.cpu().numpy(), instance=instance.cpu().numpy())
            lap("copies to the host", t)
            return out, m

        dev, m = device_form()
        for k in ("coord", "color", "normal", "segment", "instance"):
            assert ref[k].dtype == dev[k].dtype and ref[k].tobytes() == dev[k].tobytes(), k
        used = (ref["segment"] >= 0).sum(1)
        print("rows with 0 / 1 / 2 / 3 labels:", [int((used == k).sum()) for k in range(4)], flush=True)
        total = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_form()
            total.append(time.perf_counter() - t0)
        for _ in range(args.repeats):
            device_form(clock=True)

        # ---- the new kernels alone -----------------------------------------------------------------------------------------------------
        coord, faces = m["coord"], m["faces"]
        lib, p, st = nv.lib(), nv._p, nv._stream
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        cross = torch.empty((n_faces, 3), dtype=torch.float64, device="cuda")
        ms = {}
        ms["ss_mesh_face_cross_f64"] = event_windows(lambda: lib.ss_mesh_face_cross_f64(p(coord), p(faces), n_faces, n, p(cross), p(status), st()), args.iters)
        order, idx_ptr, head, n_runs = nv._mesh_incidence(faces, n)
        normal = torch.zeros((n, 3), device="cuda")
        ms["ss_mesh_vertex_normals_f64"] = event_windows(lambda: lib.ss_mesh_vertex_normals_f64(p(cross), p(faces), p(order), p(idx_ptr), p(head), p(n_runs),
                                                                                                 n_faces, n, p(normal), st()), args.iters)
        seg_indices, groups = host_labels()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
        seg, first3, tl, to = up(seg_indices), up(groups["first3"]), up(groups["table_label"]), up(groups["table_object"])
        S, G = first3.shape[0], tl.numel()
        count, size = torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(G, dtype=torch.int32, device="cuda")
        ms["ss_spp_segment_hist"] = event_windows(lambda: lib.ss_spp_segment_hist(p(seg), n, S, p(count), st()), args.iters)
        ms["ss_spp_group_sizes"] = event_windows(lambda: lib.ss_spp_group_sizes(p(first3), p(count), S, G, p(size), st()), args.iters)
        size = nv.spp_group_sizes(first3, nv.spp_segment_hist(seg, S), G)
        o1, o2 = (torch.empty((n, 3), dtype=torch.int16, device="cuda") for _ in range(2))
        ms["ss_spp_labels"] = event_windows(lambda: lib.ss_spp_labels(p(seg), n, None, p(first3), S, p(tl), p(to), p(size), G, n, -1, p(o1), p(o2), st()), args.iters)
        assert int(status.item()) == 0 and o1.cpu().numpy().tobytes() == ref["segment"].tobytes()
        nbytes = kernel_bytes(n, n_faces, S, G)

    print("| form | total s | read / decode | normals | labels |")
    print("|---|---|---|---|---|")
    print("| numpy | %.3f | %.3f | %.3f | %.3f |" % ((sum(numpy_s),) + numpy_s))
    print("| device | %.4f | | | |" % median(total))
    print("| device stage | ms |")
    print("|---|---|")
    for k, v in stage.items():
        print("| %s | %.2f |" % (k, median(v) * 1e3))
    print("| kernel | ms | GB/s of bytes moved | share of 8 TB/s |")
    print("|---|---|---|---|")
    for k, t in ms.items():
        print("| %s | %.4f | %.0f | %.3f |" % (k, t, nbytes[k] / t / 1e6, nbytes[k] / (t * 1e-3) / PEAK_BYTES_PER_S))
    print(json.dumps(dict(n=n, n_faces=n_faces, n_groups=args.groups, first3_rows=S, numpy_s=dict(zip(("read", "normals", "labels"), numpy_s)),
                          device_s=median(total), device_stage_ms={k: median(v) * 1e3 for k, v in stage.items()},
                          kernels={k: dict(ms=t, bytes_moved=nbytes[k], frac_of_peak=nbytes[k] / (t * 1e-3) / PEAK_BYTES_PER_S) for k, t in ms.items()},
                          speedup=sum(numpy_s) / median(total))))


if __name__ == "__main__":
    main()
