#!/usr/bin/env python
"""One synthetic scene (default: a cloud of 1,000,000 labelled points on the walls and floor of a 15 m x 12 m x 3 m room, 20 chunks of
100,000 Gaussian centres each, drawn around 6 x 6 m windows of the same surfaces) from page-cached .npy files to pc_coord.npy /
pc_segment*.npy in every chunk folder, in three forms, stage by stage:

  host    the reference-shaped form: scipy's cKDTree over the cloud, per chunk `query(k=16, workers=16)`, the distance mask,
          np.unique, fancy indexing per asset, np.save.
  torch   one pointops.knn_query per chunk on the device (the grid is rebuilt per chunk), the fp32 distance mask and
          torch.unique(idx[mask]) per chunk, index_select per asset, one download per asset and chunk.
  device  pointcept_api.pc_labels.attach_point_cloud: one knn_query per batch, ss_pc_mark + ss_pc_compact, the grouped gather, one
          download per batch.

Stages: read (np.load), search (tree build + query | knn_query), select (mask + unique | mark + compact), gather (+ download), write
(np.save).  Each form runs --repeats times after one warm-up run; a stage is timed with a host clock around work that ends in a device
synchronise; the table shows the median run.  Before anything is timed the three forms' files are compared at the small --check-n size
(the torch form selects in fp32 like the device form but tests the limit in fp32; the host form selects in fp64: rows may differ at
near-ties, so the counts of differing chunks are printed, not asserted).

  gather  ss_chunk_gather_group alone over the (chunk, asset) problems of the device form: --iters relaunches between one HIP event
          pair, median of 7 windows; bytes = rows read + rows written + the int32 indices read, as a share of the 8 TB/s peak.

Needs a GPU: there is no CPU path.  Prints a markdown table and one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12
SPLIT, SCENE, CHUNK_SPLIT = "val", "scene0000_00", "val_grid1.0cm_chunk6x6_stride3x3"
K, LIMIT = 16, 0.25


def median(v):
    return sorted(v)[len(v) // 2]


def surface_points(g, n, lo, hi, jitter):
    """n points on the floor and the four walls of the room, inside the x / y window [lo, hi), `jitter` metres off the surface"""
    p = (lo + g.random((n, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    which = g.integers(0, 3, n)
    p[which == 0, 2] = 0                                                   # floor
    p[which == 1, 0] = np.where(g.random((which == 1).sum()) < 0.5, lo[0], hi[0])      # the window's x faces stand in for walls
    p[which == 2, 1] = np.where(g.random((which == 2).sum()) < 0.5, lo[1], hi[1])
    return (p + g.standard_normal((n, 3), dtype=np.float32) * np.float32(jitter)).astype(np.float32)


def write_scene(root, n_cloud, n_chunks, n_gauss, seed=0):
    g = np.random.default_rng(seed)
    src = os.path.join(root, "pc", SPLIT, SCENE)
    os.makedirs(src)
    cells = [(x, y) for x in range(0, 15, 3) for y in range(0, 12, 3)]
    per = -(-n_cloud // len(cells))
    cloud = np.concatenate([surface_points(g, per, np.float32([x, y, 0]), np.float32([x + 3, y + 3, 3]), 0.005) for x, y in cells])[:n_cloud]
    cloud = cloud[g.permutation(n_cloud)]
    raw = dict(coord=cloud, segment20=g.integers(-1, 20, n_cloud).astype(np.int16), segment200=g.integers(-1, 200, n_cloud).astype(np.int16),
               segment_nyu_160=g.integers(0, 160, n_cloud).astype(np.int32))
    for k, v in raw.items():
        np.save(os.path.join(src, k + ".npy"), v)
    origins = [(x, y) for x in range(0, 12, 3) for y in range(0, 9, 3)]
    for c in range(n_chunks):
        x, y = origins[c % len(origins)]
        d = os.path.join(root, "gs", CHUNK_SPLIT, f"{SCENE}_{c}")
        os.makedirs(d)
        pick = cloud[(cloud[:, 0] >= x) & (cloud[:, 0] < x + 6) & (cloud[:, 1] >= y) & (cloud[:, 1] < y + 6)]
        centres = pick[g.integers(0, len(pick), n_gauss)] + g.standard_normal((n_gauss, 3), dtype=np.float32) * np.float32(0.05)
        np.save(os.path.join(d, "coord.npy"), centres.astype(np.float32))
    return os.path.join(root, "gs"), os.path.join(root, "pc")


def chunk_dirs(gs_root):
    sub = os.path.join(gs_root, CHUNK_SPLIT)
    return [os.path.join(sub, f"{SCENE}_{c}") for c in range(len(os.listdir(sub)))]


def timed(prof, key, fn, *args, sync=False):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    if sync:
        torch.cuda.synchronize()
    prof[key] = prof.get(key, 0.0) + time.perf_counter() - t0
    return out


def load_inputs(gs_root, pc_root, prof):
    src = os.path.join(pc_root, SPLIT, SCENE)
    cloud = timed(prof, "read", np.load, os.path.join(src, "coord.npy"))
    segs = {f[:-4]: timed(prof, "read", np.load, os.path.join(src, f)) for f in sorted(os.listdir(src)) if f.startswith("segment")}
    chunks = [timed(prof, "read", np.load, os.path.join(d, "coord.npy")) for d in chunk_dirs(gs_root)]
    return cloud, segs, chunks


def save_outputs(d, coord, segs, prof):
    timed(prof, "write", np.save, os.path.join(d, "pc_coord.npy"), coord)
    for n, a in segs.items():
        timed(prof, "write", np.save, os.path.join(d, f"pc_{n}.npy"), a)


def host_form(gs_root, pc_root, prof):
    from scipy.spatial import cKDTree
    cloud, segs, chunks = load_inputs(gs_root, pc_root, prof)
    tree = timed(prof, "search", cKDTree, cloud)
    for d, xyz in zip(chunk_dirs(gs_root), chunks):
        dist, idx = timed(prof, "search", lambda: tree.query(xyz, k=K, workers=16))
        rows = timed(prof, "select", lambda: np.unique(idx[dist <= LIMIT]))
        coord, out = timed(prof, "gather", lambda: (cloud[rows], {n: a[rows] for n, a in segs.items()}))
        save_outputs(d, coord, out, prof)


def torch_form(gs_root, pc_root, prof):
    from scenesplat_amd import pointops
    cloud, segs, chunks = load_inputs(gs_root, pc_root, prof)
    dev = torch.device("cuda")
    cloud_d, segs_d = timed(prof, "upload", lambda: (torch.from_numpy(cloud).to(dev), {n: torch.from_numpy(a).to(dev) for n, a in segs.items()}), sync=True)
    off = torch.tensor([cloud.shape[0]], dtype=torch.int32, device=dev)
    for d, xyz in zip(chunk_dirs(gs_root), chunks):
        q = timed(prof, "upload", lambda: torch.from_numpy(xyz).to(dev), sync=True)
        idx, dist = timed(prof, "search", lambda: pointops.knn_query(K, cloud_d, off, q, torch.tensor([q.shape[0]], dtype=torch.int32, device=dev)), sync=True)
        rows = timed(prof, "select", lambda: torch.unique(idx[(dist <= LIMIT) & (idx >= 0)]).long(), sync=True)
        coord, out = timed(prof, "gather", lambda: (cloud_d[rows].cpu().numpy(), {n: a[rows].cpu().numpy() for n, a in segs_d.items()}), sync=True)
        save_outputs(d, coord, out, prof)


def device_form(gs_root, pc_root, prof):
    from scenesplat_amd.pointcept_api import pc_labels
    pc_labels.PROFILE = prof
    try:
        pc_labels.attach_point_cloud(gs_root, pc_root, k_neighbors=K, dist_limit=LIMIT, scene_level=())
    finally:
        pc_labels.PROFILE = None
    prof["select"] = prof.pop("mark_compact", 0.0)
    prof["gather"] = prof.get("gather", 0.0) + prof.pop("download", 0.0)


FORMS = dict(host=host_form, torch=torch_form, device=device_form)


def read_outputs(gs_root):
    return [{f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.startswith("pc_")} for d in chunk_dirs(gs_root)]


def compare(n_cloud, n_chunks, n_gauss):
    """the three forms at a small size -> (chunks where torch differs from device, chunks where host differs from device, kept rows)"""
    outs = {}
    for name, fn in FORMS.items():
        root = tempfile.mkdtemp(prefix="pc_attach_check_")
        try:
            gs_root, pc_root = write_scene(root, n_cloud, n_chunks, n_gauss, seed=1)
            fn(gs_root, pc_root, {})
            outs[name] = read_outputs(gs_root)
        finally:
            shutil.rmtree(root)

    def equal(a, b):
        return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)

    return (sum(not equal(a, b) for a, b in zip(outs["device"], outs["torch"])), sum(not equal(a, b) for a, b in zip(outs["device"], outs["host"])),
            sum(o["pc_coord.npy"].shape[0] for o in outs["device"]))


def gather_alone(gs_root, pc_root, iters):
    """the grouped gather of the device form's problems, relaunched on resident tables"""
    from scenesplat_amd import grouped, native as nv
    from scenesplat_amd.pointcept_api import pc_labels as pl
    cloud, segs, chunks = load_inputs(gs_root, pc_root, {})
    dev = torch.device("cuda", torch.cuda.current_device())
    keep, cloud_d, assets = pl._cloud_arena(cloud, segs, dev)
    M = cloud.shape[0]
    q = torch.from_numpy(np.concatenate(chunks)).to(dev)
    q_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
    q_offset = torch.from_numpy(q_off.astype(np.int32)).to(dev)
    from scenesplat_amd import pointops
    idx, _ = pointops.knn_query(K, cloud_d, torch.tensor([M], dtype=torch.int32, device=dev), q, q_offset[-1:])
    bitmap, _, _ = nv.pc_mark(cloud_d, q, q_offset, idx, LIMIT)
    tile_base, counts = nv.pc_compact_scan(bitmap, M)
    counts = counts.cpu().numpy().astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(counts)])
    rows = nv.pc_compact(bitmap, M, tile_base, int(row_off[-1]))
    desc, used = [], 0
    for c in range(len(chunks)):
        for a in assets:
            desc.append((a[1], used, rows.data_ptr() + 4 * int(row_off[c]), int(counts[c]), a[4], 0, M, M))
            used += pl._aligned(int(counts[c]) * a[4])
    stage = torch.empty(used, dtype=torch.uint8, device=dev)
    desc = np.array(desc, dtype=np.int64)
    desc[:, 1] += stage.data_ptr()
    nbytes = int((desc[:, 3] * (2 * desc[:, 4] + 4)).sum())
    nv.chunk_gather_group(desc, dev)
    torch.cuda.synchronize()
    windows = []
    for _ in range(7):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            nv.chunk_gather_group(desc, dev)
        e.record()
        e.synchronize()
        windows.append(s.elapsed_time(e) / iters * 1e-3)
    t = median(windows)
    return dict(seconds=t, bytes=nbytes, share_of_peak=nbytes / t / PEAK_BYTES_PER_S, rows=int(counts.sum()), problems=int(desc.shape[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cloud", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check-n", type=int, default=60_000, help="cloud points of the comparison run (4 chunks of a tenth of it)")
    cfg = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pc_attach: needs a GPU")
    differ_torch, differ, kept = compare(cfg.check_n, 4, cfg.check_n // 10)
    print(f"check on 4 chunks ({kept} kept rows): chunks where the torch form (fp32 limit test) differs from the device form: {differ_torch}; "
          f"where the host form (fp64 selection) differs: {differ}", flush=True)
    root = tempfile.mkdtemp(prefix="pc_attach_bench_")
    result = dict(cloud=cfg.cloud, chunks=cfg.chunks, gaussians=cfg.gaussians, k=K, dist_limit=LIMIT, check_host_differs=differ, check_torch_differs=differ_torch)
    try:
        gs_root, pc_root = write_scene(root, cfg.cloud, cfg.chunks, cfg.gaussians)
        for name, fn in FORMS.items():
            runs = []
            for r in range(1 + (cfg.host_repeats if name == "host" else cfg.repeats)):
                prof = {}
                t0 = time.perf_counter()
                fn(gs_root, pc_root, prof)
                torch.cuda.synchronize()
                prof["total"] = time.perf_counter() - t0
                if r:
                    runs.append(prof)
            runs.sort(key=lambda p: p["total"])
            result[name] = {k: round(v, 6) for k, v in runs[len(runs) // 2].items()}
            print(name, result[name], flush=True)
        result["kept_rows"] = sum(o["pc_coord.npy"].shape[0] for o in read_outputs(gs_root))
        result["gather_alone"] = gather_alone(gs_root, pc_root, cfg.iters)
    finally:
        shutil.rmtree(root)
    stages = ("read", "upload", "search", "select", "gather", "write", "total")
    print("\n| form | " + " | ".join(stages) + " |\n|---|" + "---|" * len(stages))
    for name in FORMS:
        print(f"| {name} | " + " | ".join(f"{result[name].get(s, 0.0) * 1e3:.1f}" for s in stages) + " |")
    ga = result["gather_alone"]
    print(f"\n(ms)  gather alone: {ga['seconds'] * 1e6:.1f} us, {ga['bytes'] / 1e6:.1f} MB, {ga['share_of_peak']:.1%} of {PEAK_BYTES_PER_S / 1e12:.0f} TB/s")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
