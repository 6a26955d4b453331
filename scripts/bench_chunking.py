#!/usr/bin/env python
"""One synthetic scene (default 2,000,000 Gaussians in a 15 m x 12 m room, 768-wide fp16 lang_feat, u8 colour, f32 the rest, i64
labels) from page-cached .npy files to the chunked split on disk (grid_size 0.01, 6x6 chunks, stride 3x3), in two forms:

  numpy   the reference-shaped form: fp32 recentre, lang_feat normalised in place with numpy, the per-row Python loop that groups rows
          by grid cell and one np.random.choice per occupied cell, one boolean mask over the scene per chunk, asset[mask] per asset,
          np.save per file.
  device  pointcept_api.preprocessing.chunk_scene: one packed upload, the kernels of csrc/chunking.hip, one download per staging batch,
          np.save from views of the pinned staging buffer.

The device form is run --repeats times after one warm-up run (which also brings the files into the page cache), the numpy form
--numpy-repeats times behind it (it takes minutes, and has nothing to warm up); a run is timed with a host clock around work that
ends in a device synchronise (the device form's last step is a download that is waited for).  Inside a run
the seconds spent in np.load and in np.save are summed apart, so the table shows read / compute / write per form.  The two forms'
chunk directories are compared (same directories, same rows per chunk, every asset but lang_feat byte-equal wherever the pick is
forced) before anything is timed at the small --check-n size.

  gather  ss_chunk_gather_group alone over ALL (chunk, asset) problems of the scene into one device buffer: --iters back-to-back
          relaunches on resident descriptor tables between one HIP event pair, median of 7 windows; bytes = rows read + rows written
          + the int32 indices read, as a share of the 8 TB/s peak.

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
SPLIT, SCENE = "train", "scene0000_00"
KW = dict(grid_size=0.01, chunk_range=(6, 6), chunk_stride=(3, 3), chunk_minimum_size=10000, max_chunk_num=None)


def median(v):
    return sorted(v)[len(v) // 2]


def write_scene(root, n, lang_dim, seed=0):
    g = np.random.default_rng(seed)
    folder = os.path.join(root, SPLIT, SCENE)
    os.makedirs(folder)
    raw = dict(coord=(g.random((n, 3), dtype=np.float32) * np.float32([15, 12, 3]) - np.float32([4, 2, 1])).astype(np.float32),
               color=g.integers(0, 256, (n, 3)).astype(np.uint8), opacity=g.random((n, 1), dtype=np.float32),
               quat=g.standard_normal((n, 4), dtype=np.float32), scale=g.random((n, 3), dtype=np.float32),
               segment=g.integers(-1, 100, n).astype(np.int16), instance=g.integers(-1, 500, n).astype(np.int64),
               valid_feat_mask=(g.random(n) < 0.9).astype(np.uint8), lang_feat=g.standard_normal((n, lang_dim), dtype=np.float32).astype(np.float16))
    for k, v in raw.items():
        np.save(os.path.join(folder, k + ".npy"), v)
    return sum(v.nbytes for v in raw.values())


def numpy_form(root, out, prof, grid_size, chunk_range, chunk_stride, chunk_minimum_size, max_chunk_num):
    """the reference-shaped form (module docstring); -> chunk directories"""
    folder = os.path.join(root, SPLIT, SCENE)
    t0 = time.perf_counter()
    data = {f[:-4]: np.load(os.path.join(folder, f)) for f in os.listdir(folder) if f.endswith(".npy")}
    prof["read"] = prof.get("read", 0.0) + time.perf_counter() - t0
    coord = data["coord"] - data["coord"].min(axis=0)
    valid = data["valid_feat_mask"]
    data["lang_feat"][valid == 1] /= np.linalg.norm(data["lang_feat"][valid == 1], axis=1, keepdims=True)
    cells = np.floor(coord / grid_size).astype(int)
    groups = {}
    for i, cell in enumerate(cells):
        groups.setdefault(tuple(cell), []).append(i)
    picked = []
    for rows in groups.values():
        ok = [i for i in rows if valid[i] == 1]
        picked.append(np.random.choice(ok) if ok else rows[0])
    picked = np.array(picked)
    coord = coord[picked]
    data = {k: v[picked] for k, v in data.items()}
    top = coord.max(axis=0)[:2]
    x, y = np.meshgrid(np.arange(0, top[0] + chunk_stride[0] - chunk_range[0], chunk_stride[0]),
                       np.arange(0, top[1] + chunk_stride[1] - chunk_range[1], chunk_stride[1]), indexing="ij")
    dirs = []
    for ox, oy in zip(x.reshape(-1), y.reshape(-1)):
        mask = (coord[:, 0] >= ox) & (coord[:, 0] < ox + chunk_range[0]) & (coord[:, 1] >= oy) & (coord[:, 1] < oy + chunk_range[1])
        if mask.sum() < chunk_minimum_size:
            continue
        path = os.path.join(out, f"{SPLIT}_grid{grid_size * 100:.1f}cm_chunk{chunk_range[0]}x{chunk_range[1]}_stride{chunk_stride[0]}x{chunk_stride[1]}",
                            f"{SCENE}_{len(dirs)}")
        os.makedirs(path, exist_ok=True)
        for k, v in data.items():
            rows = v[mask]
            t0 = time.perf_counter()
            np.save(os.path.join(path, k + ".npy"), rows)
            prof["write"] = prof.get("write", 0.0) + time.perf_counter() - t0
        dirs.append(path)
    return dirs


def device_form(root, out, prof, **kw):
    from scenesplat_amd.pointcept_api import preprocessing as pp
    pp.PROFILE = prof
    try:
        dirs = pp.chunk_scene(SCENE, root, out, SPLIT, **kw)
        torch.cuda.synchronize()
    finally:
        pp.PROFILE = None
    return dirs


def timed(form, root, repeats, warmup, **kw):
    """-> medians of (total, read, write) seconds over `repeats` runs after `warmup` runs; the outputs are removed after every run"""
    rows = []
    for r in range(repeats + warmup):
        out, prof = tempfile.mkdtemp(dir=root), {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dirs = form(root, out, prof, **kw)
        total = time.perf_counter() - t0
        shutil.rmtree(out)
        if r >= warmup:
            rows.append((total, prof.get("read", 0.0), prof.get("write", 0.0)))
    return [median([row[j] for row in rows]) for j in range(3)] + [len(dirs)]


def check(root, n, lang_dim):
    """both forms on a small scene with an all-invalid mask (the pick is forced: the first row of the cell): the same files"""
    small = os.path.join(root, "check")
    write_scene(small, n, lang_dim, seed=1)
    np.save(os.path.join(small, SPLIT, SCENE, "valid_feat_mask.npy"), np.zeros(n, np.uint8))
    kw = dict(KW, chunk_minimum_size=100)
    a, b = numpy_form(small, os.path.join(small, "a"), {}, **kw), device_form(small, os.path.join(small, "b"), {}, **kw)
    assert len(a) == len(b) > 0
    for da, db in zip(a, b):
        assert os.path.basename(da) == os.path.basename(db) and sorted(os.listdir(da)) == sorted(os.listdir(db))
        for f in os.listdir(da):
            va, vb = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
            assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), (da, f)
    shutil.rmtree(small)
    return len(a)


def gather_alone(root, iters, windows=7):
    """ss_chunk_gather_group over every (chunk, asset) problem of the scene at once -> (seconds per launch, bytes moved, problems, workgroups)"""
    from scenesplat_amd import grouped, native as nv
    from scenesplat_amd.pointcept_api import preprocessing as pp
    dev = torch.device("cuda", torch.cuda.current_device())
    arrays = pp.load_scene(os.path.join(root, SPLIT, SCENE))
    n = pp.check_assets(arrays)
    arena, offsets, assets = pp._upload(arrays, n, dev)
    del arrays
    coord = arena[offsets["coord"]:offsets["coord"] + n * 12].view(torch.float32).view(n, 3)
    valid = arena[offsets[pp._VALID]:offsets[pp._VALID] + n]
    extent = nv.chunk_extent(coord)
    rec = nv.chunk_recentre(coord, extent)
    ext = extent.cpu().numpy()
    pick = pp.subsample_rows(rec, KW["grid_size"], ext[3:] - ext[:3], valid, 0)
    xs, ys = pp.chunk_origins(nv.chunk_extent(rec, pick).cpu().numpy()[3:5], KW["chunk_range"], KW["chunk_stride"])
    counts, row_off, rows = pp.chunk_rows(rec, pick, xs, ys, KW["chunk_range"], KW["chunk_stride"])
    kept = pp.select_chunks(counts, KW["chunk_minimum_size"])
    sizes = [(c, a, -(-int(counts[c]) * a[3] // 64) * 64) for c in kept for a in assets]
    stage = torch.empty(sum(s for _, _, s in sizes), dtype=torch.uint8, device=dev)
    desc, off, moved = [], 0, 0
    for c, a, s in sizes:
        desc.append((arena.data_ptr() + offsets[a[0]], stage.data_ptr() + off, rows.data_ptr() + 4 * int(row_off[c]), int(counts[c]), a[3],
                     pick.data_ptr(), n, pick.numel()))
        off += s
        moved += int(counts[c]) * (2 * a[3] + 8)                   # the row read and written, idx and pick[idx] read
    desc = np.asarray(desc, dtype=np.int64)
    per = np.array([nv.lib().ss_chunk_gather_rows_per_workgroup(int(rb)) for rb in desc[:, 4]], dtype=np.int64)
    starts = grouped.starts((desc[:, 3] + per - 1) // per)
    tables = grouped.launch("ss_chunk_gather_group", desc, starts, dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            grouped.relaunch("ss_chunk_gather_group", tables, starts[-1])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters * 1e-3)
    return median(times), moved, len(desc), starts[-1], int(pick.numel()), int(sum(counts[c] for c in kept))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--lang-dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-repeats", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--check-n", type=int, default=200000)
    ap.add_argument("--tmp", default=None, help="where the scene and the chunked splits are written (default: the system's temporary folder)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_chunking.py needs a GPU"
    with tempfile.TemporaryDirectory(dir=args.tmp) as root:
        res = dict(n=args.n, lang_dim=args.lang_dim, check_chunks=check(root, args.check_n, 16))
        res["file_mb"] = write_scene(root, args.n, args.lang_dim) / 1e6
        # the device form first: its warm-up run also brings the files into the page cache for both forms
        for name, form, reps, warm in (("device", device_form, args.repeats, 1), ("numpy", numpy_form, args.numpy_repeats, 0)):
            total, read, write, chunks = timed(form, root, reps, warm, **KW)
            res.update({name + "_s": total, name + "_read_s": read, name + "_write_s": write, name + "_chunks": chunks})
            print(name, res[name + "_s"], flush=True)
        sec, moved, nprob, wgs, kept_rows, gathered = gather_alone(root, args.iters)
        res.update(gather_ms=sec * 1e3, gather_mb=moved / 1e6, gather_tb_s=moved / sec / 1e12, gather_share_of_peak=moved / sec / PEAK_BYTES_PER_S,
                   gather_problems=nprob, gather_workgroups=wgs, subsampled_rows=kept_rows, gathered_rows=gathered)
    print("| form | total (s) | np.load (s) | np.save (s) | rest (s) | chunks |\n|---|---|---|---|---|---|")
    for k in ("numpy", "device"):
        t, r, w = res[k + "_s"], res[k + "_read_s"], res[k + "_write_s"]
        print("| %s | %.2f | %.2f | %.2f | %.2f | %d |" % (k, t, r, w, t - r - w, res[k + "_chunks"]))
    print("\nss_chunk_gather_group alone (%d problems, %d workgroups, %d rows): %.3f ms, %.1f MB moved, %.2f TB/s = %.2f of the 8 TB/s peak"
          % (res["gather_problems"], res["gather_workgroups"], res["gathered_rows"], res["gather_ms"], res["gather_mb"], res["gather_tb_s"],
             res["gather_share_of_peak"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
