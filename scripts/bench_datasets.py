#!/usr/bin/env python
"""One scene of 200,000 Gaussians (768-wide fp16 lang_feat, u8 colour, f64 coord, f32 the rest, i64 labels) from page-cached .npy
files to the device dict of ScanNetGSDataset.get_data, in three forms:

  host    what a user writes without the dataset layer: np.load per asset, numpy astype / clip / reshape on the host, then one
          torch.from_numpy(v).cuda() per asset (pageable memory: each copy is synchronous).
  ingest  pointcept_api.datasets: np.load per asset, ONE pack into a pinned slot, ONE copy, ONE ss_ingest_group launch
          (prefetch off, so the read and the pack are inside the timed region; lang_feat comes back as a view of the arena).
  cached  the same with cache_bytes covering the scene: no file read, no copy; one ss_ingest_group launch that also clones lang_feat.

Each form: --warmup calls, then --repeats calls, every call between one HIP event pair and one host-clock pair with a device sync at
its end; the median of both is printed (these are call times with their host work, not kernel times).
  kernel  the ss_ingest_group launch of the cached form alone: --iters back-to-back relaunches on resident descriptor tables between
          one event pair, median over 7 windows; the bytes the launch reads and writes (0.63 GB, beyond the 256 MiB Infinity Cache)
          over that time as a share of the 8 TB/s peak.  The row-gather kernel's share (the roofline row of README.md, 0.67-0.70) is the neighbour.

Needs a GPU: there is no CPU path.  Prints a markdown table and one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def median(v):
    return sorted(v)[len(v) // 2]


def write_scene(folder, n, lang_dim, seed=0):
    g = np.random.RandomState(seed)
    os.makedirs(folder)
    raw = dict(coord=g.rand(n, 3) * 8.0, color=g.randint(0, 256, (n, 3)).astype(np.uint8), opacity=g.rand(n).astype(np.float32),
               quat=g.randn(n, 4).astype(np.float32), scale=(g.rand(n, 3) * 2.0).astype(np.float32), normal=g.randn(n, 3).astype(np.float32),
               segment20=g.randint(-1, 20, (n, 1)).astype(np.int64), instance=g.randint(-1, 50, n).astype(np.int64),
               valid_feat_mask=(g.rand(n) < 0.9).astype(np.uint8), lang_feat=g.randn(n, lang_dim).astype(np.float16))
    for k, v in raw.items():
        np.save(os.path.join(folder, k + ".npy"), v)
    return raw


def host_form(folder, names):
    """the hand-written form: numpy on the host, one upload per asset"""
    d = {k: np.load(os.path.join(folder, k + ".npy")) for k in names}
    for k in ("coord", "color", "normal", "quat"):
        d[k] = d[k].astype(np.float32)
    d["opacity"] = d["opacity"].astype(np.float32).reshape(-1, 1)
    d["scale"] = d["scale"].astype(np.float32).clip(0, 1.5)
    d["lang_feat"] = d["lang_feat"].astype(np.float16)
    d["valid_feat_mask"] = d["valid_feat_mask"].astype(bool)
    d["segment"] = d.pop("segment20").reshape([-1]).astype(np.int32)
    d["instance"] = d["instance"].reshape([-1]).astype(np.int32)
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def timed(fn, warmup, repeats):
    """-> (median event ms, median host ms) of one call, a device sync at the end of each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, host = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
        del out
    return median(ev), median(host)


def kernel_alone(ds, path, iters, windows=7):
    """the launch of a cache hit on resident tables -> (seconds per launch, bytes read + written per launch)"""
    from scenesplat_amd import grouped, native as nv
    arena, (desc, offsets, specs, _) = ds.stager.cache[path]
    outs, rows, moved = [], [], 0
    for j, spec in enumerate(specs):
        t = torch.empty(spec["shape"], dtype=getattr(torch, spec["dtype"]), device="cuda")
        outs.append(t)
        row = desc[j].copy()
        row[0] += arena.data_ptr()
        row[1] = t.data_ptr()
        rows.append(row)
        src_code = int(desc[j, 3]) & 0xff
        src_bytes = {0: 8, 1: 4, 2: 2, 3: 1, 4: 1, 5: 2, 6: 4, 7: 8, 8: 1}[src_code]
        moved += int(desc[j, 2]) * src_bytes + t.numel() * t.element_size()
    table = np.stack(rows)
    per = nv.lib().ss_ingest_group_elems_per_workgroup()
    starts = grouped.starts((table[:, 2] + per - 1) // per)
    tables = grouped.launch("ss_ingest_group", table, starts, torch.device("cuda"))
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            grouped.relaunch("ss_ingest_group", tables, starts[-1])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters * 1e-3)
    return median(times), moved, len(rows), starts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--lang-dim", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_datasets.py needs a GPU"
    from scenesplat_amd.pointcept_api import build_dataset
    with tempfile.TemporaryDirectory() as root:
        folder = os.path.join(root, "val", "scene0000_00")
        raw = write_scene(folder, args.n, args.lang_dim)
        file_bytes = sum(v.nbytes for v in raw.values())
        ds = build_dataset(dict(type="ScanNetGSDataset", split="val", data_root=root, prefetch=False))
        cached = build_dataset(dict(type="ScanNetGSDataset", split="val", data_root=root, prefetch=False, cache_bytes=2 * file_bytes))
        names = ds.asset_names(folder)
        ref, got = host_form(folder, names), ds.get_data(0)          # (also the page-cache warm-up) -- and the forms agree
        assert sorted(ref) == sorted(k for k in got if k != "name") and all(torch.equal(ref[k], got[k]) for k in ref)
        hit = cached.get_data(0)
        hit = cached.get_data(0)
        assert cached.stats["cache_hit"] == 1 and all(torch.equal(ref[k], hit[k]) for k in ref)
        del ref, got, hit
        res = dict(n=args.n, lang_dim=args.lang_dim, file_mb=file_bytes / 1e6)
        res["host_event_ms"], res["host_ms"] = timed(lambda: host_form(folder, names), args.warmup, args.repeats)
        res["ingest_event_ms"], res["ingest_ms"] = timed(lambda: ds.get_data(0), args.warmup, args.repeats)
        res["cached_event_ms"], res["cached_ms"] = timed(lambda: cached.get_data(0), args.warmup, args.repeats)
        sec, moved, nprob, wgs = kernel_alone(cached, cached.data_list[0], args.iters)
        res.update(kernel_us=sec * 1e6, kernel_mb=moved / 1e6, kernel_tb_s=moved / sec / 1e12, kernel_share_of_peak=moved / sec / PEAK_BYTES_PER_S,
                   kernel_problems=nprob, kernel_workgroups=wgs, host_fallback=ds.stats["host_fallback"])
        ds.stager.close()
        cached.stager.close()
    print("| form | call, host clock (ms) | call, HIP events (ms) |\n|---|---|---|")
    for k, label in (("host", "host: numpy casts + one upload per asset"), ("ingest", "ingest: one pack, one copy, one launch"),
                     ("cached", "cache hit: one launch")):
        print("| %s | %.2f | %.2f |" % (label, res[k + "_ms"], res[k + "_event_ms"]))
    print("\nss_ingest_group alone (%d problems, %d workgroups): %.1f us, %.1f MB moved, %.2f TB/s = %.2f of the 8 TB/s peak"
          % (res["kernel_problems"], res["kernel_workgroups"], res["kernel_us"], res["kernel_mb"], res["kernel_tb_s"], res["kernel_share_of_peak"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
