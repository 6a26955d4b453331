#!/usr/bin/env python
"""The head of the shipped training transform list (CenterShift ... ChromaticJitter, pointcept_api/transform.py) on the device,
timed on a synthetic SceneSplat-like sample at n = 200,000 and n = 800,000 Gaussians.

  chain    Compose(fuse=True) and Compose(fuse=False) over the same list and the same recorded draws (every op fires; dropout keeps
           80 %), alternating in one process.  One HIP event pair around each call, the sample restored from a master copy before
           every call outside the timed region (the ops work in place); warm-up calls first, median over --repeats calls.  The
           figure holds the bounding-box readbacks (host syncs) and the host's enqueue time: it is a call time, not a kernel time.
  kernels  each of the four kernels alone: --iters back-to-back launches between one event pair (a window of 0.1 s and more), each
           launch on the next of enough copies of the sample that the coord arrays alone exceed 600 MiB, so that no launch finds its
           rows in the 256 MiB Infinity Cache; median over the windows, and the bytes the algorithm moves (coord 12, quat 16,
           scale 12, normal 12, colour 12 bytes per row, read and written where updated) over that time as a share of the 8 TB/s peak.

  --cloud  the point cloud beside the Gaussians (pc_coord / pc_segment): m = 1,000,000 points beside 1,000,000 Gaussians, grid 0.02.
           The cloud's rigid pass (ss_aug_gaussians on pc_coord alone, HBM-resident as under `kernels`), gpu_transforms.grid_sample_pc
           as a call and split into key build, sort, partition and pick (--cloud-iters back-to-back calls between one event pair,
           median over the windows), and the same pick written with torch ops (gather, compare, where, scatter_reduce, modulo) on
           the same partition, checked to give the same rows.

The CPU chain of the reference is not timed here.  Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12

HEAD = [dict(type="CenterShift", apply_z=True), dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=0.2),
        dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5),
        dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=0.5),
        dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=0.5),
        dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5), dict(type="RandomJitter", sigma=0.005, clip=0.01),
        dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]),
        dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None), dict(type="ChromaticTranslation", p=0.95, ratio=0.05),
        dict(type="ChromaticJitter", p=0.95, std=0.05)]
PARAMS = [{}, dict(fired=True, seed=1), dict(fired=True, angle=0.7), dict(fired=True, angle=0.02), dict(fired=True, angle=-0.03),
          dict(scale=[1.04]), dict(flip_x=True, flip_y=True), dict(seed=2), dict(fired=True, seed=3), dict(fired=True, blend=0.4),
          dict(fired=True, tr=[5.0, -7.0, 3.0]), dict(fired=True, seed=4)]


def sample(n, dev, seed=0):
    """a room-sized slab of Gaussians (8 x 6 x 3 m), as the datasets hand it over after the upload"""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)       # noqa: E731
    nrm = torch.randn(n, 3, device=dev, generator=g)
    return dict(coord=r(n, 3) * torch.tensor([8.0, 6.0, 3.0], device=dev), color=r(n, 3) * 255, opacity=r(n, 1),
                quat=torch.randn(n, 4, device=dev, generator=g), scale=r(n, 3) * 0.05, normal=nrm / nrm.norm(dim=1, keepdim=True),
                segment=torch.randint(-1, 20, (n,), device=dev, generator=g), lang_feat=torch.randn(n, 16, device=dev, generator=g),
                valid_feat_mask=(r(n) < 0.9).long())


def median(v):
    return sorted(v)[len(v) // 2]


def time_chain(n, dev, warmup, repeats):
    from scenesplat_amd.pointcept_api import Compose
    master = sample(n, dev)
    comps = {"fused": Compose(HEAD, fuse=True), "op by op": Compose(HEAD, fuse=False)}
    ms = {k: [] for k in comps}
    for it in range(warmup + repeats):
        for name, comp in comps.items():
            d = {k: v.clone() for k, v in master.items()}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            comp(d, params=PARAMS)
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


def time_kernels(n, dev, iters, repeats, resident_mib):
    """Each launch works on the next of `sets` copies of the sample, enough copies that their coord arrays alone exceed `resident_mib`
    (more than the 256 MiB Infinity Cache): a launch finds none of its rows in cache, so bytes over time is an HBM rate."""
    import ctypes
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api.transform import box_blur3
    sets = max(2, -(-resident_mib * (1 << 20) // (12 * n)))               # sized by the smallest array a pass touches alone (coord)
    ds = []
    for k in range(sets):
        d = sample(n, dev, seed=k)
        ds.append({key: d[key] for key in ("coord", "quat", "scale", "normal", "color")})
    aff = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0]                # the identity, evaluated in full: repeated application does not drift
    rq = [1.0, 0, 0, 0]
    lin = aff[:9]
    bb = nv.aug_bbox(ds[0]["coord"]).cpu().numpy()
    dim = np.floor((bb[3:] - bb[:3]) / 0.2).astype(int) + 3
    grid = box_blur3(torch.randn(*dim.tolist(), 3, device=dev)).contiguous()
    origin = (bb[:3] - 0.2).tolist()
    lo, hi = [0.0] * 3, [255.0] * 3
    # the box without the wrapper's two allocations per call: partials and result allocated once, the C entry called directly
    lib, part, out6 = nv.lib(), torch.empty((nv.lib().ss_aug_bbox_blocks(n), 6), device=dev), torch.empty(6, device=dev)
    aff_c, stream = (ctypes.c_float * 12)(*aff), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def bbox(d):
        rc = lib.ss_aug_bbox(ctypes.c_void_p(d["coord"].data_ptr()), n, aff_c, ctypes.c_void_p(part.data_ptr()),
                             ctypes.c_void_p(out6.data_ptr()), stream)
        assert rc == 0
    cases = {
        "k_aug_bbox (+ finish), pending affine": (bbox, 12 * n),
        "k_aug_gaussians: coord + quat + scale + normal, flip, own jitter": (
            lambda d: nv.aug_gaussians_(d["coord"], d["quat"], d["scale"], d["normal"], affine=aff, rquat=rq, flip=3,
                                        scale_mul=[1.0, 1.0, 1.0], lin=lin, jitter=(1e-6, 1e-5), seed=7), 2 * (12 + 16 + 12 + 12) * n),
        "k_aug_gaussians: coord only (a CenterShift alone)": (lambda d: nv.aug_gaussians_(d["coord"], affine=aff), 2 * 12 * n),
        "k_aug_elastic, grid %s" % "x".join(map(str, dim.tolist())): (
            lambda d: nv.aug_elastic_(d["coord"], grid, origin, 0.2, 1e-4), 2 * 12 * n),
        "k_aug_color: contrast + translation + own jitter": (
            lambda d: nv.aug_color_(d["color"], 7, lo, hi, 0.1, [0.5, -0.5, 0.25], 0.001, None, 9, False), 2 * 12 * n),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        for d in ds[:10]:
            fn(d)
        us = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for i in range(iters):
                fn(ds[i % sets])
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / iters)
        out[name] = dict(us=us, bytes=nbytes)
    return out, sets


def time_cloud(m, n, grid, dev, iters, repeats, resident_mib):
    """-> {name: dict(us=[per call, one per window], note)} for the cloud of m points beside n Gaussians"""
    from scenesplat_amd import gpu_transforms as gt, native as nv
    g = torch.Generator(device=dev).manual_seed(11)
    box = torch.tensor([8.0, 6.0, 3.0], device=dev)
    sets = max(2, -(-resident_mib * (1 << 20) // (12 * m)))
    clouds = [torch.rand(m, 3, device=dev, generator=g) * box for _ in range(sets)]
    pc = clouds[0]
    seg = torch.randint(-1, 20, (m,), device=dev, generator=g)
    gauss = sample(n, dev)["coord"]                                   # the Gaussians the cloud lies beside: allocated, as in a real call
    aff = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0]
    key = gt._voxel_keys(pc, grid)[1]
    order = nv.argsort_i64(key, 63, want_inverse=False, want_sorted=False)[0][0]
    cluster, idx_ptr, _, n_out = nv.pool_partition(key[0], order, 0)
    n_cells = int(n_out.item())

    def torch_pick():
        o = order.long()
        cell = cluster.long()[o]                                      # the cell of every sorted position
        lab = seg[o]
        pos = torch.arange(m, device=dev)
        cand = torch.where(lab != -1, pos, pos + m)                   # labelled members sort in front of the others
        best = torch.full((n_cells,), 2 * m, dtype=torch.int64, device=dev).scatter_reduce(0, cell, cand, "amin")
        return o[best % m]
    want = nv.voxel_pick_labelled(order, idx_ptr, n_cells, seg, -1).long()
    assert torch.equal(want, torch_pick()) and torch.equal(want, gt.grid_sample_pc(pc, grid, seg))
    turn = [0]

    def rigid():
        turn[0] += 1
        nv.aug_gaussians_(coord=clouds[turn[0] % sets], affine=aff)
    cases = {
        "rigid pass over the cloud (ss_aug_gaussians, coord only), %d copies" % sets: rigid,
        "grid_sample_pc, whole call (one n_cells readback)": lambda: gt.grid_sample_pc(pc, grid, seg),
        "  keys (floor, min, pack: torch)": lambda: gt._voxel_keys(pc, grid),
        "  sort (ss_argsort_i64, 63 bits)": lambda: nv.argsort_i64(key, 63, want_inverse=False, want_sorted=False),
        "  partition (ss_pool_partition)": lambda: nv.pool_partition(key[0], order, 0),
        "  pick (ss_voxel_pick_labelled)": lambda: nv.voxel_pick_labelled(order, idx_ptr, n_cells, seg, -1),
        "  pick, no labels": lambda: nv.voxel_pick_labelled(order, idx_ptr, n_cells, None, -1),
        "the same pick in torch ops (gather x3, compare, where, scatter_reduce, modulo)": torch_pick,
    }
    out = {}
    for name, fn in cases.items():
        for _ in range(5):
            fn()
        us = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / iters)
        out[name] = dict(us=us)
    del gauss
    return out, n_cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", action="store_true", help="time the point cloud beside the Gaussians instead of the chain")
    ap.add_argument("--cloud-points", type=int, default=1000000)
    ap.add_argument("--cloud-gaussians", type=int, default=1000000)
    ap.add_argument("--cloud-grid", type=float, default=0.02)
    ap.add_argument("--cloud-iters", type=int, default=200, help="back-to-back calls per cloud timing window")
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 800000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10000, help="back-to-back launches per kernel timing window (0.1 s and more)")
    ap.add_argument("--resident-mib", type=int, default=600, help="the kernel loops rotate over copies of the sample that together exceed this")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a GPU: the transforms have no CPU path")
    dev = torch.device("cuda")
    if args.cloud:
        m, n = args.cloud_points, args.cloud_gaussians
        res, n_cells = time_cloud(m, n, args.cloud_grid, dev, args.cloud_iters, max(3, args.repeats // 3), args.resident_mib)
        print(f"\n## cloud of m = {m:,} points beside {n:,} Gaussians, grid {args.cloud_grid}: {n_cells:,} occupied cells "
              f"({args.cloud_iters} calls per window)\n")
        print("| step | us per call: median | min - max |")
        print("|---|---|---|")
        for name, k in res.items():
            print(f"| {name} | {median(k['us']):.1f} | {min(k['us']):.1f} - {max(k['us']):.1f} |")
        print(json.dumps(dict(cloud=dict(m=m, n=n, grid=args.cloud_grid, n_cells=n_cells, steps=res))))
        return
    result = {}
    for n in args.sizes:
        ms = time_chain(n, dev, args.warmup, args.repeats)
        print(f"\n## n = {n:,}: head of the list, {len(HEAD)} ops, every op fires ({args.repeats} calls after {args.warmup} warm-up calls)\n")
        print("| Compose | ms per call: median | min - max | Gaussians / s |")
        print("|---|---|---|---|")
        for name, v in ms.items():
            print(f"| {name} | {median(v):.3f} | {min(v):.3f} - {max(v):.3f} | {n / (median(v) * 1e-3) / 1e6:.1f} M |")
        ks, sets = time_kernels(n, dev, args.iters, max(3, args.repeats // 3), args.resident_mib)
        print(f"\n| kernel ({args.iters} launches per window over {sets} copies of the sample) | us per launch: median | min - max | bytes moved | rate, share of 8 TB/s |")
        print("|---|---|---|---|---|")
        for name, k in ks.items():
            med = median(k["us"])
            rate = k["bytes"] / (med * 1e-6)
            print(f"| {name} | {med:.1f} | {min(k['us']):.1f} - {max(k['us']):.1f} | {k['bytes'] / 1e6:.1f} MB | {rate / 1e12:.2f} TB/s, "
                  f"{100 * rate / PEAK_BYTES_PER_S:.0f} % |")
        result[str(n)] = dict(chain_ms=ms, kernels=ks)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
