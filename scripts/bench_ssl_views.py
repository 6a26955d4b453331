#!/usr/bin/env python
"""The colour chain, the sparse voxel blur and one ContrastiveViewsGenerator_SSL call (pointcept_api/transform.py, csrc/ssl_views.hip)
on the device, timed as scripts/bench_augment.py times the augmentation head.

  chain      ss_color_chain on 300,000 colours: the four jitter steps + grayscale with and without the contrast step (its reduction
             pass).  --iters back-to-back launches between one HIP event pair, each on the next of enough copies that the arrays
             exceed 600 MiB (no launch finds its rows in the 256 MiB Infinity Cache); median over the windows; the bytes the
             algorithm moves (12 read + 12 written per row, 12 more read per contrast step) over that time as a share of the 8 TB/s
             peak.  Beside it the same steps written with torch ops (fp32, hue in fp32), checked against the kernel.
  blur       ss_voxel_blur on 300,000 occupied voxels of a 2 cm grid over the shell of a 6 x 5 x 2.6 m room (300 x 250 x 130 cells,
             3 % occupied), colour + opacity + scale + quat as the shipped lists blur them, sigma 0.5 / 1.0 / 2.0 (r = 1 / 2 / 4).
             One event pair per call, the arrays restored from a master copy outside the timed region, median over --repeats.
             Beside it the reference's algorithm in torch on the device: scatter into the dense grid, three separable passes
             (2r + 1 shifted multiply-adds each, `reflect` border), gather, divide -- checked against the kernel.  That dense form
             needs the grid (0.47 GB per copy here); the hash needs 35 MB.
  generator  one ContrastiveViewsGenerator_SSL call of the scannet ssl-pretrain list (tests/golden/ssl_configs.txt, as shipped) on
             800,000 Gaussians on the shell of an 8 x 6 x 3 m room, fuse=True and fuse=False, the same draws every call (the first
             seed that blurs global view 0 at sigma 0.9 .. 1.3 and at least one local view),
             one event pair per call + the host clock: a call time with its readbacks, not a kernel time.  Beside it the same
             lists on the same draws written with torch ops alone (torch_generator: sort-based crop and GridSample, the colour steps
             above, the dense blur grid over each view's box).

The reference's numpy / scipy timings are recorded by tests/golden/make_golden_ssl_views.py (`time_*` in ssl_views.npz) and printed
beside these.  Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line."""
import argparse
import ast
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12
JITTER = [(4, 0.06), (1, 1.2), (3, 0.9), (5, 0.0)]
JITTER_CONTRAST = [(4, 0.06), (1, 1.2), (2, 0.8), (3, 0.9), (5, 0.0)]


def median(v):
    return sorted(v)[len(v) // 2]


def window(fn, iters, windows=7, warm=2):
    """median time of one call of fn(i) over `windows` windows of `iters` back-to-back calls"""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e-3)
    return median(out)


def per_call(fn, restore, repeats, warm=2):
    """median time of fn() with restore() outside the timed region"""
    out = []
    for k in range(warm + repeats):
        restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            out.append((a.elapsed_time(b) * 1e-3, time.perf_counter() - t0))
    return median([o[0] for o in out]), median([o[1] for o in out])


# ---- the colour steps in torch ----------------------------------------------------------------------------------------------------
def torch_gray(c):
    return 0.2989 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2]


def torch_hue(c, f):
    rgb = c / 255.0
    r, g, b = rgb.unbind(1)
    maxc, minc = rgb.max(1).values, rgb.min(1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.remainder(h / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + f, 1.0)
    i = torch.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.long() % 6
    v = maxc
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * fr)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - fr))).clamp(0, 1)
    sel = lambda *opts: torch.stack(opts, 1).gather(1, i[:, None])[:, 0]       # noqa: E731
    return torch.stack([sel(v, q, p, p, t, v), sel(t, v, v, q, p, p), sel(p, p, t, v, v, q)], 1) * 255.0


def torch_chain(c, steps):
    for code, f in steps:
        if code == 1:
            c = (f * c).clamp(0, 255)
        elif code == 2:
            c = (f * c + (1 - f) * torch_gray(c).mean()).clamp(0, 255)
        elif code == 3:
            c = (f * c + (1 - f) * torch_gray(c)[:, None]).clamp(0, 255)
        elif code == 4:
            c = torch_hue(c, f)
        else:
            c = torch_gray(c)[:, None].expand(-1, 3).contiguous()
    return c


# ---- the reference's dense blur in torch ------------------------------------------------------------------------------------------
def shell_voxels(n, size, seed):
    """n distinct cells on the two outermost layers of a box of `size` cells (walls, floor, ceiling), shuffled"""
    g = np.random.RandomState(seed)
    size = np.asarray(size)
    pts = np.zeros((0, 3), dtype=np.int64)
    while len(pts) < n:
        p = (g.rand(200000, 3) * size).astype(np.int64)
        ax = g.randint(0, 3, len(p))
        p[np.arange(len(p)), ax] = np.where(g.rand(len(p)) < 0.5, g.randint(0, 2, len(p)), size[ax] - 1 - g.randint(0, 2, len(p)))
        pts = np.unique(np.concatenate([pts, p]), axis=0)
    return pts[g.permutation(len(pts))[:n]]


def reflect_pad(x, dim, r):
    """scipy's `reflect` border (torch's own "reflect" is scipy's "mirror"): r < size"""
    lo = x.narrow(dim, 0, r).flip(dim)
    hi = x.narrow(dim, x.shape[dim] - r, r).flip(dim)
    return torch.cat([lo, x, hi], dim)


def dense_blur(gc, mask, arrays, sigma, size):
    """GSGaussianBlurVoxelOpc as the reference writes it, on the device: (channels, X, Y, Z) grid, separable passes, gather"""
    r = int(2.0 * sigma + 0.5)
    vals = torch.cat(arrays + [torch.ones_like(arrays[0][:, :1])], 1)[mask]
    g = gc[mask].long()
    grid = torch.zeros((vals.shape[1], *size), device=gc.device)
    grid[:, g[:, 0], g[:, 1], g[:, 2]] = vals.t()
    if r > 0:
        x = torch.arange(-r, r + 1, device=gc.device, dtype=torch.float64)
        w = torch.exp(-0.5 * x * x / sigma ** 2)
        w = (w / w.sum()).tolist()
        for dim in (1, 2, 3):                             # a separable pass per axis as 2r + 1 shifted multiply-adds (no MIOpen solver involved)
            ext = reflect_pad(grid, dim, r)
            acc = ext.narrow(dim, 0, grid.shape[dim]) * w[0]
            for k in range(1, 2 * r + 1):
                acc.add_(ext.narrow(dim, k, grid.shape[dim]), alpha=w[k])
            grid = acc
    got = grid[:, g[:, 0], g[:, 1], g[:, 2]].t()
    res = got[:, :-1] / (got[:, -1:] + 1e-7)
    out, c0 = [], 0
    for a in arrays:
        o = a.clone()
        o[mask] = res[:, c0:c0 + a.shape[1]]
        out.append(o)
        c0 += a.shape[1]
    return out


# ---- the generator's lists in plain torch -------------------------------------------------------------------------------------------
def draw_views(gen, seed, data):
    """the params lists ContrastiveViewsGenerator_SSL.apply would draw from `seed`, in its run order: both forms replay the same draws"""
    subs = [gen.global_base_transform, gen.local_base_transform, gen.global_transform0, gen.global_transform1] + \
        [gen.local_transform] * gen.local_crop_num
    rngs = [np.random.default_rng(q) for q in np.random.SeedSequence(seed).spawn(len(subs))]
    return [[t.draw(rng, data) for t in sub.transforms] for sub, rng in zip(subs, rngs)]


def torch_list(cfgs, params, d):
    """one sub-list of the generator with torch ops only: the reference's algorithms (dense blur grid included) on device tensors"""
    for c, p in zip(cfgs, params):
        t = c["type"]
        if t == "CenterShift":
            lo, hi = d["coord"].amin(0), d["coord"].amax(0)
            shift = torch.stack([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2] if c.get("apply_z", True) else lo[2] * 0])
            d["coord"] = d["coord"] - shift
        elif t == "RandomFlip":
            fx_, fy_ = p["flip_x"], p["flip_y"]
            if fx_ or fy_:
                sign = torch.tensor([-1.0 if fx_ else 1.0, -1.0 if fy_ else 1.0, 1.0], device=d["coord"].device)
                d["coord"] = d["coord"] * sign
                q = d["quat"] / d["quat"].norm(dim=1, keepdim=True)
                qs = torch.tensor([1.0, -1.0 if fy_ else 1.0, -1.0 if fx_ else 1.0, -1.0 if fx_ != fy_ else 1.0], device=q.device)
                q = q * qs                                           # F R F: a reflected axis negates the two other vector components
                v = q[:, [1, 2, 3, 0]]
                lead = v.gather(1, (v * v).argmax(1, keepdim=True))
                d["quat"] = torch.where(lead < 0, -q, q)             # scipy's from_matrix sign
        elif t == "SphereCropRandomMaxPoints":
            n = d["coord"].shape[0]
            if n > p["point_max"]:
                ci = min(int(p["u"] * n), n - 1)
                idx = (d["coord"] - d["coord"][ci]).square().sum(1).argsort(stable=True)[:p["point_max"]]
                d = {k: v[idx] for k, v in d.items()}
        elif t == "RandomColorJitter":
            steps = [(i + 1, p[nm]) for i, nm in ((i, ("brightness", "contrast", "saturation", "hue")[i]) for i in p["order"]) if p[nm] is not None]
            d["color"] = torch_chain(d["color"], steps)
        elif t == "RandomColorGrayScale":
            if p["fired"]:
                d["color"] = torch_chain(d["color"], [(5, 0.0)])
        elif t == "GridSample":
            gc = torch.floor(d["coord"] / c["grid_size"]).long()
            gc = gc - gc.amin(0)
            key = (gc[:, 0] << 42) | (gc[:, 1] << 21) | gc[:, 2]
            skey, order = key.sort(stable=True)
            _, count = torch.unique_consecutive(skey, return_counts=True)
            start = count.cumsum(0) - count
            g = torch.Generator(device=key.device).manual_seed(int(p["seed"]) % (1 << 62))
            idx = order[start + torch.randint(0, 1 << 30, (count.numel(),), device=key.device, generator=g) % count]
            for k in c["keys"]:
                if k in d:
                    d[k] = d[k][idx]
            if c.get("return_grid_coord"):
                d["grid_coord"] = gc[idx].int()
        elif t == "GSGaussianBlurVoxelOpc":
            if p["fired"]:
                gcv = d["grid_coord"].long()
                gcv = gcv - gcv.amin(0)
                size = tuple((gcv.amax(0) + 1).tolist())
                keys = ["color"] + [k for k in ("opacity", "scale", "quat") if k in c["extra_keys"]]
                out = dense_blur(gcv, (d["opacity"] > 0.5).reshape(-1), [d[k] for k in keys], p["sigma"], size)
                d.update(dict(zip(keys, out)))
                if "quat" in keys:
                    d["quat"] = d["quat"] / d["quat"].norm(dim=1, keepdim=True)
        elif t == "NormalizeColor":
            d["color"] = d["color"] / 127.5 - 1
        elif t not in ("RandomColorSolarize", "ToTensor"):
            raise NotImplementedError(t)
    return d


def torch_generator(gcfg, views, data):
    keys = gcfg["view_keys"]
    clone = lambda d: {k: d[k].clone() for k in keys}       # noqa: E731
    gb = torch_list(gcfg["global_base_transform"], views[0], clone(data))
    out = {"global_crop0": torch_list(gcfg["global_transform0"], views[2], clone(gb)),
           "global_crop1": torch_list(gcfg["global_transform1"], views[3], clone(gb))}
    lb = torch_list(gcfg["local_base_transform"], views[1], clone(data))
    for i in range(gcfg["local_crop_num"]):
        out["local_crop%d" % i] = torch_list(gcfg["local_transform"], views[4 + i], clone(lb))
    return {"%s_%s" % (v, k): t for v, d in out.items() for k, t in d.items()}


def shell_sample(n, dev, seed=0):
    """Gaussians on the surfaces of an 8 x 6 x 3 m room, 4 cm thick"""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)       # noqa: E731
    box = torch.tensor([8.0, 6.0, 3.0], device=dev)
    coord = r(n, 3) * box
    ax = torch.randint(0, 3, (n,), device=dev, generator=g)
    depth = r(n) * 0.04
    side = r(n) < 0.5
    rows = torch.arange(n, device=dev)
    coord[rows, ax] = torch.where(side, depth, box[ax] - depth)
    return dict(coord=coord, color=r(n, 3) * 255, opacity=r(n, 1), quat=torch.randn(n, 4, device=dev, generator=g), scale=r(n, 3) * 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300000)
    ap.add_argument("--gen-n", type=int, default=800000)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip-dense", action="store_true")
    args = ap.parse_args()
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import Compose
    dev = torch.device("cuda")
    res = {}
    ref = {}
    gpath = os.path.join(ROOT, "tests", "golden", "ssl_views.npz")
    if os.path.exists(gpath):
        z = np.load(gpath)
        ref = {k: float(z[k]) for k in z.files if k.startswith("time_") and z[k].ndim == 0}

    # ---- colour chain ----
    n = args.n
    copies = max(2, int(600 * 2 ** 20 / (n * 12)) + 1)
    g = torch.Generator(device=dev).manual_seed(0)
    master = torch.rand(copies, n, 3, device=dev, generator=g) * 255
    print("## colour chain, n = %d (%d copies, %.0f MiB)\n" % (n, copies, master.numel() * 4 / 2 ** 20))
    print("| steps | kernel | share of 8 TB/s | torch ops | torch / kernel | max difference |")
    print("|---|---|---|---|---|---|")
    for name, steps in (("jitter (4 steps) + grayscale, no contrast", JITTER), ("the same with the contrast step", JITTER_CONTRAST)):
        work = master.clone()
        t_k = window(lambda i: nv.color_chain_(work[i % copies], steps), args.iters)
        t_t = window(lambda i: torch_chain(work[i % copies], steps), max(4, args.iters // 4))
        a = master[0].clone()
        nv.color_chain_(a, steps)
        diff = float((a - torch_chain(master[0], steps)).abs().max())
        nbytes = n * 12 * (2 + sum(c == 2 for c, _ in steps))
        print("| %s | %.1f us | %.0f %% | %.1f us | %.1fx | %.2g |" % (name, t_k * 1e6, 100 * nbytes / t_k / PEAK_BYTES_PER_S, t_t * 1e6, t_t / t_k, diff))
        res["chain_" + ("contrast" if len(steps) == 5 else "plain")] = dict(kernel_us=t_k * 1e6, torch_us=t_t * 1e6, max_diff=diff)
    if "time_jitter_300k" in ref:
        print("\nreference (numpy, one CPU core), RandomColorJitter with all four steps at 300,000 points: %.0f ms" % (ref["time_jitter_300k"] * 1e3))
    del master, work

    # ---- blur ----
    size = (300, 250, 130)
    pts = shell_voxels(n, size, 8)
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)       # noqa: E731
    gc = torch.from_numpy(pts.astype(np.int32)).to(dev)
    m = dict(color=r(n, 3) * 255, opacity=r(n, 1), scale=r(n, 3), quat=torch.randn(n, 4, device=dev, generator=g))
    mask = (m["opacity"] > 0.5).reshape(-1)
    w = {k: v.clone() for k, v in m.items()}

    def restore():
        for k in w:
            w[k].copy_(m[k])
    print("\n## voxel blur, %d voxels on the shell of a %d x %d x %d grid, %d masked, colour + opacity + scale + quat\n" % (n, *size, int(mask.sum())))
    print("| sigma | r | hash + gather (ss_voxel_blur) | dense grid in torch | dense / sparse | max difference (colour) | reference (scipy, CPU) |")
    print("|---|---|---|---|---|---|---|")
    for sigma in (0.5, 1.0, 2.0):
        t_k, _ = per_call(lambda: nv.voxel_blur_(gc, mask, w["color"], sigma, opacity=w["opacity"], scale=w["scale"], quat=w["quat"],
                                                 normalize_quat=False), restore, args.repeats)
        restore()
        nv.voxel_blur_(gc, mask, w["color"], sigma, opacity=w["opacity"], scale=w["scale"], quat=w["quat"], normalize_quat=False)
        t_d, diff = float("nan"), float("nan")
        if not args.skip_dense:
            arrays = [m["color"], m["opacity"], m["scale"], m["quat"]]
            t_d, _ = per_call(lambda: dense_blur(gc, mask, arrays, sigma, size), lambda: None, max(3, args.repeats // 3), warm=1)
            diff = float((dense_blur(gc, mask, arrays, sigma, size)[0] - w["color"]).abs().max())
        rt = ref.get("time_blur_sigma_%s" % sigma)
        print("| %.1f | %d | %.2f ms | %.2f ms | %.1fx | %.2g | %s |" % (sigma, int(2 * sigma + 0.5), t_k * 1e3, t_d * 1e3, t_d / t_k, diff,
                                                                       "-" if rt is None else "%.1f s" % rt))
        res["blur_sigma_%s" % sigma] = dict(sparse_ms=t_k * 1e3, dense_ms=t_d * 1e3, max_diff=diff)
    print("\nworkspace of the hash: %.1f MiB; the dense grid: %.0f MiB per copy" %
          (nv.lib().ss_voxel_blur_workspace_bytes(n) / 2 ** 20, 12 * size[0] * size[1] * size[2] * 4 / 2 ** 20))
    del m, w

    # ---- one generator call ----
    with open(os.path.join(ROOT, "tests", "golden", "ssl_configs.txt")) as f:
        cfg = ast.literal_eval(f.read())["configs/scannet/ssl-pretrain-scannet-all-base.py"]
    gcfg = next(c for c in cfg if c["type"] == "ContrastiveViewsGenerator_SSL")
    src = shell_sample(args.gen_n, dev)
    print("\n## one ContrastiveViewsGenerator_SSL call, %d Gaussians (the scannet ssl-pretrain list's generator as shipped)\n" % args.gen_n)
    print("| | device time | host wall time | rows of the views | views blurred (sigma) |")
    print("|---|---|---|---|---|")
    names = ("global_crop0", "global_crop1", "local_crop0", "local_crop1", "local_crop2")
    views = None
    for fuse in (True, False):
        gen = Compose([gcfg], fuse=fuse).transforms[0]
        if views is None:
            seed = 0                                     # the first seed whose draws blur global view 0 at sigma 0.9 .. 1.3 and a local view too
            while True:
                views = draw_views(gen, seed, src)
                sig = [p["sigma"] for v in views[2:] for p in v if "sigma" in p]
                if sig[0] is not None and 0.9 <= sig[0] <= 1.3 and any(x is not None for x in sig[2:]):
                    break
                seed += 1
            blurred = ["%.2f" % p["sigma"] if p.get("fired") else "-" for v in views[2:] for p in v if "sigma" in p]
        out = {}

        def call():
            out.clear()
            out.update(gen.apply({k: v for k, v in src.items()}, dict(views=views)))
        t_dev, t_wall = per_call(call, lambda: None, max(3, args.repeats // 2), warm=1)
        rows = [int(out["%s_coord" % v].shape[0]) for v in names]
        print("| Compose(fuse=%s) | %.1f ms | %.1f ms | %s | %s |" % (fuse, t_dev * 1e3, t_wall * 1e3, rows, blurred))
        res["generator_fuse_%s" % fuse] = dict(device_ms=t_dev * 1e3, wall_ms=t_wall * 1e3, rows=rows)
    if not args.skip_dense:
        tout = {}

        def tcall():
            tout.clear()
            tout.update(torch_generator(gcfg, views, src))
        t_dev, t_wall = per_call(tcall, lambda: None, 3, warm=1)
        trows = [int(tout["%s_coord" % v].shape[0]) for v in names]
        print("| the same lists and draws as torch ops (dense blur grid) | %.1f ms | %.1f ms | %s | |" % (t_dev * 1e3, t_wall * 1e3, trows))
        assert trows == rows, (trows, rows)
        res["generator_torch"] = dict(device_ms=t_dev * 1e3, wall_ms=t_wall * 1e3, rows=trows)
    if "time_generator_800k" in ref:
        print("reference (numpy / scipy, CPU, its own draws): %.1f s" % ref["time_generator_800k"])
    print()
    print(json.dumps(dict(bench="ssl_views", n=n, gen_n=args.gen_n, **res)))


if __name__ == "__main__":
    main()
