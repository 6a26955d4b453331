#!/usr/bin/env python
"""The headless splat renderer (pointcept_api.render, csrc/splat.hip) on a synthetic room of 200,000 and 1,000,000 Gaussians that are
already on the device, 1280 x 720, fitted "iso" camera, both modes.  Per size and mode:

  kernels   each entry point alone on resident data, called through the C interface with every output and workspace allocated
            beforehand (the argsort through its wrapper, which allocates its buffers per call): --iters back-to-back launches between
            one HIP event pair after a warm-up; the median and the spread (min .. max) of 5 windows.  A step of a few microseconds is
            bound by the rate at which the host launches, not by the kernel: the figure is an upper bound on the kernel's time.
            P = the (Gaussian, tile) pairs of the view; pairs sorted per second = P over the argsort's time;
            pixel-Gaussian evaluations per second = 256 P over the composite's time (an upper figure: a tile whose 256 pixels have all
            stopped leaves its list early, so fewer evaluations than 256 P are made).
  call      one render_scene(scene on the device, camera) end to end, a host clock around work that ends in a device synchronise,
            median of --repeats; the composite kernel's share of it.
  agg       for orientation only: matplotlib's Agg backend drawing a 3-D scatter of a 10 % sample of the same scene offscreen into a
            1280 x 720 file (what the reference's matplotlib backend shows in a window).  A number to report, not a bar to pass.

Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line per size and mode."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTH, HEIGHT = 1280, 720


def median(v):
    return sorted(v)[len(v) // 2]


def room(n, seed):
    """n Gaussians on the floor, the four walls and a few boxes of an 8 x 6 x 3 m room: flat discs of 1 to 6 cm lying in their surface"""
    rng = np.random.default_rng(seed)
    size = np.array([8.0, 6.0, 3.0])
    face = rng.integers(0, 6, n)                                         # floor twice as dense as a wall; 5: furniture
    p = rng.uniform(0.0, 1.0, (n, 3)) * size
    normal_axis = np.where(face <= 1, 2, np.where(face <= 3, 0, 1))
    normal_axis = np.where(face == 5, rng.integers(0, 3, n), normal_axis)
    side = rng.integers(0, 2, n)
    rows = np.arange(n)
    p[rows, normal_axis] = np.where(face <= 1, 0.0, side * size[normal_axis])
    boxes = face == 5
    centre = rng.uniform([1.0, 1.0, 0.0], [7.0, 5.0, 0.0], (8, 3))[rng.integers(0, 8, n)]
    p[boxes] = (centre + rng.uniform(-0.5, 0.5, (n, 3)) * [1.0, 1.0, 0.0] + rng.uniform(0, 1, (n, 1)) * [0, 0, 0.9])[boxes]
    scale = np.exp(rng.uniform(np.log(0.01), np.log(0.06), (n, 3)))
    scale[rows, normal_axis] *= 0.1
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)) + 0.05 * rng.standard_normal((n, 4))
    color = np.clip(0.5 + 0.5 * np.sin(p * [1.3, 1.7, 2.1] + face[:, None]), 0, 1)
    return dict(coord=p.astype(np.float32), scale=scale.astype(np.float32), quat=quat.astype(np.float32),
                opacity=rng.uniform(0.3, 1.0, n).astype(np.float32), color=color.astype(np.float32))


def event_ms(fn, iters, windows=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return median(out), min(out), max(out)


def host_ms(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return median(out)


def agg_ms(scene, repeats):
    """matplotlib (Agg): a 3-D scatter of a 10 % sample into a 1280 x 720 file"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    rng = np.random.default_rng(0)
    n = len(scene["coord"])
    idx = rng.choice(n, n // 10, replace=False)
    xyz, col = scene["coord"][idx], scene["color"][idx]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(repeats + 1):
            t = time.perf_counter()
            fig = plt.figure(figsize=(WIDTH / 100.0, HEIGHT / 100.0), dpi=100)
            ax = fig.add_subplot(111, projection="3d")
            ax.scatter(xyz[:, 0], xyz[:, 1], xyz[:, 2], c=col, s=1, alpha=0.6)
            fig.savefig(os.path.join(tmp, f"agg_{k}.png"))
            plt.close(fig)
            out.append((time.perf_counter() - t) * 1e3)
    return median(out[1:])


def run(n, mode, iters, repeats, save):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import render as rd
    host = room(n, 1)
    scene = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    cam = rd.fit_camera(host["coord"], WIDTH, HEIGHT, 60.0, "iso")
    block = cam.packed()
    tiles_x, tiles_y = -(-WIDTH // rd.TILE), -(-HEIGHT // rd.TILE)
    args = (scene["coord"], scene["scale"], scene["quat"], scene["opacity"], scene["color"], block, mode)
    proj = nv.splat_project(*args)
    ws = torch.empty(max(nv.splat_offsets_workspace_bytes(n), 256), dtype=torch.uint8, device="cuda")
    offsets, totals = nv.splat_offsets(proj["tiles_touched"], workspace=ws)
    P, visible = (int(v) for v in totals.tolist())
    keys, rows = nv.splat_keys(proj["depth"], proj["rect"], proj["tiles_touched"], offsets, P, tiles_x, tiles_y)
    key_bits = 32 + (tiles_x * tiles_y - 1).bit_length()
    order, _, skeys = nv.argsort_i64(keys.view(1, P), key_bits, want_inverse=False, want_sorted=True)
    ranges, sorted_rows = nv.splat_ranges(skeys.view(P), order.view(P), rows, tiles_x * tiles_y)
    out = tuple(torch.empty(s, dtype=torch.float32, device="cuda") for s in ((HEIGHT, WIDTH, 3), (HEIGHT, WIDTH), (HEIGHT, WIDTH)))
    bg = (1.0, 1.0, 1.0)
    lens = (ranges[:, 1] - ranges[:, 0]).float()
    lib, stream = nv.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def direct(fn, *a):
        """the C entry point on buffers that exist already: no allocation, no validation in Python"""
        def go():
            rc = fn(*a, stream)
            assert rc == 0, rc
        return go

    kt = dict(project=event_ms(direct(lib.ss_splat_project, ptr(scene["coord"]), ptr(scene["scale"]), ptr(scene["quat"]), ptr(scene["opacity"]),
                                      ptr(scene["color"]), n, block.ctypes.data, nv.SPLAT_MODES[mode], 1.0, 2.0, ptr(proj["mean2d"]),
                                      ptr(proj["conic_opacity"]), ptr(proj["depth"]), ptr(proj["rect"]), ptr(proj["radius"]),
                                      ptr(proj["tiles_touched"])), iters),
              offsets=event_ms(direct(lib.ss_splat_offsets, ptr(proj["tiles_touched"]), n, ptr(offsets), ptr(totals), ptr(ws), ws.numel()), iters),
              keys=event_ms(direct(lib.ss_splat_keys, ptr(proj["depth"]), ptr(proj["rect"]), ptr(proj["tiles_touched"]), ptr(offsets), n, P,
                                   tiles_x, tiles_y, ptr(keys), ptr(rows)), iters),
              argsort=event_ms(lambda: nv.argsort_i64(keys.view(1, P), key_bits, want_inverse=False, want_sorted=True), iters),
              ranges=event_ms(direct(lib.ss_splat_ranges, ptr(skeys), ptr(order), ptr(rows), P, tiles_x * tiles_y, ptr(ranges), ptr(sorted_rows)),
                              iters),
              composite=event_ms(lambda: nv.splat_composite(proj["mean2d"], proj["conic_opacity"], scene["color"], proj["depth"], ranges,
                                                            sorted_rows, WIDTH, HEIGHT, bg, out=out), iters))
    call = host_ms(lambda: rd.render_scene(scene, cam, mode=mode), repeats)
    res = rd.render_scene(scene, cam, mode=mode)
    if save:
        os.makedirs(save, exist_ok=True)
        rd.save_image(os.path.join(save, f"room_{n}_{mode}.png"), res["image"])
    agg = agg_ms(host, 2) if mode == "pointcloud" else None
    comp = kt["composite"][0]
    print(f"\n### {n:,} Gaussians, {mode}, {WIDTH} x {HEIGHT}\n")
    print(f"{visible:,} rows in view, P = {P:,} pairs over {tiles_x * tiles_y:,} tiles (longest list {int(lens.max()):,}, mean {float(lens.mean()):.0f}); "
          f"mean alpha of the image {float(res['alpha'].mean()):.3f}\n")
    print("| kernel | ms (median of 5 windows) | min .. max | rate |\n|---|---|---|---|")
    rates = dict(project=f"{n / kt['project'][0] / 1e6:.2f} G rows/s", argsort=f"{P / kt['argsort'][0] / 1e6:.2f} G pairs sorted/s",
                 composite=f"{256.0 * P / comp / 1e6:.1f} G pixel-Gaussian evaluations/s (upper figure)")
    for name in ("project", "offsets", "keys", "argsort", "ranges", "composite"):
        m = kt[name]
        print(f"| `{name}` | {m[0]:.3f} | {m[1]:.3f} .. {m[2]:.3f} | {rates.get(name, '')} |")
    total = sum(v[0] for v in kt.values())
    print(f"\n| form | ms |\n|---|---|\n| the six steps, summed | {total:.3f} |\n| `render_scene` end to end | {call:.2f} |")
    print(f"| the composite kernel's share of the call | {comp / call:.2f} |")
    if agg is not None:
        print(f"| matplotlib Agg, 3-D scatter of {n // 10:,} sampled points into a {WIDTH} x {HEIGHT} file (for orientation) | {agg:.0f} |")
    print(json.dumps(dict(n=n, mode=mode, pairs=P, visible=visible, kernels_ms={a: b[0] for a, b in kt.items()},
                          kernels_spread={a: b[1:] for a, b in kt.items()}, call_ms=call, composite_share=comp / call,
                          pairs_sorted_per_s=P / kt["argsort"][0] * 1e3, evaluations_per_s_upper=256.0 * P / comp * 1e3, agg_ms=agg)),
          flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=[200_000, 1_000_000])
    p.add_argument("--modes", nargs="+", default=["gaussians", "pointcloud"])
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--save", help="a folder for the rendered images")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat needs a GPU: there is no CPU path")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for n in args.rows:
        for mode in args.modes:
            run(n, mode, args.iters, args.repeats, args.save)


if __name__ == "__main__":
    main()
