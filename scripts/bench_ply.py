#!/usr/bin/env python
"""One synthetic 3DGS checkpoint (default 1,000,000 Gaussians, the standard 62-float vertex of 248 bytes) written to a temporary folder
and read back page-cached, decoded into coord / color / opacity / scale / quat in two forms:

  numpy   the reference-shaped form: the vertex block viewed through a structured dtype (what plyfile hands out), fourteen strided
          column extractions, then exp, the sigmoid, the row norm, the sign flip and the colour quantisation as separate numpy passes.
  device  pointcept_api.gaussian_ply.load_gaussian_ply: file -> pinned -> device in pieces, one ss_ply_decode launch per piece.

Each form is run --repeats times after a warm-up run (which also brings the file into the page cache) and timed with a host clock around
work that ends in a device synchronise.  The device form's two host steps are also timed on their own, written out in the script as the
loader does them: the file read into a pinned buffer, and the copy of that buffer to the device (waited for).

  decode  ss_ply_decode alone over the whole resident vertex block: --iters back-to-back launches between one HIP event pair, median of
          7 windows; bytes/s of RECORDS READ (n x 248; the 51 output bytes per row are not counted) as a share of the 8 TB/s peak, and
          beside it ss_gather_rows on the `gather_hbm` probe of bench.py's roofline block (scripts/roofline_probes.py), timed the same way.

The two forms are compared before anything is timed (coord / color / quat bytes; scale / opacity within 5 fp32 ulp of each other).
Needs a GPU: there is no CPU path.  Prints a markdown table and one JSON line."""
import argparse
import importlib.util
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
NAMES = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)] + ["opacity"]
         + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])
DTYPE = np.dtype([(k, "<f4") for k in NAMES])


def median(v):
    return sorted(v)[len(v) // 2]


def write_checkpoint(path, n, seed=0):
    g = np.random.default_rng(seed)
    raw = g.standard_normal((n, len(NAMES)), dtype=np.float32)
    cols = {k: i for i, k in enumerate(NAMES)}
    raw[:, :3] *= 5
    raw[:, cols["opacity"]] *= 4
    raw[:, cols["scale_0"]:cols["scale_0"] + 3] = g.uniform(-8, 1, (n, 3)).astype(np.float32)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n" % (n, "".join(f"property float {k}\n" for k in NAMES))
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(raw.tobytes())
    return len(head), raw.nbytes


def numpy_form(path, offset, n):
    """read_gaussian_attributes as the reference writes it, on a structured view of the file's bytes"""
    with open(path, "rb") as f:
        f.seek(offset)
        vertex = np.frombuffer(f.read(n * DTYPE.itemsize), dtype=DTYPE, count=n)
    data = {}
    data["coord"] = np.stack((vertex["x"].astype(np.float32), vertex["y"].astype(np.float32), vertex["z"].astype(np.float32)), axis=-1)
    data["opacity"] = 1 / (1 + np.exp(-vertex["opacity"].astype(np.float32)))
    scales = np.zeros((n, 3), dtype=np.float32)
    for i in range(3):
        scales[:, i] = vertex[f"scale_{i}"].astype(np.float32)
    data["scale"] = np.exp(scales)
    rots = np.zeros((n, 4), dtype=np.float32)
    for i in range(4):
        rots[:, i] = vertex[f"rot_{i}"].astype(np.float32)
    rots = rots / (np.linalg.norm(rots, axis=1, keepdims=True) + 1e-9)
    data["quat"] = rots * np.sign(rots[:, 0])[:, None]
    dc = np.zeros((n, 3, 1), dtype=np.float32)
    for i in range(3):
        dc[:, i, 0] = vertex[f"f_dc_{i}"].astype(np.float32)
    pc = (dc.reshape(-1, 3) * 0.28209479177387814).astype(np.float32) + 0.5
    data["color"] = (np.clip(pc, 0, 1) * 255).astype(np.uint8)
    return data


def device_form(path):
    from scenesplat_amd.pointcept_api import gaussian_ply as gp
    out = gp.load_gaussian_ply(path, "cuda")
    torch.cuda.synchronize()
    return out


def host_steps(path, offset, nbytes, repeats):
    """medians of the seconds of (pinned allocation, file read into it, upload) as load_gaussian_ply does them"""
    alloc, read, up = [], [], []
    stage = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for _ in range(repeats):
        t0 = time.perf_counter()
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        alloc.append(time.perf_counter() - t0)
        view = host.numpy()
        with open(path, "rb", buffering=0) as f:
            f.seek(offset)
            t0 = time.perf_counter()
            assert f.readinto(memoryview(view)) == nbytes
            read.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage.copy_(host, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        up.append(time.perf_counter() - t0)
        del host, view
    return median(alloc), median(read), median(up)


def event_windows(run, iters, windows=7):
    """median over `windows` of the average launch time (ms) of `iters` back-to-back launches between one HIP event pair"""
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-gather", action="store_true", help="skip the ss_gather_rows probe (it builds a 2.5 GB working set)")
    args = ap.parse_args()
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import gaussian_ply as gp

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "point_cloud.ply")
        offset, nbytes = write_checkpoint(path, args.n)
        header = gp.read_ply_header(path)
        assert (header.count, header.stride, header.data_offset) == (args.n, DTYPE.itemsize, offset)
        ref, dev = numpy_form(path, offset, args.n), {k: v.cpu().numpy() for k, v in device_form(path).items()}
        for k in ("coord", "color", "quat"):
            assert ref[k].tobytes() == dev[k].tobytes(), k
        for k in ("scale", "opacity"):
            apart = np.abs(ref[k].view(np.int32).astype(np.int64) - dev[k].view(np.int32).astype(np.int64)).max()
            assert apart <= 5, (k, apart)             # (numpy's fp32 sigmoid lies up to 3.2 ulp from the fp64 value, the device half an ulp)

        rows = {}
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            numpy_form(path, offset, args.n)
            t.append(time.perf_counter() - t0)
        rows["numpy"] = dict(total=median(t))
        t = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_form(path)
            t.append(time.perf_counter() - t0)
        alloc, read, up = host_steps(path, offset, nbytes, args.repeats)
        rows["device"] = dict(total=median(t), pinned_alloc=alloc, read=read, upload=up)

        # the kernel alone, on the resident vertex block
        with open(path, "rb") as f:
            f.seek(offset)
            block = torch.frombuffer(bytearray(f.read(nbytes)), dtype=torch.uint8).cuda()
        offsets, n_scale, n_rot = gp.gaussian_columns(header)
        n = args.n
        out = (torch.empty((n, 3), device="cuda"), torch.empty((n, 3), dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda"),
               torch.empty((n, n_scale), device="cuda"), torch.empty((n, n_rot), device="cuda"))
        ms = event_windows(lambda: nv.ply_decode(block, n, header.stride, offsets, n_scale, n_rot, *out), args.iters)
        # (a piece that starts 8 mod 16: the 8-byte loads)
        ms4 = event_windows(lambda: nv.ply_decode(block[header.stride:], n - 1, header.stride, offsets, n_scale, n_rot, *out), args.iters)
        decode = dict(ms=ms, bytes_read=nbytes, gb_per_s=nbytes / ms / 1e6, frac_of_peak=nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S,
                      ms_8byte_path=ms4, gb_per_s_8byte_path=(nbytes - header.stride) / ms4 / 1e6,
                      gb_per_s_read_and_written=(nbytes + n * 51) / ms / 1e6)
        # (the 248 MB block fits the 256 MiB Infinity Cache: the same records four times over do not)
        reps = 4
        big = block.repeat(reps)
        out = (torch.empty((reps * n, 3), device="cuda"), torch.empty((reps * n, 3), dtype=torch.uint8, device="cuda"), torch.empty(reps * n, device="cuda"),
               torch.empty((reps * n, n_scale), device="cuda"), torch.empty((reps * n, n_rot), device="cuda"))
        msb = event_windows(lambda: nv.ply_decode(big, reps * n, header.stride, offsets, n_scale, n_rot, *out), max(2, args.iters // reps))
        decode.update(ms_beyond_cache=msb, n_beyond_cache=reps * n, gb_per_s_beyond_cache=reps * nbytes / msb / 1e6,
                      frac_of_peak_beyond_cache=reps * nbytes / (msb * 1e-3) / PEAK_BYTES_PER_S)
        del block, big, out
        gather = None
        if not args.no_gather:
            spec = importlib.util.spec_from_file_location("roofline_probes", os.path.join(ROOT, "scripts", "roofline_probes.py"))
            rp = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(rp)
            p = rp.build(which=("gather_hbm",))[0]
            gms = event_windows(p["run"], 10)
            gather = dict(ms=gms, bytes=p["bytes"], gb_per_s=p["bytes"] / gms / 1e6, frac_of_peak=p["bytes"] / (gms * 1e-3) / PEAK_BYTES_PER_S, note=p["note"])

    print("| form | total ms | pinned allocation ms | file read ms | upload ms |")
    print("|---|---|---|---|---|")
    print("| numpy | %.1f | | | |" % (rows["numpy"]["total"] * 1e3))
    print("| device | %.1f | %.1f | %.1f | %.1f |" % tuple(rows["device"][k] * 1e3 for k in ("total", "pinned_alloc", "read", "upload")))
    print("ss_ply_decode: %.3f ms, %.0f GB/s of records read (%.1f %% of 8 TB/s); 8-byte path %.3f ms, %.0f GB/s" % (
        decode["ms"], decode["gb_per_s"], 100 * decode["frac_of_peak"], decode["ms_8byte_path"], decode["gb_per_s_8byte_path"]))
    print("ss_ply_decode over %d records (beyond the Infinity Cache): %.3f ms, %.0f GB/s (%.1f %% of 8 TB/s)" % (
        decode["n_beyond_cache"], decode["ms_beyond_cache"], decode["gb_per_s_beyond_cache"], 100 * decode["frac_of_peak_beyond_cache"]))
    if gather:
        print("ss_gather_rows (gather_hbm probe): %.3f ms, %.0f GB/s (%.1f %% of 8 TB/s)" % (gather["ms"], gather["gb_per_s"], 100 * gather["frac_of_peak"]))
    print(json.dumps(dict(n=args.n, record_bytes=DTYPE.itemsize, forms=rows, decode=decode, gather_rows=gather,
                          speedup=rows["numpy"]["total"] / rows["device"]["total"])))


if __name__ == "__main__":
    main()
