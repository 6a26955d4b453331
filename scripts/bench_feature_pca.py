#!/usr/bin/env python
"""PCA colours of a feature matrix (pointcept_api.feature_pca, csrc/feature_pca.hip) at 200,000 and 1,000,000 rows of 768 fp32
features that are already on the device (clustered unit rows with a common mean, drawn on the device from a seed).  Per size:

  kernels   each entry point alone on resident data with its workspace allocated beforehand: --iters back-to-back launches between one
            HIP event pair after a warm-up, median of 5 windows.  The Gram matrix as TFLOP/s over the tile pairs it computes
            (pairs x 128 x 128 x 2 N) and as a share of the 157 TFLOP/s fp32 matrix peak; the passes over all rows as bytes read and
            written against the 8 TB/s peak.
  call      one pca_colors(features) end to end, a host clock around work that ends in a device synchronise, median of --repeats.
  torch     the same quantities from library calls on the device, measured the same way in the same process: mean, x.T @ x,
            x @ comp.T, amin and amax (no shift, no fp64 combination, not reproducible run to run).
  numpy     the host form in fp32 (what scikit-learn's covariance_eigh solver does): the download it needs, mean, centred Gram, eigh,
            projection, colours.

The colours of the device form and of the numpy form are compared before anything is timed.  There is no pass / fail bar on time.
Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line per size."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12
PEAK_F32_MATRIX = 157e12


def median(v):
    return sorted(v)[len(v) // 2]


def features(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(6, d, device="cuda", generator=g), dim=1)
    w = torch.tensor([0.30, 0.24, 0.18, 0.13, 0.09, 0.06], device="cuda")
    lab = torch.multinomial(w, n, replacement=True, generator=g)
    common = torch.nn.functional.normalize(torch.randn(1, d, device="cuda", generator=g), dim=1)
    x = centres[lab]
    x += (0.35 / d ** 0.5) * torch.randn(n, d, device="cuda", generator=g)
    x += 3.0 * common
    return torch.nn.functional.normalize(x, dim=1).contiguous()


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
    return median(out)


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


def numpy_form(x_dev, k):
    """-> (colours, seconds of the download, of the rest)"""
    t0 = time.perf_counter()
    x = x_dev.cpu().numpy()
    t1 = time.perf_counter()
    m = x.mean(axis=0)
    xc = x - m
    w, v = np.linalg.eigh((xc.T @ xc) / np.float32(len(x) - 1))
    comp = v[:, np.argsort(-w, kind="stable")[:k]].T.copy()
    for row in comp:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1
    y = xc @ comp.T
    mn = y.min(axis=0)
    r = y.max(axis=0) - mn
    r[r == 0] = 1
    colours = np.clip((y - mn) / r, 0, 1)
    return colours, t1 - t0, time.perf_counter() - t1


def run(n, d, k, iters, repeats):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import pca_colors
    x = features(n, d, 1)
    out = pca_colors(x, n_components=k)
    ref, _, _ = numpy_form(x, k)
    diff = float(np.abs(out["colors"].cpu().numpy() - ref).max())
    shift = torch.from_numpy(out["mean"].astype(np.float32)).cuda()
    comp = torch.from_numpy(out["components"].astype(np.float32)).cuda()
    off = torch.zeros(k, device="cuda")
    lib = nv.lib()
    ws_g = torch.empty(nv.pca_gram_workspace_bytes(n, d), dtype=torch.uint8, device="cuda")
    ws_s = torch.empty(lib.ss_pca_col_sums_workspace_bytes(n, d), dtype=torch.uint8, device="cuda")
    ws_p = torch.empty(max(lib.ss_pca_project_workspace_bytes(n), 256), dtype=torch.uint8, device="cuda")
    y, ext = nv.pca_project(x, comp, shift, off, workspace=ws_p)
    t = dict(col_sums=event_ms(lambda: nv.pca_col_sums(x, shift, workspace=ws_s), iters),
             gram=event_ms(lambda: nv.pca_gram(x, shift, workspace=ws_g), iters),
             project=event_ms(lambda: nv.pca_project(x, comp, shift, off, workspace=ws_p), iters),
             colors=event_ms(lambda: nv.pca_colors(y, ext), iters))
    ntiles = (d + 127) // 128
    pairs = ntiles * (ntiles + 1) // 2
    gram_flop = pairs * 128 * 128 * 2 * n
    item = x.element_size()
    traffic = dict(col_sums=n * d * item, project=n * d * item + n * k * 4, colors=n * k * 4 + n * 12)
    call = host_ms(lambda: pca_colors(x, n_components=k), repeats)
    tt = dict(mean=event_ms(lambda: x.mean(0), iters), gram=event_ms(lambda: x.T @ x, iters),
              project=event_ms(lambda: x @ comp.T, iters), extremes=event_ms(lambda: (y.amin(0), y.amax(0)), iters))
    _, t_down, t_rest = numpy_form(x, k)
    print(f"\n### {n:,} x {d} fp32, k = {k} (workspace of the Gram matrix: {ws_g.numel() / 2 ** 20:.1f} MiB, "
          f"{nv.pca_gram_share_rows(n, d):,} rows per share)\n")
    print(f"colours of the device form against the fp32 numpy form: largest difference {diff:.3g}\n")
    print("| kernel | ms | rate | share of peak |\n|---|---|---|---|")
    print(f"| `ss_pca_gram` | {t['gram']:.3f} | {gram_flop / t['gram'] / 1e9:.1f} TFLOP/s over {pairs} tile pairs | "
          f"{gram_flop / (t['gram'] * 1e-3) / PEAK_F32_MATRIX:.2f} of 157 TFLOP/s |")
    for name in ("col_sums", "project", "colors"):
        rate = traffic[name] / (t[name] * 1e-3)
        print(f"| `ss_pca_{name}` | {t[name]:.3f} | {rate / 1e12:.2f} TB/s | {rate / PEAK_BYTES_PER_S:.2f} of 8 TB/s |")
    print("\n| form | ms |\n|---|---|")
    print(f"| `pca_colors` end to end (two column-sum passes, Gram, eigh on the host, projection, colours) | {call:.1f} |")
    print(f"| torch on the device: `mean` {tt['mean']:.3f} + `x.T @ x` {tt['gram']:.3f} + `x @ comp.T` {tt['project']:.3f} + "
          f"`amin` / `amax` {tt['extremes']:.3f} | {sum(tt.values()):.3f} |")
    print(f"| numpy on the host in fp32: download {t_down * 1e3:.0f} + the rest {t_rest * 1e3:.0f} | {(t_down + t_rest) * 1e3:.0f} |")
    print(json.dumps(dict(n=n, d=d, k=k, kernels_ms=t, gram_tflops=gram_flop / t["gram"] / 1e9, call_ms=call, torch_ms=tt,
                          numpy_download_ms=t_down * 1e3, numpy_rest_ms=t_rest * 1e3, colour_difference=diff)), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=[200_000, 1_000_000])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--components", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_pca needs a GPU: there is no CPU path")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for n in args.rows:
        run(n, args.dim, args.components, args.iters, args.repeats)


if __name__ == "__main__":
    main()
