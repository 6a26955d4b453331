#!/usr/bin/env python
"""Text queries on scene features (pointcept_api.text_query, csrc/text_query.hip) at 200,000 and 1,000,000 rows of 768 fp16 features
that are already on the device, against Q = 1, 8 and 32 unit text embeddings (both drawn on the device from a seed).  Per size and Q:

  kernels   each entry point alone on resident data with its workspace allocated beforehand: --iters back-to-back launches between one
            HIP event pair after a warm-up; the median and the spread (min .. max) of 5 windows.  The score pass as bytes read and
            written over time against the 8 TB/s peak, and as fp32 MFMA work (the tile always holds 32 query slots: 64 N Dp FLOP)
            against the 157 TFLOP/s fp32 matrix peak.  The select pass with a threshold only, and with a cap that binds (top-k).
  call      one query_scene(features, embeddings) per method end to end, a host clock around work that ends in a device synchronise,
            median of --repeats.
  torch     the same answers from library calls on the device, measured the same way in the same process:
            F.normalize(x.float()) @ t.T, then >= and nonzero per query, or torch.topk and a sort of its rows.

The selections of the two forms are compared before anything is timed (the scores differ in their last bits, so a row whose score is
within 1e-5 of the threshold may differ; the count of such rows is printed).  There is no pass / fail bar on time.
Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line per size and Q."""
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
import torch.nn.functional as F  # noqa: E402

PEAK_BYTES_PER_S = 8e12
PEAK_F32_MATRIX = 157e12
THRESHOLD = 0.15
TOPK = 30000


def median(v):
    return sorted(v)[len(v) // 2]


def inputs(n, d, q, seed):
    """unit text rows; features = a text row of a 32-row bank (or none) plus noise: a few per cent of the rows answer each query"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bank = F.normalize(torch.randn(32, d, device="cuda", generator=g), dim=1)
    lab = torch.randint(0, 64, (n,), device="cuda", generator=g)
    x = (1.0 / d ** 0.5) * torch.randn(n, d, device="cuda", generator=g)
    hit = lab < 32
    x[hit] += 0.5 * bank[lab[hit]]
    return x.half().contiguous(), bank[:q].contiguous()


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


def torch_scores(x, t):
    return F.normalize(x.float(), dim=1) @ t.T                           # (N, Q)


def torch_threshold(x, t):
    s = torch_scores(x, t)
    return [torch.nonzero(s[:, q] >= THRESHOLD).squeeze(1) for q in range(t.shape[0])]


def torch_topk(x, t, k):
    s = torch_scores(x, t)
    return [torch.sort(torch.topk(s[:, q], k).indices).values for q in range(t.shape[0])]


def run(n, d, q, iters, repeats):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import query_scene
    x, t = inputs(n, d, q, 1)
    k = min(TOPK, n)
    out = query_scene(x, t, method="threshold", threshold=THRESHOLD, return_scores=True)
    ref = torch_threshold(x, t)
    near = int(((out["scores"] - THRESHOLD).abs() < 1e-5).sum())
    differ = 0
    for a, b in zip(out["indices"], ref):
        ma, mb = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
        ma[a.long()] = True
        mb[b] = True
        differ += int((ma ^ mb).sum())
    scores = out["scores"]
    ws_s = torch.empty(max(nv.query_scores_workspace_bytes(n, q), 256), dtype=torch.uint8, device="cuda")
    ws_l = torch.empty(max(nv.query_select_workspace_bytes(n, q), 256), dtype=torch.uint8, device="cuda")
    tau, nocap, cap = np.full(q, THRESHOLD, dtype=np.float32), np.full(q, -1), np.full(q, k)
    bitmap, _, counts = nv.query_select(scores, tau, nocap, workspace=ws_l)
    tile_base, _ = nv.pc_compact_scan(bitmap, n)
    total = int(counts.sum())
    kt = dict(scores=event_ms(lambda: nv.query_scores(x, t, workspace=ws_s), iters),
              select_threshold=event_ms(lambda: nv.query_select(scores, tau, nocap, workspace=ws_l), iters),
              select_topk=event_ms(lambda: nv.query_select(scores, np.full(q, -np.inf, dtype=np.float32), cap, workspace=ws_l), iters),
              compact=event_ms(lambda: (nv.pc_compact_scan(bitmap, n), nv.pc_compact(bitmap, n, tile_base, total)), iters),
              best=event_ms(lambda: nv.query_best(scores, bitmap), iters))
    calls = dict(threshold=host_ms(lambda: query_scene(x, t, method="threshold", threshold=THRESHOLD), repeats),
                 adaptive=host_ms(lambda: query_scene(x, t, method="adaptive"), repeats),
                 topk=host_ms(lambda: query_scene(x, t, method="topk", k=k), repeats))
    tt = dict(scores=event_ms(lambda: torch_scores(x, t), iters),
              threshold=host_ms(lambda: torch_threshold(x, t), repeats), topk=host_ms(lambda: torch_topk(x, t, k), repeats))
    dp = (d + 63) // 64 * 64
    traffic = n * d * x.element_size() + q * n * 4
    ms = kt["scores"][0]
    print(f"\n### {n:,} x {d} fp16, Q = {q}\n")
    print(f"threshold {THRESHOLD}: {total:,} rows selected over the {q} queries; rows that differ from the torch form: {differ} "
          f"({near} scores lie within 1e-5 of the threshold)\n")
    print("| kernel | ms (median of 5 windows) | min .. max | rate |\n|---|---|---|---|")
    print(f"| `ss_query_scores` | {ms:.3f} | {kt['scores'][1]:.3f} .. {kt['scores'][2]:.3f} | {traffic / ms / 1e9:.2f} TB/s = "
          f"{traffic / (ms * 1e-3) / PEAK_BYTES_PER_S:.2f} of 8 TB/s; {64 * n * dp / ms / 1e9:.1f} TFLOP/s of MFMA = "
          f"{64 * n * dp / (ms * 1e-3) / PEAK_F32_MATRIX:.2f} of 157 TFLOP/s |")
    for name, what in (("select_threshold", "threshold only"), ("select_topk", f"the {k:,} best"), ("compact", "bitmaps -> rows"),
                       ("best", "best query per row")):
        print(f"| `{name}` ({what}) | {kt[name][0]:.3f} | {kt[name][1]:.3f} .. {kt[name][2]:.3f} | |")
    print("\n| form | ms |\n|---|---|")
    for m in ("threshold", "adaptive", "topk"):
        print(f"| `query_scene(method=\"{m}\")` end to end | {calls[m]:.2f} |")
    print(f"| torch: `F.normalize(x.float()) @ t.T` alone (device events) | {tt['scores'][0]:.3f} ({tt['scores'][1]:.3f} .. "
          f"{tt['scores'][2]:.3f}) |")
    print(f"| torch: scores, `>=`, `nonzero` per query, end to end | {tt['threshold']:.2f} |")
    print(f"| torch: scores, `topk({k})`, sort per query, end to end | {tt['topk']:.2f} |")
    print(json.dumps(dict(n=n, d=d, q=q, kernels_ms={a: b[0] for a, b in kt.items()}, kernels_spread={a: b[1:] for a, b in kt.items()},
                          scores_tb_per_s=traffic / ms / 1e9, call_ms=calls, torch_scores_ms=tt["scores"][0],
                          torch_threshold_ms=tt["threshold"], torch_topk_ms=tt["topk"], rows_differing=differ, near_threshold=near)),
          flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=[200_000, 1_000_000])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--queries", type=int, nargs="+", default=[1, 8, 32])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_query needs a GPU: there is no CPU path")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for n in args.rows:
        for q in args.queries:
            run(n, args.dim, q, args.iters, args.repeats)


if __name__ == "__main__":
    main()
