#!/usr/bin/env python
"""The kernels behind HueSaturationTranslation, NormalizeCoord and InstanceParser (csrc/augment.hip), timed at n = 200,000 and
n = 2,000,000 rows, and InstanceParser as a call against the same parse written with torch ops.

  kernels  --iters back-to-back launches between one HIP event pair, each launch on the next of enough copies of its input that
           the copies together exceed 600 MiB (more than the 256 MiB Infinity Cache: no launch finds its rows in cache); median
           over the windows, and the bytes the algorithm moves over that time as a share of the 8 TB/s peak:
             ss_aug_hsv            colour read and written, 24 bytes per row
             ss_aug_moments        coord read, 12 bytes per row (the partials and the finish are a few KiB)
             ss_instance_boxes     order read and coord gathered through it, 16 bytes per row (300 instances, the rows in random order)
             ss_instance_scatter   cluster read, instance (int64) and centroid written, 24 bytes per row
  parser   InstanceParser.apply on 300 instances (one call: isin, the id range readback, radix argsort, partition, K readback, the
           two kernels) against a torch restatement on the device: unique(return_inverse) and one masked min / max / mean per
           instance, as the reference loops.  One event pair per call, median over --repeats calls after warm-up; call times with
           their host syncs, not kernel times.

Needs a GPU: there is no CPU path.  Prints markdown tables and one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12
INSTANCES = 300


def median(v):
    return sorted(v)[len(v) // 2]


def sample(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return dict(coord=torch.rand(n, 3, device=dev, generator=g) * torch.tensor([8.0, 6.0, 3.0], device=dev),
                color=torch.rand(n, 3, device=dev, generator=g) * 255,
                segment=torch.randint(-1, 20, (n,), device=dev, generator=g),
                instance=torch.randint(0, INSTANCES, (n,), device=dev, generator=g) * 3 - 1)      # ids with gaps, -1 among them


def windows(fn, sets, iters, repeats):
    for k in range(min(sets, 10)):
        fn(k)
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(iters):
            fn(i % sets)
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / iters)
    return us


def time_kernels(n, dev, iters, repeats, resident_mib):
    import ctypes
    from scenesplat_amd import native as nv
    sets = max(2, -(-resident_mib * (1 << 20) // (12 * n)))
    ds = [sample(n, dev, k) for k in range(sets)]
    lib, stream = nv.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    hs = (ctypes.c_double * 2)(0.13, 1.1)
    aff = (ctypes.c_double * 12)(0.9, -0.1, 0.0, 0.1, 0.9, 0.0, 0.0, 0.0, 1.0, -4.0, -3.0, -1.5)
    part = torch.empty((lib.ss_aug_moments_blocks(n), 4), dtype=torch.float64, device=dev)
    out4 = torch.empty(4, dtype=torch.float64, device=dev)
    # the CSR of every copy, built once outside the timed region
    csr = []
    for d in ds:
        key = d["instance"].long() + 1
        order = nv.argsort_i64(key[None], 12, want_inverse=False, want_sorted=False)[0][0]
        cluster, idx_ptr, _, n_out = nv.pool_partition(key, order, 0)
        csr.append((order, idx_ptr, cluster, int(n_out.item())))
    bbox = torch.empty((INSTANCES, 8), device=dev)
    cen = torch.empty((INSTANCES, 3), device=dev)
    inst_out = torch.empty(n, dtype=torch.int64, device=dev)
    cen_out = torch.empty((n, 3), device=dev)
    vac = (ctypes.c_int64 * 2)(0, 1)

    def hsv(k):
        assert lib.ss_aug_hsv(p(ds[k]["color"]), n, hs, stream) == 0

    def moments(k, affine=None):
        assert lib.ss_aug_moments(p(ds[k]["coord"]), n, affine, p(part), p(out4), stream) == 0

    def boxes(k):
        order, idx_ptr, _, K = csr[k]
        assert lib.ss_instance_boxes(p(ds[k]["coord"]), p(ds[k]["segment"]), p(order), p(idx_ptr), K, vac, 2, p(bbox), p(cen), stream) == 0

    def scatter(k):
        assert lib.ss_instance_scatter(p(csr[k][2]), n, csr[k][3], p(cen), p(inst_out), 1, -1, p(cen_out), stream) == 0
    cases = {"ss_aug_hsv": (hsv, 24 * n), "ss_aug_moments, no affine": (moments, 12 * n),
             "ss_aug_moments, pending affine": (lambda k: moments(k, aff), 12 * n),
             "ss_instance_boxes, %d instances" % INSTANCES: (boxes, 16 * n), "ss_instance_scatter": (scatter, 24 * n)}
    return {name: dict(us=windows(fn, sets, iters, repeats), bytes=nbytes) for name, (fn, nbytes) in cases.items()}, sets


def torch_parser(coord, segment, instance, ignore=(-1, 0, 1), inst_ignore=-1):
    """the reference's loop with torch ops on the device"""
    mask = ~torch.isin(segment, torch.tensor(ignore, device=segment.device))
    instance[~mask] = inst_ignore
    unique, inverse = torch.unique(instance[mask], return_inverse=True)
    instance[mask] = inverse
    K = len(unique)
    centroid = torch.full((coord.shape[0], 3), float(inst_ignore), device=coord.device)
    bbox = torch.full((K, 8), float(inst_ignore), device=coord.device)
    vacancy = torch.tensor([v for v in ignore if v >= 0], device=coord.device)
    for k in range(K):
        m = instance == k
        c = coord[m]
        lo, hi, mean = c.min(0).values, c.max(0).values, c.mean(0)
        cls = segment[m][0]
        centroid[m] = mean
        bbox[k] = torch.cat([(hi + lo) / 2, hi - lo, torch.zeros(1, device=coord.device), (cls - (cls > vacancy).sum()).float()[None]])
    return instance, centroid, bbox


def time_parser(n, dev, warmup, repeats):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    op = TRANSFORMS.build(dict(type="InstanceParser"))
    master = sample(n, dev, 0)
    ours = op.apply({k: v.clone() for k, v in master.items()}, {})
    inst, cen, box = torch_parser(master["coord"], master["segment"], master["instance"].clone())
    assert torch.equal(ours["instance"], inst) and torch.equal(ours["bbox"][:, :8], box)
    assert (ours["instance_centroid"] - cen).abs().max().item() < 1e-4     # torch's fp32 mean against the fp64 sum
    ms = {"InstanceParser.apply": [], "torch restatement": []}
    for it in range(warmup + repeats):
        for name in ms:
            d = {k: v.clone() for k, v in master.items()}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            if name == "torch restatement":
                torch_parser(d["coord"], d["segment"], d["instance"])
            else:
                op.apply(d, {})
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms, int(box.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 2000000])
    ap.add_argument("--iters", type=int, default=2000, help="back-to-back launches per kernel timing window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resident-mib", type=int, default=600)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_rest.py needs a GPU: the transforms have no CPU path")
    dev = torch.device("cuda")
    result = {}
    for n in args.sizes:
        ks, sets = time_kernels(n, dev, args.iters, args.repeats, args.resident_mib)
        print(f"\n## n = {n:,}\n")
        print(f"| kernel ({args.iters} launches per window over {sets} copies) | us per launch: median | min - max | bytes moved | rate, share of 8 TB/s |")
        print("|---|---|---|---|---|")
        for name, k in ks.items():
            med = median(k["us"])
            rate = k["bytes"] / (med * 1e-6)
            print(f"| {name} | {med:.1f} | {min(k['us']):.1f} - {max(k['us']):.1f} | {k['bytes'] / 1e6:.1f} MB | {rate / 1e12:.2f} TB/s, "
                  f"{100 * rate / PEAK_BYTES_PER_S:.0f} % |", flush=True)
        ms, K = time_parser(n, dev, args.warmup, args.repeats)
        print(f"\n| InstanceParser, {K} instances ({args.repeats} calls after {args.warmup} warm-up calls) | ms per call: median | min - max |")
        print("|---|---|---|")
        for name, v in ms.items():
            print(f"| {name} | {median(v):.3f} | {min(v):.3f} - {max(v):.3f} |", flush=True)
        result[str(n)] = dict(kernels=ks, parser_ms=ms, instances=K)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
