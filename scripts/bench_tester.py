#!/usr/bin/env python
"""The steps of the open-vocabulary test stage after the accumulation, at one ScanNet200-sized scene: 1,000,000 grid points x 200
classes expanded to 2,000,000 original Gaussians, 2,000 instances.

  (a) native.vocab_finish against the torch sequence it replaces (engines/test.py:372-394): topk(3) | max + threshold, [inverse],
      the pred_label_mapping loop.  Algorithmic bytes: n C 4 read + m k 4 written, over the 8 TB/s HBM peak.
  (b) pointops.clustering_voting against the reference's numpy loop on the host (utils/misc.py:98-125).

Device events after warm-up; the two forms of (a) alternate in one process and their results are compared on the timed inputs.
    python scripts/bench_tester.py [--n 1000000] [--classes 200] [--m 2000000] [--instances 2000] [--reps 10]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scenesplat_amd import native as nv, pointops

HBM_PEAK = 8.0e12


def torch_sequence(pred, k, threshold, ignore_index, inverse, mapping):
    if k > 1:
        lab = pred.topk(k, dim=1)[1]
    else:
        mx, lab = pred.max(1)
        lab[mx < threshold] = ignore_index
    lab = lab[inverse]
    for key, item in mapping.items():
        lab[lab == key] = item
    return lab


def numpy_clustering_voting(pred, instance, ignore_index):
    out = pred.copy()
    for i in np.unique(instance):
        if i == ignore_index:
            continue
        rows = instance == i
        vals, counts = np.unique(pred[rows], return_counts=True)
        out[rows] = vals[np.argmax(counts)]
    return out


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--m", type=int, default=2_000_000)
    ap.add_argument("--instances", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tester: needs the GPU (no CPU timing stands in for it)")
    n, C, m = a.n, a.classes, a.m
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand(n, C, device="cuda", generator=g) * 3.0
    inv_random = torch.randint(0, n, (m,), device="cuda", generator=g)
    inverses = dict(sorted=torch.sort(inv_random)[0], random=inv_random)   # the two ends: a real inverse is spatially coherent, between them
    mapping = {4: 1, 5: 2}
    lut = pointops.label_map_lut(mapping, C, -1, device="cuda")
    print(f"(a) vocab_finish, n = {n} x C = {C} -> m = {m}")
    for k, thr, order in ((1, 1.0, "sorted"), (3, 0.0, "sorted"), (1, 1.0, "random"), (3, 0.0, "random")):
        inverse = inverses[order]
        ours = lambda: nv.vocab_finish(pred, k=k, threshold=thr, ignore_index=-1, inverse=inverse, lut=lut)
        ref = lambda: torch_sequence(pred, k, thr, -1, inverse, mapping)
        # torch.topk leaves the order of equal values open (about one row in a thousand of 200 random floats holds an equal pair):
        # where the two differ, the values at the differing classes must be equal
        raw = nv.vocab_finish(pred, k=k, threshold=0.0).long()
        tk = pred.topk(k, dim=1)[1]
        ties = int((raw != tk).any(1).sum())
        same = torch.equal(pred.gather(1, raw), pred.gather(1, tk)) and \
            (ties > 0 or torch.equal(ours().reshape(-1).long(), ref().reshape(-1)))
        for _ in range(3):
            ours(); ref()
        t_ours, t_ref = [], []
        for _ in range(3):                                 # alternate: the machine is shared
            t_ours.append(timed(ours, a.reps))
            t_ref.append(timed(ref, a.reps))
        by = n * C * 4 + m * k * 4
        mo, mr = min(t_ours), min(t_ref)
        print(f"  k = {k}, {order} inverse: vocab_finish {mo:.3f} ms (runs {', '.join('%.3f' % t for t in t_ours)}), torch sequence {mr:.3f} ms "
              f"(runs {', '.join('%.3f' % t for t in t_ref)}): {mr / mo:.2f}x; {by / 1e6:.0f} MB algorithmic -> "
              f"{by / mo / 1e9:.2f} TB/s = {by / (mo * 1e-3) / HBM_PEAK:.2f} of the 8 TB/s peak; results equal: {same} ({ties} rows differ by the order of equal values)")
    print(f"(b) clustering_voting, m = {m}, {a.instances} instances, {C} classes")
    inst = (torch.randint(0, a.instances, (m // 50 + 1,), device="cuda", generator=g).repeat_interleave(50)[:m] * 7 - 1)   # runs of 50 rows; id -1 = none
    lab = torch.randint(-1, C, (m,), device="cuda", generator=g).int()
    ours = lambda: pointops.clustering_voting(lab, inst, -1, C)
    dense = torch.unique(inst, return_inverse=True)[1].int() - 1
    kern = lambda: nv.cluster_vote(lab, dense.contiguous(), a.instances, C, -1)
    out = ours()
    for _ in range(3):
        ours(); kern()
    t_full = min(timed(ours, a.reps) for _ in range(3))
    t_kern = min(timed(kern, a.reps) for _ in range(3))
    lab_h, inst_h = lab.cpu().numpy(), inst.cpu().numpy()
    t0 = time.perf_counter()
    ref = numpy_clustering_voting(lab_h, inst_h, -1)
    t_host = (time.perf_counter() - t0) * 1e3
    print(f"  clustering_voting {t_full:.3f} ms (of which ss_cluster_vote {t_kern:.3f} ms; the rest is torch.unique + the range check), "
          f"numpy loop on the host {t_host:.1f} ms (one run, without the copies): {t_host / t_full:.0f}x; results equal: "
          f"{np.array_equal(out.cpu().numpy(), ref)}")


if __name__ == "__main__":
    main()
