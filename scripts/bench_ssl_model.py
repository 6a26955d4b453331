#!/usr/bin/env python
"""The kernels of the SimDINO pretraining model (csrc/ssl_model.hip) and one whole training step, each beside the torch formulation of the
reference's own code on the same GPU (pointcept/models/simdinov2.py).

  mask       DefaultContrastiverSimDinoV2.mask_generator for one global view (B samples of --points rows, `patch` mode at
             --mask-grid-size): a call time with its two host reads, HIP event pair per call + the host clock.  Beside it the
             reference's per-sample loop in torch on the device (unique / sort / index_put with its .item() reads), on the same draws.
  token      mask token forward + backward on (n, 32) fp32 rows, 30 % masked; torch: index_put of the token / index of the gradient.
  ema        the grouped EMA launch over the parameters of the full-size backbone; torch: _foreach_mul_ + _foreach_add_(alpha=).
  step       one DefaultSSLPreTrainer-style step (forward of 2 global + 3 local views through teacher / student, backward, AdamW,
             EMA) of the full-size model under bf16 autocast at --step-points rows per global view.  No torch counterpart exists
             (the reference's model needs spconv / flash-attn); the parent commit has nothing to compare with.

Warm-up first, medians over --repeats.  Needs a GPU: there is no CPU path.  Prints a markdown table and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, repeats, warm=3):
    """(median device ms, median host ms) of one call of fn()"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return median(dev), median(host)


def room(n, seed):
    """n distinct voxels on the shell of a room, int32 (n, 3)"""
    g = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n / 3))) + 8
    cells = g.choice(3 * side * side, size=n, replace=False)
    face, rest = cells // (side * side), cells % (side * side)
    a, b = rest // side, rest % side
    z = np.zeros_like(a)
    gc = np.where(face[:, None] == 0, np.stack([a + 1, b + 1, z], 1), np.where(face[:, None] == 1, np.stack([z, a + 1, b + 1], 1), np.stack([a + 1, z, b + 1], 1)))
    return torch.from_numpy(gc.astype(np.int32))


def torch_mask_generator(offset, grid_coord, mask_grid_size, flagged, draws):
    """The reference's `patch` loop in torch ops on the device, on given draws (per flagged sample: perm of the patches, rate)."""
    off = torch.nn.functional.pad(offset, (1, 0))
    masks, weights = [], []
    for i in range(len(offset)):
        n_i = int(off[i + 1] - off[i])
        if not flagged[i]:
            masks.append(torch.zeros(n_i, dtype=torch.bool, device=offset.device))
            weights.append(torch.ones(n_i, dtype=torch.float16, device=offset.device))
            continue
        c = torch.floor(grid_coord[off[i]:off[i + 1]] / mask_grid_size).int()
        c = c - c.min(dim=0)[0]
        ext = c.max(dim=0)[0].long() + 1
        cluster_key = c[:, 0].long() + c[:, 1].long() * ext[0] + c[:, 2].long() * ext[0] * ext[1]
        unique, cluster, counts = torch.unique(cluster_key, sorted=True, return_inverse=True, return_counts=True)
        patch_num, patch_max = unique.shape[0], counts.max().item()
        p2p = cluster.new_zeros(patch_num, patch_max)
        p2p_mask = torch.lt(torch.arange(patch_max, device=offset.device).unsqueeze(0), counts.unsqueeze(-1))
        p2p[p2p_mask] = torch.sort(cluster)[1]
        perm, rate = draws[i]
        k = int(patch_num * rate)
        patch_mask = torch.zeros(patch_num, dtype=torch.bool)
        patch_mask[perm[:k]] = True
        patch_mask = patch_mask.to(offset.device)
        point_mask = torch.zeros(n_i, dtype=torch.bool, device=offset.device)
        point_mask[p2p[patch_mask][p2p_mask[patch_mask]]] = True
        masks.append(point_mask)
        weights.append(torch.ones(n_i, dtype=torch.float16, device=offset.device) * (1 / max(k, 1)))
    masks, weights = torch.cat(masks), torch.cat(weights)
    return masks, weights[masks]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000, help="rows per sample of the mask / token benchmarks")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--mask-grid-size", type=float, default=3.0)
    ap.add_argument("--step-points", type=int, default=40000, help="rows per sample and global view of the whole step (local crops: a quarter)")
    ap.add_argument("--step-batch", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import MODELS
    dev = torch.device("cuda")
    rows, res = [], {}

    # ---- mask generator ----------------------------------------------------------------------------------------------------------------
    backbone = dict(type="PT-v3m1-simdino", in_channels=11, order=("z", "z-trans", "hilbert", "hilbert-trans"),
                    enc_patch_size=(1024,) * 5, dec_patch_size=(1024,) * 4, pooling_reduce="max")
    model = MODELS.build(dict(type="DefaultContrastiverSimDinoV2", backbone_out_channels=512, enable_mae_loss=True, backbone=backbone,
                              mask_grid_size=args.mask_grid_size, mask_sample_probability=1.0))
    gc = torch.cat([room(args.points, 10 + i) for i in range(args.batch)]).to(dev)
    offset = (torch.arange(1, args.batch + 1) * args.points).to(dev)

    def ours():
        torch.manual_seed(0); np.random.seed(0)
        return model.mask_generator(offset, gc)
    torch.manual_seed(0); np.random.seed(0)
    torch.randperm(args.batch)
    _, _, cnt = nv.mask_patches(gc, offset.int(), args.mask_grid_size)
    cnt = cnt.tolist()
    draws = []
    for i in range(args.batch):
        perm = torch.randperm(cnt[i])
        draws.append((perm, np.random.uniform(*model.mask_ratio_min_max)))

    def theirs():
        return torch_mask_generator(offset, gc, args.mask_grid_size, [1] * args.batch, draws)
    m0, w0 = ours()
    m1, w1 = theirs()
    assert torch.equal(m0, m1) and torch.equal(w0, w1), "mask generator differs from the torch formulation"
    for name, fn in (("mask_generator (HIP)", ours), ("mask_generator (torch loop)", theirs)):
        d, h = timed(fn, args.repeats)
        rows.append((name, "%d x %d rows, grid %.1f" % (args.batch, args.points, args.mask_grid_size), d, h))
        res[name] = dict(device_ms=d, host_ms=h)

    # ---- mask token ----------------------------------------------------------------------------------------------------------------------
    n, C = args.batch * args.points, 32
    x = torch.randn(n, C, device=dev, requires_grad=True)
    tok = torch.randn(1, C, device=dev, requires_grad=True)
    cot = torch.randn(n, C, device=dev)

    def token_ours():
        x.grad = tok.grad = None
        SF.mask_token(x, m0, tok).backward(cot)

    def token_torch():
        x.grad = tok.grad = None
        y = x.clone()
        y[m0] = tok.to(y.dtype)
        y.backward(cot)
    for name, fn in (("mask token fwd+bwd (HIP)", token_ours), ("mask token fwd+bwd (torch index_put)", token_torch)):
        d, h = timed(fn, args.repeats)
        rows.append((name, "%d x %d fp32, %.0f %% masked" % (n, C, 100.0 * m0.float().mean().item()), d, h))
        res[name] = dict(device_ms=d, host_ms=h)

    # ---- EMA --------------------------------------------------------------------------------------------------------------------------------
    model = model.to(dev)
    teacher, student = model._ema_pairs()
    numel = sum(t.numel() for t in teacher)

    def ema_torch():
        with torch.no_grad():
            tl = [t.data for t in teacher]
            torch._foreach_mul_(tl, 0.996)
            torch._foreach_add_(tl, [s.data for s in student], alpha=1 - 0.996)
    for name, fn in (("update_teacher (HIP, one launch)", lambda: model.update_teacher(0.996)), ("update_teacher (torch _foreach)", ema_torch)):
        d, h = timed(fn, args.repeats)
        rows.append((name, "%d tensors, %.1f M parameters" % (len(teacher), numel / 1e6), d, h))
        res[name] = dict(device_ms=d, host_ms=h, gbytes_per_s=12 * numel / (d * 1e-3) / 1e9)

    # ---- one whole step ------------------------------------------------------------------------------------------------------------------------
    if not args.skip_step:
        from scenesplat_amd.pointcept_api import RUNTIME, bench_runtime
        RUNTIME.update(bench_runtime())               # the execution knobs bench.py times
        model.mask_sample_probability = 0.5
        model.train()
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, eps=1e-4)
        inp = {}
        views = [("global_crop0", args.step_points), ("global_crop1", args.step_points)] + [("local_crop%d" % i, args.step_points // 4) for i in range(3)]
        for vi, (name, pts) in enumerate(views):
            g = torch.cat([room(pts, 100 * vi + i) for i in range(args.step_batch)]).to(dev)
            inp[name + "_grid_coord"], inp[name + "_coord"] = g, g.float() * 0.02
            inp[name + "_feat"] = torch.randn(len(g), 11, device=dev)
            inp[name + "_offset"] = (torch.arange(1, args.step_batch + 1) * pts).to(dev)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = model(inp, 0.05)
            opt.zero_grad(set_to_none=True)
            out["loss"].backward()
            opt.step()
            model.update_teacher(0.996)
        d, h = timed(step, max(5, args.repeats // 3), warm=2)
        rows.append(("training step (bf16 autocast)", "B = %d, %d rows per sample and global view" % (args.step_batch, args.step_points), d, h))
        res["training step"] = dict(device_ms=d, host_ms=h, peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30)

    print("| what | shape | device ms | host ms |\n|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %.3f | %.3f |" % r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
