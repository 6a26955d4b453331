#!/usr/bin/env python
"""Semantic-segmentation measurements (DefaultSegmentorV2, the ScanNet 20-class config), one JSON line on stdout:

  step   training step (forward + backward) of the config's model on room-102400 with 14 features (room_chunk + 3 unit-normal
         columns), bench_runtime() under bf16 autocast: ms/step eager and under steady-state replay, Gaussians/s
  loss   CrossEntropyLoss + LovaszLoss (multiclass) forward + backward alone on bf16 logits at (204,800 x 20), (204,800 x 200) and
         (2,457,600 x 20) -- one SphereCrop sample and the config's 12 samples per GPU -- against a plain-torch restatement of the
         reference loop (labels.unique() + one torch.sort per present class), on the same GPU
  iou    the evaluator's counts kernel (fused arg-max + histograms) at 1 M x 20 fp32 logits: ms and bytes / time against 8 TB/s

    python scripts/bench_semseg.py [--part step,loss,iou] [--steps K] [--warmup W]
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of the same script."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from scenesplat_amd import native as nv
from scenesplat_amd.pointcept_api import MODELS, RUNTIME, bench_runtime, build_criteria
from scenesplat_amd.pointcept_api.seg import seg_loss_release

SCANNET20 = dict(type="DefaultSegmentorV2", num_classes=20, backbone_out_channels=64,
                 backbone=dict(type="PT-v3m1", in_channels=14, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
                               enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
                               enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
                               dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024,) * 4, mlp_ratio=4, qkv_bias=True, qk_scale=None,
                               attn_drop=0.0, proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=False,
                               enable_flash=True, upcast_attention=False, upcast_softmax=False, cls_mode=False),
                 criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                           dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)])


def log(*a):
    print("[semseg]", *a, file=sys.stderr, flush=True)


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_step(steps, warmup):
    from scenesplat_amd.steady_state import SteadyStateStep
    from scenesplat_amd.synthetic import room_chunk
    RUNTIME.update(bench_runtime())
    torch.manual_seed(0)
    model = MODELS.build(SCANNET20).cuda().train()
    d = room_chunk(256, 0, lang_dim=0, num_classes=20)
    g = torch.Generator().manual_seed(1)
    d["feat"] = torch.cat([d["feat"], F.normalize(torch.randn(len(d["feat"]), 3, generator=g), dim=1)], 1)
    data = {k: v.cuda() for k, v in d.items() if k != "valid_feat_mask"}
    n = data["feat"].shape[0]

    def fwd_bwd(plan, tensors):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(dict(tensors, plan=plan))
        out["loss"].backward()
        return {"loss": out["loss"]}

    def eager():
        model.zero_grad(set_to_none=True)
        return fwd_bwd(model.backbone.prepare_plan(data), data)

    ms_eager = _timed(eager, steps, warmup)
    log(f"eager {ms_eager:.2f} ms/step")
    steady = SteadyStateStep(fwd_bwd, [p for p in model.parameters() if p.requires_grad], warmup=1)

    def replay():
        model.zero_grad(set_to_none=True)
        return steady(model.backbone.prepare_plan(data), data, key=((), True))

    ms_replay = _timed(replay, steps, max(warmup, 4))
    log(f"replay {ms_replay:.2f} ms/step; {steady.replays} replays, {steady.eager_steps} eager steps, refused: {steady.refused}")
    return dict(gaussians=n, ms_eager=ms_eager, ms_replay=ms_replay, replays=steady.replays, refused=steady.refused,
                gaussians_per_s_replay=n / ms_replay * 1e3, gaussians_per_s_eager=n / ms_eager * 1e3,
                peak_mem_GB=torch.cuda.max_memory_allocated() / 2 ** 30)


def torch_pair(logits, labels, ignore=-1):
    """The reference loop restated in plain torch (losses/misc.py:35-62, losses/lovasz.py:121-176)."""
    x = logits.float()
    ce = F.cross_entropy(x, labels, ignore_index=ignore)
    p = x.softmax(1)
    valid = labels != ignore
    vp, vl = p[valid], labels[valid]
    losses = []
    for c in vl.unique():
        fg = (vl == c).float()
        err = (fg - vp[:, c]).abs()
        es, perm = torch.sort(err, 0, descending=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        jac[1:] = jac[1:] - jac[:-1]
        losses.append(torch.dot(es, jac))
    return ce + torch.stack(losses).mean()


def bench_loss(steps, warmup):
    out = {}
    crit = build_criteria(SCANNET20["criteria"])
    for n, C, present in ((204800, 20, 20), (204800, 200, 100), (2457600, 20, 20)):
        g = torch.Generator(device="cuda").manual_seed(n + C)
        logits = (torch.randn(n, C, device="cuda", generator=g) * 2).bfloat16().requires_grad_(True)
        labels = torch.randint(0, present, (n,), device="cuda", generator=g) * (C // present)
        labels[torch.rand(n, device="cuda", generator=g) < 0.1] = -1

        def ours():
            logits.grad = None
            model_like = crit.criteria[1].sums(logits, labels, share=True)      # the segmentor's single shared pass
            loss = crit(logits, labels)
            loss.backward()
            del model_like
            seg_loss_release()

        def ref():
            logits.grad = None
            torch_pair(logits, labels).backward()

        t_k = _timed(ours, steps, warmup)
        t_t = _timed(ref, steps, warmup)
        key = f"{n}x{C}"
        out[key] = dict(ms_kernel=t_k, ms_torch=t_t, speedup=t_t / t_k, present_classes=present)
        log(f"loss pair {key}: kernel {t_k:.3f} ms, torch restatement {t_t:.3f} ms ({t_t / t_k:.1f}x)")
    return out


def bench_iou(steps, warmup):
    n, C = 1 << 20, 20
    logits = torch.randn(n, C, device="cuda")
    tgt = torch.randint(-1, C, (n,), device="cuda")
    t = _timed(lambda: nv.seg_iou(tgt, C, -1, logits=logits), steps, warmup)
    nbytes = n * C * 4 + n * 8
    log(f"seg_iou {n}x{C}: {t * 1e3:.1f} us, {nbytes / t / 1e9:.2f} TB/s")
    return dict(n=n, classes=C, ms=t, bytes=nbytes, tb_per_s=nbytes / t / 1e9, frac_of_8tbs=nbytes / t / 1e9 / 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="step,loss,iou")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"metric": "DefaultSegmentorV2 (ScanNet 20) step, loss pair and IoU counts", "device": torch.cuda.get_device_name(0)}
    parts = a.part.split(",")
    if "loss" in parts:
        res["loss_pair_fwd_bwd"] = bench_loss(a.steps, a.warmup)
    if "iou" in parts:
        res["seg_iou"] = bench_iou(max(a.steps, 20), a.warmup)
    if "step" in parts:
        res["step"] = bench_step(a.steps, a.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
