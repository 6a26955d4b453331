#!/usr/bin/env python
"""Optimizer step of the lang-pretrain model in isolation: gradient clipping + AdamW over its 363 real parameter shapes
(91.7 M fp32 parameters, two groups: 39 tensors at lr 6e-3 and 324 "block" tensors at lr 6e-4, weight decay 0.05, clip_grad 1.0).

  a  clip_grad_norm_ + torch.optim.AdamW            (torch's default path: what Trainer.run_step runs with type="AdamW")
  b  clip_grad_norm_ + torch.optim.AdamW(fused=True)
  c  FusedAdamW(max_grad_norm=1.0)                  (csrc/optim.hip: three launches, p.grad left untouched)

All three run in one process on the same seeded gradients, in alternating blocks of --steps steps, --repeats times.  A step is
timed with a HIP event pair around clip + step; the gradients are restored from a master copy before every step, outside the
timed region and for every variant alike (clip_grad_norm_ scales them in place; the copy also leaves the caches in the same
state for all three).  Two timings: `idle GPU` starts each step on an idle GPU, so it is the larger of the host's enqueue time and
the GPU's work; `busy GPU` puts a --plug-ms busy kernel in front of each step, so the host enqueues while the GPU is occupied (the
situation behind a backward pass) and the events see the GPU's work alone, unless enqueueing takes longer than the plug.  `host`
is the time the Python thread needs to enqueue a step.  The update kernel's floor is 32 bytes per
parameter (read p, g, m, v; write p, m, v); `share` is that traffic over the step time as a share of 8 TB/s.

Needs a GPU: there is no CPU path.  Prints a markdown table and one JSON line."""
import argparse
import ast
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CONFIG = "configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py"
PEAK_BYTES_PER_S = 8e12


def lang_pretrain_groups():
    """[(lr, [shape, ...]), ...] of the shipped config's model, grouped as engine.build_optimizer groups them."""
    from scenesplat_amd.pointcept_api import MODELS
    with open(os.path.join(ROOT, "tests", "golden", "lang_configs.txt")) as f:
        cfg = ast.literal_eval(f.read())[CONFIG]
    model = MODELS.build(cfg["model"])
    groups = [(cfg["optimizer"]["lr"], [])] + [(pd["lr"], []) for pd in cfg["param_dicts"]]
    for name, p in model.named_parameters():
        for i, pd in enumerate(cfg["param_dicts"]):
            if pd["keyword"] in name:
                groups[i + 1][1].append(tuple(p.shape))
                break
        else:
            groups[0][1].append(tuple(p.shape))
    return groups, cfg["optimizer"]["weight_decay"], cfg["clip_grad"]


class Variant:
    def __init__(self, name, groups, wd, clip, init, dev):
        from scenesplat_amd.optim import FusedAdamW
        self.name, self.clip = name, clip
        self.params = [torch.nn.Parameter(t.clone()) for t in init]
        for p in self.params:
            p.grad = torch.empty_like(p)
        pg, k = [], 0
        for lr, shapes in groups:
            pg.append(dict(params=self.params[k:k + len(shapes)], lr=lr))
            k += len(shapes)
        if name == "c":
            self.opt = FusedAdamW(pg, weight_decay=wd, max_grad_norm=clip)
        else:
            self.opt = torch.optim.AdamW(pg, weight_decay=wd, fused=(name == "b"))
        self.grads = [p.grad for p in self.params]
        self.ms, self.host_ms, self.plug_ms = [], [], []

    def step(self):
        if self.name != "c":
            torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.opt.step()

    def block(self, master, steps, record=True, plug_cycles=0):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        host = 0.0
        for a, b in pairs:
            torch._foreach_copy_(self.grads, master)
            if plug_cycles:
                torch.cuda._sleep(plug_cycles)         # the GPU is busy while the host enqueues the step, as behind a backward pass
            a.record()
            t0 = time.perf_counter()
            self.step()
            host += time.perf_counter() - t0
            b.record()
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in pairs) / steps
        if record and plug_cycles:
            self.plug_ms.append(ms)
        elif record:
            self.ms.append(ms)
            self.host_ms.append(host * 1e3 / steps)

    def peak_delta(self, master):
        torch._foreach_copy_(self.grads, master)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        self.step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--plug-ms", type=float, default=4.0, help="length of the busy kernel in front of each step of the second timing (0: skip it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py needs a GPU: FusedAdamW has no CPU path")
    dev = torch.device("cuda")
    groups, wd, clip = lang_pretrain_groups()
    shapes = [s for _, ss in groups for s in ss]
    nparam = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    init = [torch.randn(s, device=dev, generator=gen) * 0.02 for s in shapes]
    master = [torch.randn(s, device=dev, generator=gen) * 0.01 for s in shapes]          # global norm about 96: the clip is active
    variants = [Variant(n, groups, wd, clip, init, dev) for n in "abc"]
    for v in variants:
        v.block(master, args.warmup, record=False)
    plug_cycles = 0
    if args.plug_ms > 0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000); a.record(); torch.cuda._sleep(10000000); b.record(); torch.cuda.synchronize()
        plug_cycles = int(1e7 * args.plug_ms / a.elapsed_time(b))
    for _ in range(args.repeats):
        for v in variants:
            v.block(master, args.steps)
        for v in variants:
            if plug_cycles:
                v.block(master, args.steps, plug_cycles=plug_cycles)
    peaks = {v.name: v.peak_delta(master) for v in variants}
    a, c = variants[0], variants[2]
    diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.params, c.params))
    scale = max(float(p.detach().abs().max()) for p in a.params)
    total_steps = args.warmup + args.repeats * args.steps * (2 if plug_cycles else 1) + 1
    label = dict(a="clip_grad_norm_ + AdamW (default)", b="clip_grad_norm_ + AdamW(fused=True)", c="FusedAdamW")
    print(f"{len(shapes)} tensors in {[len(ss) for _, ss in groups]}, {nparam / 1e6:.2f} M parameters, clip_grad {clip}, "
          f"{args.repeats} x {args.steps} steps per variant after {args.warmup} warm-up steps, grad norm {float(c.opt.last_grad_norm):.2f}")
    print("| variant | idle GPU: ms/step (each repeat) | median | host ms/step | busy GPU: ms/step (each repeat) | median | 32 B/param over it, share of 8 TB/s | peak memory of one step |")
    print("|---|---|---|---|---|---|---|---|")
    result = dict(tensors=len(shapes), params=nparam, steps=args.steps, repeats=args.repeats)
    for v in variants:
        med = sorted(v.ms)[len(v.ms) // 2]
        pmed = sorted(v.plug_ms)[len(v.plug_ms) // 2] if v.plug_ms else med
        rate = 32.0 * nparam / (pmed * 1e-3)
        print(f"| {v.name}: {label[v.name]} | {', '.join(f'{m:.3f}' for m in v.ms)} | {med:.3f} | {sorted(v.host_ms)[len(v.host_ms) // 2]:.3f} | "
              f"{', '.join(f'{m:.3f}' for m in v.plug_ms)} | {pmed:.3f} | {rate / 1e12:.2f} TB/s, {100 * rate / PEAK_BYTES_PER_S:.0f} % | {peaks[v.name] / 2**20:.1f} MiB |")
        result[v.name] = dict(ms=v.ms, median_ms=med, host_ms=v.host_ms, busy_gpu_ms=v.plug_ms, busy_gpu_median_ms=pmed, peak_step_bytes=peaks[v.name])
    print(f"max |w_c - w_a| after {total_steps} steps: {diff:.3e} (largest |w| {scale:.3e})")
    result.update(max_abs_weight_diff_c_vs_a=diff, max_abs_weight=scale, total_steps=total_steps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
