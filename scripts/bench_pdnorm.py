#!/usr/bin/env python
"""What PDNorm costs in the replayed training step of the full lang-pretrain backbone (synthetic.LANG_PTV3, the benchmark's room
workload of 102,400 Gaussians, bf16 autocast, bench_runtime()), three configurations in ONE process:

  off       pdnorm_bn = pdnorm_ln = False                (the model bench.py times)
  select    PDNorm on every norm, three conditions, adaptive=False: the selected norms' own parameters, no extra kernel
  adaptive  + the prompt modulation of all PDNorm layers: one grouped launch forward, one (plus its finish) backward

Each configuration's forward + backward (random cotangent fed as the output gradient, as bench.py does) is captured once
(steady_state.SteadyStateStep) and then replayed in alternating blocks of --steps steps, --repeats times; a step is timed with a
HIP event pair around the replay, the plan of the step built before the first event.  Prints the median and the spread of the
block medians per configuration, and one JSON line.

--count CONFIG: run only that configuration, --steps replays after the capture and nothing else: the run to put under a kernel
trace, where the launches of a replayed step are the kernels from one k_cast_bf16_group (the first kernel of the captured step)
to the next.

Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CONDITIONS = ("ScanNet", "S3DIS", "Structured3D")
CONFIGS = {"off": {}, "select": dict(pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=False, pdnorm_conditions=CONDITIONS),
           "adaptive": dict(pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=True, pdnorm_conditions=CONDITIONS)}


def build(name, data, dev):
    from scenesplat_amd.pointcept_api import MODELS
    from scenesplat_amd.steady_state import SteadyStateStep
    from scenesplat_amd.synthetic import LANG_PTV3
    torch.manual_seed(1234)
    model = MODELS.build(dict(type="PT-v3m1", **LANG_PTV3, **CONFIGS[name])).to(dev).train()
    extra = {}
    if name != "off":
        extra["condition"] = [CONDITIONS[1]]
    if name == "adaptive":
        extra["context"] = torch.randn(1, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(9)).requires_grad_(True)

    def fwd_bwd(plan, t):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(dict(feat=t["feat"], grid_coord=data["grid_coord"], offset=data["offset"], plan=plan, **extra))
        torch.autograd.backward(out.feat, grad_tensors=t["cot"])
        return {"feat": out.feat}
    params = list(model.parameters()) + ([extra["context"]] if name == "adaptive" else [])
    steady = SteadyStateStep(fwd_bwd, params, warmup=1)
    nparam = sum(p.numel() for p in model.parameters())
    nmod = sum(p.numel() for n, p in model.named_parameters() if ".modulation." in n)
    return dict(model=model, steady=steady, params=params, nparam=nparam, nmod=nmod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--count", choices=list(CONFIGS), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pdnorm.py needs a GPU")
    from scenesplat_amd.pointcept_api import RUNTIME, bench_runtime
    from scenesplat_amd.synthetic import LANG_PTV3, room_chunk
    dev = torch.device("cuda", 0)
    RUNTIME.update(bench_runtime())
    data = {k: v.to(dev) for k, v in room_chunk(n_side=args.n_side, seed=0, lang_dim=0).items()}
    n = data["feat"].shape[0]
    cot = torch.randn(n, LANG_PTV3["dec_channels"][0], device=dev, generator=torch.Generator(device=dev).manual_seed(7)).to(torch.bfloat16)
    names = [args.count] if args.count else list(CONFIGS)
    runs = {nm: build(nm, data, dev) for nm in names}

    def step(r, timed=False):
        for p in r["params"]:
            p.grad = None
        plan = r["model"].prepare_plan(data)
        if not timed:
            r["steady"](plan, {"feat": data["feat"], "cot": cot})
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r["steady"](plan, {"feat": data["feat"], "cot": cot})
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for nm, r in runs.items():
        for _ in range(6):                      # eager, sync-checked, capture, then replays
            step(r); torch.cuda.synchronize()
            if r["steady"].replays >= 2:
                break
        if r["steady"].replays == 0:
            raise SystemExit(f"{nm}: the step was not captured: {r['steady'].refused}")
        print(f"[bench_pdnorm] {nm}: {r['nparam'] / 1e6:.1f} M parameters ({r['nmod'] / 1e6:.1f} M in modulation Linears), replaying", file=sys.stderr, flush=True)
    if args.count:
        for _ in range(args.steps):
            step(runs[args.count]); torch.cuda.synchronize()
        return
    blocks = {nm: [] for nm in names}
    for _ in range(args.repeats):
        for nm in names:
            ts = [step(runs[nm], timed=True) for _ in range(args.steps)]
            blocks[nm].append(statistics.median(ts))
    res = {}
    print("| configuration | parameters (M) | ms / replayed step (median of block medians) | block medians |")
    print("|---|---|---|---|")
    for nm in names:
        med = statistics.median(blocks[nm])
        res[nm] = dict(ms=med, blocks=blocks[nm], params_m=runs[nm]["nparam"] / 1e6, modulation_m=runs[nm]["nmod"] / 1e6)
        print(f"| {nm} | {runs[nm]['nparam'] / 1e6:.1f} | {med:.2f} | {', '.join('%.2f' % b for b in blocks[nm])} |")
    print(json.dumps(dict(bench="pdnorm", steps=args.steps, repeats=args.repeats, n=n, results=res)))


if __name__ == "__main__":
    main()
