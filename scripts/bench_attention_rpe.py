#!/usr/bin/env python
"""Window attention with relative position encoding (csrc/attention_rpe.hip) in isolation, on room-102400 (100 windows of
1024 points along the z curve), at the dec0 shape (H 16, d 48) and an encoder shape (H 2, d 16), bf16:

  a  window_attn_rpe_fwd / _bwd, MFMA        the new kernels: bias looked up inside the kernels, dtable without atomics
  b  window_attn_fwd / _bwd, MFMA            the bias-free kernels of the packed (n, 3C) layout: a / b is the cost of the bias
  c  torch, bias materialised                what a user has without the kernels, the reference's own formulation: the
                                             (W, H, K, K) bias gathered from the table (the relative positions are cached, as the
                                             reference caches them), (q * scale) @ k^T + bias, float softmax, @ v; autograd
                                             backward.  Runs on --torch-windows windows (the bias of all 100 does not fit a
                                             sensible memory budget at H 16) and is reported per window.

All variants run in one process in alternating blocks of --steps calls, --repeats times, after --warmup calls each; a block is
timed with one HIP event pair and ends in a synchronise.  `fwd` is the forward call alone, `fwd+bwd` forward and backward (for
c: autograd with gradients for q, k, v and the table).  Needs a GPU: there is no CPU path.  Prints a markdown table and one
JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [("dec0", 16, 48), ("enc", 2, 16)]
K = 1024


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_rpe.py needs a GPU: the attention kernels have no CPU path")
    from scenesplat_amd import native as nv
    from scenesplat_amd.plan import build_plan
    from scenesplat_amd.pointcept_api.ptv3 import RPE
    from scenesplat_amd.synthetic import room_grid
    gc = torch.from_numpy(room_grid(256, 0)).cuda()
    n = gc.shape[0]
    plan = build_plan(gc, torch.tensor([n]).cuda(), ("z", "z-trans"), ())
    lv = plan.levels[0]
    win = lv.window(0, K)
    W = win.num_windows
    assert win.max_window == K and win.n_pad == n, "room-102400 is 100 full windows"
    result = dict(n=n, windows=W, K=K, steps=args.steps, repeats=args.repeats, torch_windows=args.torch_windows)
    rows = []
    for name, H, d in SHAPES:
        C = H * d
        g = torch.Generator(device="cuda").manual_seed(H * d)
        qkv = torch.randn(n, 3 * C, device="cuda", generator=g).to(torch.bfloat16)
        dout = torch.randn(n, C, device="cuda", generator=g).to(torch.bfloat16)
        rpe = RPE(K, H)
        table = (torch.randn(3 * rpe.rpe_num, H, device="cuda", generator=g) * 0.5).contiguous()
        scale, pb = d ** -0.5, rpe.pos_bnd
        o_a, lse_a = nv.window_attn_rpe_fwd(qkv, win, lv.grid_coord, table, pb, H, scale, nv.ATTN_MFMA)
        o_b, lse_b = nv.window_attn_fwd(qkv, win, H, scale, nv.ATTN_MFMA)
        # c: the first Wc windows, gathered once outside the timed region
        Wc = args.torch_windows
        slots = win.gidx[:Wc * K].long()
        q, k, v = (qkv[slots].view(Wc, K, 3, H, d).permute(2, 0, 3, 1, 4)[i].contiguous().requires_grad_(True) for i in range(3))
        gcw = lv.grid_coord[slots].view(Wc, K, 3).long()
        rel = gcw.unsqueeze(2) - gcw.unsqueeze(1)                                  # (Wc, K, K, 3), cached by the reference
        idx = (rel.clamp(-pb, pb) + pb + torch.arange(3, device="cuda") * rpe.rpe_num).reshape(-1)
        tab_c = table.clone().requires_grad_(True)
        cot = dout[win.sidx[:Wc * K].long().clamp(min=0)].view(Wc, K, H, d).permute(0, 2, 1, 3).contiguous()

        def c_fwd():
            bias = tab_c.index_select(0, idx).view(Wc, K, K, 3, H).sum(3).permute(0, 3, 1, 2)
            attn = ((q * scale) @ k.transpose(-2, -1)).float() + bias
            return torch.softmax(attn, -1).to(v.dtype) @ v

        def c_fwd_bwd():
            out = c_fwd()
            torch.autograd.grad(out, (q, k, v, tab_c), cot)

        # the torch formulation and the kernels agree on those windows (a is what is being timed, not a different function)
        with torch.no_grad():
            ref = c_fwd().permute(0, 2, 1, 3).reshape(Wc * K, C).float()
        got = torch.zeros_like(ref)
        sid = win.sidx[:Wc * K].long()
        got[sid >= 0] = o_a[sid[sid >= 0]].float()
        ref[sid < 0] = 0
        err = (got - ref).abs().max().item()
        variants = {
            "a fwd": lambda: nv.window_attn_rpe_fwd(qkv, win, lv.grid_coord, table, pb, H, scale, nv.ATTN_MFMA),
            "b fwd": lambda: nv.window_attn_fwd(qkv, win, H, scale, nv.ATTN_MFMA),
            "c fwd": lambda: torch.no_grad()(c_fwd)(),
            "a fwd+bwd": lambda: (nv.window_attn_rpe_fwd(qkv, win, lv.grid_coord, table, pb, H, scale, nv.ATTN_MFMA),
                                  nv.window_attn_rpe_bwd(qkv, o_a, dout, lse_a, win, lv.grid_coord, table, pb, H, scale, nv.ATTN_MFMA)),
            "b fwd+bwd": lambda: (nv.window_attn_fwd(qkv, win, H, scale, nv.ATTN_MFMA),
                                  nv.window_attn_bwd(qkv, o_b, dout, lse_b, win, H, scale, nv.ATTN_MFMA)),
            "c fwd+bwd": c_fwd_bwd,
        }
        ms = {kname: [] for kname in variants}
        for kname, fn in variants.items():
            timed(fn, args.warmup)
        for _ in range(args.repeats):
            for kname, fn in variants.items():
                ms[kname].append(timed(fn, args.steps))
        per_win = {kname: (Wc if kname[0] == "c" else W) for kname in variants}
        med = {kname: sorted(v_)[len(v_) // 2] for kname, v_ in ms.items()}
        us = {kname: 1e3 * med[kname] / per_win[kname] for kname in variants}
        for kname in variants:
            rows.append(f"| {name} H {H} d {d} | {kname} | {per_win[kname]} | {', '.join(f'{m:.3f}' for m in ms[kname])} | {med[kname]:.3f} | {us[kname]:.2f} |")
        ratios = {f"{p} a/b": us[f"a {p}"] / us[f"b {p}"] for p in ("fwd", "fwd+bwd")}
        ratios.update({f"{p} c/a": us[f"c {p}"] / us[f"a {p}"] for p in ("fwd", "fwd+bwd")})
        result[name] = dict(H=H, d=d, pos_bnd=pb, ms=ms, median_ms=med, us_per_window=us, ratios=ratios, max_abs_err_a_vs_c=err)
        rows.append(f"| {name} | ratios per window | | " + ", ".join(f"{k_} {v_:.2f}" for k_, v_ in ratios.items()) + f" | max abs err a vs c {err:.4f} | |")
        del q, k, v, rel, idx, cot
        torch.cuda.empty_cache()
    print(f"room-102400: {W} windows of {K}, {args.repeats} x {args.steps} calls per variant after {args.warmup} warm-up calls; c on {args.torch_windows} windows")
    print("| shape | variant | windows | ms per call (each repeat) | median ms | us per window |")
    print("|---|---|---|---|---|---|")
    print("\n".join(rows))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
