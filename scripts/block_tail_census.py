#!/usr/bin/env python
"""Census of the Block tail (attention output -> end of the Block) on the benchmark shapes, per launch, with HIP events around a replayed hipGraph:
forward  proj | add+LN2 seam | fc1 | GELU | fc2 | add seam, backward the six launches in reverse (input-gradient side only: the
weight gradients are queued and grouped per stage either way).  One table per level with at most 256 channels; when the library
has the fused pair (ss_block_tail_fwd / _bwd) its two launches are timed beside the chain.
   python scripts/block_tail_census.py [repeats]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from scenesplat_amd import native as nv, functional as SF

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 20
# (name, rows, channels, Blocks) of the room-102400 benchmark step (synthetic.LANG_PTV3)
LEVELS = [("enc0", 102400, 32, 2), ("enc1", 25600, 64, 2), ("enc2", 6400, 128, 2), ("enc3", 1600, 256, 6), ("dec2", 6400, 256, 2)]
dev = "cuda"
bf = torch.bfloat16


def timed(fn):
    """microseconds per launch of fn(): REP launches captured into one hipGraph (as the benchmark step replays them: no host cost
    between launches), median of five replays."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REP):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / REP * 1e3)
    return sorted(ts)[2]


def census(n, C):
    g = torch.Generator(device=dev).manual_seed(C)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    H = 4 * C
    feat, x = r(n, C).to(bf), r(n, C)
    wp, w1, w2 = (r(C, C) / C ** 0.5).to(bf), (r(H, C) / C ** 0.5).to(bf), (r(C, H) / H ** 0.5).to(bf)
    wpt, w1t, w2t = wp.t().contiguous(), w1.t().contiguous(), w2.t().contiguous()
    bp, b1, b2 = r(C).to(bf), r(H).to(bf), r(C).to(bf)
    gam, bet = 1 + 0.1 * r(C), 0.1 * r(C)
    rs1 = (torch.rand(n, device=dev, generator=g) < 0.85).float() / 0.85
    rs2 = (torch.rand(n, device=dev, generator=g) < 0.85).float() / 0.85
    nt = C * H >= 65536          # the layers that keep an (in, out) copy today run their dgrad in the NT form
    y1 = F.linear(feat, wp, bp)
    xmid, _, h2, mean, rstd = nv.add_layernorm_fwd(x, y1, rs1, gam, bet, 1e-5, True, False, bf)
    u = F.linear(h2, w1, b1)
    a = nv.gelu(u)
    y2 = F.linear(a, w2, b2)
    gx = r(n, C)
    _, dy2, _, _ = nv.add_layernorm_bwd(gx, None, None, None, None, None, None, rs2, torch.float32, bf)
    da = dy2 @ w2
    du = nv.gelu(u, da)
    dh2 = du @ w1
    gmid, dy1, _, _ = nv.add_layernorm_bwd(gx, None, dh2, xmid, mean, rstd, gam, rs1, torch.float32, bf, reduce=False)
    fwd = [("proj", lambda: F.linear(feat, wp, bp)),
           ("add+LN2", lambda: nv.add_layernorm_fwd(x, y1, rs1, gam, bet, 1e-5, True, False, bf)),
           ("fc1", lambda: F.linear(h2, w1, b1)),
           ("GELU", lambda: nv.gelu(u)),
           ("fc2", lambda: F.linear(a, w2, b2)),
           ("add", lambda: nv.add_layernorm_fwd(xmid, y2, rs2, None, None, 0.0, True, False, bf))]
    bwd = [("add'", lambda: nv.add_layernorm_bwd(gx, None, None, None, None, None, None, rs2, torch.float32, bf)),
           ("fc2 dgrad", (lambda: F.linear(dy2, w2t)) if nt else (lambda: dy2 @ w2)),
           ("GELU'", lambda: nv.gelu(u, da)),
           ("fc1 dgrad", (lambda: F.linear(du, w1t)) if nt else (lambda: du @ w1)),
           ("add+LN2'", lambda: nv.add_layernorm_bwd(gx, None, dh2, xmid, mean, rstd, gam, rs1, torch.float32, bf, reduce=False)),
           ("proj dgrad", lambda: dy1 @ wp)]
    tf, tb = [(k, timed(f)) for k, f in fwd], [(k, timed(f)) for k, f in bwd]
    fused = None
    if hasattr(SF, "block_tail_fwd_raw") and hasattr(nv.lib(), "ss_block_tail_fwd"):
        bp32, b132, b232 = bp.float(), b1.float(), b2.float()
        args = (feat, x, rs1, rs2, wp, bp32, w1, b132, w2, b232, gam, bet, 1e-5, False)
        outs = SF.block_tail_fwd_raw(*args)
        f_us = timed(lambda: SF.block_tail_fwd_raw(*args))
        bargs = (gx, None, outs["x_mid"], outs["mean"], outs["rstd"], outs["u"], rs1, rs2, gam, wpt, w1t, w2t)
        b_us = timed(lambda: SF.block_tail_bwd_raw(*bargs))
        fused = (f_us, b_us)
    return tf, tb, fused


def main():
    print(f"# Block tail census ({torch.cuda.get_device_name(0)}, {REP} launches per figure replayed from a hipGraph, microseconds)\n")
    total = 0.0
    tot_fused = 0.0
    for name, n, C, nblk in LEVELS:
        tf, tb, fused = census(n, C)
        sf, sb = sum(t for _, t in tf), sum(t for _, t in tb)
        print(f"## {name}: {n} x {C}, {nblk} Blocks\n")
        print("| direction | " + " | ".join(k for k, _ in tf) + " | sum |")
        print("|---|" + "---|" * (len(tf) + 1))
        print("| forward | " + " | ".join(f"{t:.1f}" for _, t in tf) + f" | {sf:.1f} |")
        print("| backward (" + ", ".join(k for k, _ in tb) + ") | " + " | ".join(f"{t:.1f}" for _, t in tb) + f" | {sb:.1f} |")
        if fused is not None:
            print(f"| fused pair | forward {fused[0]:.1f} | backward {fused[1]:.1f} | | | | | {fused[0] + fused[1]:.1f} |")
            tot_fused += nblk * (fused[0] + fused[1])
        print(f"\nper Block {sf + sb:.1f} us, level {nblk * (sf + sb) / 1e3:.3f} ms\n")
        total += nblk * (sf + sb)
    print(f"**chain total over the 14 Blocks: {total / 1e3:.3f} ms per step**")
    if tot_fused:
        print(f"**fused pair total over the 14 Blocks: {tot_fused / 1e3:.3f} ms per step**")


if __name__ == "__main__":
    main()
