"""GPU parity of the relative-position-encoding window attention (enable_rpe=True; csrc/attention_rpe.hip and the RPE
instantiation of csrc/attention_simt.hip): the kernels against the reference module's golden vectors
(tests/golden/make_golden_rpe.py), the MFMA pair against the fp32-math SIMT pair, a zero table against the bias-free kernels,
and the tiny PT-v3m1 with RPE end to end."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ptv3 as optv3

pytestmark = pytest.mark.gpu
ORD = ("z", "z-trans", "hilbert", "hilbert-trans")
IMPLS = [("simt", torch.float32, 3e-5), ("simt", torch.bfloat16, 3e-2), ("mfma", torch.bfloat16, 3e-2)]
_FX = {}


def fixture(golden_dir):
    """attention_rpe.npz and its continuation files (one key space), read once"""
    if not _FX:
        for fn in sorted(glob.glob(os.path.join(golden_dir, "attention_rpe*.npz"))):
            with np.load(fn) as z:
                _FX.update({k: z[k] for k in z.files})
    return _FX


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def impl_code(impl):
    from scenesplat_amd import native as nv
    return nv.ATTN_SIMT if impl == "simt" else nv.ATTN_MFMA


def room(n_side, seed):
    """floor n x n + two walls n x h, shuffled: three axes with different extents (z offsets never reach the clamp)"""
    h = max(2, n_side * 72 // 256)
    xs, ys = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    floor = np.stack([xs.ravel(), ys.ravel(), np.zeros(n_side * n_side, int)], 1)
    yy, zz = np.meshgrid(np.arange(n_side), np.arange(1, h + 1), indexing="ij")
    wa = np.stack([np.zeros(yy.size, int), yy.ravel(), zz.ravel()], 1)
    wb = np.stack([np.full(yy.size, n_side - 1), yy.ravel(), zz.ravel()], 1)
    gc = np.concatenate([floor, wa, wb]).astype(np.int64)
    return gc[torch.randperm(len(gc), generator=torch.Generator().manual_seed(seed)).numpy()]


@pytest.mark.parametrize("name", ["r_h2d16", "r_h2d48", "r_short"])
@pytest.mark.parametrize("impl,dtype,tol", IMPLS)
def test_window_attention_rpe_matches_reference_module(golden_dir, name, impl, dtype, tol):
    """qkv Linear -> RPE windows -> proj Linear against the reference SerializedAttention(enable_rpe=True) with a std-1
    table: output, dx and every parameter gradient (rpe.rpe_table included); padded tail window; r_short runs at the
    run-time window length 40.  Bounds: those of test_window_attention_matches_reference_module."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd.plan import build_plan
    from scenesplat_amd.pointcept_api.ptv3 import SerializedAttention
    fx = fixture(golden_dir)
    C, H, K, oi = [int(v) for v in fx[f"{name}_cfg"]]
    sd = {k[len(name) + 4:]: torch.from_numpy(fx[k]) for k in fx if k.startswith(name + "_sd_")}
    att = SerializedAttention(C, H, K, order_index=oi, enable_rpe=True, enable_flash=False)
    assert set(att.state_dict()) == set(sd) and att.rpe.pos_bnd == int(fx[f"{name}_pos_bnd"])
    plan = build_plan(dev(fx[f"{name}_gc"]), dev(fx[f"{name}_offset"]), ORD, ())
    lv = plan.levels[0]
    Kw = att.rpe_window_size(lv)
    assert Kw == int(fx[f"{name}_K"])
    win = lv.window(oi, Kw)
    assert win.n_pad > win.n and win.max_window == Kw            # the fixture exercises duplicate padding
    x = dev(fx[f"{name}_x"]).requires_grad_(True)
    p = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    qkv = F.linear(x, p["qkv.weight"], p["qkv.bias"])
    a = SF.window_attention_rpe(qkv.to(dtype), win, lv.grid_coord, p["rpe.rpe_table"], att.rpe.pos_bnd, H, (C // H) ** -0.5,
                                impl_code(impl))
    y = F.linear(a.float(), p["proj.weight"], p["proj.bias"])
    (y * dev(fx[f"{name}_cot"])).sum().backward()
    ref_y = torch.from_numpy(fx[f"{name}_y"])
    scale = ref_y.abs().max().item()
    ref_dx = torch.from_numpy(fx[f"{name}_dx"])
    print(name, impl, dtype, "y err", (y.detach().cpu() - ref_y).abs().max().item(), "dx err", (x.grad.cpu() - ref_dx).abs().max().item())
    for k in p:
        r = torch.from_numpy(fx[f"{name}_grad_{k}"])
        print("  grad", k, ((p[k].grad.cpu() - r).norm() / r.norm()).item())
    assert (y.detach().cpu() - ref_y).abs().max() <= tol * max(1.0, scale)
    assert (x.grad.cpu() - ref_dx).abs().max() <= tol * max(1.0, ref_dx.abs().max().item()) * 2
    for k in p:
        r = torch.from_numpy(fx[f"{name}_grad_{k}"])
        assert (p[k].grad.cpu() - r).norm() <= tol * 4 * r.norm() + 1e-5, k


def indexed_bins(gc, win, pos_bnd):
    """(3 rpe_num,) bool: table rows some (query, key) pair of some window indexes"""
    rn = 2 * pos_bnd + 1
    hit = torch.zeros(3 * rn, dtype=torch.bool)
    gidx, ws = win.gidx.cpu().long(), win.win_start.cpu().tolist()
    for a, b in zip(ws[:-1], ws[1:]):
        g = gc[gidx[a:b]]
        for ax in range(3):
            d = (g[:, None, ax] - g[None, :, ax]).clamp(-pos_bnd, pos_bnd) + pos_bnd
            hit[ax * rn + torch.unique(d)] = True
    return hit


@pytest.mark.parametrize("H,d,K,counts", [(1, 16, 1024, [1100]), (2, 32, 256, [700, 300]), (1, 64, 128, [333]), (4, 48, 64, [200])])
def test_window_attention_rpe_mfma_matches_simt_fwd_bwd(H, d, K, counts):
    """MFMA kernels against the fp32-math SIMT kernels on identical bf16 inputs: forward, dQ, dK, dV (bounds of
    test_window_attention_mfma_matches_simt_fwd_bwd) and dtable; table rows that no pair indexes are exactly 0 in both, on a
    workspace the test pre-fills with NaN."""
    from scenesplat_amd import native as nv
    from scenesplat_amd.plan import build_plan
    from scenesplat_amd.pointcept_api.ptv3 import RPE
    g = torch.Generator().manual_seed(H * d)
    n = sum(counts)
    gc = torch.from_numpy(room(28, 2)[:n])
    plan = build_plan(gc.cuda(), torch.tensor(counts).cumsum(0).cuda(), ("hilbert", "z"), ())
    lv = plan.levels[0]
    win = lv.window(1, K)
    pos_bnd = RPE(K, H).pos_bnd
    C = H * d
    qkv = (torch.randn(n, 3 * C, generator=g) * 1.5).to(torch.bfloat16).cuda()
    dout = torch.randn(n, C, generator=g).to(torch.bfloat16).cuda()
    table = torch.randn(3 * (2 * pos_bnd + 1), H, generator=g).cuda()
    scale = d ** -0.5
    o_s, lse_s = nv.window_attn_rpe_fwd(qkv, win, lv.grid_coord, table, pos_bnd, H, scale, nv.ATTN_SIMT)
    o_m, lse_m = nv.window_attn_rpe_fwd(qkv, win, lv.grid_coord, table, pos_bnd, H, scale, nv.ATTN_MFMA)
    o_0, _ = nv.window_attn_fwd(qkv, win, H, scale, nv.ATTN_SIMT)
    assert (o_s.float() - o_0.float()).abs().max() > 0.3          # the bias matters on this input
    assert torch.allclose(lse_m, lse_s, atol=2e-2, rtol=1e-3)
    assert (o_m.float() - o_s.float()).abs().max() < 3e-2
    res = {}
    for nm, impl in (("simt", nv.ATTN_SIMT), ("mfma", nv.ATTN_MFMA)):
        nbytes = nv.window_attn_rpe_bwd_workspace_bytes(qkv, win, H, pos_bnd)
        ws = torch.full((max(nbytes, 256) // 4,), float("nan"), device="cuda").view(torch.uint8)
        dqkv, dt = nv.window_attn_rpe_bwd(qkv, o_s, dout, lse_s, win, lv.grid_coord, table, pos_bnd, H, scale, impl, workspace=ws)
        res[nm] = (dqkv.float(), dt)
    g_s, g_m = res["simt"][0], res["mfma"][0]
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        a, b = g_m[:, sl], g_s[:, sl]
        rel = (a - b).norm() / b.norm()
        print(name, "rel", rel.item(), "max", (a - b).abs().max().item())
        assert rel < 2e-2, (name, rel.item())
        assert (a - b).abs().max() < 0.05 * b.abs().max() + 1e-2, name
    t_s, t_m = res["simt"][1].cpu(), res["mfma"][1].cpu()
    rel = (t_m - t_s).norm() / t_s.norm()
    print("dtable rel", rel.item(), "max", (t_m - t_s).abs().max().item(), "of", t_s.abs().max().item())
    assert torch.isfinite(t_s).all() and torch.isfinite(t_m).all()
    assert rel < 2e-2, rel.item()
    assert (t_m - t_s).abs().max() < 0.05 * t_s.abs().max() + 1e-2
    hit = indexed_bins(gc, win, pos_bnd)
    print("table rows never indexed:", int((~hit).sum()), "of", hit.numel())
    if K == 1024:
        assert int((~hit).sum()) >= 48          # the z extent of the room is far inside the clamp
    assert (t_s[~hit] == 0).all() and (t_m[~hit] == 0).all()
    assert t_s[hit].abs().max() > 0


@pytest.mark.parametrize("H,d", [(4, 16), (2, 32), (2, 48), (1, 64)])
@pytest.mark.parametrize("impl,dtype,tol", IMPLS)
def test_zero_table_reproduces_plain_window_attention(impl, dtype, tol, H, d):
    """every head dim of the kernels; on the SIMT path both sides are instantiations of one kernel template"""
    from scenesplat_amd import functional as SF
    from scenesplat_amd.plan import build_plan
    g = torch.Generator().manual_seed(5)
    counts, K = [150, 210], 40
    n, C = sum(counts), H * d
    gc = torch.from_numpy(room(28, 3)[:n])
    plan = build_plan(gc.cuda(), torch.tensor(counts).cumsum(0).cuda(), ORD, ())
    lv = plan.levels[0]
    win = lv.window(2, K)
    assert win.n_pad > win.n
    qkv0 = torch.randn(n, 3 * C, generator=g).to(dtype).cuda()
    cot = torch.randn(n, C, generator=g).cuda()
    table = torch.zeros(3 * 25, H, device="cuda", requires_grad=True)
    qa, qb = qkv0.clone().requires_grad_(True), qkv0.clone().requires_grad_(True)
    ya = SF.window_attention_rpe(qa, win, lv.grid_coord, table, 12, H, d ** -0.5, impl_code(impl))
    yb = SF.window_attention(qb, win, H, d ** -0.5, impl_code(impl))
    (ya.float() * cot).sum().backward()
    (yb.float() * cot).sum().backward()
    sc = max(1.0, yb.float().abs().max().item())
    assert (ya.float() - yb.float()).abs().max() <= tol * sc
    assert (qa.grad.float() - qb.grad.float()).abs().max() <= tol * max(1.0, qb.grad.float().abs().max().item()) * 2
    assert table.grad is not None and torch.isfinite(table.grad).all() and table.grad.abs().max() > 0


def build_tiny_rpe(golden_dir):
    from scenesplat_amd.pointcept_api import MODELS
    fx = fixture(golden_dir)
    cfg = {k[9:]: (tuple(v.tolist()) if v.ndim else v.item()) for k, v in fx.items() if k.startswith("tiny_cfg_")}
    model = MODELS.build(dict(type="PT-v3m1", **cfg, drop_path=0.0, shuffle_orders=False, enable_rpe=True, enable_flash=False))
    sd = dict(optv3.init_state_dict(cfg, seed=11))
    tables = [k for k in model.state_dict() if k.endswith("rpe.rpe_table")]
    for i, k in enumerate(tables):
        sd[k] = torch.randn(model.state_dict()[k].shape, generator=torch.Generator().manual_seed(1000 + i))
    model.load_state_dict(sd, strict=True)
    return fx, model.cuda(), tables


def run_tiny(model, fx, autocast=False):
    model.zero_grad()
    feat = torch.from_numpy(fx["tiny_feat"]).cuda().requires_grad_(True)
    torch.manual_seed(77)   # the reference drew the pooling curve shuffles from this seed (make_golden_rpe.py)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = model(dict(feat=feat, grid_coord=torch.from_numpy(fx["tiny_gc"]).cuda(), offset=torch.from_numpy(fx["tiny_offset"]).cuda()))
    y = out.feat.float()
    (y * torch.from_numpy(fx["tiny_cot"]).cuda()).sum().backward()
    return y.detach().cpu(), feat.grad.cpu()


def test_tiny_ptv3_with_rpe_fp32_matches_reference(golden_dir, monkeypatch):
    """bounds of test_tiny_ptv3_fp32_matches_reference; the run-time window length per block is the reference's"""
    from scenesplat_amd import native as nv
    fx, model, tables = build_tiny_rpe(golden_dir)
    seen = []
    orig = nv.window_attn_rpe_fwd
    monkeypatch.setattr(nv, "window_attn_rpe_fwd", lambda qkv, win, *a: (seen.append((win.max_window, a[-1])), orig(qkv, win, *a))[1])
    model.eval()
    y, dfeat = run_tiny(model, fx)
    assert [k for k, _ in seen] == fx["tiny_K"].tolist() and all(i == nv.ATTN_SIMT for _, i in seen)
    ref = torch.from_numpy(fx["tiny_y"])
    print("tiny y err", (y - ref).abs().max().item())
    assert torch.allclose(y, ref, atol=2e-3, rtol=2e-3), (y - ref).abs().max()
    r = torch.from_numpy(fx["tiny_dfeat"])
    assert (dfeat - r).norm() <= 2e-3 * r.norm()
    params = dict(model.named_parameters())
    grads = [k for k in fx if k.startswith("tiny_grad_")]
    assert len(grads) == 4 and sum(k.endswith("rpe_table") for k in grads) == 2
    for k in grads:
        gq, r = params[k[10:]].grad.cpu(), torch.from_numpy(fx[k])
        print("  grad", k[10:], ((gq - r).norm() / r.norm()).item())
        assert (gq - r).norm() <= 3e-3 * r.norm() + 1e-5, (k, (gq - r).norm() / r.norm())


def test_tiny_ptv3_with_rpe_trains_a_step_under_bf16_autocast(golden_dir, monkeypatch):
    from scenesplat_amd import native as nv
    fx, model, tables = build_tiny_rpe(golden_dir)
    seen = []
    orig = nv.window_attn_rpe_fwd
    monkeypatch.setattr(nv, "window_attn_rpe_fwd", lambda qkv, win, *a: (seen.append((qkv.dtype, a[-1])), orig(qkv, win, *a))[1])
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    before = {k: model.state_dict()[k].clone() for k in tables}
    y, dfeat = run_tiny(model, fx, autocast=True)
    assert len(seen) == 7 and all(dt == torch.bfloat16 and i == nv.ATTN_MFMA for dt, i in seen)      # head dims 16 and 48
    assert torch.isfinite(y).all() and torch.isfinite(dfeat).all()
    params = dict(model.named_parameters())
    for k in tables:
        gq = params[k].grad
        assert gq is not None and gq.dtype == torch.float32 and torch.isfinite(gq).all() and gq.abs().max() > 0, k
    opt.step()
    for k in tables:
        assert torch.isfinite(model.state_dict()[k]).all() and not torch.equal(model.state_dict()[k], before[k]), k
