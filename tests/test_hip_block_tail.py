"""GPU: the fused Block tail (csrc/block_tail.hip, SF.block_tail) -- proj + residual + LN2 + fc1 + GELU + fc2 + residual in one
launch each way at C in {32, 64, 128, 256} -- against the six-launch chain it replaces and a float64 restatement of the chain.

Criterion of the comparisons: per tensor, the relative L2 error (against float64, no intermediate rounding, same bf16 inputs and
weights) of the fused path is at most 1.5 x that of the unfused path, 3 x for tensors under 4,096 elements.  Both paths round at
the same points and differ only in the order of their fp32 sums, so the two errors should be equal; 1.5 covers scatter, 3 the
small tensors where a few rounding flips dominate.  Every measured pair is printed before it is asserted (pytest -s)."""
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CHANNELS = (32, 64, 128, 256)
BF = torch.bfloat16


@pytest.fixture
def all_widths(monkeypatch):
    """Every instantiated width is eligible in the kernel-level tests (the model's default bound, SF.BLOCK_TAIL_MAX_CHANNELS = 64,
    excludes the wide levels for speed, not for correctness: profiles/block_tail.md).  The dispatch tests run under the default."""
    from scenesplat_amd import functional as SF
    monkeypatch.setattr(SF, "BLOCK_TAIL_MAX_CHANNELS", 256)


def _R():
    from scenesplat_amd import functional as SF
    return SF.block_tail_rows()


class _Tail(nn.Module):
    """The parameters of one Block tail, every value bf16-representable (the float64 reference then starts from exactly the
    operands both GPU paths read), with their bf16 shadows and (in, out) copies registered and current."""

    def __init__(self, C, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.proj, self.fc1, self.fc2, self.ln2 = nn.Linear(C, C), nn.Linear(C, 4 * C), nn.Linear(4 * C, C), nn.LayerNorm(C)
        with torch.no_grad():
            for p in self.parameters():
                fan = p.shape[1] if p.dim() == 2 else None
                v = torch.randn(p.shape, generator=g) / (fan ** 0.5 if fan else 4.0)
                if p is self.ln2.weight:
                    v = 1.0 + v
                p.copy_(v.to(BF).float())

    def shadows(self):
        from scenesplat_amd import functional as SF
        ps = [p for m in (self.proj, self.fc1, self.fc2) for p in (m.weight, m.bias)]
        src, dst = SF.register_shadows(ps)
        SF.register_transposed([self.proj.weight, self.fc1.weight, self.fc2.weight])
        SF.refresh_shadows(src, dst)
        return self


def _inputs(C, n, scales, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    feat = torch.randn(n, C, device="cuda", generator=g).to(BF)
    x = torch.randn(n, C, device="cuda", generator=g)
    gx = torch.randn(n, C, device="cuda", generator=g)
    gc = torch.randn(n, C, device="cuda", generator=g).to(BF)
    rs1 = rs2 = None
    if scales:      # DropPath scales: Bernoulli(0.7) / 0.7, about 30 % zeros
        rs1 = (torch.rand(n, device="cuda", generator=g) < 0.7).float() / 0.7
        rs2 = (torch.rand(n, device="cuda", generator=g) < 0.7).float() / 0.7
    return feat, x, gx, gc, rs1, rs2


def _unfused(m, feat, x, rs1, rs2, want_copy):
    """Today's chain on the library's own ops; -> dict of forward tensors (autograd-connected where the ops are)."""
    from scenesplat_amd import functional as SF, native as nv
    y1 = SF.linear(feat, m.proj.weight, m.proj.bias)
    x_mid, h2, _ = SF.add_layer_norm(x, y1, rs1, m.ln2.weight, m.ln2.bias, m.ln2.eps, False, BF)
    a = SF.linear_gelu(h2, m.fc1.weight, m.fc1.bias)
    y2 = SF.linear(a, m.fc2.weight, m.fc2.bias)
    x_out, _, xcopy = SF.add_layer_norm(x_mid, y2, rs2, None, None, 0.0, want_copy, BF)
    with torch.no_grad():        # the tensors the chain does not hand out: the same calls its nodes make
        u = torch.nn.functional.linear(h2.detach(), SF.bf16_of(m.fc1.weight), SF.bf16_of(m.fc1.bias))
        _, _, _, mean, rstd = nv.add_layernorm_fwd(x.detach().contiguous(), y1.detach().contiguous(), rs1, m.ln2.weight.detach(),
                                                   m.ln2.bias.detach(), m.ln2.eps, True, False, BF)
    return dict(x_mid=x_mid, mean=mean, rstd=rstd, h2=h2, u=u, a=a, x_out=x_out, xcopy=xcopy)


def _reference(m, feat, x, rs1, rs2, gx, gc):
    """float64, plain torch ops, no intermediate rounding -> (forward dict, gradient dict)."""
    d = torch.float64
    P = {k: p.detach().to(d).requires_grad_(True) for k, p in m.named_parameters()}
    f, xx = feat.to(d).requires_grad_(True), x.to(d).requires_grad_(True)
    s1 = rs1.to(d)[:, None] if rs1 is not None else 1.0
    s2 = rs2.to(d)[:, None] if rs2 is not None else 1.0
    x_mid = xx + s1 * (f @ P["proj.weight"].t() + P["proj.bias"])
    mean = x_mid.mean(1)
    var = ((x_mid - mean[:, None]) ** 2).mean(1)
    rstd = (var + m.ln2.eps).rsqrt()
    h2 = (x_mid - mean[:, None]) * rstd[:, None] * P["ln2.weight"] + P["ln2.bias"]
    u = h2 @ P["fc1.weight"].t() + P["fc1.bias"]
    a = 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    x_out = x_mid + s2 * (a @ P["fc2.weight"].t() + P["fc2.bias"])
    cot = gx.to(d) + (gc.to(d) if gc is not None else 0.0)
    (x_out * cot).sum().backward()
    fwd = dict(x_mid=x_mid, mean=mean, rstd=rstd, h2=h2, u=u, a=a, x_out=x_out, xcopy=x_out)
    grads = dict(g_mid=xx.grad, dfeat=f.grad, **{k: p.grad for k, p in P.items()})
    return {k: v.detach() for k, v in fwd.items()}, grads


def _rel(t, ref):
    return float((t.detach().to(torch.float64) - ref).norm() / ref.norm().clamp_min(1e-300))


def _check(tag, pairs):
    """pairs: name -> (fused, unfused, reference).  Prints every measured pair, then asserts the ratio bound."""
    bad = []
    for k, (fu, un, ref) in pairs.items():
        ef, eu = _rel(fu, ref), _rel(un, ref)
        bound = 1.5 if ref.numel() >= 4096 else 3.0
        print(f"{tag} {k:12s} numel {ref.numel():7d} fused {ef:.3e} unfused {eu:.3e} ratio {ef / eu if eu else float('inf') if ef else 1.0:.3f} bound {bound}")
        if ef > bound * eu:
            bad.append((k, ef, eu))
    assert not bad, (tag, bad)


def _run_pair(C, n, scales, want_copy, seed):
    from scenesplat_amd import functional as SF
    m = _Tail(C, seed).cuda().shadows()
    feat, x, gx, gc, rs1, rs2 = _inputs(C, n, scales, seed + 1)
    gc = gc if want_copy else None
    ref_f, ref_g = _reference(m, feat, x, rs1, rs2, gx, gc)
    out = {}
    for path in ("fused", "unfused"):
        f, xx = feat.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            if path == "fused":
                assert SF.block_tail_eligible(xx, m.proj, m.ln2, m.fc1, m.fc2)
                raw = SF.block_tail_fwd_raw(f.detach(), xx.detach(), rs1, rs2, SF.bf16_of(m.proj.weight), m.proj.bias.detach(),
                                            SF.bf16_of(m.fc1.weight), m.fc1.bias.detach(), SF.bf16_of(m.fc2.weight), m.fc2.bias.detach(),
                                            m.ln2.weight.detach(), m.ln2.bias.detach(), m.ln2.eps, want_copy)
                x_out, xcopy = SF.block_tail(f, xx, rs1, rs2, m.proj, m.ln2, m.fc1, m.fc2, want_copy)
                assert torch.equal(x_out, raw["x_out"])
                fw = dict(raw, x_out=x_out, xcopy=xcopy)
            else:
                fw = _unfused(m, f, xx, rs1, rs2, want_copy)
        outs, cots = [fw["x_out"]], [gx]
        if want_copy:
            outs.append(fw["xcopy"]); cots.append(gc)
        torch.autograd.backward(outs, cots)
        out[path] = (fw, dict(g_mid=xx.grad, dfeat=f.grad))
        m.zero_grad(set_to_none=True)
    return m, out, ref_f, ref_g


@pytest.mark.parametrize("want_copy", [False, True])
@pytest.mark.parametrize("scales", [False, True])
@pytest.mark.parametrize("nk", ["1", "R-1", "R+1", "2R+3"])
@pytest.mark.parametrize("C", CHANNELS)
def test_fused_pair_is_as_close_to_float64_as_the_chain(C, nk, scales, want_copy, all_widths):
    R = _R()
    n = {"1": 1, "R-1": R - 1, "R+1": R + 1, "2R+3": 2 * R + 3}[nk]
    m, out, ref_f, ref_g = _run_pair(C, n, scales, want_copy, 100 * C + n)
    (ff, fg), (uf, ug) = out["fused"], out["unfused"]
    keys = ["x_mid", "mean", "rstd", "h2", "u", "a", "x_out"] + (["xcopy"] if want_copy else [])
    pairs = {k: (ff[k], uf[k], ref_f[k]) for k in keys}
    pairs.update({k: (fg[k], ug[k], ref_g[k]) for k in ("g_mid", "dfeat")})
    _check(f"C={C} n={n} scales={int(scales)} copy={int(want_copy)}", pairs)


@pytest.mark.parametrize("scales", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_parameter_gradients_through_a_stage(C, scales, monkeypatch, all_widths):
    """dWp, dbp, dW1, db1, dW2, db2, dgamma2, dbeta2 of both paths through a real stage_begin / identity-node flush on 257 rows
    (the stage opens from LINEAR_WGRAD_MIN_ROWS rows on: lowered for this test, for both paths alike)."""
    from scenesplat_amd import functional as SF
    monkeypatch.setattr(SF, "LINEAR_WGRAD_MIN_ROWS", 1)
    n = 257
    m = _Tail(C, 7 * C).cuda().shadows()
    feat, x, gx, gc, rs1, rs2 = _inputs(C, n, scales, 7 * C + 1)
    _, ref_g = _reference(m, feat, x, rs1, rs2, gx, None)
    got = {}
    for path in ("fused", "unfused"):
        m.zero_grad(set_to_none=True)
        f, xx = feat.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            SF.stage_begin([m.proj, m.ln2, m.fc1, m.fc2], n)
            assert SF._STAGE["cur"] is not None
            if path == "fused":
                x_out, _ = SF.block_tail(f, xx, rs1, rs2, m.proj, m.ln2, m.fc1, m.fc2, False)
            else:
                x_out = _unfused(m, f, xx, rs1, rs2, False)["x_out"]
            SF.stage_end()
        x_out.backward(gx)
        got[path] = {k: p.grad.clone() for k, p in m.named_parameters()}
        got[path].update(g_mid=xx.grad, dfeat=f.grad)
    _check(f"C={C} n={n} scales={int(scales)} stage", {k: (got["fused"][k], got["unfused"][k], ref_g[k]) for k in ref_g})


@pytest.mark.parametrize("C", CHANNELS)
def test_zero_row_scales_and_reproducibility(C):
    """rs1 == 0 rows: x_mid is x bit for bit; rs2 == 0 rows: x_out is x_mid bit for bit and the dy2 / du rows are exactly zero;
    two runs of forward + backward give identical bits."""
    from scenesplat_amd import functional as SF
    R = _R()
    n = 2 * R + 3
    m = _Tail(C, 3 * C).cuda().shadows()
    feat, x, gx, gc, rs1, rs2 = _inputs(C, n, True, 3 * C + 1)
    assert (rs1 == 0).any() and (rs2 == 0).any() and (rs1 != 0).any() and (rs2 != 0).any()
    w = [SF.bf16_of(p) for p in (m.proj.weight, m.fc1.weight, m.fc2.weight)]
    wt = [SF.bf16_t_of(p) for p in (m.proj.weight, m.fc1.weight, m.fc2.weight)]

    def run():
        o = SF.block_tail_fwd_raw(feat, x, rs1, rs2, w[0], m.proj.bias.detach(), w[1], m.fc1.bias.detach(), w[2], m.fc2.bias.detach(),
                                  m.ln2.weight.detach(), m.ln2.bias.detach(), m.ln2.eps, True)
        b = SF.block_tail_bwd_raw(gx, gc, o["x_mid"], o["mean"], o["rstd"], o["u"], rs1, rs2, m.ln2.weight.detach(), *wt)
        return o, b
    o, (g_mid, dfeat, dy2, du, dy1, part) = run()
    z1, z2 = rs1 == 0, rs2 == 0
    assert torch.equal(o["x_mid"][z1], x[z1])
    assert torch.equal(o["x_out"][z2], o["x_mid"][z2])
    assert not torch.equal(o["x_out"][~z2], o["x_mid"][~z2])
    assert (dy2[z2] == 0).all() and (du[z2] == 0).all() and (du[~z2] != 0).any()
    o2, b2 = run()
    for k in o:
        assert torch.equal(o[k].view(torch.int16 if o[k].dtype == BF else torch.int32), o2[k].view(torch.int16 if o2[k].dtype == BF else torch.int32)), k
    for t, t2 in zip((g_mid, dfeat, dy2, du, dy1, part), b2):
        assert torch.equal(t.view(torch.int16 if t.dtype == BF else torch.int32), t2.view(torch.int16 if t2.dtype == BF else torch.int32))


@pytest.mark.parametrize("nblocks", [1, 2, 4])
@pytest.mark.parametrize("C", CHANNELS)
def test_backward_workgroups_that_walk_several_tiles(C, nblocks):
    """The backward's grid-stride form (a level of more than 32,768 rows: 1,024 workgroups walk several row tiles each, the LDS
    tiles are reused and the dgamma / dbeta sums carry over) forced on 257 rows = 9 tiles by launching 1, 2 or 4 workgroups:
    every row-wise output equals the one-tile-per-workgroup launch bit for bit, and the reduced dgamma / dbeta are as close to
    float64 as that launch's (same ratio bound: only the order of the fp32 sums differs)."""
    from scenesplat_amd import functional as SF
    n = 257
    m = _Tail(C, 11 * C).cuda().shadows()
    feat, x, gx, gc, rs1, rs2 = _inputs(C, n, True, 11 * C + 1)
    _, ref_g = _reference(m, feat, x, rs1, rs2, gx, gc)
    w = [SF.bf16_of(p) for p in (m.proj.weight, m.fc1.weight, m.fc2.weight)]
    wt = [SF.bf16_t_of(p) for p in (m.proj.weight, m.fc1.weight, m.fc2.weight)]
    o = SF.block_tail_fwd_raw(feat, x, rs1, rs2, w[0], m.proj.bias.detach(), w[1], m.fc1.bias.detach(), w[2], m.fc2.bias.detach(),
                              m.ln2.weight.detach(), m.ln2.bias.detach(), m.ln2.eps, False)
    args = (gx, gc, o["x_mid"], o["mean"], o["rstd"], o["u"], rs1, rs2, m.ln2.weight.detach(), *wt)
    one = SF.block_tail_bwd_raw(*args)
    few = SF.block_tail_bwd_raw(*args, nblocks=nblocks)
    assert one[5].shape[1] == 9 and few[5].shape[1] == nblocks
    for a, b in zip(one[:5], few[:5]):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))
    r1, r2 = one[5].sum(1), few[5].sum(1)
    _check(f"C={C} nblocks={nblocks}", {"ln2.weight": (r2[0], r1[0], ref_g["ln2.weight"]), "ln2.bias": (r2[1], r1[1], ref_g["ln2.bias"])})


# ---- dispatch ---------------------------------------------------------------------------------------------------------------
def _tiny(**kw):
    from scenesplat_amd.pointcept_api import MODELS
    cfg = dict(type="PT-v3m1", in_channels=11, order=("z", "z-trans"), stride=(2,), enc_depths=(1, 1), enc_channels=(64, 64),
               enc_num_head=(4, 4), enc_patch_size=(64, 64), cls_mode=True, drop_path=0.0, shuffle_orders=False)
    cfg.update(kw)
    torch.manual_seed(5)
    return MODELS.build(cfg).cuda().train()


@pytest.fixture
def bench_knobs():
    """The execution knobs of the benchmark (MFMA window attention, bf16 conv) for the model-level tests."""
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import RUNTIME
    old = dict(RUNTIME)
    RUNTIME.update(attn_impl=nv.ATTN_MFMA, conv_dtype=torch.bfloat16)
    yield
    RUNTIME.clear(); RUNTIME.update(old)


def _tiny_data(n=257):
    g = torch.Generator().manual_seed(9)
    lin = torch.randperm(512, generator=g)[:n]
    gc = torch.stack([lin // 64, (lin // 8) % 8, lin % 8], 1).int()
    return dict(feat=torch.randn(n, 11, generator=g).cuda(), grid_coord=gc.cuda(), offset=torch.tensor([n]).cuda())


def _fused_calls(model, data, autocast=True):
    from scenesplat_amd import functional as SF
    before = SF.BLOCK_TAIL_CALLS
    if autocast:
        with torch.autocast("cuda", dtype=BF):
            out = model(dict(data)).feat
    else:
        out = model(dict(data)).feat
    out.float().square().sum().backward()
    bad = [k for k, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not bad, bad
    return SF.BLOCK_TAIL_CALLS - before


def test_block_dispatch(bench_knobs):
    from scenesplat_amd.pointcept_api import RUNTIME
    data = _tiny_data()
    model = _tiny()
    assert _fused_calls(model, data) == 2                      # both Blocks (64 channels, 257 rows and the pooled level)
    assert _fused_calls(model, data, autocast=False) == 0
    old = dict(RUNTIME)
    RUNTIME["fuse_block_tail"] = False
    try:
        assert _fused_calls(model, data) == 0
    finally:
        RUNTIME.clear(); RUNTIME.update(old)
    assert _fused_calls(_tiny(mlp_ratio=2), data) == 0
    pd = _tiny(pdnorm_ln=True, pdnorm_adaptive=False, pdnorm_conditions=("A", "B"))
    assert _fused_calls(pd, dict(data, condition=["A"])) == 0


def _tail_weights(model):
    from scenesplat_amd.pointcept_api.ptv3 import Block
    # (weights of 65,536 elements and more on the two finest levels keep an (in, out) copy for their own NT dgrad, fused tail or not)
    return [w for b in model.modules() if isinstance(b, Block) for w in (b.attn.proj.weight, b.mlp[0].fc1.weight, b.mlp[0].fc2.weight)
            if w.numel() < 65536]


def test_default_channel_bound_and_untouched_seam_path(bench_knobs, monkeypatch):
    """The shipped bound: 64 channels unless SS_BLOCK_TAIL_MAX_CHANNELS says otherwise.  A 128-channel Block takes the seam path
    under it and keeps today's dgrad form (no (in, out) copies registered for it); raising the bound fuses it; switching the fused
    tail off drops the copies of a 64-channel model again."""
    import os
    from scenesplat_amd import functional as SF
    from scenesplat_amd.pointcept_api import RUNTIME
    assert SF.BLOCK_TAIL_MAX_CHANNELS == int(os.environ.get("SS_BLOCK_TAIL_MAX_CHANNELS", "64"))
    monkeypatch.setattr(SF, "BLOCK_TAIL_MAX_CHANNELS", 64)
    data = _tiny_data()
    wide = _tiny(enc_channels=(128, 128), enc_num_head=(8, 8))
    assert _fused_calls(wide, data) == 0
    assert len(_tail_weights(wide)) == 2 and all(SF.bf16_t_of(w) is None for w in _tail_weights(wide))
    monkeypatch.setattr(SF, "BLOCK_TAIL_MAX_CHANNELS", 128)
    assert _fused_calls(wide, data) == 2
    assert all(SF.bf16_t_of(w) is not None for w in _tail_weights(wide))
    monkeypatch.setattr(SF, "BLOCK_TAIL_MAX_CHANNELS", 64)
    assert _fused_calls(wide, data) == 0
    assert all(SF.bf16_t_of(w) is None for w in _tail_weights(wide))
    narrow = _tiny()
    assert _fused_calls(narrow, data) == 2 and len(_tail_weights(narrow)) == 6 and all(SF.bf16_t_of(w) is not None for w in _tail_weights(narrow))
    old = dict(RUNTIME)
    RUNTIME["fuse_block_tail"] = False
    try:
        assert _fused_calls(narrow, data) == 0 and all(SF.bf16_t_of(w) is None for w in _tail_weights(narrow))
    finally:
        RUNTIME.clear(); RUNTIME.update(old)


def test_fused_and_seam_paths_agree_on_a_model(bench_knobs):
    """The same tiny model, fused tail on and off: output rows and parameter gradients agree to the bf16 step's own noise."""
    from scenesplat_amd.pointcept_api import RUNTIME
    data = _tiny_data()
    model = _tiny()
    res = {}
    old = dict(RUNTIME)
    try:
        for on in (True, False):
            RUNTIME["fuse_block_tail"] = on
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=BF):
                out = model(dict(data)).feat
            out.float().square().sum().backward()
            res[on] = (out.detach().float(), {k: p.grad.clone() for k, p in model.named_parameters()})
    finally:
        RUNTIME.clear(); RUNTIME.update(old)
    assert (res[True][0] - res[False][0]).norm() <= 1e-2 * res[False][0].norm()
    num = sum(float((res[True][1][k] - res[False][1][k]).norm()) ** 2 for k in res[True][1]) ** 0.5
    den = sum(float(res[False][1][k].norm()) ** 2 for k in res[True][1]) ** 0.5
    assert num <= 2e-2 * den, num / den


def test_steady_state_replay_matches_the_eager_step(bench_knobs):
    """A two-Block model on the fused tail: the captured step, replayed with other features, equals the eager step."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd.steady_state import SteadyStateStep
    data = _tiny_data()
    model = _tiny()
    n = data["feat"].shape[0]

    def fn(plan, t):
        with torch.autocast("cuda", dtype=BF):
            out = model(dict(feat=t["feat"], grid_coord=data["grid_coord"], offset=data["offset"], plan=plan))
        torch.autograd.backward(out.feat, grad_tensors=t["cot"])
        return {"feat": out.feat}
    steady = SteadyStateStep(fn, list(model.parameters()), warmup=1)
    rows_out = model.prepare_plan(data).levels[-1].n          # (cls_mode: the output lives on the pooled level)
    g = torch.Generator(device="cuda").manual_seed(2)
    for it in range(4):
        feat = torch.randn(n, 11, device="cuda", generator=g)
        cot = torch.randn(rows_out, 64, device="cuda", generator=g).to(BF)
        model.zero_grad(set_to_none=True)
        before = SF.BLOCK_TAIL_CALLS
        ref = fn(model.prepare_plan(data), dict(feat=feat, cot=cot))["feat"].detach().float().clone()
        assert SF.BLOCK_TAIL_CALLS - before == 2
        rg = {k: p.grad.clone() for k, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        out = steady(model.prepare_plan(data), dict(feat=feat, cot=cot))["feat"].float()
        assert steady.refused is None, steady.refused
        assert (out - ref).norm() <= 1e-2 * ref.norm(), (it, float((out - ref).norm() / ref.norm()))
        num = sum(float((p.grad - rg[k]).norm()) ** 2 for k, p in model.named_parameters()) ** 0.5
        den = sum(float(v.norm()) ** 2 for v in rg.values()) ** 0.5
        assert num <= 2e-2 * den, (it, num / den)
    assert steady.replays >= 2
