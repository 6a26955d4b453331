"""GPU tests of PDNorm / PPT-v1m2: the grouped modulation kernels (csrc/pdnorm.hip) against fp64, selection purity against the plain
model, parity with the reference's fixtures (tests/golden/pdnorm*.npz, make_golden_pdnorm.py), launch counts, the split backward,
PPT-v1m2 end to end and the steady-state replay with alternating conditions."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TINY = dict(in_channels=11, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2),
            enc_depths=(1, 1, 2), enc_channels=(16, 32, 64), enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 16),
            dec_depths=(2, 1), dec_channels=(48, 32), dec_num_head=(1, 2), dec_patch_size=(64, 64))       # make_golden_rpe.TINY_CFG
CONDITIONS = ("A", "B", "C")
U = 2.0 ** -23


def backbone_cfg(adaptive=True, affine=True, **kw):
    return dict(dict(type="PT-v3m1", **TINY, enable_flash=False, drop_path=0.0, shuffle_orders=False, pdnorm_bn=True, pdnorm_ln=True,
                     pdnorm_adaptive=adaptive, pdnorm_affine=affine, pdnorm_conditions=CONDITIONS), **kw)


def seeded_state(state_dict):
    """The fixture model's parameters and buffers (make_golden_pdnorm.py): the i-th tensor in state-dict order is
    randn(shape, Generator().manual_seed(2000 + i)), / sqrt(fan_in) for matrices and conv weights; running_var = 0.5 + rand."""
    out = {}
    for i, (k, v) in enumerate(state_dict.items()):
        g = torch.Generator().manual_seed(2000 + i)
        if not v.is_floating_point():
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            t = torch.randn(v.shape, generator=g)
            out[k] = t / (v[0].numel() ** 0.5) if v.dim() > 1 else t
    return out


def context_of(j, channels=256):
    return torch.randn((1, channels), generator=torch.Generator().manual_seed(3000 + j))


@pytest.fixture(scope="module")
def cloud(golden_dir):
    fx = np.load(os.path.join(golden_dir, "ptv3_tiny.npz"))
    return {k: torch.from_numpy(fx[k]).cuda() for k in ("gc", "offset", "feat", "cot")}


def run_backbone(model, cloud, cond, context=None, autocast=False, cut=None, feat_grad=True):
    feat = cloud["feat"].clone().requires_grad_(feat_grad)
    d = dict(feat=feat, grid_coord=cloud["gc"], offset=cloud["offset"], condition=cond)
    if context is not None:
        d["context"] = context
    if cut is not None:
        d["backward_cut"] = cut
    torch.manual_seed(77)                       # the pooling curve shuffles, as the reference drew them
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = model(d)
    return out.feat, feat


# ---- 7. grouped kernels against fp64 -------------------------------------------------------------------------------------------
WIDTHS = (4, 20, 32, 48, 100, 768)


def make_rows(L, Cc, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = []
    for l in range(L):
        C = WIDTHS[l % len(WIDTHS)]
        affine = (l % 3 != 1) if L > 1 else True
        W = torch.randn(2 * C, Cc, device="cuda", generator=g) / Cc ** 0.5
        b = torch.randn(2 * C, device="cuda", generator=g)
        rows.append((W, b, torch.randn(C, device="cuda", generator=g) if affine else None,
                     torch.randn(C, device="cuda", generator=g) if affine else None))
    ctx = (torch.rand(1, Cc, device="cuda", generator=g) * 40 - 20)            # SiLU's tails ...
    ctx[0, ::7] = 0.0                                                          # ... and exact zeros
    ctx[0, 1], ctx[0, 2] = 20.0, -20.0
    dge = [torch.randn(r[0].shape[0] // 2, device="cuda", generator=g) for r in rows]
    dbe = [torch.randn(r[0].shape[0] // 2, device="cuda", generator=g) for r in rows]
    if L == 7:
        dge[3], dbe[5] = None, None            # a norm that sent no gradient counts as zeros
    return rows, ctx, dge, dbe


def check(name, got, ref, terms, absval):
    """|got - fp64 reference| <= (terms + 8) * 2^-23 * (the formula with every term replaced by its absolute value), per element."""
    bound = (terms + 8) * U * absval
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"  {name}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


@pytest.mark.parametrize("Cc", [256, 24])
@pytest.mark.parametrize("L", [1, 7, 83])
def test_grouped_modulation_kernels_match_fp64(L, Cc):
    from scenesplat_amd import native as nv
    rows, ctx, dge, dbe = make_rows(L, Cc, seed=100 * L + Cc)
    tab = nv.PDNormTable(rows, Cc)
    assert tab.vec4 == 1          # Cc = 24 and 256 both take 16-byte lanes (the one-element-per-lane kernels: next test)
    c32 = ctx.reshape(-1).contiguous()
    geff, beff, ops = nv.pdnorm_mod_fwd(c32, tab)
    dctx, dW, db, dg, dbt = nv.pdnorm_mod_bwd(c32, tab, ops, dge, dbe)
    # twice on the same inputs: bit-equal, dcontext included
    geff2, beff2, ops2 = nv.pdnorm_mod_fwd(c32, tab)
    dctx2, dW2, db2, dg2, dbt2 = nv.pdnorm_mod_bwd(c32, tab, ops2, dge, dbe)
    assert torch.equal(ops, ops2) and torch.equal(dctx, dctx2)
    for a, b in zip(geff + beff + dW + db + [t for t in dg + dbt if t is not None],
                    geff2 + beff2 + dW2 + db2 + [t for t in dg2 + dbt2 if t is not None]):
        assert torch.equal(a, b)
    x = c32.double()
    sg = 1.0 / (1.0 + torch.exp(-x))
    s = x * sg
    dsilu, dsilu_abs = sg * (1 + x * (1 - sg)), sg * (1 + x.abs() * (1 - sg))
    acc, acc_abs, terms_ctx, off = torch.zeros(Cc, dtype=torch.float64, device="cuda"), torch.zeros(Cc, dtype=torch.float64, device="cuda"), 0, 0
    for l, (W, b, gamma, beta) in enumerate(rows):
        C = W.shape[0] // 2
        Wd, bd = W.double(), b.double()
        lin, lin_abs = Wd @ s + bd, Wd.abs() @ s.abs() + bd.abs()
        shift, scale, a_shift, a_scale = lin[:C], lin[C:], lin_abs[:C], lin_abs[C:]
        gm = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device="cuda")
        bt = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        o = ops[off:off + C]
        check(f"ops[{l}]", o, 1 + scale, Cc + 2, 1 + a_scale)
        check(f"gamma_eff[{l}]", geff[l], gm * (1 + scale), Cc + 2, gm.abs() * (1 + a_scale))
        check(f"beta_eff[{l}]", beff[l], bt * (1 + scale) + shift, 2 * Cc + 3, bt.abs() * (1 + a_scale) + a_shift)
        ge = dge[l].double() if dge[l] is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        be = dbe[l].double() if dbe[l] is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        dbr = torch.cat([be, ge * gm + be * bt])
        dbr_abs = torch.cat([be.abs(), ge.abs() * gm.abs() + be.abs() * bt.abs()])
        check(f"db[{l}]", db[l], dbr, 2, dbr_abs)
        check(f"dW[{l}]", dW[l], dbr[:, None] * s[None, :], 2, dbr_abs[:, None] * s.abs()[None, :])
        if gamma is not None:
            check(f"dgamma[{l}]", dg[l], ge * o.double(), 1, ge.abs() * o.double().abs())
            check(f"dbeta[{l}]", dbt[l], be * o.double(), 1, be.abs() * o.double().abs())
        else:
            assert dg[l] is None and dbt[l] is None
        acc += Wd.t() @ dbr
        acc_abs += Wd.abs().t() @ dbr_abs
        terms_ctx += 3 * C if gamma is not None else 2 * C
        off += C
    check("dcontext", dctx, dsilu * acc, terms_ctx, dsilu_abs * acc_abs)


def test_grouped_modulation_scalar_lanes_and_split_sum():
    """A context that is not 16-byte aligned takes the one-element-per-lane kernels: same bounds hold (checked against the 16-byte
    result within twice the forward bound's scale), and the two-part sum of dcontext equals two launches over the two parts."""
    from scenesplat_amd import native as nv
    rows, ctx, dge, dbe = make_rows(7, 24, seed=5)
    tab = nv.PDNormTable(rows, 24)
    c_al = ctx.reshape(-1).contiguous()
    c_un = torch.empty(25, device="cuda")[1:]
    c_un.copy_(c_al)
    assert c_un.data_ptr() % 16 != 0 and tab.vec4 == 1
    g1, b1, o1 = nv.pdnorm_mod_fwd(c_al, tab)
    g2, b2, o2 = nv.pdnorm_mod_fwd(c_un, tab)
    # same terms in another order: both lie within (Cc + 2 + 8) u |.|-formula of the exact value, so within twice that of each other
    for a, b in zip(g1 + b1, g2 + b2):
        assert torch.allclose(a, b, rtol=0, atol=2 * (2 * 24 + 11) * U * 40.0)          # |.|-formula <= ~40 at these sizes (|s| <= 20, |W| ~ 0.2)
    # split sum: rows [0, 4) and [4, 7) as two groups against one group with split_row = 4
    d_one = nv.pdnorm_mod_bwd(c_al, tab, o1, dge, dbe, split_row=4)[0]
    ta, tb = nv.PDNormTable(rows[:4], 24), nv.PDNormTable(rows[4:], 24)
    na = sum(tab.widths[:4])
    d_a = nv.pdnorm_mod_bwd(c_al, ta, o1[:na].contiguous(), dge[:4], dbe[:4])[0]
    d_b = nv.pdnorm_mod_bwd(c_al, tb, o1[na:].contiguous(), dge[4:], dbe[4:])[0]
    assert torch.equal(d_one, d_a + d_b)


def test_grouped_modulation_argument_handling():
    from scenesplat_amd import native as nv
    rows, ctx, dge, dbe = make_rows(1, 24, seed=1)
    tab = nv.PDNormTable(rows, 24)
    c32 = ctx.reshape(-1).contiguous()
    out = torch.full((3 * 4,), 7.0, device="cuda")
    desc = tab.desc.copy()
    desc[:, 5], desc[:, 6], desc[:, 7] = out.data_ptr(), out.data_ptr() + 16, out.data_ptr() + 32
    from scenesplat_amd import grouped
    d_dev, s_dev = grouped._upload_descriptors(desc, tab.starts, tab.dev)
    lib, p, st = nv.lib(), nv._p, nv._stream()
    null = ctypes.c_void_p(0)
    assert lib.ss_pdnorm_mod_fwd(p(d_dev), p(s_dev), 0, 0, p(c32), 24, 0, st) == 0                # L = 0: SS_OK, no launch
    assert lib.ss_pdnorm_mod_bwd(p(d_dev), p(s_dev), 0, 0, p(c32), 24, 0, 0, null, null, st) == 0
    assert lib.ss_pdnorm_mod_fwd(null, p(s_dev), 1, 1, p(c32), 24, 0, st) == 1                    # null table: SS_ERR_ARG
    assert lib.ss_pdnorm_mod_bwd(null, p(s_dev), 1, 1, p(c32), 24, 0, 0, p(out), p(out), st) == 1
    assert lib.ss_pdnorm_mod_fwd(p(d_dev), p(s_dev), 1, 1, p(c32), 0, 0, st) == 1                 # Cc <= 0
    assert lib.ss_pdnorm_mod_fwd(p(d_dev), p(s_dev), 1, 1, p(c32), -4, 0, st) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                            # outputs untouched
    cpu_rows = [tuple(t.cpu() if t is not None else None for t in rows[0])]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.PDNormTable(cpu_rows, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.pdnorm_mod_fwd(c32.cpu(), tab)
    from scenesplat_amd import functional as SF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.pdnorm_modulation(SF.PDNormGroup(rows), ctx.cpu())


# ---- standalone PDNorm layer (the reference's call on a Point), fused and unfused widths ---------------------------------------
@pytest.mark.parametrize("C", [6, 32])
@pytest.mark.parametrize("kind,affine,train", [("bn", True, True), ("bn", False, False), ("ln", True, False), ("ln", False, False)])
def test_pdnorm_layer_matches_its_restatement(C, kind, affine, train):
    """norm_c(feat) * (1 + scale) + shift with shift, scale = Linear(silu(context)).chunk(2), restated in fp64.  C = 6 takes the
    unfused path (the fused norm kernels need C % 4 == 0).  Tolerance: outputs are O(10), each the result of a few hundred fp32
    roundings at most (n = 200 rows of batch statistics, 256 context channels): 300 * 2^-24 * 10 ~ 2e-4, allclose(1e-4, 1e-4)
    on typical, not worst-case, accumulation."""
    from functools import partial
    from scenesplat_amd.pointcept_api import PDNorm, Point
    torch.manual_seed(3)
    layer = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01, affine=affine) if kind == "bn" else partial(torch.nn.LayerNorm, elementwise_affine=affine)
    m = PDNorm(C, layer, conditions=CONDITIONS, adaptive=True)
    m.load_state_dict(seeded_state(m.state_dict()))
    m = m.cuda().train(train)
    x = torch.randn(200, C, device="cuda", requires_grad=True)
    ctx = context_of(1).cuda().requires_grad_(True)
    rm0 = m.norm[1].running_mean.clone() if kind == "bn" else None
    y = m(Point(feat=x, condition=["B"], context=ctx))["feat"]
    cot = torch.randn(200, C, device="cuda")
    (y * cot).sum().backward()
    xd, cd = x.detach().double().requires_grad_(True), ctx.detach().double().requires_grad_(True)
    n1 = m.norm[1]
    gm = n1.weight.detach().double() if affine else None
    bt = n1.bias.detach().double() if affine else None
    if kind == "bn":
        yn = F.batch_norm(xd, rm0.double() if not train else None, n1.running_var.double() if not train else None, gm, bt, train, 0.0, n1.eps)
    else:
        yn = F.layer_norm(xd, (C,), gm, bt, n1.eps)
    lin = m.modulation[1]
    shift, scale = F.linear(F.silu(cd), lin.weight.detach().double(), lin.bias.detach().double()).chunk(2, dim=1)
    yr = yn * (1.0 + scale) + shift
    (yr * cot.double()).sum().backward()
    assert torch.allclose(y.double(), yr, atol=1e-4, rtol=1e-4), float((y.double() - yr).abs().max())
    assert torch.allclose(x.grad.double(), xd.grad, atol=1e-4, rtol=1e-4)
    assert (ctx.grad.double() - cd.grad).norm() <= 1e-4 * cd.grad.norm()
    if kind == "bn":
        for j in (0, 2):            # only the selected condition's buffers move
            assert int(m.norm[j].num_batches_tracked) == 0 and bool((m.norm[j].running_mean == seeded_state(m.state_dict())[f"norm.{j}.running_mean"].cuda()).all())
        assert int(m.norm[1].num_batches_tracked) == (1 if train else 0)


# ---- 8. selection is pure ------------------------------------------------------------------------------------------------------
def _plain_twin(pd_model, c, **kw):
    """The plain PT-v3m1 (flags off) loaded with the c-th copy of every norm's parameters and buffers; -> (model, plain key -> pd key)."""
    from scenesplat_amd.pointcept_api import MODELS, PDNorm
    cfg = dict(backbone_cfg(), pdnorm_bn=False, pdnorm_ln=False, **kw)
    plain = MODELS.build(cfg).cuda()
    pd_names = [n for n, m in pd_model.named_modules() if isinstance(m, PDNorm)]
    sd, src, mapping = pd_model.state_dict(), {}, {}
    for k in plain.state_dict():
        owner = [n for n in pd_names if k.startswith(n + ".")]
        pk = k if not owner else owner[0] + f".norm.{c}." + k[len(owner[0]) + 1:]
        src[k], mapping[k] = sd[pk].clone(), pk
    plain.load_state_dict(src, strict=True)
    return plain, mapping


def _grads(model):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}


def _compare_grads_as_repeats_allow(plain_runs, got, mapping, label):
    """Two runs of the same kernels on the same operands: if the plain model's gradients repeat bit for bit, require bit equality; otherwise, per tensor, at most four times
    the largest difference the two plain runs showed."""
    g1, g2 = plain_runs
    repeat = all(torch.equal(g1[k], g2[k]) for k in g1 if g1[k] is not None)
    print(f"{label}: the reference run's gradients {'repeat bit for bit: bit equality required' if repeat else 'do not repeat: 4x their spread allowed'}")
    for k, pk in mapping.items():
        if g1[k] is None:
            continue
        assert got[pk] is not None, pk
        if repeat:
            assert torch.equal(got[pk], g1[k]), (pk, float((got[pk] - g1[k]).abs().max()))
        else:
            spread = float((g1[k] - g2[k]).abs().max())
            assert float((got[pk] - g1[k]).abs().max()) <= 4 * spread, (pk, spread)


@pytest.mark.parametrize("pre_norm", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_selection_is_pure(cloud, mode, pre_norm):
    from scenesplat_amd.pointcept_api import MODELS
    c = 2
    pd = MODELS.build(backbone_cfg(adaptive=False, affine=True, pre_norm=pre_norm))
    pd.load_state_dict(seeded_state(pd.state_dict()))
    pd = pd.cuda()
    plain, mapping = _plain_twin(pd, c, pre_norm=pre_norm)
    init = {k: v.clone() for k, v in pd.state_dict().items()}
    runs = []
    for _ in range(2):
        st = {k: v.clone() for k, v in plain.state_dict().items()}
        plain.train(mode == "train"); plain.zero_grad(set_to_none=True)
        y0, f0 = run_backbone(plain, cloud, None)
        (y0 * cloud["cot"]).sum().backward()
        runs.append((_grads(plain), f0.grad.clone()))
        plain_after = {k: v.clone() for k, v in plain.state_dict().items()}
        plain.load_state_dict(st)                         # (the second run starts from the same running statistics)
    pd.train(mode == "train"); pd.zero_grad(set_to_none=True)
    y1, f1 = run_backbone(pd, cloud, [CONDITIONS[c], "ignored"])
    (y1 * cloud["cot"]).sum().backward()
    assert torch.equal(y1, y0)                            # same kernels on the same operands
    got = _grads(pd)
    got["__feat__"] = f1.grad
    g1, g2 = dict(runs[0][0], __feat__=runs[0][1]), dict(runs[1][0], __feat__=runs[1][1])
    _compare_grads_as_repeats_allow((g1, g2), got, {k: mapping.get(k, k) for k in g1}, f"selection[{mode}, pre_norm={pre_norm}]")
    # unselected conditions: no gradient, no buffer moved; the selected one's buffers moved exactly as the plain model's did
    after = pd.state_dict()
    back = {pk: k for k, pk in mapping.items()}
    for k, v in after.items():
        if k in back:
            assert torch.equal(v, plain_after[back[k]]), k
        else:
            assert torch.equal(v, init[k]), k
            if k.endswith("num_batches_tracked"):
                assert int(v) == 0
    moved = [k for k in after if k.endswith("running_mean") and not torch.equal(after[k], init[k])]
    assert (len(moved) == 7 and all(f".norm.{c}." in k for k in moved)) if mode == "train" else not moved
    for k, g in got.items():
        if k != "__feat__" and k not in mapping.values():
            assert g is None or not bool(g.any()), k


# ---- 9. parity with the reference ----------------------------------------------------------------------------------------------
PARITY_GRADS = ("enc.enc1.block0.norm1.0.modulation.1.weight", "dec.dec0.block0.cpe.2.modulation.1.weight", "enc.enc2.block1.attn.qkv.weight")
NORM_W = "enc.enc2.block0.norm2.0.norm.%d.weight"


def _parity_model(affine):
    from scenesplat_amd.pointcept_api import MODELS
    model = MODELS.build(backbone_cfg(adaptive=True, affine=affine))
    model.load_state_dict(seeded_state(model.state_dict()), strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("cond", ["B", "C"])
@pytest.mark.parametrize("affine", [True, False])
def test_tiny_pdnorm_fp32_matches_reference(golden_dir, cloud, affine, cond):
    fx = np.load(os.path.join(golden_dir, f"pdnorm_aff{int(affine)}_{cond}.npz"))
    j = CONDITIONS.index(cond)
    model = _parity_model(affine)
    ctx = context_of(j).cuda().requires_grad_(True)
    y, feat = run_backbone(model, cloud, [cond], ctx)
    (y * cloud["cot"]).sum().backward()
    y, ref = y.detach().float().cpu(), torch.from_numpy(fx["y"])
    cosd = 1 - F.cosine_similarity(y, ref, dim=1)
    print("cosine distance max %.3e, |y - ref| max %.3e" % (cosd.max(), (y - ref).abs().max()))
    assert cosd.max() < 1e-5, cosd.max()
    assert torch.allclose(y, ref, atol=2e-3, rtol=2e-3), (y - ref).abs().max()
    r = torch.from_numpy(fx["dfeat"])
    assert (feat.grad.cpu() - r).norm() <= 2e-3 * r.norm()
    r = torch.from_numpy(fx["dcontext"])
    assert (ctx.grad.cpu() - r).norm() <= 3e-3 * r.norm() + 1e-5, (ctx.grad.cpu() - r).norm() / r.norm()
    params = dict(model.named_parameters())
    names = list(PARITY_GRADS) + ([NORM_W % j] if affine else [])
    for pn in names:
        g, r = params[pn].grad.cpu(), torch.from_numpy(fx["grad_" + pn])
        assert (g - r).norm() <= 3e-3 * r.norm() + 1e-5, (pn, (g - r).norm() / r.norm())
    if affine:
        other = params[NORM_W % ((j + 1) % 3)].grad
        assert bool(fx["unselected_grad_is_none_or_zero"]) and (other is None or not bool(other.any()))


@pytest.mark.parametrize("cond", ["B", "C"])
@pytest.mark.parametrize("affine", [True, False])
def test_tiny_pdnorm_bf16_autocast_within_cosine_budget(golden_dir, cloud, affine, cond):
    from scenesplat_amd.pointcept_api import RUNTIME
    fx = np.load(os.path.join(golden_dir, f"pdnorm_aff{int(affine)}_{cond}.npz"))
    model = _parity_model(affine)
    old = dict(RUNTIME)
    try:
        RUNTIME["conv_dtype"] = torch.bfloat16
        with torch.no_grad():
            y, _ = run_backbone(model, cloud, [cond], context_of(CONDITIONS.index(cond)).cuda(), autocast=True, feat_grad=False)
    finally:
        RUNTIME.clear(); RUNTIME.update(old)
    cosd = 1 - F.cosine_similarity(y.float().cpu(), torch.from_numpy(fx["y"]), dim=1)
    print("bf16 cosine distance: mean %.3e max %.3e" % (cosd.mean(), cosd.max()))
    assert cosd.mean() < 1e-4 and cosd.max() < 2e-3


# ---- 10. launch count, 11. split backward ---------------------------------------------------------------------------------------
class _Count:
    def __init__(self, monkeypatch):
        from scenesplat_amd import native as nv
        self.fwd = self.bwd = 0
        f0, b0 = nv.pdnorm_mod_fwd, nv.pdnorm_mod_bwd

        def f(*a, **k):
            self.fwd += 1
            return f0(*a, **k)

        def b(*a, **k):
            self.bwd += 1
            return b0(*a, **k)
        monkeypatch.setattr(nv, "pdnorm_mod_fwd", f)
        monkeypatch.setattr(nv, "pdnorm_mod_bwd", b)


def _ppt(backbone_mode=False, **kw):
    from scenesplat_amd.pointcept_api import MODELS
    model = MODELS.build(dict(type="PPT-v1m2", backbone=backbone_cfg(**kw), criteria=[dict(type="CrossEntropyLoss", ignore_index=-1)],
                              backbone_out_channels=48, context_channels=256, conditions=CONDITIONS, num_classes=(5, 7, 4),
                              backbone_mode=backbone_mode))
    model.load_state_dict(seeded_state(model.state_dict()), strict=True)
    return model.cuda()


def _ppt_input(cloud, cond, segment_classes=None, cut=None):
    d = dict(feat=cloud["feat"].clone(), grid_coord=cloud["gc"], offset=cloud["offset"], coord=cloud["gc"].float() * 0.02, condition=[cond])
    if segment_classes:
        d["segment"] = torch.randint(0, segment_classes, (cloud["feat"].shape[0],), generator=torch.Generator().manual_seed(4)).cuda()
    if cut is not None:
        d["backward_cut"] = cut
    return d


def test_one_modulation_launch_each_way_two_under_a_cut(cloud, monkeypatch):
    from scenesplat_amd.pointcept_api.ptv3 import backward_in_two
    model = _ppt(backbone_mode=True).train()
    cnt = _Count(monkeypatch)
    torch.manual_seed(77)
    y = model(_ppt_input(cloud, "B"))
    (y * cloud["cot"]).sum().backward()
    assert (cnt.fwd, cnt.bwd) == (1, 1)
    cut = []
    torch.manual_seed(77)
    y = model(_ppt_input(cloud, "B", cut=cut))
    backward_in_two([y], [cloud["cot"]], cut)
    assert (cnt.fwd, cnt.bwd) == (3, 3)
    # non-adaptive: no modulation launch at all
    from scenesplat_amd.pointcept_api import MODELS
    sel = MODELS.build(backbone_cfg(adaptive=False)).cuda().train()
    y, _ = run_backbone(sel, cloud, "A")
    (y * cloud["cot"]).sum().backward()
    assert (cnt.fwd, cnt.bwd) == (3, 3)


def test_split_backward_gives_the_plain_backward_gradients(cloud):
    from scenesplat_amd.pointcept_api.ptv3 import backward_in_two
    model = _ppt(backbone_mode=True).train()
    init = {k: v.clone() for k, v in model.state_dict().items()}

    def run(split):
        model.load_state_dict(init)
        model.zero_grad(set_to_none=True)
        cut = [] if split else None
        torch.manual_seed(77)
        y = model(_ppt_input(cloud, "C", cut=cut))
        if split:
            assert len(cut) == 2
            backward_in_two([y], [cloud["cot"]], cut)
        else:
            (y * cloud["cot"]).sum().backward()
        return _grads(model)
    g1, g2, got = run(False), run(False), run(True)
    assert got["embedding_table.weight"] is not None and bool(got["embedding_table.weight"][2].any())
    _compare_grads_as_repeats_allow((g1, g2), got, {k: k for k in g1}, "split backward")


def test_autocast_backward_with_grouped_stage_reductions_matches_the_ungrouped_one(cloud):
    """Under bf16 autocast the LayerNorm seams leave the partial sums of dgamma_eff / dbeta_eff to their stage's grouped reduction,
    which must have run before the modulation backward reads them.  With grouping switched off every seam reduces on its own: the
    same fp32 partials (a few hundred per channel at most) summed in another order, so the gradients agree to ~1e-6 relative;
    1e-4 of the norm leaves room for nothing but that (a gradient read before its reduction is garbage or zero)."""
    from scenesplat_amd import functional as SF
    model = _ppt(backbone_mode=True).train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    names = [k for k, _ in model.named_parameters() if ".modulation.1." in k or k == "embedding_table.weight" or ".norm." in k]
    got = {}
    old = SF.WGRAD_GROUP_MAX_ROWS
    try:
        for grouped in (True, False):
            SF.WGRAD_GROUP_MAX_ROWS = old if grouped else 0
            model.load_state_dict(init); model.zero_grad(set_to_none=True)
            torch.manual_seed(77)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = model(_ppt_input(cloud, "B"))
            (y.float() * cloud["cot"]).sum().backward()
            got[grouped] = _grads(model)
    finally:
        SF.WGRAD_GROUP_MAX_ROWS = old
    assert cloud["feat"].shape[0] >= SF.LINEAR_WGRAD_MIN_ROWS        # (the finest level does open a stage)
    checked = 0
    for k in names:
        a, b = got[True][k], got[False][k]
        if b is None:
            assert a is None or not bool(a.any()), k
            continue
        assert a is not None and bool(torch.isfinite(a).all()), k
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12, (k, float((a - b).norm() / b.norm()))
        checked += 1
    assert checked > 40


# ---- 12. PPT-v1m2 end to end ---------------------------------------------------------------------------------------------------
def test_ppt_v1m2_end_to_end(cloud):
    from scenesplat_amd.pointcept_api import Point
    model = _ppt().train()
    out = model(_ppt_input(cloud, "B", segment_classes=7))
    assert set(out) == {"loss"} and bool(torch.isfinite(out["loss"]))
    out["loss"].backward()
    ge = model.embedding_table.weight.grad
    assert bool(ge[1].any()) and not bool(ge[0].any()) and not bool(ge[2].any())
    assert model.seg_heads[1].weight.grad is not None and bool(model.seg_heads[1].weight.grad.any())
    for i in (0, 2):
        assert model.seg_heads[i].weight.grad is None and model.seg_heads[i].bias.grad is None
    model.eval()

    def fwd(m, d):
        torch.manual_seed(0)             # (the pooling stages shuffle their curve orders in every forward)
        return m(d)
    with torch.no_grad():
        d = _ppt_input(cloud, "B", segment_classes=7)
        out = fwd(model, d)
        assert set(out) == {"loss", "seg_logits"} and out["seg_logits"].shape == (cloud["feat"].shape[0], 7)
        out2 = fwd(model, _ppt_input(cloud, "B"))
        assert set(out2) == {"seg_logits"} and torch.equal(out2["seg_logits"], out["seg_logits"])
        # the wrapper's arithmetic, restated: embedding lookup -> backbone -> the condition's head (-> criteria)
        d3 = _ppt_input(cloud, "B")
        d3["context"] = F.embedding(torch.tensor([1], device="cuda"), model.embedding_table.weight)
        feat = fwd(model.backbone, Point(d3))["feat"]
        assert torch.equal(out2["seg_logits"], F.linear(feat, model.seg_heads[1].weight, model.seg_heads[1].bias))
        assert abs(float(out["loss"]) - float(F.cross_entropy(out["seg_logits"].float(), d["segment"], ignore_index=-1))) < 1e-4 * max(1.0, abs(float(out["loss"])))
        with pytest.raises(AssertionError):
            model(_ppt_input(cloud, "ScanNet"))
    bb = _ppt(backbone_mode=True).eval()
    with torch.no_grad():
        f = bb(_ppt_input(cloud, "A"))
    assert torch.is_tensor(f) and f.shape == (cloud["feat"].shape[0], 48)


# ---- 13. steady-state replay with alternating conditions -----------------------------------------------------------------------
def test_trainer_steady_state_replays_per_condition_and_matches_the_eager_trainer():
    """After test_hip_round2.py::test_trainer_steady_state_option_replays_and_matches_the_eager_trainer: six steps alternating two
    conditions; each condition is captured under its own steady_key and the weights end where the eager trainer's do (bf16 noise apart,
    that test's bar)."""
    import tempfile
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import RUNTIME, engine
    from scenesplat_amd.synthetic import room_chunk
    small = dict(TINY, enc_depths=(1, 1, 1), enc_channels=(16, 32, 48), enc_num_head=(1, 2, 3), dec_depths=(1, 1))

    def loader(k=6):
        base = room_chunk(n_side=40, seed=3, lang_dim=0, num_classes=4)
        g = torch.Generator().manual_seed(0)
        out = []
        for i in range(k):
            d = {kk: (v.clone() if torch.is_tensor(v) else v) for kk, v in base.items()}
            d["feat"] = torch.randn(d["feat"].shape, generator=g)
            d["condition"] = [("A", "B")[i % 2]]
            out.append(d)
        return out

    def cfg(tmp, steady):
        bb = dict(type="PT-v3m1", **small, drop_path=0.0, shuffle_orders=False, pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=True,
                  pdnorm_conditions=("A", "B"))
        return dict(model=dict(type="PPT-v1m2", backbone=bb, criteria=[dict(type="CrossEntropyLoss", ignore_index=-1)],
                               backbone_out_channels=48, conditions=("A", "B"), num_classes=(4, 4)),
                    device="cuda", eval_epoch=1, save_path=tmp, enable_amp=True, clip_grad=1.0, steady_state=steady,
                    optimizer=dict(type="AdamW", lr=2e-3, weight_decay=0.05),
                    scheduler=dict(type="OneCycleLR", max_lr=2e-3, pct_start=0.3, anneal_strategy="cos", div_factor=10.0, final_div_factor=100.0),
                    hooks=[])
    old = dict(RUNTIME)
    try:
        RUNTIME.update(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA)
        with tempfile.TemporaryDirectory() as tmp:
            weights = {}
            for steady in (False, True):
                torch.manual_seed(21)
                tr = engine.Trainer(cfg(tmp, steady), train_loader=loader())
                tr.train()
                weights[steady] = torch.cat([p.detach().float().flatten() for p in tr.model.parameters()])
                if steady:
                    assert tr._steady is not None and tr._steady.refused is None, tr._steady.refused
                    # per condition: warm-up, checked step, then the graph
                    assert tr._steady.replays == 2 and tr._steady.eager_steps == 4, (tr._steady.replays, tr._steady.eager_steps)
                    assert len(tr._steady._graphs) == 2
    finally:
        RUNTIME.clear(); RUNTIME.update(old)
    rel = float((weights[True] - weights[False]).norm() / weights[False].norm())
    print("steady vs eager trainer: relative weight difference %.3e" % rel)
    assert rel < 2e-2, rel
