"""csrc/norm.hip (and the two grouped helpers) against float64 on the CPU at the shapes where the kernels change path.

Every reference is the plain torch composition of the same operation in float64 on the CPU, applied to the same rounded
inputs (a bf16 input enters the reference as the bf16 value it is; cotangents of bf16 outputs are bf16-representable, so
autograd's cast of the incoming gradient rounds nothing).

Tolerances.  The element-wise ones are those of the three functional tests in tests/test_hip_ops.py, by dtype.  Where a
bound is "derived" (sections A, C, D: every BatchNorm quantity and every affine gradient), the same operation also runs
through torch's own fp32 kernels on the device (F.batch_norm / F.layer_norm, forward and backward) on the same input;
its error against the fp64 reference is measured, and the bound for the HIP path is the LARGER of the existing tolerance
and 8x that error.  The factor 8 covers a different, equally valid fp32 summation order over at most 1024 partials.  The
yardstick is torch's kernel, never the kernel under test.  The torch errors measured on an MI355X are written next to
the constants below; set SS_NORM_EDGES_REPORT=1 to print every figure of a run.
"""
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("SS_NORM_EDGES_REPORT", "0") == "1"
YARD = 8.0          # bound = max(existing tolerance, YARD x error of torch's fp32 device kernel against fp64)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# ---- the existing tolerances (tests/test_hip_ops.py), by dtype of the tensor that carries the rounding -----------------------
# BatchNorm (test_fused_batchnorm_gelu_against_torch): y allclose(atol = rtol = 2e-5 | 2e-2); dx allclose(atol = 2 x that, rtol =
# 1e-3 | 5e-2); dweight / dbias relative norm rt = 2e-4 | 8e-3; running statistics allclose(atol = 1e-5, rtol = 1e-4).
# torch's fp32 device kernels against fp64, measured on an MI355X for section A (fp32 input, training; max over n, presets, GELU):
#     column means (r)      y         dx        dweight   dbias     running_mean  running_var     HIP path: y       dx
#     0                     7.4e-7    1.1e-6    1.7e-7    1.4e-7    9.6e-8        1.0e-7                    1.6e-6  1.8e-6
#     30  (n >= 9)          9.8e-6    4.8e-6    5.6e-6    4.9e-6    1.9e-6        1.1e-7                    2.2e-6  1.9e-6
#     100 (n >= 9)          3.1e-5    1.3e-5    1.8e-5    1.4e-5    7.7e-6        1.4e-7                    5.5e-6  8.6e-6
#     n = 2, r = 30 | 100   1.1e-5 | 1.4e-4   3.2e-5 | 8.3e-4 (two rows 0.1 apart: fp32 cannot hold the mean; the HIP path measures the same)
# so the bound 8 x torch is 2.5e-4 for y (1.1e-3 at n = 2), 1.0e-4 for dx (6.6e-3 at n = 2), 1.4e-4 relative for dweight / dbias and
# 6.2e-5 for running_mean at r = 100; at r = 0 the existing tolerances below are the larger ones and hold.  Eval mode: y 3.3e-5 at
# |y| = 200 (inside rtol), dx 7.4e-7.  bf16 input: torch (fp32 math) <= 7.0e-5, the bf16 tolerances hold (HIP 1.6e-2 = half a bf16 ulp).
# Constant column: torch y 8.1e-6, dx 9.9e-4; HIP y 1.2e-6, dx 8.0e-6.  Torch-ops branch (n = 2111, r = 100): torch y 3.4e-5, HIP 3.3e-6.
BN_TOL = {F32: dict(y=(2e-5, 2e-5), dx=(4e-5, 1e-3), rt=2e-4), BF16: dict(y=(2e-2, 2e-2), dx=(4e-2, 5e-2), rt=8e-3)}
BN_RUNNING = (1e-5, 1e-4)
# LayerNorm seams (test_fused_add_layernorm_against_torch / test_fused_ln_add_ln_against_torch)
LN_XOUT = (1e-6, 1e-5)                       # fp32 sum x + s*y
LN_H = {F32: (1e-5, 1e-5), BF16: (2e-2, 2e-2)}
LN_XCOPY = (1e-2, 8e-3)                      # bf16 rounding of the fused sum
LN_GIN = {F32: (2e-5, 1e-2), BF16: (3e-2, 1e-2)}
LN_PTOL = {F32: 1e-3, BF16: 8e-3}            # relative norm of dgamma / dbeta, by dtype of h
# torch's fp32 F.layer_norm backward on the device against fp64, measured on an MI355X over every shape of sections C, D and E, relative
# norm: dgamma <= 1.9e-7, dbeta <= 2.4e-7 (HIP path: <= 1.9e-7) -> 8 x = 1.9e-6 < LN_PTOL, so LN_PTOL is the bound that holds.  BatchNorm
# at those shapes: torch dweight 1.6e-7, dbias 1.2e-7 (HIP 4.0e-7, 2.0e-7); y 1.2e-6, dx 6.3e-6 (HIP 3.4e-6, 5.9e-6): BN_TOL holds.


def _rep(*a):
    if REPORT:
        print(*a, flush=True)


def _close(name, got, ref, atol, rtol, yard=None, fails=None):
    """|got - ref| <= max(atol + rtol |ref|, YARD * max|yard - ref|), element-wise."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    ye = 0.0
    if yard is not None:
        ye = (yard.detach().double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
        bound = torch.clamp(bound, min=YARD * ye)
    worst = (err - bound).max().item() if ref.numel() else -1.0
    _rep(f"    {name}: max err {err.max().item() if ref.numel() else 0:.3e}  torch-fp32 err {ye:.3e}  (atol {atol:g} rtol {rtol:g})")
    ok = bool(torch.isfinite(got).all()) and worst <= 0
    if not ok and fails is not None:
        fails.append(f"{name}: max err {err.max().item():.3e} (torch fp32 {ye:.3e}, atol {atol:g}, rtol {rtol:g})")
    return ok


def _norm_close(name, got, ref, tol, yard=None, fails=None):
    """||got - ref|| <= max(tol, YARD * ||yard - ref|| / ||ref||) * ||ref||."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    rn = ref.norm().item()
    err = (got - ref).norm().item()
    ye = (yard.detach().double().cpu() - ref).norm().item() if yard is not None else 0.0
    rel, yrel = (err / rn, ye / rn) if rn > 0 else (err, ye)
    _rep(f"    {name}: rel norm err {rel:.3e}  torch-fp32 {yrel:.3e}  (tol {tol:g})")
    ok = bool(torch.isfinite(got).all()) and err <= max(tol, YARD * yrel) * rn
    if not ok and fails is not None:
        fails.append(f"{name}: rel norm err {rel:.3e} (torch fp32 {yrel:.3e}, tol {tol:g})")
    return ok


def _none_or_zero(g):
    return g is None or not bool(g.ne(0).any())


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


# =====================================================================================================================
# BatchNorm: plain torch composition, used in fp64 on the CPU (the reference) and in fp32 on the device (the yardstick)
# =====================================================================================================================
def _torch_bn(x, w, b, rm, rv, nbt, training, momentum, eps, act, cot, dtype, device):
    """F.batch_norm (+ F.gelu) forward and backward -> dict of y, dx, dw, db, rm, rv, nbt (buffers updated as nn.BatchNorm1d does)"""
    x, w, b = (t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in (x, w, b))
    rm, rv = rm.detach().to(device=device, dtype=dtype).clone(), rv.detach().to(device=device, dtype=dtype).clone()
    nbt = int(nbt)
    factor = 0.0
    if training:
        nbt += 1
        factor = 1.0 / nbt if momentum is None else momentum
    y = F.batch_norm(x, rm, rv, w, b, training, factor, eps)
    if act:
        y = F.gelu(y)
    y.backward(cot.to(device=device, dtype=dtype))
    return dict(y=y, dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv, nbt=nbt)


def _hip_bn(x, w, b, rm, rv, nbt, training, momentum, eps, act, cot, buffer_dtype=F32):
    from scenesplat_amd import functional as SF
    C = x.shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
        bn.running_mean = rm.clone().to(buffer_dtype); bn.running_var = rv.clone().to(buffer_dtype)
        bn.num_batches_tracked.fill_(int(nbt))
    bn = bn.cuda().train(training)
    xg = x.cuda().requires_grad_(True)
    y = SF.batch_norm_act(xg, bn, act)
    assert y.dtype == x.dtype and y.shape == x.shape
    y.backward(cot.to(y.dtype).cuda())
    return dict(y=y, dx=xg.grad, dw=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var,
                nbt=int(bn.num_batches_tracked), beta=b)


def _bn_case(tag, x, rm, rv, training, act, momentum=0.01, nbt=3, buffer_dtype=F32, fails=None):
    """One BatchNorm run against fp64 with the derived bound; x carries the dtype."""
    n, C = x.shape
    g = _gen(n, C, 77)
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    cot = torch.randn(n, C, generator=g).to(x.dtype).float()
    eps = 1e-3
    ref = _torch_bn(x, w, b, rm, rv, nbt, training, momentum, eps, act, cot, F64, "cpu")
    yard = _torch_bn(x, w, b, rm, rv, nbt, training, momentum, eps, act, cot, F32, "cuda")
    got = _hip_bn(x, w, b, rm, rv, nbt, training, momentum, eps, act, cot, buffer_dtype)
    _rep(f"  {tag}")
    tol = BN_TOL[x.dtype]
    fl = [] if fails is None else fails
    pre = len(fl)
    _close(f"{tag} y", got["y"], ref["y"], *tol["y"], yard=yard["y"], fails=fl)
    _close(f"{tag} dx", got["dx"], ref["dx"], *tol["dx"], yard=yard["dx"], fails=fl)
    _norm_close(f"{tag} dweight", got["dw"], ref["dw"], tol["rt"], yard=yard["dw"], fails=fl)
    _norm_close(f"{tag} dbias", got["db"], ref["db"], tol["rt"], yard=yard["db"], fails=fl)
    _close(f"{tag} running_mean", got["rm"], ref["rm"], *BN_RUNNING, yard=yard["rm"], fails=fl)
    _close(f"{tag} running_var", got["rv"], ref["rv"], *BN_RUNNING, yard=yard["rv"], fails=fl)
    if got["nbt"] != ref["nbt"]:
        fl.append(f"{tag} num_batches_tracked {got['nbt']} != {ref['nbt']}")
    if fails is None:
        assert not fl, "\n".join(fl)
    return got, ref, len(fl) == pre


# ---- A. conditioning ------------------------------------------------------------------------------------------------
# The same cases on the parent commit's kernels (shift = running_mean), one run on an MI355X, fp32 input, training, n = 2111, max |y - fp64|:
#     r = 30:  3.7e-4 (running_mean = 0)   2.2e-3 (= -batch mean)   1.5e-6 (= batch mean)       bound 6.7e-5
#     r = 100: 4.5e-3 (running_mean = 0)   3.7e-2 (= -batch mean)   3.1e-6 (= batch mean)       bound 2.4e-4
# (running_var off by 2.2e-4, dx by 4.8e-2 at r = 100; at n = 2: y 5.4e-2, dx 1.6).  With the shift taken from row 0 of the batch every
# preset measures the same: 2.0e-6 (r = 30), 3.2e-6 (r = 100).
A_SIGNS = (1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 0.0)
_A_INPUT = {}


def _a_input(n, r):
    """column c = m_c + randn, m = r * A_SIGNS; computed once per (n, r) and left unchanged"""
    if (n, r) not in _A_INPUT:
        g = _gen(n, r, 1)
        _A_INPUT[(n, r)] = torch.tensor(A_SIGNS) * r + torch.randn(n, 8, generator=g)
    return _A_INPUT[(n, r)]


@pytest.mark.parametrize("preset", ["zeros", "batch_mean", "minus_batch_mean"])
@pytest.mark.parametrize("r", [0, 30, 100])
@pytest.mark.parametrize("n", [2, 9, 2111, 40001])
def test_batchnorm_conditioning_against_fp64(n, r, preset):
    """Training and eval, fp32 and bf16 input, with and without GELU: y, dx, dweight, dbias, the updated running statistics and
    the batch counter against fp64 F.batch_norm, whatever the distance between the running mean and the batch mean."""
    fails = []
    for dtype, training, act in itertools.product((F32, BF16), (True, False), (False, True)):
        x = _a_input(n, r).to(dtype)
        bm = x.double().mean(0)
        rm = {"zeros": torch.zeros(8), "batch_mean": bm.float(), "minus_batch_mean": -bm.float()}[preset]
        rv = 1 + 0.2 * torch.rand(8, generator=_gen(n, r, 2))
        tag = f"n={n} r={r} rm={preset} {str(dtype)[6:]} {'train' if training else 'eval'}{' gelu' if act else ''}:"
        _bn_case(tag, x, rm, rv, training, act, fails=fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("act", [False, True])
def test_batchnorm_constant_column(dtype, act):
    """A column whose every entry is 3.7: y there is act(beta), running_var moves toward 0.  Kept apart from the cases above:
    rstd = eps^-1/2 = 31.6 amplifies any error of the mean in this column."""
    n, C, col = 2111, 8, 5
    x = torch.randn(n, C, generator=_gen(n, 3)).to(dtype)
    x[:, col] = 3.7
    rm, rv = torch.zeros(C), 1 + 0.2 * torch.rand(C, generator=_gen(n, 4))
    got, ref, _ = _bn_case(f"constant column {str(dtype)[6:]}{' gelu' if act else ''}:", x, rm, rv, True, act)
    beta = got["beta"][col].double()
    want = F.gelu(beta) if act else beta
    ycol = got["y"][:, col].double().cpu()
    assert bool((ycol == ycol[0]).all())                                   # one value down the whole column
    assert abs(ycol[0].item() - want.item()) <= BN_TOL[dtype]["y"][0] + BN_TOL[dtype]["y"][1] * abs(want.item())
    if not act and dtype == F32:
        assert ycol[0].item() == beta.float().item()                       # (x - mean) is exactly 0: y is beta itself
    assert abs(got["rv"][col].item() - 0.99 * rv[col].item()) <= 1e-6 * rv[col].item()
    assert abs(got["rm"][col].item() - 0.01 * x[0, col].float().item()) <= 1e-6


@pytest.mark.parametrize("branch", ["momentum_none", "fp64_buffers"])
@pytest.mark.parametrize("preset", ["zeros", "minus_batch_mean"])
def test_batchnorm_torch_ops_branch_is_conditioned_too(branch, preset):
    """momentum = None (cumulative average) or non-fp32 buffers take the torch-ops branch of _BatchNormAct.forward: same bound."""
    n, r = 2111, 100
    x = _a_input(n, r)
    bm = x.double().mean(0)
    rm = torch.zeros(8) if preset == "zeros" else -bm.float()
    rv = 1 + 0.2 * torch.rand(8, generator=_gen(n, r, 2))
    momentum, bdt = (None, F32) if branch == "momentum_none" else (0.01, F64)
    for act in (False, True):
        _bn_case(f"{branch} rm={preset}{' gelu' if act else ''}:", x, rm, rv, True, act, momentum=momentum, nbt=3, buffer_dtype=bdt)


# =====================================================================================================================
# The three LayerNorm entry points: torch compositions (fp64 CPU reference / fp32 device yardstick) and the HIP path
# =====================================================================================================================
def _leaf(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype).requires_grad_(True)


def _torch_add_ln(x, y, rs, gam, bet, cots, dtype, device, eps=1e-5):
    """cots = (cx, ch, cc), each a tensor or None (output not consumed); the bf16 copy is straight-through for the gradient"""
    x, y, gam, bet = (_leaf(t, dtype, device) for t in (x, y, gam, bet))
    v = x + (rs.to(device=device, dtype=dtype)[:, None] * y if rs is not None else y)
    h = F.layer_norm(v, (x.shape[1],), gam, bet, eps) if gam is not None else None
    outs = [(o, c) for o, c in zip((v, h, v), cots) if c is not None and o is not None]
    torch.autograd.backward([o for o, _ in outs], [c.to(device=device, dtype=dtype) for _, c in outs])
    return dict(xout=v, h=h, dx=x.grad, dy=y.grad, dg=None if gam is None else gam.grad, db=None if bet is None else bet.grad)


def _hip_add_ln(x, y, rs, gam, bet, cots, h_dtype, eps=1e-5):
    from scenesplat_amd import functional as SF
    xg, yg, gg, bg = (None if t is None else t.cuda().requires_grad_(True) for t in (x, y, gam, bet))
    xo, h, xc = SF.add_layer_norm(xg, yg, None if rs is None else rs.cuda(), gg, bg, eps, True, h_dtype)
    assert xo.dtype == F32 and xc.dtype == BF16 and (h is None) == (gam is None) and (h is None or h.dtype == h_dtype)
    outs = [(o, c) for o, c in zip((xo, h, xc), cots) if c is not None and o is not None]
    torch.autograd.backward([o for o, _ in outs], [c.to(o.dtype).cuda() for o, c in outs])
    return dict(xout=xo, h=h, xcopy=xc, dx=xg.grad, dy=yg.grad, dg=None if gg is None else gg.grad, db=None if bg is None else bg.grad)


def _check_add_ln(tag, got, ref, yard, xdt, ydt, hdt, fails):
    _rep(f"  {tag}")
    _close(f"{tag} xout", got["xout"], ref["xout"], *LN_XOUT, fails=fails)
    _close(f"{tag} xcopy", got["xcopy"], ref["xout"], *LN_XCOPY, fails=fails)
    if ref["h"] is not None:
        _close(f"{tag} h", got["h"], ref["h"], *LN_H[hdt], fails=fails)
    lo = BF16 if BF16 in (xdt, ydt, hdt) else F32
    for k, dt in (("dx", xdt), ("dy", ydt)):
        if ref[k] is None:
            if not _none_or_zero(got[k]):
                fails.append(f"{tag} {k}: gradient without a consumer")
        else:
            _close(f"{tag} {k}", got[k], ref[k], *LN_GIN[BF16 if dt == BF16 else lo], fails=fails)
    for k in ("dg", "db"):
        if ref[k] is None:
            if not _none_or_zero(got[k]):
                fails.append(f"{tag} {k}: gradient without a consumer")
        else:
            _norm_close(f"{tag} {k}", got[k], ref[k], LN_PTOL[hdt], yard=yard[k], fails=fails)


def _add_ln_case(tag, n, C, xdt, ydt, hdt, fails, rowscale=True, affine=True, consume=(True, True, True), seed=0):
    g = _gen(n, C, seed, 11)
    x, y = torch.randn(n, C, generator=g).to(xdt), (torch.randn(n, C, generator=g) * 1.5 + 0.25).to(ydt)
    rs = None
    if rowscale:
        rs = (torch.rand(n, generator=g) < 0.7).float() / 0.7
        rs[0] = 0.0                                                        # at least one dropped row, at least one kept
        rs[n - 1] = 1.0 / 0.7
    gam, bet = (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)) if affine else (None, None)
    cx, ch, cc = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g).to(hdt).float(), torch.randn(n, C, generator=g).to(BF16).float()
    cots = tuple(c if use else None for c, use in zip((cx, ch, cc), consume))
    ref = _torch_add_ln(x, y, rs, gam, bet, cots, F64, "cpu")
    yard = _torch_add_ln(x, y, rs, gam, bet, cots, F32, "cuda")
    got = _hip_add_ln(x, y, rs, gam, bet, cots, hdt)
    _check_add_ln(tag, got, ref, yard, xdt, ydt, hdt, fails)
    if rs is not None and got["dy"] is not None:
        dropped = got["dy"].float().cpu()[rs == 0]
        if bool(dropped.ne(0).any()):
            fails.append(f"{tag} dy: rows with rowscale 0 must get an exactly zero gradient")


def _torch_ln(x, gam, bet, cot, dtype, device, eps=1e-5):
    x, gam, bet = (_leaf(t, dtype, device) for t in (x, gam, bet))
    h = F.layer_norm(x, (x.shape[1],), gam, bet, eps)
    h.backward(cot.to(device=device, dtype=dtype))
    return dict(h=h, dx=x.grad, dg=gam.grad, db=bet.grad)


def _ln_case(tag, n, C, dt, fails):
    from scenesplat_amd import functional as SF
    g = _gen(n, C, 12)
    x = (torch.randn(n, C, generator=g) * 2 + 0.5).to(dt)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    cot = torch.randn(n, C, generator=g).to(dt).float()
    ref, yard = _torch_ln(x, gam, bet, cot, F64, "cpu"), _torch_ln(x, gam, bet, cot, F32, "cuda")
    xg, gg, bg = x.cuda().requires_grad_(True), gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    h = SF.layer_norm(xg, gg, bg, 1e-5)
    assert h.dtype == dt
    h.backward(cot.to(dt).cuda())
    _rep(f"  {tag}")
    _close(f"{tag} h", h, ref["h"], *LN_H[dt], fails=fails)
    _close(f"{tag} dx", xg.grad, ref["dx"], LN_GIN[dt][0], 2e-2, fails=fails)            # rtol of the plain-LN part of the existing test
    _norm_close(f"{tag} dg", gg.grad, ref["dg"], LN_PTOL[dt], yard=yard["dg"], fails=fails)
    _norm_close(f"{tag} db", bg.grad, ref["db"], LN_PTOL[dt], yard=yard["db"], fails=fails)


def _torch_ln2(x, t, p, cots, dtype, device, eps=1e-5):
    x, t = _leaf(x, dtype, device), _leaf(t, dtype, device)
    p = [_leaf(q, dtype, device) for q in p]
    C = x.shape[1]
    xo = x + F.layer_norm(t, (C,), p[0], p[1], eps)
    h = F.layer_norm(xo, (C,), p[2], p[3], eps)
    outs = [(o, c) for o, c in zip((xo, h), cots) if c is not None]
    torch.autograd.backward([o for o, _ in outs], [c.to(device=device, dtype=dtype) for _, c in outs])
    return dict(xout=xo, h=h, dx=x.grad, dt=t.grad, p=[q.grad for q in p])


def _ln2_case(tag, n, C, xdt, tdt, hdt, fails, consume=(True, True)):
    """existing metric of test_fused_ln_add_ln_against_torch (max err / max(1, max|ref|) < 2e-2 on the bf16-carried tensors, 2e-4
    elsewhere) for outputs and input gradients; the four affine gradients as relative norms (LN_PTOL or 8x torch's fp32 error)"""
    from scenesplat_amd import functional as SF
    g = _gen(n, C, 13)
    x, t = torch.randn(n, C, generator=g).to(xdt), (torch.randn(n, C, generator=g) * 2 + 0.5).to(tdt)
    p = [torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.5 + 1.0,
         torch.randn(C, generator=g) * 0.3]
    cx, ch = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g).to(hdt).float()
    cots = tuple(c if use else None for c, use in zip((cx, ch), consume))
    ref, yard = _torch_ln2(x, t, p, cots, F64, "cpu"), _torch_ln2(x, t, p, cots, F32, "cuda")
    ln0, ln1 = torch.nn.LayerNorm(C, eps=1e-5), torch.nn.LayerNorm(C, eps=1e-5)
    with torch.no_grad():
        ln0.weight.copy_(p[0]); ln0.bias.copy_(p[1]); ln1.weight.copy_(p[2]); ln1.bias.copy_(p[3])
    ln0, ln1 = ln0.cuda(), ln1.cuda()
    xg, tg = x.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    xo, h = SF.ln_add_ln(xg, tg, ln0, ln1, hdt)
    assert xo.dtype == F32 and h.dtype == hdt
    outs = [(o, c) for o, c in zip((xo, h), cots) if c is not None]
    torch.autograd.backward([o for o, _ in outs], [c.to(o.dtype).cuda() for o, c in outs])
    _rep(f"  {tag}")
    lo = BF16 in (xdt, tdt, hdt)
    for name, a, b, low in (("xout", xo, ref["xout"], False), ("h", h, ref["h"], lo), ("dx", xg.grad, ref["dx"], lo), ("dt", tg.grad, ref["dt"], lo)):
        b = b.detach().double()
        err = (a.detach().double().cpu() - b).abs().max().item() / max(1.0, b.abs().max().item())
        _rep(f"    {tag} {name}: scaled max err {err:.3e}")
        if not err < (2e-2 if low else 2e-4):
            fails.append(f"{tag} {name}: scaled max err {err:.3e}")
    gots = [ln0.weight.grad, ln0.bias.grad, ln1.weight.grad, ln1.bias.grad]
    for i, name in enumerate(("dgamma0", "dbeta0", "dgamma1", "dbeta1")):
        if ref["p"][i] is None:
            if not _none_or_zero(gots[i]):
                fails.append(f"{tag} {name}: gradient without a consumer")
        else:
            _norm_close(f"{tag} {name}", gots[i], ref["p"][i], LN_PTOL[hdt], yard=yard["p"][i], fails=fails)


def _bn_shape_case(tag, n, C, dt, training, fails):
    g = _gen(n, C, 14)
    x = (torch.randn(n, C, generator=g) * 1.7 + 0.3).to(dt)
    rm, rv = 0.2 * torch.randn(C, generator=g), 1 + 0.2 * torch.rand(C, generator=g)
    _bn_case(tag, x, rm, rv, training, True, fails=fails)


# ---- C. row regimes: 1 .. 9 rows (partial workgroups, idle waves), 2 rows per wave below 32768, 8 from 32768, ragged above -------
ROWS = [1, 3, 4, 5, 8, 9, 32767, 32768, 40001]


@pytest.mark.parametrize("n", ROWS)
def test_layernorm_seams_row_regimes(n):
    fails = []
    for C, xdt, ydt, hdt in ((32, F32, F32, F32), (260, BF16, BF16, BF16)):
        d = f"n={n} C={C} {str(xdt)[6:]}"
        _add_ln_case(f"add_layer_norm {d}:", n, C, xdt, ydt, hdt, fails, rowscale=n > 1)
        _ln_case(f"layer_norm {d}:", n, C, xdt, fails)
        _ln2_case(f"ln_add_ln {d}:", n, C, xdt, ydt, hdt, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", ROWS)
def test_batchnorm_row_regimes(n):
    fails = []
    for training in (True, False):
        if training and n == 1:
            continue                              # nn.BatchNorm1d itself refuses one value per channel in training mode
        _bn_shape_case(f"batch_norm_act n={n} C=32 {'train' if training else 'eval'}:", n, 32, F32, training, fails)
    assert not fails, "\n".join(fails)


# ---- D. channel edges: the smallest width, both sides of every IT = ceil(C / 256) boundary, and the rejected widths ----------------
@pytest.mark.parametrize("C", [4, 8, 252, 256, 260, 512, 516, 1020, 1024])
def test_norm_channel_edges(C):
    n, fails = 37, []
    _add_ln_case(f"add_layer_norm C={C}:", n, C, F32, F32, F32, fails)
    _ln_case(f"layer_norm C={C}:", n, C, F32, fails)
    _ln2_case(f"ln_add_ln C={C}:", n, C, F32, F32, F32, fails)
    for training in (True, False):
        _bn_shape_case(f"batch_norm_act C={C} {'train' if training else 'eval'}:", n, C, F32, training, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", [6, 1028])
def test_norm_rejects_bad_widths_from_every_entry_point(C):
    """C % 4 != 0 and C > 1024 are refused on the host (SS_ERR_ARG -> NativeError), before any launch."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd._lib import NativeError
    n = 37
    x, y = torch.randn(n, C).cuda(), torch.randn(n, C).cuda()
    gam, bet = torch.ones(C).cuda().requires_grad_(True), torch.zeros(C).cuda().requires_grad_(True)
    with pytest.raises(NativeError, match="status 1"):
        SF.add_layer_norm(x, y, None, gam, bet, 1e-5, True, F32)
    with pytest.raises(NativeError, match="status 1"):
        SF.add_layer_norm(x, y, None, None, None, 1e-5, True, F32)
    with pytest.raises(NativeError, match="status 1"):
        SF.layer_norm(x, gam, bet, 1e-5)
    ln0, ln1 = torch.nn.LayerNorm(C).cuda(), torch.nn.LayerNorm(C).cuda()
    with pytest.raises(NativeError, match="status 1"):
        SF.ln_add_ln(x, y, ln0, ln1, F32)
    for training in (True, False):
        bn = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).cuda().train(training)
        with pytest.raises(NativeError, match="status 1"):
            SF.batch_norm_act(x, bn, True)
        assert not bool(bn.running_mean.ne(0).any()) and not bool(bn.running_var.ne(1).any()) and int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("C", [6, 1028])
def test_norm_bad_widths_leave_outputs_untouched(C):
    """The C-ABI entry points themselves: status SS_ERR_ARG, and output tensors prefilled with a sentinel stay as they were."""
    from scenesplat_amd import native as nv
    n, nb, SENT = 37, 5, -7.25
    p, st = nv._p, nv._stream()
    inp = lambda *s: torch.randn(*s, device="cuda")
    out = lambda *s: torch.full(s, SENT, device="cuda")
    x, y, gh, mean, rstd, stats, gam, bet = inp(n, C), inp(n, C), inp(n, C), inp(n), inp(n), inp(n, 4), inp(C), inp(C)
    cm, cr = inp(C), inp(C).abs() + 0.5
    outs = []

    def o(*s):
        outs.append(out(*s))
        return p(outs[-1])
    L, ERR = nv.lib(), 1
    assert L.ss_add_layernorm_fwd(p(x), 0, p(y), 0, None, p(gam), p(bet), 1e-5, o(n, C), 0, None, o(n, C), 0, o(n), o(n), n, C, st) == ERR
    assert L.ss_add_layernorm_bwd(p(gh), 0, None, 0, p(gh), 0, p(x), 0, p(mean), p(rstd), p(gam), None, o(n, C), 0, o(n, C), 0,
                                  o(nb, C), o(nb, C), n, C, nb, st) == ERR
    assert L.ss_ln_add_ln_fwd(p(x), 0, p(y), 0, p(gam), p(bet), 1e-5, p(gam), p(bet), 1e-5, o(n, C), o(n, C), 0, o(n, 4), n, C, st) == ERR
    assert L.ss_ln_add_ln_bwd(p(gh), p(gh), 0, p(x), p(y), 0, p(stats), p(gam), p(gam), o(n, C), 0, o(n, C), 0, o(4, nb, C), n, C, nb, st) == ERR
    assert L.ss_col_stats(p(x), 0, o(C), o(nb, C), o(nb, C), n, C, nb, st) == ERR
    assert L.ss_bn_act_fwd(p(x), 0, p(cm), p(cr), p(gam), p(bet), 1, o(n, C), 0, n, C, st) == ERR
    assert L.ss_bn_act_bwd_reduce(p(gh), 0, p(x), 0, p(cm), p(cr), p(gam), p(bet), 1, o(nb, C), o(nb, C), n, C, nb, st) == ERR
    assert L.ss_bn_act_bwd_apply(p(gh), 0, p(x), 0, p(cm), p(cr), p(gam), p(bet), 1, p(cm), p(cr), o(n, C), 0, n, C, st) == ERR
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENT).all())


# ---- E. gradient-presence combinations (set_materialize_grads(False): absent cotangents reach the kernels as NULL) -------------
SUBSETS3 = [s for s in itertools.product((False, True), repeat=3) if any(s)]        # (xout, h, xcopy)


@pytest.mark.parametrize("rowscale", [False, True])
@pytest.mark.parametrize("C", [48, 768])
def test_add_layernorm_every_subset_of_consumed_outputs(C, rowscale):
    n, fails = 1037, []
    for (xdt, ydt, hdt), sub in itertools.product(((F32, F32, F32), (F32, BF16, BF16)), SUBSETS3):
        names = "+".join(nm for nm, use in zip(("xout", "h", "xcopy"), sub) if use)
        _add_ln_case(f"add_layer_norm C={C} {str(hdt)[6:]} rowscale={rowscale} consume {names}:", n, C, xdt, ydt, hdt, fails,
                     rowscale=rowscale, consume=sub)
    for sub in ((True, False, False), (False, False, True), (True, False, True)):   # gamma = None: the pure add
        names = "+".join(nm for nm, use in zip(("xout", "h", "xcopy"), sub) if use)
        _add_ln_case(f"pure add C={C} rowscale={rowscale} consume {names}:", n, C, F32, BF16, F32, fails, rowscale=rowscale,
                     affine=False, consume=sub)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", [48, 768])
def test_ln_add_ln_every_subset_of_consumed_outputs(C):
    n, fails = 1037, []
    for (xdt, tdt, hdt), sub in itertools.product(((F32, F32, F32), (F32, BF16, BF16)), ((True, False), (False, True), (True, True))):
        names = "+".join(nm for nm, use in zip(("xout", "h"), sub) if use)
        _ln2_case(f"ln_add_ln C={C} {str(hdt)[6:]} consume {names}:", n, C, xdt, tdt, hdt, fails, consume=sub)
    assert not fails, "\n".join(fails)


# ---- F. native.group_partial_sums ---------------------------------------------------------------------------------------------
def test_group_partial_sums_against_fp64():
    """Every (K, nb, C) of the grid in ONE launch: 32-stride main loop (nb > 24), 8-stride tail, fewer rows than row groups (nb < 8),
    a partial last workgroup (K * C = 8, 144).  Bound: a destination is a sum of at most 1024 fp32 terms, accumulated in chains of
    at most 32 terms and an 11-term tree, so |err| <= 43 * 2^-24 * sum|terms| = 2.6e-6 * sum|terms| in the worst case and about
    sqrt(43) * 2^-24 = 4e-7 for rounding errors of random sign: 1e-6 relative to sum|terms| element-wise, and 1e-6 relative
    in norm over a destination."""
    from scenesplat_amd import native as nv
    g = _gen(6)
    PAD, SENT = 8, -12345.0
    probs = list(itertools.product((2, 4), (1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 1024), (4, 36, 260, 1024)))
    parts = [torch.randn(K, nb, C, generator=g) for K, nb, C in probs]
    offs, total = [], PAD
    for K, nb, C in probs:
        offs.append(total)
        total += K * C + PAD
    runs = []
    dev_parts = [p_.cuda() for p_ in parts]
    for _ in range(2):
        buf = torch.full((total,), SENT, device="cuda")
        nv.group_partial_sums([(dp, buf[o:o + K * C].view(K, C)) for dp, o, (K, nb, C) in zip(dev_parts, offs, probs)])
        runs.append(buf)
    assert torch.equal(runs[0], runs[1])                                   # two launches: bit-identical
    host = runs[0].cpu()
    own = torch.zeros(total, dtype=torch.bool)
    fails = []
    for part, o, (K, nb, C) in zip(parts, offs, probs):
        own[o:o + K * C] = True
        got = host[o:o + K * C].view(K, C).double()
        ref, mag = part.double().sum(1), part.double().abs().sum(1)
        err = (got - ref).abs()
        rel = (err.norm() / ref.norm()).item()
        _rep(f"  group_partial_sums K={K} nb={nb} C={C}: rel norm {rel:.2e}, max err / sum|terms| {(err / mag).max().item():.2e}")
        if not (rel <= 1e-6 and bool((err <= 1e-6 * mag).all())):
            fails.append(f"K={K} nb={nb} C={C}: rel norm {rel:.2e}, max err / sum|terms| {(err / mag).max().item():.2e}")
    assert not fails, "\n".join(fails)
    assert bool((host[~own] == SENT).all())                                # the elements next to every destination


# ---- G. native.cast_bf16_group ------------------------------------------------------------------------------------------------
def test_cast_bf16_group_bits_and_edges():
    """8-element vector bodies, the scalar tail and a second workgroup (8192 elements each) in ONE launch; bit-equal to
    Tensor.to(bfloat16) on the CPU (round to nearest even) on ordinary and special values; a NaN stays a NaN."""
    from scenesplat_amd import native as nv
    g = _gen(7)
    big = torch.finfo(F32).max
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -133, 2.0 ** -134,
                            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,
                            big, -big, 3.3895313892515355e38, 65504.0, 2.0 ** -126], dtype=F32)
    nan_bits = torch.tensor([0x7fc00001, -1, 0x7f800001], dtype=torch.int64).to(torch.int32).view(F32)   # payloads, sign, signalling
    PAD, SENT = 16, 0x5a5a
    edge = torch.cat([special, nan_bits])                                  # 23 values
    srcs = []
    for numel in (1, 7, 8, 9, 8191, 8192, 8193, 16389):
        s = torch.randn(numel, generator=g) * 10.0 ** torch.randint(-3, 4, (numel,), generator=g).float()
        if numel > 64:
            s[16:16 + len(edge)] = edge                                    # every edge value through the 8-element vector bodies
            s[numel - 7:] = edge[3:10]                                     # ... and some through the scalar tail of this size
        srcs.append(s)
    for k in range(0, len(edge), 7):                                       # numel = 7 is all scalar tail: every edge value through it
        s = torch.randn(7, generator=g)
        s[:len(edge[k:k + 7])] = edge[k:k + 7]
        srcs.append(s)
    srcs.append(edge[4:5].clone())                                         # numel = 1: the NaN alone
    srcs.append(torch.cat([edge[8:16], edge[16:17]]))                      # numel = 9: one body, one tail element
    srcs.append(edge[:8].clone())                                          # numel = 8: exactly one body
    fulls = [torch.full((s.numel() + PAD,), SENT, dtype=torch.int16, device="cuda") for s in srcs]
    dsts = [f[:s.numel()].view(BF16) for f, s in zip(fulls, srcs)]
    nv.cast_bf16_group([s.cuda() for s in srcs], dsts)
    torch.cuda.synchronize()
    fails = []
    for j, (s, full) in enumerate(zip(srcs, fulls)):
        numel = s.numel()
        got = full.cpu()
        want = s.to(BF16).view(torch.int16)
        nan = torch.isnan(s)
        if not bool(torch.isnan(got[:numel].view(BF16)[nan]).all()):                            # NaN stays NaN, whatever its payload
            fails.append(f"tensor {j} (numel {numel}): a NaN did not stay NaN")
        keep = ~nan           # a NaN has no reference encoding: the CPU cast itself writes 0x7fc0 from its scalar path and 0xffff from its vector path
        for i in torch.nonzero((got[:numel] != want) & keep).flatten().tolist()[:8]:
            fails.append(f"tensor {j} (numel {numel}) [{i}]: fp32 bits {s.view(torch.int32)[i].item() & 0xffffffff:#010x} -> "
                         f"{got[i].item() & 0xffff:#06x}, CPU {want[i].item() & 0xffff:#06x}")
        if not bool((got[numel:] == SENT).all()):                                                # past numel: untouched
            fails.append(f"tensor {j} (numel {numel}): wrote past numel")
    assert not fails, "\n".join(fails)
    # the edge values mean what the issue says they mean
    w = special.to(BF16)
    assert w[10].item() == 1.0 and w[11].item() == 1.015625 and torch.isinf(w[15]) and torch.isinf(w[16]) and w[5].item() != 0.0
