"""GPU tests of the grouped-launch idiom (csrc/grouped.h, scenesplat_amd/grouped.py): the owner lookup of every grouped kernel on tables
of 1 .. 1000 problems whose workgroup counts cycle through (1, 1, 3, 1, 2), so that one-workgroup problems sit on every side of
multi-workgroup ones and both the first and the last workgroup of first, middle and last problems are looked up at every depth of
the binary search.  A workgroup that found the wrong owner would read another problem's descriptor row: one grouped launch is compared
bit for bit with one launch per problem, and with the plain torch expression under the bars of the kernels' own tests."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPROBS = (1, 2, 3, 127, 128, 129, 1000)
WG = (1, 1, 3, 1, 2)                 # workgroups of problem j: WG[j % 5]
U = 2.0 ** -23
GAP = 8                              # untouched elements between the problems of a flat buffer


def wg_counts(nprob):
    return [WG[j % len(WG)] for j in range(nprob)]


def ragged_numels(nprob, per):
    """w workgroups = w - 1 full ones and a last one of r elements, r cycling through the edges of the 8-element lanes"""
    tails = (per, 1, 7, 8, 9, per - 1)
    return [(w - 1) * per + tails[j % len(tails)] for j, w in enumerate(wg_counts(nprob))]


def layout(numels, unaligned=False):
    """-> (element offset of every problem in one flat buffer, the buffer's length, ownership mask).  Offsets are multiples of 8
    elements (16-byte aligned for 2- and 4-byte elements); unaligned: every third problem starts one element further."""
    offs, o = [], GAP
    for j, n in enumerate(numels):
        offs.append(o + (1 if unaligned and j % 3 == 1 else 0))
        o = (offs[-1] + n + GAP + 7) // 8 * 8
    own = np.zeros(o, dtype=bool)
    for a, n in zip(offs, numels):
        own[a:a + n] = True
    return offs, o, torch.from_numpy(own).cuda()


def views(flat, offs, numels, shapes=None):
    return [flat[a:a + n].view(shapes[j]) if shapes else flat[a:a + n] for j, (a, n) in enumerate(zip(offs, numels))]


class Flags:
    """Named device-side verdicts, read back once."""

    def __init__(self):
        self.names, self.flags = [], []

    def add(self, name, ok):
        self.names.append(name); self.flags.append(ok.reshape(()))

    def check(self):
        bad = [n for n, ok in zip(self.names, torch.stack(self.flags).cpu().tolist()) if not ok]
        assert not bad, bad[:8]


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_starts_refuses_2_to_the_31_workgroups():
    from scenesplat_amd import grouped
    assert grouped.starts([]) == [0] and grouped.starts([1, 0, 3]) == [0, 1, 1, 4]
    assert grouped.starts([2 ** 30, 2 ** 30 - 1])[-1] == 2 ** 31 - 1
    with pytest.raises(RuntimeError, match="2\\^31 workgroups"):
        grouped.starts([2 ** 30, 2 ** 30])


@pytest.mark.parametrize("nprob", NPROBS)
def test_cast_group_equals_single_launches(nprob):
    from scenesplat_amd import native as nv
    numels = ragged_numels(nprob, nv.lib().ss_cast_bf16_group_elems_per_workgroup())
    offs, total, own = layout(numels)
    src = torch.randn(total, device="cuda", generator=gen(nprob))
    srcs = views(src, offs, numels)
    outs = []
    for grouped_launch in (True, False):
        dst = torch.full((total,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        dsts = views(dst, offs, numels)
        if grouped_launch:
            nv.cast_bf16_group(srcs, dsts)
        else:
            for s, d in zip(srcs, dsts):
                nv.cast_bf16_group([s], [d])
        outs.append(dst.view(torch.int16))
    assert torch.equal(outs[0], outs[1])
    want = torch.where(own, src.to(torch.bfloat16).view(torch.int16), torch.full_like(outs[0], 0x5a5a))
    assert torch.equal(outs[0], want)                    # .to(bfloat16) inside the problems, nothing written between them


def _tile_problems(nprob, kind):
    """shapes with exactly WG[j % 5] tiles of 64 x 64 and ragged edges"""
    if kind == "transpose":
        return [(64 * w - 5, 37) for w in wg_counts(nprob)]
    return [(64 * w - 5, 1, 37) if j % 2 == 0 else (59, w, 37) for j, w in enumerate(wg_counts(nprob))]      # (cout, taps, cin)


@pytest.mark.parametrize("nprob", NPROBS)
def test_transpose_group_equals_single_launches(nprob):
    from scenesplat_amd import native as nv
    shapes = _tile_problems(nprob, "transpose")
    numels = [r * c for r, c in shapes]
    offs, total, own = layout(numels)
    src = torch.randn(total, device="cuda", generator=gen(nprob)).to(torch.bfloat16)
    srcs = views(src, offs, numels, shapes)
    outs = []
    for grouped_launch in (True, False):
        dst = torch.full((total,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        dsts = views(dst, offs, numels, [(c, r) for r, c in shapes])
        if grouped_launch:
            nv.transpose16_group(list(zip(srcs, dsts)))
        else:
            for pair in zip(srcs, dsts):
                nv.transpose16_group([pair])
        outs.append(dst)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    want = torch.full((total,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    for s, d in zip(srcs, views(want, offs, numels, [(c, r) for r, c in shapes])):
        d.copy_(s.t())
    assert torch.equal(outs[0].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("nprob", NPROBS)
def test_weight_mirror_group_equals_single_launches(nprob):
    from scenesplat_amd import native as nv
    assert nv.lib().ss_subm_weight_mirror_group_tile() == 64
    shapes = _tile_problems(nprob, "mirror")
    numels = [co * t * ci for co, t, ci in shapes]
    offs, total, own = layout(numels)
    src = torch.randn(total, device="cuda", generator=gen(nprob)).to(torch.bfloat16)
    ws = views(src, offs, numels, shapes)
    out_shapes = [(ci, t, co) for co, t, ci in shapes]
    outs = []
    for grouped_launch in (True, False):
        dst = torch.full((total,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        wts = views(dst, offs, numels, out_shapes)
        if grouped_launch:
            nv.subm_weight_mirror_group(list(zip(ws, wts)))
        else:
            for pair in zip(ws, wts):
                nv.subm_weight_mirror_group([pair])
        outs.append(dst)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    want = torch.full((total,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    for w, d in zip(ws, views(want, offs, numels, out_shapes)):
        d.copy_(w.flip(1).permute(2, 1, 0))
    assert torch.equal(outs[0].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("nprob", NPROBS)
def test_partial_sums_group_equals_single_launches(nprob):
    """K * C = per * w - 3 outputs over nb = 9 partial rows; the bars of test_group_partial_sums_against_fp64 (1e-6 of sum|terms| per
    element, 1e-6 in norm): a destination sums 9 terms."""
    from scenesplat_amd import native as nv
    per, nb = nv.lib().ss_group_partial_sums_outputs_per_workgroup(), 9
    kc = [per * w - 3 for w in wg_counts(nprob)]
    shapes = [(3, nb, n // 3) if n % 3 == 0 else (1, nb, n) for n in kc]
    g = gen(nprob)
    parts = [torch.randn(s, device="cuda", generator=g) for s in shapes]
    offs, total, own = layout(kc)
    outs = []
    for grouped_launch in (True, False):
        dst = torch.full((total,), -12345.0, device="cuda")
        items = list(zip(parts, views(dst, offs, kc, [(s[0], s[2]) for s in shapes])))
        if grouped_launch:
            nv.group_partial_sums(items)
        else:
            for it in items:
                nv.group_partial_sums([it])
        outs.append(dst)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][~own] == -12345.0).all())
    flags = Flags()
    for j, (part, got) in enumerate(zip(parts, views(outs[0], offs, kc))):
        ref, mag = part.double().sum(1).reshape(-1), part.double().abs().sum(1).reshape(-1)
        err = (got.double() - ref).abs()
        flags.add(f"problem {j}", (err.norm() <= 1e-6 * ref.norm()) & (err <= 1e-6 * mag).all())
    flags.check()


# ---- the fp32 elementwise kernels: aligned tables of every size, and one table that mixes 16-byte and one-element lanes ------------
F32_CASES = [(n, False) for n in NPROBS] + [(129, True)]
F32_IDS = [f"{n}{'-unaligned' if u else ''}" for n, u in F32_CASES]


def _f32_problems(nprob, unaligned):
    from scenesplat_amd import native as nv
    numels = ragged_numels(nprob, nv.lib().ss_optim_group_elems_per_workgroup())
    offs, total, own = layout(numels, unaligned)
    return numels, offs, total, own


@pytest.mark.parametrize("nprob,unaligned", F32_CASES, ids=F32_IDS)
def test_ema_group_equals_single_launches(nprob, unaligned):
    from scenesplat_amd import native as nv
    numels, offs, total, own = _f32_problems(nprob, unaligned)
    g = gen(nprob)
    t0, s = torch.randn(total, device="cuda", generator=g), torch.randn(total, device="cuda", generator=g)
    students = views(s, offs, numels)
    if unaligned:
        assert any(v.data_ptr() % 16 for v in students) and any(v.data_ptr() % 16 == 0 for v in students)
    m = 0.996
    outs = []
    for grouped_launch in (True, False):
        t = t0.clone()
        teachers = views(t, offs, numels)
        if grouped_launch:
            nv.ema_group(teachers, students, m)
        else:
            for a, b in zip(teachers, students):
                nv.ema_group([a], [b], m)
        outs.append(t)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][~own], t0[~own])
    # the bar of test_ema_group_matches_fp64: three fp32 roundings of terms no larger than max(|t|, |s|)
    exact = m * t0.double() + (1.0 - m) * s.double()
    bound = 2.0 ** -22 * torch.maximum(t0.abs(), s.abs()).double()
    assert bool((((outs[0].double() - exact).abs() <= bound) | ~own).all())


@pytest.mark.parametrize("nprob,unaligned", F32_CASES, ids=F32_IDS)
def test_adamw_group_equals_single_launches(nprob, unaligned):
    from scenesplat_amd import native as nv
    numels, offs, total, own = _f32_problems(nprob, unaligned)
    g = gen(nprob)
    p0, gr, m0 = (torch.randn(total, device="cuda", generator=g) for _ in range(3))
    v0 = torch.randn(total, device="cuda", generator=g).abs()
    record = torch.tensor([3.0, 0.37], device="cuda")                       # [norm, clip coefficient]
    hyper = [(1e-2, 0.1, 0.9, 0.999, 1e-8, 3), (6e-4, 0.0, 0.85, 0.99, 1e-6, 1), (3e-3, 0.05, 0.95, 0.95, 1e-8, 40)]
    scal = [(1 - lr * wd, 1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, lr / (1 - b1 ** t)) for lr, wd, b1, b2, eps, t in hyper]
    outs = []
    for grouped_launch in (True, False):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        rows = [r + (scal[j % 3],) for j, r in enumerate(zip(*(views(x, offs, numels) for x in (p, gr, m, v))))]
        if grouped_launch:
            nv.adamw_group(rows, record)
        else:
            for r in rows:
                nv.adamw_group([r], record)
        outs.append((p, m, v))
    for a, b, init in zip(outs[0], outs[1], (p0, m0, v0)):
        assert torch.equal(a, b)
        assert torch.equal(a[~own], init[~own])
    # the bar of test_native_bindings_directly against fp64 (a few fp32 roundings of the largest value), with the table taken as one
    # tensor: like that test's tensor, every table holds at least one full workgroup of 8,192 elements
    gd = (gr * 0.37).double()
    refs = [x.double() for x in (p0, m0, v0)]
    for j, (a, n) in enumerate(zip(offs, numels)):
        lr, wd, b1, b2, eps, t = hyper[j % 3]
        sl = slice(a, a + n)
        md = m0[sl].double() + (gd[sl] - m0[sl].double()) * (1 - b1)
        vd = v0[sl].double() * b2 + (1 - b2) * gd[sl] * gd[sl]
        refs[0][sl] = p0[sl].double() * (1 - lr * wd) - lr / (1 - b1 ** t) * (md / (vd.sqrt() / math.sqrt(1 - b2 ** t) + eps))
        refs[1][sl], refs[2][sl] = md, vd
    for nm, got, ref in zip("pmv", outs[0], refs):
        err, scale = float((got.double() - ref).abs().max()), float(ref[own].abs().max())
        print(f"adamw {nm}: max err {err:.3e} = {err / scale / 2.0 ** -24:.2f} * 2^-24 * max|ref|")
        assert err <= 4 * 2.0 ** -24 * scale


@pytest.mark.parametrize("nprob,unaligned", F32_CASES, ids=F32_IDS)
def test_grad_sqnorm_group_equals_single_launches(nprob, unaligned):
    """The fp64 partial sums of the workgroups, grouped against one launch per tensor, bit for bit; the record against the host fp64 sum
    of those partials and against the fp64 norm (1e-6 relative, the bar of test_last_grad_norm_matches_fp64_norm)."""
    from scenesplat_amd import native as nv
    numels, offs, total, own = _f32_problems(nprob, unaligned)
    flat = torch.randn(total, device="cuda", generator=gen(nprob))
    grads = views(flat, offs, numels)
    nwg = sum(wg_counts(nprob))
    rec = nv.grad_norm_group(grads, 1.0).clone()
    buf = nv._norm_partials(flat.device, nwg)                                 # the per-workgroup partials of the last call
    part = buf[:nwg].clone()
    rec2 = nv.grad_norm_group(grads, 1.0)
    assert torch.equal(rec, rec2) and torch.equal(part, buf[:nwg])            # two grouped runs: bit-identical
    single = []
    for g, w in zip(grads, wg_counts(nprob)):
        nv.grad_norm_group([g], 1.0)
        single.append(nv._norm_partials(flat.device, w)[:w].clone())
    single = torch.cat(single)
    assert torch.equal(part, single)
    host = math.sqrt(float(np.sum(single.cpu().numpy(), dtype=np.float64)))
    norm = float(torch.where(own, flat, torch.zeros_like(flat)).double().norm())
    print(f"grad norm {float(rec[0]):.9g}, host sum of partials {host:.9g}, fp64 {norm:.9g}")
    assert abs(float(rec[0]) - host) <= 1e-6 * host and abs(float(rec[0]) - norm) <= 1e-6 * norm
    assert abs(float(rec[1]) - min(1.0, 1.0 / (norm + 1e-6))) <= 1e-6


# ---- PDNorm and the grouped weight gradient at their own granularity -----------------------------------------------------------------
def _close(got, ref, terms, absval):
    """the bound of test_hip_pdnorm.check: (terms + 8) * 2^-23 * (the formula with every term replaced by its absolute value)"""
    return ((got.double() - ref).abs() <= (terms + 8) * U * absval).all()


@pytest.mark.parametrize("nprob", NPROBS)
def test_pdnorm_tables_match_fp64(nprob):
    """Layers of 16 * (w - 1) + r channels (16 per workgroup), forward and backward, against fp64 with the bars of
    test_grouped_modulation_kernels_match_fp64."""
    from scenesplat_amd import native as nv
    per, Cc = nv.lib().ss_pdnorm_channels_per_workgroup(), 24
    tails = (1, 7, 8, 9, per - 1, per)
    widths = [(w - 1) * per + tails[j % len(tails)] for j, w in enumerate(wg_counts(nprob))]
    g = gen(nprob)
    rows = []
    for j, C in enumerate(widths):
        affine = j % 3 != 1
        rows.append((torch.randn(2 * C, Cc, device="cuda", generator=g) / Cc ** 0.5, torch.randn(2 * C, device="cuda", generator=g),
                     torch.randn(C, device="cuda", generator=g) if affine else None,
                     torch.randn(C, device="cuda", generator=g) if affine else None))
    ctx = torch.rand(Cc, device="cuda", generator=g) * 8 - 4
    dge = [torch.randn(C, device="cuda", generator=g) if j % 7 != 3 else None for j, C in enumerate(widths)]
    dbe = [torch.randn(C, device="cuda", generator=g) if j % 7 != 5 else None for j, C in enumerate(widths)]
    tab = nv.PDNormTable(rows, Cc)
    assert tab.starts[-1] == sum(wg_counts(nprob)) and tab.vec4 == 1
    geff, beff, ops = nv.pdnorm_mod_fwd(ctx, tab)
    dctx, dW, db, dg, dbt = nv.pdnorm_mod_bwd(ctx, tab, ops, dge, dbe)
    x = ctx.double()
    sg = 1.0 / (1.0 + torch.exp(-x))
    s = x * sg
    dsilu, dsilu_abs = sg * (1 + x * (1 - sg)), sg * (1 + x.abs() * (1 - sg))
    acc, acc_abs = torch.zeros(Cc, dtype=torch.float64, device="cuda"), torch.zeros(Cc, dtype=torch.float64, device="cuda")
    terms_ctx, off, flags = 0, 0, Flags()
    for l, (W, b, gamma, beta) in enumerate(rows):
        C = widths[l]
        Wd, bd = W.double(), b.double()
        lin, lin_abs = Wd @ s + bd, Wd.abs() @ s.abs() + bd.abs()
        shift, scale, a_shift, a_scale = lin[:C], lin[C:], lin_abs[:C], lin_abs[C:]
        gm = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device="cuda")
        bt = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        o = ops[off:off + C]
        ok = _close(o, 1 + scale, Cc + 2, 1 + a_scale) & _close(geff[l], gm * (1 + scale), Cc + 2, gm.abs() * (1 + a_scale))
        ok = ok & _close(beff[l], bt * (1 + scale) + shift, 2 * Cc + 3, bt.abs() * (1 + a_scale) + a_shift)
        ge = dge[l].double() if dge[l] is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        be = dbe[l].double() if dbe[l] is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        dbr = torch.cat([be, ge * gm + be * bt])
        dbr_abs = torch.cat([be.abs(), ge.abs() * gm.abs() + be.abs() * bt.abs()])
        ok = ok & _close(db[l], dbr, 2, dbr_abs) & _close(dW[l], dbr[:, None] * s[None, :], 2, dbr_abs[:, None] * s.abs()[None, :])
        if gamma is not None:
            ok = ok & _close(dg[l], ge * o.double(), 1, ge.abs() * o.double().abs())
            ok = ok & _close(dbt[l], be * o.double(), 1, be.abs() * o.double().abs())
        else:
            assert dg[l] is None and dbt[l] is None
        flags.add(f"layer {l} (C = {C})", ok)
        acc += Wd.t() @ dbr
        acc_abs += Wd.abs().t() @ dbr_abs
        terms_ctx += 3 * C if gamma is not None else 2 * C
        off += C
    flags.add("dcontext", _close(dctx, dsilu * acc, terms_ctx, dsilu_abs * acc_abs))
    flags.check()


@pytest.mark.parametrize("nprob", [n for n in NPROBS if n <= 128])
def test_linear_wgrad_group_tables_match_fp32_reference(nprob):
    """Problems of one and of several workgroups in turn (the planner's own counts), against the fp32 product with the bars of
    test_linear_wgrad_group_matches_fp32_reference.  The kernel adds its shares with fp32 atomics: nothing here is compared bitwise."""
    import ctypes
    from scenesplat_amd import native as nv
    lib = nv.lib()
    by_count = {1: (64, 8, 8), 2: (640, 8, 16), 3: (2047, 64, 192)}          # (m, k_in, n_out) of a problem of WG[j % 5] = 1, 2, 3
    shapes = [by_count[w] for w in wg_counts(nprob)]
    tiles = sum(lib.ss_linear_wgrad_tiles(k, n) for _, k, n in shapes)
    words = np.zeros(8, dtype=np.int64)
    planned = [lib.ss_linear_wgrad_group_plan2(m, k, n, tiles, ctypes.c_void_p(words.ctypes.data)) for m, k, n in shapes]
    assert min(planned) == 1 and (nprob < 3 or max(planned) > 1), planned      # single- and multi-workgroup problems side by side
    g = gen(nprob)
    items, refs = [], []
    for j, (m, k, n) in enumerate(shapes):
        x = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(m, n, device="cuda", generator=g).to(torch.bfloat16)
        items.append((x, dy, torch.zeros(n, k, device="cuda"), torch.zeros(n, device="cuda") if j % 2 == 0 else None))
        refs.append((dy.float().t() @ x.float(), dy.float().sum(0)))
    nv.linear_wgrad_group(items)
    flags = Flags()
    for j, ((x, dy, dw, db), (rw, rb)) in enumerate(zip(items, refs)):
        flags.add(f"dw[{j}]", (dw - rw).norm() <= 1e-5 * rw.norm())
        if db is not None:
            flags.add(f"db[{j}]", (db - rb).norm() <= 1e-5 * rb.norm())
    flags.check()
