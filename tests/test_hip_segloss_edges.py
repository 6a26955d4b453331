"""GPU: the loss pair of csrc/seg_loss.hip past one scan tile (4096 sorted elements), one trip of the row loop (262 144 rows) and one
trip of the tile scan (256 tiles), against the float64 references of tests/segloss_cases.py; the segmented sort as the loss calls it
(32 key bits, the foreground flag above them, up to 256 segments); the one-pass backward as a unit; the evaluator's counts.
tests/test_segloss_host.py pins the case builders and the margins on the CPU; profiles/segloss_edges.md records the measured errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_cases as sc  # noqa: E402
from segloss_cases import BF16, F32, U  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_DTYPES = [(name, dtype) for name in sc.ALL_CASES for dtype in sc.case_dtypes(name)]


@pytest.fixture(scope="module")
def nv():
    from scenesplat_amd import native
    return native


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(name, dtype):
    c = sc.case(name)
    seen = None
    if c.seen is not None:
        seen = torch.zeros(c.C, dtype=torch.uint8)
        seen[c.seen] = 1
        seen = seen.cuda()
    return c, sc.case_logits(name, dtype).cuda(), c.labels.cuda(), sc.NO_IGNORE if c.ignore is None else c.ignore, seen


def _forward(nv, name, dtype):
    """the kernel's outputs and its own probabilities exp(x - m) / s from rowstat, formed on the device"""
    c, x, lab, ign, seen = _operands(name, dtype)
    sums, rowstat, glov, present = nv.seg_loss_fwd(x, lab, ign, seen, True)
    p = torch.exp(x.float() - rowstat[:, :1]) / rowstat[:, 1:]
    return c, (x, lab, ign, seen), (sums, rowstat, glov, present), p


# =====================================================================================================================
# the sort as the loss calls it
# =====================================================================================================================
@pytest.mark.parametrize("n", sc.SORT_N)
@pytest.mark.parametrize("K", sc.SORT_SEGMENTS)
def test_argsort_on_32_bits_carries_bit_32_along(nv, K, n):
    keys = sc.sort_keys(K, n)
    order, inverse, skeys = nv.argsort_i64(keys.cuda(), 32)
    kn = keys.numpy()
    ref = np.stack([np.argsort(k & 0xFFFFFFFF, kind="stable") for k in kn])
    assert np.array_equal(order.cpu().numpy(), ref)
    assert np.array_equal(skeys.cpu().numpy(), np.take_along_axis(kn, ref, 1))
    assert np.array_equal(np.take_along_axis(inverse.cpu().numpy(), ref, 1), np.broadcast_to(np.arange(n), (K, n)))


# =====================================================================================================================
# forward
# =====================================================================================================================
def _implied_count(got, k, gts, cf, cfp):
    """the cumulative foreground count through rank k that the kernel's value implies: the count near the true one (cf through k,
    cfp through k - 1) whose float32 J_k - J_{k-1} has the kernel's bits, or None"""
    for delta in sorted(range(-4, 5), key=abs):
        for dprev in (delta, 0):                                    # the element before it may lie in a tile with the right offset
            a, b = torch.tensor([cf + delta, cfp + dprev], dtype=F32), torch.tensor([k + 1 - cf - delta, k - cfp - dprev], dtype=F32)
            J = 1.0 - (gts - a) / (gts + b)
            g = J[0] - (J[1] if k > 0 else 0.0)
            if float(g) == float(got):
                return cf + delta
    return None


def _assert_glov(name, got_sorted, want_sorted, fg_sorted, counts, classes, keep=None):
    """bit-equality of the kernel's gradient in sorted order (classes, m) with the float32 restatement, on the kept elements"""
    same = _bits(got_sorted) == _bits(want_sorted)
    if keep is not None:
        same = same | ~keep
    if bool(same.all()):
        return
    lines = []
    for r in (~same.all(1)).nonzero().flatten().tolist()[:4]:
        k = int((~same[r]).nonzero()[0])
        gts = float(counts[classes[r]])
        cf, cfp = int(fg_sorted[r, :k + 1].sum()), int(fg_sorted[r, :k].sum())
        tiles, per = torch.unique((~same[r]).nonzero().flatten() // sc.SL_TILE, return_counts=True)
        lines.append(f"class {classes[r]}: {int((~same[r]).sum())} of {same.shape[1]} differ, first at rank {k} (tile {k // sc.SL_TILE}): "
                     f"kernel {float(got_sorted[r, k])!r} want {float(want_sorted[r, k])!r}; foreground count through it {cf} of "
                     f"{int(gts)}, the kernel's value implies {_implied_count(got_sorted[r, k], k, gts, cf, cfp)}; differing ranks per "
                     f"tile {dict(zip(tiles.tolist()[:8], per.tolist()[:8]))}")
    raise AssertionError(f"{name}: glov differs from the float32 restatement in {int((~same.all(1)).sum())} classes\n" + "\n".join(lines))


@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_forward_against_fp64(nv, name, dtype):
    """Measured on the MI355X (profiles/segloss_edges.md): every case inside every bound below."""
    c, (x, lab, ign, seen), (sums, rowstat, glov, present), p = _forward(nv, name, dtype)
    ref = sc.case_reference(name, dtype)
    sums, rowstat, glov, present, p = sums.cpu(), rowstat.cpu(), glov.cpu(), present.cpu(), p.cpu()
    xf = sc.case_logits(name, dtype).float()
    # exact counts
    assert float(sums[1]) == ref.n_valid and float(sums[3]) == int(ref.present.sum())
    assert torch.equal(present.bool(), ref.present)
    # row statistics
    assert torch.equal(_bits(rowstat[:, 0]), _bits(xf.max(1).values))
    srel = float(((rowstat[:, 1].double() - ref.s).abs() / ref.s).max())
    print(f"    {name} {dtype}: sum of exponentials off by {srel / U:.2f} * 2^-24 relative (bound {c.C + 4})")
    assert srel <= (c.C + 4) * U
    # the Lovasz gradient
    classes = ref.present.nonzero().flatten().tolist()
    gts = ref.counts.double()[:, None]
    if c.family == "spaced":
        pdev = float((p.double() - ref.p).abs().max())
        gap = float((ref.err_sorted[:, :-1] - ref.err_sorted[:, 1:]).min())
        print(f"    {name}: the kernel's probabilities deviate from float64 by {pdev / U:.2f} * 2^-24; half the least gap {gap / 2 / U:.2f}")
        assert pdev <= 3 * U < gap / 2                             # so the float64 order is the kernel's order
        order, fs = ref.order, ref.fg_sorted
        keep = None
    else:
        e32, fg = sc.f32_errors(p, c.labels, ref.rows)             # the kernel's own probabilities: stable, ties by row
        es, perm = torch.sort(e32, dim=1, descending=True, stable=True)
        order, fs = ref.rows[perm], fg.gather(1, perm)
        flagged = sc.near_tied(es)
        if c.family == "random":
            share = float(flagged[ref.present].float().mean())
        else:                                                      # the saturated rows tie among themselves by construction
            unsat = ~torch.isin(order, c.sat_rows)
            share = float((flagged & unsat)[ref.present].sum() / unsat[ref.present].sum())
            print(f"    {name} {dtype}: near-tied share of all valid elements {100 * float(flagged[ref.present].float().mean()):.1f} %")
        print(f"    {name} {dtype}: near-tied share {100 * share:.3f} %")
        assert share <= sc.NEAR_TIE_CAP
        keep = ~flagged
        if c.family == "saturated":
            # the errors of exactly 1 (p exactly 0 on the label, exactly 1 off it) open every class's sequence as one run of exact
            # ties; the rows keep their order in it, and nothing else comes within 8 * 2^-24 of it: that run is held to bit-equality too
            ones = es == 1.0
            assert int(ones.sum()) > 500 and float(es.masked_fill(ones, 0.0).max()) < 1 - 8 * U
            keep = keep | ones
        keep = keep[ref.present]
    want = sc.jaccard_f32(fs, gts)[ref.present]
    got = glov.gather(1, order)[ref.present]
    _assert_glov(f"{name} {dtype}", got, want, fs[ref.present], ref.counts, classes, keep)
    # values
    ce, lov = float(sums[0].double() / sums[1].double()), float(sums[2].double() / sums[3].double().clamp(min=1))
    tce, tlov = sc.case_torch_f32(name, dtype)
    err = (sc.rel_err(ce, ref.ce), sc.rel_err(lov, ref.lovasz))
    terr = (sc.rel_err(tce, ref.ce), sc.rel_err(tlov, ref.lovasz))
    print(f"    VALUES {name} {dtype}: ce {ce:.7f} kernel err {err[0]:.2e} torch f32 err {terr[0]:.2e} | lovasz {lov:.7f} kernel err "
          f"{err[1]:.2e} torch f32 err {terr[1]:.2e}")
    assert err[0] <= sc.value_bound(terr[0]) and err[1] <= sc.value_bound(terr[1])


@pytest.mark.parametrize("name", ["r20-12293-seen", "spaced-1056785"])
def test_two_runs_are_bit_equal(nv, name):
    outs = []
    for _ in range(2):
        c, (x, lab, ign, seen), (sums, rowstat, glov, present), _ = _forward(nv, name, "f32")
        coef = torch.stack([1 / sums[1], 1 / sums[3]])
        outs.append((sums, glov[present.bool()], nv.seg_loss_bwd(x, lab, ign, rowstat, glov, present, coef)))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))


# =====================================================================================================================
# backward as a unit
# =====================================================================================================================
BWD_CASES = [(name, dtype) for name in ("r20-12293-seen", "r256-4097", sc.SATURATED, "spaced-262145", "spaced-270337")
             for dtype in sc.case_dtypes(name)]


def _assert_bwd(tag, got, ref, dtype):
    assert bool(torch.isfinite(got).all()), tag
    err = (got.double().cpu() - ref).abs()
    top = float(ref.abs().max())
    print(f"    {tag}: max |err| / max |ref| = {float(err.max()) / top:.2e}")
    if dtype == "f32":
        assert float(err.max()) <= 1e-5 * top, tag
    else:
        assert bool((err <= sc.bf16_bound(ref)).all()), (tag, float((err / sc.bf16_bound(ref)).max()))


@pytest.mark.parametrize("name,dtype", BWD_CASES)
def test_backward_against_fp64_on_the_kernels_own_forward(nv, name, dtype):
    c, (x, lab, ign, seen), (sums, rowstat, glov, present), _ = _forward(nv, name, dtype)
    xf = sc.case_logits(name, dtype).float()
    host = (rowstat.cpu(), glov.cpu(), present.cpu())
    for coef in ((0.37, -1.9), (1.0 / float(sums[1]), 1.0 / float(sums[3]))):
        cdev = torch.tensor(coef, dtype=F32, device="cuda")
        got = nv.seg_loss_bwd(x, lab, ign, rowstat, glov, present, cdev)
        assert got.dtype == x.dtype
        ref = sc.bwd_reference(xf, c.labels, *host, cdev.cpu().tolist(), c.ignore)
        _assert_bwd(f"{name} {dtype} coef {coef[0]:.3g}, {coef[1]:.3g}", got, ref, dtype)
        assert bool((got[~ref_valid(c)] == 0).all())
    # the cross-entropy term alone
    cdev = torch.tensor((0.37, -1.9), dtype=F32, device="cuda")
    got = nv.seg_loss_bwd(x, lab, ign, rowstat, None, None, cdev)
    _assert_bwd(f"{name} {dtype} ce only", got, sc.bwd_reference(xf, c.labels, host[0], None, None, (0.37, -1.9), c.ignore), dtype)


def ref_valid(c):
    return sc.valid_mask(c.labels, c.C, c.ignore).cuda()


@pytest.mark.parametrize("name", ["r20-12293-seen", "r256-4097"])
def test_backward_never_reads_the_gradient_of_a_class_that_is_not_present(nv, name):
    c, (x, lab, ign, seen), (sums, rowstat, glov, present), _ = _forward(nv, name, "f32")
    assert int((present == 0).sum()) > 0
    poisoned = glov.clone()
    poisoned[present == 0] = float("nan")
    cdev = torch.tensor((0.37, -1.9), dtype=F32, device="cuda")
    got = nv.seg_loss_bwd(x, lab, ign, rowstat, poisoned, present, cdev)
    zeroed = glov.clone()
    zeroed[present == 0] = 0.0
    ref = sc.bwd_reference(c.logits, c.labels, rowstat.cpu(), zeroed.cpu(), present.cpu(), (0.37, -1.9), c.ignore)
    _assert_bwd(f"{name} poisoned", got, ref, "f32")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_saturated_rows_are_finite_and_carry_no_lovasz_gradient(nv, dtype):
    c, (x, lab, ign, seen), (sums, rowstat, glov, present), p = _forward(nv, sc.SATURATED, dtype)
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(glov).all()) and bool(torch.isfinite(rowstat).all())
    valid = ref_valid(c)
    for coef in ((0.0, 1.0), (1.0 / float(sums[1]), 1.0 / float(sums[3]))):
        d = nv.seg_loss_bwd(x, lab, ign, rowstat, glov, present, torch.tensor(coef, dtype=F32, device="cuda")).float()
        assert bool(torch.isfinite(d).all())
        if coef[0] == 0.0:                                          # the Lovasz term alone
            assert bool((d[(p == 0) & valid[:, None]] == 0).all()) and int(((p == 0) & valid[:, None]).sum()) > 2000
            up = c.sat_rows[c.sat_kind < 2].cuda()                  # +200 * one_hot: every p of the row is 0 or 1
            assert bool(((p[up] == 0) | (p[up] == 1)).all()) and bool((d[up] == 0).all())
            assert float(d.abs().max()) > 0


# =====================================================================================================================
# through the modules
# =====================================================================================================================
@pytest.mark.parametrize("name", ["spaced-8193", "r20-12293-seen", "r20-8193-noignore"])
@pytest.mark.parametrize("through_criteria", [False, True])
def test_modules_return_the_direct_path_combined_by_hand(nv, name, through_criteria):
    from scenesplat_amd.pointcept_api import LOSSES, build_criteria
    c, (x, lab, ign, seen), _, _ = _forward(nv, name, "f32")
    ce_ignore = -1 if c.ignore is None else c.ignore               # every label valid there: CrossEntropyLoss needs an integer
    cfgs = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=ce_ignore),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=c.ignore, class_seen=c.seen)]
    xg = x.clone().requires_grad_(True)
    if through_criteria:
        crit = build_criteria(cfgs)
        ce, lov = crit.criteria[0](xg, lab), crit.criteria[1](xg, lab)
        total = crit(xg, lab)
    else:
        ce, lov = LOSSES.build(cfgs[0])(xg, lab), LOSSES.build(cfgs[1])(xg, lab)
        total = ce + lov
    total.backward()
    # by hand
    s_ce, rs_ce, _, _ = nv.seg_loss_fwd(x, lab, ce_ignore, None, False)
    s, rowstat, glov, present = nv.seg_loss_fwd(x, lab, ign, seen, True)
    zero = torch.zeros((), device="cuda")
    d = nv.seg_loss_bwd(x, lab, ce_ignore, rs_ce, None, None, torch.stack([1 / s_ce[1], zero])) + \
        nv.seg_loss_bwd(x, lab, ign, rowstat, glov, present, torch.stack([zero, 1 / s[3].clamp(min=1.0)]))
    assert torch.equal(ce.detach(), s_ce[0] / s_ce[1]) and torch.equal(lov.detach(), s[2] / s[3].clamp(min=1.0))
    assert torch.equal(total.detach(), s_ce[0] / s_ce[1] + s[2] / s[3].clamp(min=1.0))
    assert torch.equal(s_ce[:2], s[:2])
    err = float((xg.grad - d).abs().max() / d.abs().max())
    assert err <= 4 * U, err
    ref = sc.case_reference(name)
    assert sc.rel_err(ce.detach(), ref.ce) < 1e-5 and sc.rel_err(lov.detach(), ref.lovasz) < 1e-5


# =====================================================================================================================
# evaluator counts
# =====================================================================================================================
@pytest.mark.parametrize("ignore", sc.IOU_IGNORE)
@pytest.mark.parametrize("C", sc.IOU_C)
@pytest.mark.parametrize("n", sc.IOU_N)
def test_seg_iou_counts_at_block_and_trip_edges(nv, n, C, ignore):
    logits, tgt, pred = sc.iou_case(n, C, ignore)
    tn = tgt.numpy()
    want = sc.iou_counts(pred.numpy().astype(np.int64), tn, C, ignore)
    assert np.array_equal(nv.seg_iou(tgt.cuda(), C, ignore, pred=pred.cuda()).cpu().numpy(), want)
    want = sc.iou_counts(sc.argmax_lowest(logits).astype(np.int64), tn, C, ignore)
    for lg in (logits, logits.to(BF16)):
        got = nv.seg_iou(tgt.cuda(), C, ignore, logits=lg.cuda()).cpu().numpy()
        assert np.array_equal(got, want), (str(lg.dtype), np.abs(got - want).max())
    assert want[2].sum() == int(((tn >= 0) & (tn < C)).sum())
