"""csrc/scan.hip, csrc/head.hip and AggregatedContrastiveLoss at the edges of their dispatch, against float64 on the CPU.

ss_feat_text_scan picks k_feat_text_scan<NT> from the class count (NT in 2, 4, 7, 8, 10, 13, 16); ss_lang_head_fwd / _bwd pick
k_head_fwd<IT> / k_head_bwd<IT> from IT = ceil(C / 256) in 1..8 and cap the grid at 1024 blocks of four rows.  lang_cases.py lists
the shapes and names the instance each takes; test_lang_host.py pins the references, the exact-logit construction and the margin
between torch's own fp32 and the bounds used here.

Scan.  The exact cases draw feat and text from {-2..2}/8: every fp32 accumulation order gives the exact logit, so the arg-max has
to equal numpy.argmax of the float64 logits (first occurrence = lowest class among equal maxima) in EVERY row; tied maxima occur
in 2..28 of 300 rows.  Probabilities are held to 2e-4 (the bar of test_open_vocab_scan_against_reference_math).
Head.  fp32: p atol 2e-7 rtol 1e-6, sums[0..1] 3e-6 relative, sums[2] exact (the bars of test_fused_head_matches_oracle), the
gradient 1e-5 PER ROW.  Stored in bf16: |out - ref| <= 2^-8 |ref| + 1e-5 max|ref row|.
Contrastive.  loss 1e-5 absolute, gradient atol 2e-7 rtol 1e-3 (the bars of test_lang_head_matches_reference).

With normalisation and no gradient arriving at p, the zero-target row's exact gradient is 0 (its d p = 2 c1 p is radial and is
projected out); float64 returns rounding noise there, so that one row is held to 1e-5 of what cancels, 2 c1 / |f|
(lang_cases.ill_conditioned_scale).  Where w_extra is used that row's w_extra is ~ randn, which keeps the row well conditioned.

Worst values observed on an MI355X (every test prints its own next to its bound):
  scan values                 max_prob 7.6e-8, accumulated probabilities 1.7e-7                          (bound 2e-4)
  head fp32   p               0.095 of atol + rtol |ref|      (C = 48, bf16 features)
              sums            6.8e-8 relative                 (the norm-3e-9 row alone; bound 3e-6)
              gradient        3.0e-7 in the worst row         (n = 8195; bound 1e-5)
  head bf16   p               0.985 of the bound              (C = 2048; one rounding is up to 2^-8 |ref| by itself)
              sums            5.2e-8 relative                 (C = 48, bf16 features and targets; bound 3e-6)
              gradient        0.991 of the bound              (C = 2048, bf16 features and targets)
  contrastive loss            3.3e-7                          (C = 16, reduction='sum'; bound 1e-5)
              gradient        0.027 of atol + rtol |ref|      (C = 16, reduction='sum')
The arg-max equalled the reference in every row of every exact case.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lang_cases as lc  # noqa: E402
from lang_cases import BF16, F32, F64  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}       # group -> largest err / bound seen in this process


def note(group, what, err, bound):
    """print an observed error next to its bound and keep the worst ratio of the group"""
    err, bound = float(err), float(bound)
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"    [{group}] {what}: {err:.3e} (bound {bound:.3e}); worst err / bound of the group so far {WORST[group]:.3g}")
    return err <= bound


def _dtn(dtype):
    return {None: "none", F32: "f32", BF16: "bf16"}[dtype]


# =====================================================================================================================
# open-vocabulary scan
# =====================================================================================================================
def scan(feat, text, **kw):
    from scenesplat_amd import native as nv
    return nv.feat_text_scan(feat.cuda(), text.cuda(), **kw)


def check_exact_scan(n, D, C, kind="any"):
    feat, text = lc.scan_exact(n, D, C, kind)
    ref = lc.scan_exact_reference(n, D, C, kind)
    mp, am = scan(feat, text)
    assert mp.shape == (n,) and mp.dtype == F32 and am.shape == (n,) and am.dtype == torch.int32
    am, mp = am.cpu().long(), mp.cpu().double()
    bad = torch.nonzero(am != ref.argmax).flatten()
    print(f"    n={n} D={D} C={C} (NT {lc.scan_tile_count(C)}) {kind}: {int(ref.ties.sum())} rows with a tied maximum, "
          f"{len(bad)} rows with another arg-max than the reference")
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"row {r}: argmax {int(am[r])} (logit {ref.logits[r, am[r]].item() if 0 <= am[r] < C else 'out of range'}), "
                             f"reference {int(ref.argmax[r])} (logit {ref.logits[r, ref.argmax[r]].item()}), tied: {bool(ref.ties[r])}")
    assert note("scan", "max_prob", (mp - ref.max).abs().max(), lc.SCAN_ATOL)
    return ref


# NT of each C: 1, 16, 17, 32 -> 2 | 33, 64 -> 4 | 65, 112 -> 7 | 113, 128 -> 8 | 129, 160 -> 10 | 161, 208 -> 13 | 209, 255, 256 -> 16
@pytest.mark.parametrize("D", lc.SCAN_DIMS)          # 72: two k steps, the second with one live 8-wide chunk | 768: 12 full k steps
@pytest.mark.parametrize("C", lc.SCAN_CLASSES)
def test_scan_argmax_is_exact_at_every_tile_boundary(C, D):
    check_exact_scan(lc.SCAN_N, D, C)


# n: 1 -> one live row | 127, 128 -> one workgroup, the last row missing / present | 129 -> a second workgroup with one row
# C: 17 -> NT 2 | 256 -> NT 16
@pytest.mark.parametrize("n,C,D", lc.SCAN_ROW_EDGES)
def test_scan_row_count_edges(n, C, D):
    check_exact_scan(n, D, C)


# D: 8 -> one chunk of one k step | 40 -> five chunks | 64 -> exactly one k step (no second stage); C = 33 -> NT 4
@pytest.mark.parametrize("n,C,D", lc.SCAN_WIDTH_EDGES)
def test_scan_width_edges(n, C, D):
    check_exact_scan(n, D, C)


# C: 1, 17 -> NT 2 with 31 / 15 padded classes | 209 -> NT 16 with 47; n = 129: 127 padded rows in the second workgroup
@pytest.mark.parametrize("n,C,D", lc.SCAN_NEGATIVE)
def test_scan_padded_lanes_never_win_when_every_logit_is_negative(n, C, D):
    ref = check_exact_scan(n, D, C, "negative")
    assert float(ref.max.max()) < 0.5


@pytest.mark.parametrize("C", [17, 100, 256])        # NT 2, 7, 16
def test_scan_identical_text_rows_give_class_zero(C):
    ref = check_exact_scan(129, 72, C, "same-text")
    assert bool((ref.argmax == 0).all())


@pytest.mark.parametrize("C", lc.SCAN_CLASSES)       # NT as above
def test_scan_accumulates_into_a_prefilled_buffer_through_an_injection(C):
    """pred_accum[idx[i]] += probs[i]: rows outside idx keep their bits, touched rows hold sentinel + prob"""
    n, D, rows, sentinel = lc.SCAN_N, 72, 517, 0.75
    feat, text = lc.scan_exact(n, D, C)
    ref = lc.scan_exact_reference(n, D, C)
    idx = lc.scan_injection(n, rows, seed=C)
    g = torch.Generator().manual_seed(C)
    before = sentinel + torch.rand(rows, C, generator=g)                     # a different value in every cell
    pred = before.cuda()
    out = scan(feat, text, want_max=False, idx=idx.cuda(), pred_accum=pred)
    assert out == (None, None)
    pred = pred.cpu()
    untouched = torch.ones(rows, dtype=torch.bool)
    untouched[idx.long()] = False
    assert int(untouched.sum()) == rows - n and torch.equal(pred[untouched], before[untouched])
    assert note("scan", "prefilled + prob", (pred[idx.long()].double() - (before[idx.long()].double() + ref.probs)).abs().max(), lc.SCAN_ATOL)


@pytest.mark.parametrize("C", [17, 33, 65, 113, 129, 161, 256])              # NT 2, 4, 7, 8, 10, 13, 16
def test_scan_second_call_adds_the_same_amount_again(C):
    n, D, rows = lc.SCAN_N, 72, 517
    feat, text = lc.scan_exact(n, D, C)
    idx = lc.scan_injection(n, rows, seed=C).cuda()
    pred = torch.zeros(rows, C, device="cuda")
    scan(feat, text, want_max=False, idx=idx, pred_accum=pred)
    once = pred.clone()
    scan(feat, text, want_max=False, idx=idx, pred_accum=pred)
    assert torch.equal(pred, 2 * once) and float(once.sum()) > 0            # 0 + s = s and s + s = 2 s are exact in fp32
    assert note("scan", "probs", (once.cpu()[idx.cpu().long()].double() - lc.scan_exact_reference(n, D, C).probs).abs().max(), lc.SCAN_ATOL)


@pytest.mark.parametrize("C", [1, 33, 209])                                  # NT 2, 4, 16
def test_scan_without_idx_writes_row_i_to_row_i(C):
    n, D = 129, 40
    feat, text = lc.scan_exact(n, D, C)
    ref = lc.scan_exact_reference(n, D, C)
    pred = torch.full((n + 3, C), 0.25, device="cuda")                       # three rows beyond n: never touched
    scan(feat, text, want_max=False, pred_accum=pred)
    pred = pred.cpu()
    assert bool((pred[n:] == 0.25).all())
    assert note("scan", "prefilled + prob, idx=None", (pred[:n].double() - (0.25 + ref.probs)).abs().max(), lc.SCAN_ATOL)


@pytest.mark.parametrize("C", lc.SCAN_CLASSES)       # NT as above
def test_scan_max_and_accumulation_in_one_call_agree_bitwise(C):
    """the maximum is the same expression on the same accumulator as the accumulated probability"""
    n, D = lc.SCAN_N, 72
    feat, text = lc.scan_exact(n, D, C)
    ref = lc.scan_exact_reference(n, D, C)
    pred = torch.zeros(n, C, device="cuda")
    mp, am = scan(feat, text, want_max=True, pred_accum=pred)
    mp, am, pred = mp.cpu(), am.cpu().long(), pred.cpu()
    assert torch.equal(am, ref.argmax)
    assert torch.equal(mp, pred[torch.arange(n), am]) and torch.equal(mp, pred.max(1).values)
    assert note("scan", "probs", (pred.double() - ref.probs).abs().max(), lc.SCAN_ATOL)


@pytest.mark.parametrize("C", lc.SCAN_UNIT_CLASSES)  # 40 -> NT 4 | 120 -> NT 8 | 256 -> NT 16
def test_scan_values_on_random_unit_rows_at_the_unrun_tile_counts(C):
    """the inputs of test_open_vocab_scan_against_reference_math; values only (near-ties may resolve either way in fp32)"""
    n, D = 3001, 768
    feat, text = lc.scan_unit(n, D, C)
    ref = lc.scan_reference(feat, text)
    mp, am = scan(feat, text)
    am = am.cpu().long()
    assert bool(((am >= 0) & (am < C)).all())
    ok = note("scan", "max_prob, unit rows", (mp.cpu().double() - ref.max).abs().max(), lc.SCAN_ATOL)
    assert note("scan", "probs[argmax], unit rows", (ref.probs[torch.arange(n), am] - ref.max).abs().max(), lc.SCAN_ATOL) and ok


def test_scan_wrapper_refuses_what_the_library_refuses():
    z = lambda *s: torch.zeros(*s, dtype=BF16, device="cuda")  # noqa: E731
    for feat, text in ((z(5, 12), z(3, 12)), (z(5, 0), z(3, 0)), (z(5, 64), z(0, 64)), (z(5, 64), z(257, 64)), (z(5, 64), z(3, 72))):
        with pytest.raises(RuntimeError):
            scan(feat, text)
    mp, am = scan(z(0, 64), z(3, 64))                                        # no rows: empty results, no launch
    assert mp.shape == (0,) and am.shape == (0,)


# =====================================================================================================================
# distillation head
# =====================================================================================================================
def check_head(name, c, ref, p, sums, grad, extra, feat=None):
    """p, sums and the gradient against the float64 reference, each in the bound of the dtype it is stored in"""
    ok = True
    if p is not None:
        assert p.shape == ref.p.shape
        perr = (p.detach().double().cpu() - ref.p).abs()
        if p.dtype == BF16:
            ok &= note("head bf16", f"{name} p err / bound", (perr / lc.bf16_bound(ref.p).clamp(min=1e-300)).max() if perr.numel() else 0, 1.0)
        else:
            ok &= note("head fp32", f"{name} p err / (atol + rtol |ref|)", (perr / (lc.P_ATOL + lc.P_RTOL * ref.p.abs())).max() if perr.numel() else 0, 1.0)
    group = "head bf16" if (grad.dtype == BF16 or (p is not None and p.dtype == BF16)) else "head fp32"
    if ref.sums is not None:
        s = sums.detach().double().cpu()
        assert float(s[2]) == float(ref.sums[2]), (s, ref.sums)
        for k in (0, 1):
            ok &= note(group, f"{name} sums[{k}]", abs(float(s[k]) - float(ref.sums[k])), lc.SUMS_RTOL * abs(float(ref.sums[k])))
    else:
        assert sums is None
    scale = lc.ill_conditioned_scale(c, extra, feat)
    assert bool(torch.isfinite(grad).all())
    if grad.dtype == BF16:
        bound = lc.bf16_bound(ref.grad)
        for r, sc in scale.items():
            bound[r] = lc.GRAD_ROW_RTOL * sc
        gerr = (grad.double().cpu() - ref.grad).abs()
        zero = bound == 0
        assert bool((gerr[zero] == 0).all())
        ok &= note("head bf16", f"{name} gradient err / bound", (gerr[~zero] / bound[~zero]).max() if int((~zero).sum()) else 0, 1.0)
    else:
        rel, zero_ok = lc.row_rel_err(grad, ref.grad, scale)
        assert zero_ok, f"{name}: a row whose reference gradient is exactly zero is not"
        ok &= note("head fp32", f"{name} gradient, worst row (row {int(rel.argmax()) if rel.numel() else -1})", rel.max() if rel.numel() else 0, lc.GRAD_ROW_RTOL)
    assert ok, name


def head_autograd(c, extra=True, with_target=True):
    """the training / evaluation path: SF.lang_head and torch autograd around it"""
    from scenesplat_amd import functional as SF
    f = c.feat.cuda().requires_grad_(True)
    try:
        p, sums = SF.lang_head(f, c.target.cuda() if with_target else None, c.mask.cuda() if with_target else None, True)
        terms = [lc.HEAD_C0 * sums[0], lc.HEAD_C1 * sums[1]] if with_target else []
        if extra:
            terms.append((p * c.w_extra.cuda()).sum())
        sum(terms).backward()
    finally:
        SF.lang_head_release()
    return p, sums, f.grad


def head_native(c, feat_dtype=F32, target_dtype=F32, dp_dtype=F32, normalize=True, p_dtype=F32, mask=None, with_target=True):
    """ss_lang_head_fwd / _bwd through native.py, with every operand in the dtype asked for"""
    from scenesplat_amd import native as nv
    feat = c.feat.to(feat_dtype).cuda()
    target = c.target.to(target_dtype).cuda() if with_target else None
    m = (c.mask if mask is None else mask).cuda() if with_target else None
    p, sums, rowstat = nv.lang_head_fwd(feat, target, m, normalize, want_p=True, p_dtype=p_dtype)
    coef = torch.tensor([lc.HEAD_C0, lc.HEAD_C1], device="cuda") if with_target else None
    dp = c.w_extra.to(dp_dtype).cuda() if dp_dtype is not None else None
    grad = nv.lang_head_bwd(feat, target, m, normalize, rowstat, coef, dp)
    assert p.dtype == p_dtype and grad.dtype == feat_dtype and rowstat.shape == (c.n, 4)
    return p, sums, grad


def rounded_reference(c, feat_dtype=F32, target_dtype=F32, dp_dtype=F32, normalize=True, mask=None, with_target=True):
    """the float64 reference on the operands as the kernel reads them"""
    return lc.head_reference(lc.rounded(c.feat, feat_dtype), lc.rounded(c.target, target_dtype) if with_target else None,
                             c.mask if mask is None else mask, lc.rounded(c.w_extra, dp_dtype) if dp_dtype is not None else None, normalize)


# IT and the last 256-piece: 4, 8, 252 -> 1 ragged | 256 -> 1 full | 260 -> 2 ragged | 512 -> 2 full | 516 -> 3 ragged | 1024 -> 4 full |
# 1028 -> 5 ragged | 1536 -> 6 full | 1792 -> 7 full | 2044 -> 8 ragged | 2048 -> 8 full
@pytest.mark.parametrize("C", lc.HEAD_WIDTHS)
def test_head_every_width_instance(C):
    c = lc.head_case(lc.HEAD_N, C)
    p, sums, grad = head_autograd(c)
    check_head(f"C={C} IT={lc.head_it(C)}", c, lc.head_case_reference(lc.HEAD_N, C), p, sums, grad, extra=True)


# blocks x rows per wave at C = 260 (IT 2): 1, 3 -> one block, waves without a row in its reduction | 4 -> one full block |
# 5 -> two blocks | 4096 -> 1024 blocks (the cap), one row per wave | 4097 -> one wave loops twice | 8195 -> every wave twice, three thrice
@pytest.mark.parametrize("n", lc.HEAD_ROWS)
def test_head_row_count_edges(n):
    c = lc.head_case(n, lc.HEAD_ROWS_C)
    p, sums, grad = head_autograd(c)
    check_head(f"n={n}", c, lc.head_case_reference(n, lc.HEAD_ROWS_C), p, sums, grad, extra=True)


def test_head_single_valid_row():
    """n = 1 without the special rows: three of the four waves contribute nothing to a non-zero sum"""
    c = lc.head_case(1, lc.HEAD_ROWS_C, True, False)
    p, sums, grad = head_autograd(c)
    ref = lc.head_case_reference(1, lc.HEAD_ROWS_C, True, False)
    assert float(ref.sums[2]) == 1 and float(ref.sums[0]) > 0
    check_head("n=1, valid", c, ref, p, sums, grad, extra=True)


def test_head_without_rows():
    from scenesplat_amd import functional as SF
    f = torch.zeros(0, 260, device="cuda", requires_grad=True)
    try:
        p, sums = SF.lang_head(f, torch.zeros(0, 260, device="cuda"), torch.zeros(0, dtype=torch.bool, device="cuda"), True)
        (sums[0] + sums[1] + p.sum()).backward()
    finally:
        SF.lang_head_release()
    assert sums.tolist() == [0.0, 0.0, 0.0] and p.shape == (0, 260) and f.grad.shape == (0, 260)


# C: 48 -> IT 1 ragged | 260 -> IT 2 ragged | 2048 -> IT 8 full
@pytest.mark.parametrize("dp_dtype", [None, F32, BF16], ids=lambda d: "dp-" + _dtn(d))
@pytest.mark.parametrize("target_dtype", [F32, BF16], ids=lambda d: "t-" + _dtn(d))
@pytest.mark.parametrize("feat_dtype", [F32, BF16], ids=lambda d: "f-" + _dtn(d))
@pytest.mark.parametrize("C", lc.HEAD_FORM_WIDTHS)
def test_head_operand_dtypes(C, feat_dtype, target_dtype, dp_dtype):
    """every mix of fp32 / bf16 features, targets and incoming gradient; the gradient comes back in the features' dtype"""
    c = lc.head_case(lc.HEAD_N, C)
    ref = rounded_reference(c, feat_dtype, target_dtype, dp_dtype)
    p, sums, grad = head_native(c, feat_dtype, target_dtype, dp_dtype)
    check_head(f"C={C} f={_dtn(feat_dtype)} t={_dtn(target_dtype)} dp={_dtn(dp_dtype)}", c, ref, p, sums, grad, extra=dp_dtype is not None,
               feat=lc.rounded(c.feat, feat_dtype))


@pytest.mark.parametrize("C", lc.HEAD_FORM_WIDTHS)   # IT 1, 2, 8
def test_head_bf16_p_output(C):
    c = lc.head_case(lc.HEAD_N, C)
    p, sums, grad = head_native(c, p_dtype=BF16)
    check_head(f"C={C} p=bf16", c, lc.head_case_reference(lc.HEAD_N, C), p, sums, grad, extra=True)


@pytest.mark.parametrize("dp_dtype", [None, F32], ids=lambda d: "dp-" + _dtn(d))
@pytest.mark.parametrize("C", lc.HEAD_FORM_WIDTHS)   # IT 1, 2, 8
def test_head_without_normalisation_on_non_unit_rows(C, dp_dtype):
    """the standalone criteria path: p = feat, row norms 0.5..1.5"""
    from scenesplat_amd import functional as SF
    c = lc.head_case(lc.HEAD_N, C, False)
    ref = lc.head_case_reference(lc.HEAD_N, C, False, extra=dp_dtype is not None)
    p, sums, grad = head_native(c, dp_dtype=dp_dtype, normalize=False)
    assert torch.equal(p.cpu(), c.feat)
    check_head(f"C={C} normalize=False dp={_dtn(dp_dtype)}", c, ref, p, sums, grad, extra=dp_dtype is not None)
    # the same through SF.lang_head_sums, as CosineSimilarity / L2Loss call it on a pred that no fused pass produced
    f, t, m = c.feat.cuda().requires_grad_(True), c.target.cuda(), c.mask.cuda()
    try:
        s2 = SF.lang_head_sums(f, t, m)
        assert SF.lang_head_sums(f, t, m) is s2                              # the second criterion reads the first one's pass
        (lc.HEAD_C0 * s2[0] + lc.HEAD_C1 * s2[1]).backward()
    finally:
        SF.lang_head_release()
    assert torch.equal(s2, sums)
    check_head(f"C={C} lang_head_sums", c, lc.head_case_reference(lc.HEAD_N, C, False, extra=False), None, s2, f.grad, extra=False)


@pytest.mark.parametrize("C", lc.HEAD_FORM_WIDTHS)   # IT 1, 2, 8
def test_head_evaluation_form_without_a_target(C):
    c = lc.head_case(lc.HEAD_N, C)
    p, sums, grad = head_autograd(c, with_target=False)
    check_head(f"C={C} target=None", c, lc.head_case_reference(lc.HEAD_N, C, with_target=False), p, sums, grad, extra=True)


@pytest.mark.parametrize("dp_dtype", [None, F32], ids=lambda d: "dp-" + _dtn(d))
@pytest.mark.parametrize("C", [260, 2048])           # IT 2 ragged, IT 8 full
def test_head_all_false_mask(C, dp_dtype):
    c = lc.head_case(lc.HEAD_N, C)
    none = torch.zeros(c.n, dtype=torch.bool)
    p, sums, grad = head_native(c, dp_dtype=dp_dtype, mask=none)
    assert sums.tolist() == [0.0, 0.0, 0.0]
    if dp_dtype is None:
        assert bool((grad == 0).all())
        return
    check_head(f"C={C} all-false mask", c, rounded_reference(c, mask=none), p, sums, grad, extra=True)
    _, _, alone = head_native(c, with_target=False)
    assert torch.equal(grad, alone)                                          # the dp_extra path alone, bit for bit


@pytest.mark.parametrize("C", [260, 2048])           # IT 2 ragged, IT 8 full
def test_head_all_true_mask(C):
    c = lc.head_case(lc.HEAD_N, C)
    every = torch.ones(c.n, dtype=torch.bool)
    p, sums, grad = head_native(c, mask=every)
    check_head(f"C={C} all-true mask", c, rounded_reference(c, mask=every), p, sums, grad, extra=True)


def test_head_mask_forms_select_the_same_rows():
    c = lc.head_case(lc.HEAD_N, 260)
    want = head_native(c)
    for name, m in (("uint8", lc.byte_mask(c.mask)), ("float", lc.float_mask(c.mask))):
        got = head_native(c, mask=m)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
    check_head("bool mask", c, lc.head_case_reference(lc.HEAD_N, 260), *want, extra=True)


def test_head_is_reproducible_bit_for_bit():
    """no atomics: per-wave partials, per-block partials and a one-block finish in a fixed order"""
    c = lc.head_case(4097, lc.HEAD_ROWS_C)
    a, b = head_native(c), head_native(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_head_row_under_the_cosine_eps_forward_only():
    """normalize=False and a row of norm 3e-9: the cosine clamps its norm at 1e-8.  The forward is compared; the gradient only has
    to be finite -- torch's own in that corner follows from how it happens to clamp and differs by about 2 % from the closed forms."""
    c = lc.head_case(lc.HEAD_N, 260, False, True, True)
    ref = lc.head_case_reference(lc.HEAD_N, 260, False, True, True)
    p, sums, grad = head_native(c, normalize=False)
    only = torch.zeros(c.n, dtype=torch.bool)
    only[7] = True
    ref1 = lc.head_reference(c.feat, c.target, only, c.w_extra, False)
    _, sums1, grad1 = head_native(c, normalize=False, mask=only)
    ok = True
    for name, s, r in (("all valid rows", sums, ref.sums), ("the tiny row alone", sums1, ref1.sums)):
        s = s.double().cpu()
        assert float(s[2]) == float(r[2])
        for k in (0, 1):
            ok &= note("head fp32", f"norm 3e-9, {name}: sums[{k}]", abs(float(s[k]) - float(r[k])), lc.SUMS_RTOL * abs(float(r[k])))
    assert ok and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(grad1).all())
    # every other row of the full case is an ordinary one
    rel, zero_ok = lc.row_rel_err(grad, ref.grad)
    rel[7] = 0
    assert zero_ok and note("head fp32", "norm 3e-9 case, gradient of the other rows", rel.max(), lc.GRAD_ROW_RTOL)


@pytest.mark.parametrize("C", lc.HEAD_FALLBACK_WIDTHS)                       # 6: C % 4 != 0 | 2052: C > 2048
def test_head_odd_widths_take_the_masked_torch_path_and_the_kernel_refuses_them(C):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import lang
    c = lc.head_case(lc.HEAD_N, C, False)
    ref = lc.head_case_reference(lc.HEAD_N, C, False, extra=False)
    f = c.feat.cuda().requires_grad_(True)
    sums = lang._head_sums(f, c.target.cuda(), c.mask.cuda())
    (lc.HEAD_C0 * sums[0] + lc.HEAD_C1 * sums[1]).backward()
    check_head(f"C={C} fallback", c, ref, None, sums, f.grad, extra=False)
    with pytest.raises(RuntimeError):
        nv.lang_head_fwd(c.feat.cuda(), c.target.cuda(), c.mask.cuda(), False)
    with pytest.raises(RuntimeError):
        nv.lang_head_fwd(torch.zeros(5, 0, device="cuda"), None, None, True)


# =====================================================================================================================
# AggregatedContrastiveLoss
# =====================================================================================================================
def contrastive(case, reduction="mean", schedule="all", epoch_progress=None):
    from scenesplat_amd.pointcept_api import build_criteria
    crit = build_criteria([dict(type="AggregatedContrastiveLoss", temperature=0.2, reduction=reduction, loss_weight=1.0,
                                schedule=schedule, max_classes=lc.CON_MAX_CLASSES, min_count=100)])
    pred = case.pred.cuda().requires_grad_(True)
    loss = crit(pred, None, valid_feat_mask=case.mask.cuda(), segment=case.seg.cuda(), epoch_progress=epoch_progress,
                rand_keys=case.keys.cuda())
    if loss.requires_grad:
        loss.backward()
    return loss.detach().cpu(), pred.grad


def check_contrastive(name, case, loss, grad, **kw):
    rl, rg = lc.contrastive_reference(case, **kw)
    ok = note("contrastive", f"{name} loss {float(loss):.6f} vs {float(rl):.6f}", abs(float(loss) - float(rl)), lc.CON_LOSS_ATOL)
    g = torch.zeros_like(rg) if grad is None else grad.double().cpu()
    ok &= note("contrastive", f"{name} gradient err / (atol + rtol |ref|)", ((g - rg).abs() / (lc.CON_GRAD_ATOL + lc.CON_GRAD_RTOL * rg.abs())).max(), 1.0)
    assert ok, name
    return rl, rg


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_contrastive_thresholds_and_splits(C, reduction):
    """classes of 99 | 100 | 101 | 200 | 201 valid rows, a masked-out class, rows labelled -1, label max_classes - 1, equal keys"""
    case = lc.contrastive_case(C)
    loss, grad = contrastive(case, reduction)
    rl, rg = check_contrastive(f"C={C} {reduction}", case, loss, grad, reduction=reduction)
    out = ~(case.mask & torch.isin(case.seg, torch.tensor(lc.CON_QUALIFY)))
    assert float(rl) > 0.01 and bool((grad.cpu()[out] == 0).all())          # rows of no qualifying class: exactly no gradient


@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_contrastive_without_a_qualifying_class(C):
    loss, grad = contrastive(lc.contrastive_case(C, "none"))
    assert float(loss) == 0.0 and (grad is None or bool((grad == 0).all()))


@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_contrastive_with_one_qualifying_class(C):
    case = lc.contrastive_case(C, "one")
    loss, grad = contrastive(case)
    rl, _ = check_contrastive(f"C={C} one class", case, loss, grad)
    assert float(rl) == 0.0


@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_contrastive_schedule_gate(C):
    case = lc.contrastive_case(C)
    loss, grad = contrastive(case, schedule="last_75", epoch_progress=0.25)               # 0.25 <= 1 - 0.75: still off
    assert float(loss) == 0.0 and grad is None
    loss, grad = contrastive(case, schedule="last_75", epoch_progress=0.25 + 1e-6)
    rl, _ = check_contrastive(f"C={C} last_75 on", case, loss, grad, schedule="last_75", epoch_progress=0.25 + 1e-6)
    assert float(rl) > 0.01
