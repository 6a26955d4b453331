"""CPU-side pin of tests/test_hip_lang_edges.py: the exact-logit construction of the scan cases, the margin between torch's own
fp32 and the bounds the GPU tests hold the head and the contrastive loss to, the properties the case builders promise, and the
argument contract of ss_feat_text_scan / ss_lang_head_fwd / ss_lang_head_bwd on the paths that return before any launch.
No GPU needed."""
import ctypes
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lang_cases as lc  # noqa: E402
from lang_cases import BF16, F32, F64  # noqa: E402

SS_OK, SS_ERR_ARG = 0, 1
SS_F32, SS_BF16 = 0, 1


# =====================================================================================================================
# scan: the exact inputs
# =====================================================================================================================
@pytest.mark.parametrize("D,C", [(768, 256), (72, 33), (8, 1)])
def test_exact_scan_inputs_are_exact_in_every_accumulation_order(D, C):
    """entries k/8, |k| <= 2: bf16 holds them exactly, every product is a multiple of 2^-6 and |sum| <= D/16 <= 48, so fp32 adds
    of them never round: the float32 matmul equals the float64 one bit for bit, and so does a reversed-order one"""
    feat, text = lc.scan_exact(1000, D, C)
    for t in (feat, text):
        assert t.dtype == BF16 and torch.equal(t.double() * 8, (t.double() * 8).round()) and float(t.double().abs().max()) <= 0.25
        assert torch.equal(t.float().to(BF16), t)
    ref = lc.scan_reference(feat, text)
    assert torch.equal((feat.float() @ text.float().t()).double(), ref.logits)
    assert torch.equal((feat.float().flip(1) @ text.float().flip(1).t()).double(), ref.logits)
    assert torch.equal(ref.logits * 64, (ref.logits * 64).round()) and float(ref.logits.abs().max()) <= D / 16
    print(f"    D={D} C={C}: {int(ref.ties.sum())} of 1000 rows have a tied maximum")
    if C > 1:
        assert int(ref.ties.sum()) > 0


def test_scan_cases_reach_every_tile_count_and_hold_tied_rows():
    assert {lc.scan_tile_count(C) for C in lc.SCAN_CLASSES} == set(lc.SCAN_TILES)
    assert {lc.scan_tile_count(C) for C in lc.SCAN_UNIT_CLASSES} == {4, 8, 16}
    assert [lc.scan_tile_count(C) for C in (1, 32, 33, 64, 65, 112, 113, 128, 129, 160, 161, 208, 209, 256)] == \
        [2, 2, 4, 4, 7, 7, 8, 8, 10, 10, 13, 13, 16, 16]
    tied = {(D, C): int(lc.scan_exact_reference(lc.SCAN_N, D, C).ties.sum()) for D in lc.SCAN_DIMS for C in lc.SCAN_CLASSES}
    print("    tied rows of", lc.SCAN_N, "by (D, C):", tied)
    # the tie rule is exercised in every instance: some C of every tile count has a tied row at one of the widths
    for nt in lc.SCAN_TILES:
        assert sum(v for (D, C), v in tied.items() if lc.scan_tile_count(C) == nt and C > 1) > 0, nt


def test_scan_reference_takes_the_lowest_class_among_equal_maxima():
    feat = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]]).to(BF16)
    text = torch.tensor([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [0.0, 1.0]]).to(BF16)
    ref = lc.scan_reference(feat, text)
    assert ref.argmax.tolist() == [1, 0, 0] and ref.ties.tolist() == [True, True, True]
    assert torch.equal(ref.max, torch.sigmoid(torch.tensor([1.0, 1.0, -1.0], dtype=F64)))


def test_guard_cases_do_what_they_claim():
    for n, C, D in lc.SCAN_NEGATIVE:
        ref = lc.scan_exact_reference(n, D, C, "negative")
        assert float(ref.logits.max()) <= -D / 64 < 0                  # a padded lane's logit 0 would beat every class
    ref = lc.scan_exact_reference(129, 72, 33, "same-text")
    assert bool((ref.argmax == 0).all()) and bool(ref.ties.all())
    idx = lc.scan_injection(300, 500, 3)
    assert idx.dtype == torch.int32 and len(idx.unique()) == 300 and int(idx.max()) < 500


# =====================================================================================================================
# scan and head: argument errors of the library (every call returns before a launch)
# =====================================================================================================================
@pytest.fixture(scope="module")
def lib():
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    """a non-null host address for arguments that only have to be present: never dereferenced on the paths under test"""
    store = (ctypes.c_float * 64)()
    p = ctypes.cast(store, ctypes.c_void_p)
    p._keep = store
    return p


def scan_call(lib, buf, n=5, D=64, C=20, max_prob=True, argmax=True):
    return lib.ss_feat_text_scan(buf, buf, n, D, C, buf if max_prob else None, buf if argmax else None, None, None, None)


def test_scan_refuses_bad_arguments(lib, buf):
    for over in (dict(D=12), dict(D=7), dict(D=0), dict(D=-8), dict(C=0), dict(C=257), dict(n=-1), dict(argmax=False),
                 dict(max_prob=False)):
        assert scan_call(lib, buf, **over) == SS_ERR_ARG, over
        assert scan_call(lib, buf, **dict(over, n=over.get("n", 0))) == SS_ERR_ARG, over      # also without rows
    for C in (1, 256):
        assert scan_call(lib, buf, n=0, C=C, D=8) == SS_OK                                    # n = 0: no launch
    assert scan_call(lib, buf, n=0, max_prob=False, argmax=False) == SS_OK


def head_fwd_call(lib, buf, n=5, C=48, feat=True, target=True, mask=True, sums=True):
    return lib.ss_lang_head_fwd(buf if feat else None, SS_F32, buf if target else None, SS_F32, buf if mask else None, 1, None, SS_F32,
                                buf, buf, buf if sums else None, n, C, None)


def head_bwd_call(lib, buf, n=5, C=48, feat=True, target=True, mask=True, sums=True):
    return lib.ss_lang_head_bwd(buf if feat else None, SS_F32, buf if target else None, SS_F32, buf if mask else None, 1, buf, buf,
                                None, SS_F32, buf, SS_F32, n, C, None)


@pytest.mark.parametrize("call", [head_fwd_call, head_bwd_call], ids=["fwd", "bwd"])
def test_head_refuses_bad_arguments(lib, buf, call):
    for over in (dict(C=0), dict(C=6), dict(C=2052), dict(C=-4), dict(n=-1), dict(feat=False), dict(mask=False)):
        assert call(lib, buf, **over) == SS_ERR_ARG, over
    for C in (0, 6, 2052):                                   # the width is refused without rows as well
        assert call(lib, buf, n=0, C=C) == SS_ERR_ARG, C
    # n = 0 is a no-op, also with the null data pointers empty tensors have (sums = NULL here: nothing to clear, no GPU call)
    for C in (4, 2048):
        assert call(lib, buf, n=0, C=C, feat=False, target=False, mask=False, sums=False) == SS_OK
    assert lib.ss_lang_head_blocks(0) == 1 and lib.ss_lang_head_blocks(4096) == 1024 and lib.ss_lang_head_blocks(4097) == 1024
    assert lib.ss_lang_head_blocks(5) == 2


# =====================================================================================================================
# head: the case builders and the margin of the fp32 bounds
# =====================================================================================================================
def test_head_widths_reach_every_instance_full_and_ragged():
    its = {}
    for C in lc.HEAD_WIDTHS:
        its.setdefault(lc.head_it(C), set()).add("full" if C % 256 == 0 else "ragged")
    assert sorted(its) == list(range(1, 9))
    assert {it for it, forms in its.items() if "ragged" in forms} >= {1, 2, 3, 5, 8} and its[1] == its[2] == its[8] == {"full", "ragged"}
    assert [lc.head_it(C) for C in lc.HEAD_FORM_WIDTHS] == [1, 2, 8]


@pytest.mark.parametrize("n,C,normalize,specials", [(37, 260, True, True), (37, 48, False, True), (1, 260, True, True),
                                                    (8195, 260, True, True), (1, 260, True, False)])
def test_head_cases_hold_what_they_promise(n, C, normalize, specials):
    c = lc.head_case(n, C, normalize, specials)
    norms = c.feat.double().norm(dim=1)
    if specials:
        assert bool((c.feat[c.zero_feat] == 0).all()) and bool((c.target[c.zero_target] == 0).all()) and not bool(c.mask[c.masked])
        if n >= 3:
            assert bool(c.mask[c.zero_feat]) and bool(c.mask[c.zero_target]) and len({c.zero_feat, c.zero_target, c.masked}) == 3
        norms = norms[norms > 0]
    lo, hi = (1e-3, 1e3) if normalize else (0.5, 1.5)
    assert bool(((norms > lo * (1 - 1e-6)) & (norms < hi * (1 + 1e-6))).all())
    if n >= 1000:
        assert float(norms.min()) < 10 * lo and float(norms.max()) > hi / 10 if normalize else float(norms.max() - norms.min()) > 0.9
        assert 0.65 < float(c.mask.float().mean()) < 0.75
        usual = torch.arange(n) != c.zero_target                       # the zero-target row's w_extra is ~ randn (lang_cases.head_case)
        assert 0.9e-3 < float(c.w_extra[usual].std()) < 1.1e-3 and 0.8 < float(c.w_extra[c.zero_target].std()) < 1.2
    tn = c.target.double().norm(dim=1)
    assert bool(((tn - 1).abs() < 1e-6)[tn > 0].all())


@pytest.mark.parametrize("case", lc.HEAD_F32_CASES, ids=lambda c: "n%d-C%d-%s%s" % (c[0], c[1], "norm" if c[2] else "raw", "" if c[3] else "-plain"))
def test_torch_fp32_stays_under_a_quarter_of_the_head_bounds(case):
    """the reference's own rounding: torch autograd in float32 on the CPU against float64, on the inputs the GPU tests use"""
    n, C, normalize, specials = case
    c = lc.head_case(n, C, normalize, specials)
    ref = lc.head_case_reference(n, C, normalize, specials)
    got = lc.head_reference(c.feat, c.target, c.mask, c.w_extra, normalize, dtype=F32)
    rel, zero_ok = lc.row_rel_err(got.grad, ref.grad)
    serr = ((got.sums.double() - ref.sums).abs() / ref.sums.abs().clamp(min=1e-300))[:2]
    print(f"    n={n} C={C}: fp32 CPU worst per-row gradient error {rel.max().item():.2e} (bar / 4 = {lc.GRAD_ROW_RTOL / 4:.1e}), "
          f"sums {serr.max().item():.2e} (bar / 4 = {lc.SUMS_RTOL / 4:.1e})")
    assert zero_ok and float(rel.max()) <= lc.GRAD_ROW_RTOL / 4
    assert bool((serr <= lc.SUMS_RTOL / 4).all()) and float(got.sums[2]) == float(ref.sums[2]) == float(c.mask.sum())
    assert bool(((got.p.double() - ref.p).abs() <= (lc.P_ATOL + lc.P_RTOL * ref.p.abs()) / 4).all())
    # masked-out rows get a gradient only through w_extra; the zero rows carry the 1e12 / 1e20 scale factors and stay finite
    assert bool(torch.isfinite(ref.grad).all()) and bool(torch.isfinite(got.grad).all())
    if specials and n >= 3 and normalize:
        assert float(ref.grad[c.zero_feat].abs().max()) > 1e17


@pytest.mark.parametrize("C", lc.HEAD_FORM_WIDTHS)
def test_torch_fp32_without_an_extra_gradient_and_the_ill_conditioned_row(C):
    """no gradient arrives at p: the zero-target row's exact gradient is 0 and float64 returns rounding noise there, so its own
    norm is no yardstick; against what cancels (ill_conditioned_scale) torch's fp32 stays under a quarter of the bar like the rest"""
    c = lc.head_case(lc.HEAD_N, C)
    ref = lc.head_case_reference(lc.HEAD_N, C, extra=False)
    got = lc.head_reference(c.feat, c.target, c.mask, None, True, dtype=F32)
    scale = lc.ill_conditioned_scale(c, extra=False)
    assert list(scale) == [c.zero_target] and lc.ill_conditioned_scale(c, extra=True) == {}
    assert float(ref.grad[c.zero_target].norm()) < 1e-12 * scale[c.zero_target]          # float64: noise around an exact 0
    rel, zero_ok = lc.row_rel_err(got.grad, ref.grad, scale)
    print(f"    C={C}: fp32 CPU worst per-row gradient error {rel.max().item():.2e}, the zero-target row {rel[c.zero_target].item():.2e} "
          f"(bar / 4 = {lc.GRAD_ROW_RTOL / 4:.1e})")
    assert zero_ok and float(rel.max()) <= lc.GRAD_ROW_RTOL / 4
    assert bool((ref.grad[~c.mask] == 0).all()) and int((~c.mask).sum()) >= 1                 # masked-out rows: exactly zero
    # the evaluation form (no target, gradient from w_extra alone)
    ref = lc.head_case_reference(lc.HEAD_N, C, with_target=False)
    got = lc.head_reference(c.feat, None, None, c.w_extra, True, dtype=F32)
    rel, zero_ok = lc.row_rel_err(got.grad, ref.grad)
    assert zero_ok and float(rel.max()) <= lc.GRAD_ROW_RTOL / 4 and ref.sums is None


def test_head_reference_restates_the_oracle_losses():
    """sums of head_reference are the oracle's sum-reduced losses; the gradient is that of the weighted total"""
    from oracle import losses as olosses
    c = lc.head_case(37, 48)
    ref = lc.head_case_reference(37, 48)
    f = c.feat.double().requires_grad_(True)
    p = torch.nn.functional.normalize(f, p=2, dim=1)
    s0 = olosses.cosine_similarity_loss(p, c.target.double(), c.mask, reduction="sum")
    s1 = olosses.l2_loss(p, c.target.double(), c.mask, reduction="sum")
    (lc.HEAD_C0 * s0 + lc.HEAD_C1 * s1 + (p * c.w_extra.double()).sum()).backward()
    assert torch.allclose(ref.sums[:2], torch.stack([s0, s1]).detach(), rtol=1e-14, atol=0) and float(ref.sums[2]) == float(c.mask.sum())
    assert torch.allclose(ref.grad, f.grad, rtol=1e-12, atol=0) and torch.equal(ref.p, p.detach())
    # the mask forms select the same rows
    assert torch.equal(lc.float_mask(c.mask) > 0, c.mask) and torch.equal(lc.byte_mask(c.mask).bool(), c.mask)
    assert set(lc.byte_mask(c.mask).tolist()) == {0, 1, 200} and float(lc.float_mask(c.mask).min()) < -0.5


def test_bf16_bound_admits_one_rounding_and_no_value_two_steps_off():
    """storing the float64 reference in bf16 is inside bf16_bound; the bf16 two steps further from zero (>= 1.5 ulp >= 1.5 * 2^-8
    |ref| off) is outside for every element that is not small against its row"""
    ref = lc.head_case_reference(37, 260).grad
    once = ref.float().to(BF16)
    assert bool(((once.double() - ref).abs() <= lc.bf16_bound(ref)).all())
    big = ref.abs() > 0.5 * ref.abs().amax(dim=1, keepdim=True)
    off = (once.view(torch.int16) + 2).view(BF16)
    assert bool(((off.double() - ref).abs() > lc.bf16_bound(ref))[big].all()) and int(big.sum()) > 37


def test_tiny_norm_row_sits_under_the_cosine_eps():
    c = lc.head_case(37, 260, False, True, True)
    nrm = float(c.feat[7].double().norm())
    assert 2.9e-9 < nrm < 3.1e-9 and bool(c.mask[7])
    # with the clamp the row's cosine is 0.3 of the unclamped one: dropping the eps would move sums[0] by far more than its bound
    ref = lc.head_case_reference(37, 260, False, True, True)
    cos = float((c.feat[7].double() * c.target[7].double()).sum()) / nrm
    assert abs(cos * (1 - nrm / 1e-8)) > 100 * lc.SUMS_RTOL * float(ref.sums[0])


# =====================================================================================================================
# contrastive loss
# =====================================================================================================================
def _valid_counts(case):
    v = case.mask & (case.seg != -1)
    return {int(l): int((v & (case.seg == l)).sum()) for l in case.seg.unique() if l >= 0}


@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_contrastive_case_holds_what_it_promises(C):
    case = lc.contrastive_case(C)
    cnt = _valid_counts(case)
    assert cnt == {3: 99, 0: 100, 7: 101, 12: 200, 255: 201, 5: 0}
    assert int((case.seg == 5).sum()) >= 100 and int((case.seg == 3).sum()) >= 100          # large enough before the mask
    assert int((case.seg == -1).sum()) == lc.CON_UNLABELLED and int(case.seg.max()) == lc.CON_MAX_CLASSES - 1
    assert bool(((case.pred.double().norm(dim=1) - 1).abs() < 1e-6).all())
    for lab in (7, 12):                                                                       # equal keys inside a class
        k = case.keys[case.mask & (case.seg == lab)]
        assert len(k.unique()) <= 16 < len(k)
    # letting the 99-row class in changes the loss by far more than the tolerance
    l100, _ = lc.contrastive_reference(case)
    l99, _ = lc.contrastive_reference(case, min_count=99)
    print(f"    C={C}: loss {l100.item():.6f}; with the 99-row class let in {l99.item():.6f}")
    assert abs(float(l99 - l100)) > 1000 * lc.CON_LOSS_ATOL
    # ... and so does moving the n // 2 split of the odd classes by one row (keys reversed: the halves swap, 50|51 becomes 51|50)
    rev = types.SimpleNamespace(pred=case.pred, mask=case.mask, seg=case.seg, keys=1 - case.keys)
    lrev, _ = lc.contrastive_reference(rev)
    assert abs(float(lrev - l100)) > 10 * lc.CON_LOSS_ATOL
    assert _valid_counts(lc.contrastive_case(C, "none")) == {3: 99, 0: 60, 12: 1, 5: 0}
    assert _valid_counts(lc.contrastive_case(C, "one")) == {3: 99, 7: 101, 0: 60, 5: 0}


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_oracle_fp32_stays_under_a_quarter_of_the_contrastive_bounds(C, reduction):
    case = lc.contrastive_case(C)
    l64, g64 = lc.contrastive_reference(case, F64, reduction)
    l32, g32 = lc.contrastive_reference(case, F32, reduction)
    gerr = (g32.double() - g64).abs()
    room = (lc.CON_GRAD_ATOL + lc.CON_GRAD_RTOL * g64.abs()) / 4
    print(f"    C={C} {reduction}: fp32 oracle loss error {abs(float(l32) - float(l64)):.2e} (bar / 4 = {lc.CON_LOSS_ATOL / 4:.1e}), "
          f"gradient worst err / (bar / 4) = {(gerr / room).max().item():.3g}")
    assert abs(float(l32) - float(l64)) <= lc.CON_LOSS_ATOL / 4 and bool((gerr <= room).all())
    assert float(l64) > 0.01 and float(g64.abs().max()) > 1e-4
    # rows outside every qualifying class get no gradient
    out = ~(case.mask & torch.isin(case.seg, torch.tensor(lc.CON_QUALIFY)))
    assert bool((g64[out] == 0).all()) and bool((g64[~out].abs().sum(1) > 0).all())


@pytest.mark.parametrize("C", lc.CON_WIDTHS)
def test_oracle_on_the_degenerate_outcomes(C):
    for which in ("none", "one"):
        loss, grad = lc.contrastive_reference(lc.contrastive_case(C, which))
        assert float(loss) == 0.0, which                        # no class: the early return; one class: 1 x 1 logits, lse == diagonal
        assert float(grad.abs().max()) <= lc.CON_GRAD_ATOL / 4, which
    case = lc.contrastive_case(C)
    off, _ = lc.contrastive_reference(case, schedule="last_75", epoch_progress=0.25)
    on, _ = lc.contrastive_reference(case, schedule="last_75", epoch_progress=0.25 + 1e-6)
    assert float(off) == 0.0 and float(on) == float(lc.contrastive_reference(case)[0]) > 0
