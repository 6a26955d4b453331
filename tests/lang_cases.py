"""Inputs, references and bounds shared by tests/test_hip_lang_edges.py (GPU) and tests/test_lang_host.py (CPU): the open-vocabulary
scan (csrc/scan.hip), the distillation head (csrc/head.hip) and AggregatedContrastiveLoss (pointcept_api/lang.py).  Everything is
built on the CPU from seeded generators and cached; the references are torch / numpy in float64 and call nothing of the library
under test."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as olosses

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# =====================================================================================================================
# open-vocabulary scan
# =====================================================================================================================
SCAN_TILES = (2, 4, 7, 8, 10, 13, 16)         # the k_feat_text_scan<NT> instances ss_feat_text_scan dispatches to
SCAN_ATOL = 2e-4                              # the bar of test_open_vocab_scan_against_reference_math on every probability
# one below, at and above every boundary of the dispatch (16 NT classes per instance); the instance each lands in:
#   1, 16, 17, 32 -> NT 2 | 33, 64 -> NT 4 | 65, 112 -> NT 7 | 113, 128 -> NT 8 | 129, 160 -> NT 10 | 161, 208 -> NT 13 |
#   209, 255, 256 -> NT 16 (the 96 KB-LDS instance)
SCAN_CLASSES = (1, 16, 17, 32, 33, 64, 65, 112, 113, 128, 129, 160, 161, 208, 209, 255, 256)
SCAN_N, SCAN_DIMS = 300, (72, 768)            # 300 rows = 2 full workgroups of 128 + 44; 72 = 64 + 8: the k < D guard decides
SCAN_ROW_EDGES = [(n, C, 40) for n in (1, 127, 128, 129) for C in (17, 256)]       # (n, C, D): around one workgroup of 128 rows
SCAN_WIDTH_EDGES = [(129, 33, D) for D in (8, 40, 64)]                             # one partial / one full 64-wide k step
SCAN_NEGATIVE = [(129, C, 72) for C in (1, 17, 209)]                               # NT 2, 2, 16
SCAN_UNIT_CLASSES = (40, 120, 256)            # NT 4, 8, 16 on the random unit rows of the existing test


def scan_tile_count(C):
    """NT of the instance ss_feat_text_scan launches for C classes"""
    nt = (C + 15) // 16
    return next(t for t in SCAN_TILES if nt <= t)


def _eighths(shape, lo, hi, g):
    """entries k / 8 with k uniform in [lo, hi]: exact in bf16, products multiples of 2^-6"""
    return (torch.randint(lo, hi + 1, shape, generator=g).float() / 8).to(BF16)


@functools.lru_cache(maxsize=None)
def scan_exact(n, D, C, kind="any"):
    """-> (feat (n, D) bf16, text (C, D) bf16) whose logits every fp32 accumulation order computes exactly.
    'any': entries of both in {-2..2}/8.  'negative': feat in {1, 2}/8, text in {-2, -1}/8, every logit <= -D/64 < 0 -- a padded
    class or row (logit 0) would win the max.  'same-text': every text row equal, every row a C-way tie -> argmax 0."""
    g = torch.Generator().manual_seed(1_000_003 * D + 1009 * C + n + {"any": 0, "negative": 1, "same-text": 2}[kind])
    if kind == "negative":
        return _eighths((n, D), 1, 2, g), _eighths((C, D), -2, -1, g)
    feat = _eighths((n, D), -2, 2, g)
    text = _eighths((1, D), -2, 2, g).expand(C, D).contiguous() if kind == "same-text" else _eighths((C, D), -2, 2, g)
    return feat, text


@functools.lru_cache(maxsize=None)
def scan_unit(n, D, C):
    """the inputs of test_open_vocab_scan_against_reference_math: random unit rows rounded to bf16"""
    g = torch.Generator().manual_seed(C)
    feat = F.normalize(torch.randn(n, D, generator=g), dim=1).to(BF16)
    text = F.normalize(torch.randn(C, D, generator=g), dim=1).to(BF16)
    return feat, text


def scan_reference(feat, text):
    """sigmoid(feat.double() @ text.double().T) on the bf16-rounded operands -> namespace(logits, probs (n, C) f64, max (n) f64,
    argmax (n) int64, ties (n) bool).  argmax is numpy.argmax of the float64 logits: the FIRST occurrence of the maximum, i.e. the
    lowest class among equal maxima (the sigmoid is monotone, so this is the argmax of the probabilities wherever they differ)."""
    assert feat.dtype == BF16 and text.dtype == BF16
    logits = feat.double() @ text.double().t()
    probs = torch.sigmoid(logits)
    lg = logits.numpy()
    arg = np.argmax(lg, axis=1)
    ties = (lg == lg.max(axis=1, keepdims=True)).sum(axis=1) > 1
    return types.SimpleNamespace(logits=logits, probs=probs, max=torch.from_numpy(lg.max(axis=1)).sigmoid(),
                                 argmax=torch.from_numpy(arg), ties=torch.from_numpy(ties))


@functools.lru_cache(maxsize=None)
def scan_exact_reference(n, D, C, kind="any"):
    return scan_reference(*scan_exact(n, D, C, kind))


def scan_injection(n, rows, seed):
    """(n) int32: distinct destination rows in a buffer of `rows` >= n rows, in random order"""
    return torch.randperm(rows, generator=torch.Generator().manual_seed(seed))[:n].to(torch.int32)


# =====================================================================================================================
# distillation head
# =====================================================================================================================
HEAD_C0, HEAD_C1 = 0.7, 1.3                   # dL/dsums[0], dL/dsums[1] of every head test
# IT = ceil(C / 256) selects k_head_fwd<IT> / k_head_bwd<IT>; 'ragged' = the last 256-piece is partial (lanes with j >= C idle):
#   4, 8, 252 -> IT 1 ragged | 256 -> IT 1 full | 260 -> IT 2 ragged | 512 -> IT 2 full | 516 -> IT 3 ragged | 1024 -> IT 4 full |
#   1028 -> IT 5 ragged | 1536 -> IT 6 full | 1792 -> IT 7 full | 2044 -> IT 8 ragged | 2048 -> IT 8 full
HEAD_WIDTHS = (4, 8, 252, 256, 260, 512, 516, 1024, 1028, 1536, 1792, 2044, 2048)
HEAD_N = 37                                   # 10 blocks of 4 waves, the last with one row
# rows at C = 260: 1, 3 -> waves of the only block without a row | 4, 5 -> one full block (+ 1 row) | 4096 -> the 1024-block cap,
# every wave one row | 4097, 8195 -> the grid-stride loop runs a second (third) time in some waves
HEAD_ROWS = (1, 3, 4, 5, 4096, 4097, 8195)
HEAD_ROWS_C = 260
HEAD_FORM_WIDTHS = (48, 260, 2048)            # IT 1 ragged, 2 ragged, 8 full
HEAD_FALLBACK_WIDTHS = (6, 2052)              # C % 4 != 0, C > 2048: _head_sums' masked PyTorch-ROCm path

P_ATOL, P_RTOL = 2e-7, 1e-6                   # p in fp32            } the bars of test_fused_head_matches_oracle
SUMS_RTOL = 3e-6                              # sums[0], sums[1]     }
GRAD_ROW_RTOL = 1e-5                          # |row - ref row|_2 / |ref row|_2 of the fp32 gradient
HALF_ULP_BF16 = 2.0 ** -8                     # one round-to-nearest-even bf16 rounding


def head_it(C):
    return (C + 255) // 256


# every (n, C, normalize, specials) whose fp32 gradient the GPU tests hold to GRAD_ROW_RTOL; test_lang_host.py shows torch's own
# fp32 on the CPU stays under a quarter of that bar on each
HEAD_F32_CASES = sorted({(HEAD_N, C, True, True) for C in HEAD_WIDTHS + HEAD_FORM_WIDTHS}
                        | {(n, HEAD_ROWS_C, True, True) for n in HEAD_ROWS} | {(1, HEAD_ROWS_C, True, False)}
                        | {(HEAD_N, C, False, True) for C in HEAD_FORM_WIDTHS})


@functools.lru_cache(maxsize=None)
def head_case(n, C, normalize=True, specials=True, tiny_row=False):
    """-> namespace(feat, target (n, C) f32, mask (n) bool, w_extra (n, C) f32, zero_feat / zero_target / masked rows or None).
    normalize=True: feature row norms log-uniform over 1e-3..1e3; False (the standalone criteria path): norms uniform over 0.5..1.5.
    Targets are unit rows, about 70 % of the mask is true, w_extra ~ 1e-3 randn.  specials: the last row is exactly zero in feat,
    row n // 2 exactly zero in target (both valid when n >= 3) and row 0 is masked out; with n < 3 the rows coincide.
    A zero target leaves d p = 2 c1 p + w_extra: the first part is radial and the normalisation's backward projects it out, so with
    w_extra ~ 1e-3 the row's gradient would be what is left of a cancellation in ANY fp32 evaluation (torch's own is 7e-6 off
    there).  The row's w_extra is therefore ~ randn; without w_extra its exact gradient is 0, see ill_conditioned_scale().
    tiny_row (normalize=False only): row 7 is rescaled to norm 3e-9, under the cosine's eps of 1e-8."""
    g = torch.Generator().manual_seed(65537 * C + 31 * n + (0 if normalize else 7))
    d = F.normalize(torch.randn(n, C, generator=g, dtype=F64), dim=1)
    u = torch.rand(n, 1, generator=g, dtype=F64)
    norms = 10.0 ** (6 * u - 3) if normalize else 0.5 + u
    feat = (d * norms).float()
    target = F.normalize(torch.randn(n, C, generator=g, dtype=F64), dim=1).float()
    mask = torch.rand(n, generator=g) < 0.7
    w_extra = 1e-3 * torch.randn(n, C, generator=g)
    zf = zt = mo = None
    if not specials:
        mask[0] = True                                         # the plain form exists for n = 1 with a valid row
    if specials:
        zf, zt, mo = n - 1, n // 2, 0
        mask[zf] = mask[zt] = True
        mask[mo] = False
        feat[zf] = 0
        target[zt] = 0
        w_extra[zt] = torch.randn(C, generator=g)              # see below: unit scale keeps this row's gradient well conditioned
    if tiny_row:
        assert not normalize and n > 7
        feat[7] = (d[7] * 3e-9).float()
        mask[7] = True
    return types.SimpleNamespace(n=n, C=C, normalize=normalize, feat=feat, target=target, mask=mask, w_extra=w_extra,
                                 zero_feat=zf, zero_target=zt, masked=mo)


def rounded(t, dtype):
    """t as the kernel reads it when handed over in `dtype`: rounded once, widened exactly"""
    return None if t is None else t.to(dtype).float()


def head_reference(feat, target, mask, w_extra, normalize, dtype=F64):
    """torch autograd on the CPU in `dtype` over what the reference project calls: F.normalize(f, p=2, dim=1) (skipped when not
    normalize), 1 - F.cosine_similarity(p[m], t[m], dim=1) and ((p[m] - t[m]) ** 2).sum(1) summed over the valid rows m, plus
    (p * w_extra).sum() for the gradient arriving at p.  L = HEAD_C0 * sums[0] + HEAD_C1 * sums[1] + (p * w_extra).sum().
    -> namespace(p (n, C), sums (3) [cos, l2, #valid] or None without a target, grad (n, C) = dL/dfeat), all in `dtype`."""
    f = feat.to(dtype).clone().requires_grad_(True)
    p = F.normalize(f, p=2, dim=1) if normalize else f
    terms, sums = [], None
    if target is not None:
        m = mask.bool() if mask.dtype in (torch.bool, torch.uint8) else mask > 0
        t = target.to(dtype)
        s0 = (1 - F.cosine_similarity(p[m], t[m], dim=1)).sum()
        s1 = ((p[m] - t[m]) ** 2).sum(1).sum()
        terms += [HEAD_C0 * s0, HEAD_C1 * s1]
        sums = torch.stack([s0.detach(), s1.detach(), m.sum().to(dtype)])
    if w_extra is not None:
        terms.append((p * w_extra.to(dtype)).sum())
    sum(terms).backward()
    return types.SimpleNamespace(p=p.detach(), sums=sums, grad=f.grad)


@functools.lru_cache(maxsize=None)
def head_case_reference(n, C, normalize=True, specials=True, tiny_row=False, extra=True, with_target=True):
    c = head_case(n, C, normalize, specials, tiny_row)
    return head_reference(c.feat, c.target if with_target else None, c.mask, c.w_extra if extra else None, normalize)


def ill_conditioned_scale(case, extra, feat=None):
    """{row: scale}: with normalize and no gradient arriving at p, the zero-target row's d p = 2 c1 p is radial and its exact
    gradient s (d p - p (p . d p)) is 0 -- every evaluation (float64 included) returns the rounding of that cancellation.  The row
    is held to GRAD_ROW_RTOL of what cancels, s |d p| = 2 c1 / |f|, instead of its own (meaningless) norm."""
    if extra or not case.normalize or case.zero_target is None or not bool(case.mask[case.zero_target]):
        return {}
    nf = float((case.feat if feat is None else feat)[case.zero_target].double().norm())
    return {case.zero_target: 2 * HEAD_C1 / nf} if nf > 0 else {}


def row_rel_err(got, ref, scale=None):
    """-> (rel (n) f64, zero_ok bool): |row - ref row|_2 / |ref row|_2 for every row whose reference is not exactly zero (0 for the
    others), and whether every row whose reference IS exactly zero is exactly zero in `got`.  scale {row: s}: those rows are divided
    by s instead (ill_conditioned_scale)."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.norm(dim=1)
    for r, s in (scale or {}).items():
        den[r] = s
    zero = den == 0
    rel = torch.where(zero, torch.zeros_like(den), (got - ref).norm(dim=1) / den.clamp(min=1e-300))
    return rel, bool((got[zero] == 0).all())


def bf16_bound(ref):
    """a value stored in bf16 lies within one rounding of the reference: 2^-8 |ref| for the rounding itself, 1e-5 max|ref row| for
    the fp32 arithmetic in front of it (GRAD_ROW_RTOL of the row's largest element)"""
    ref = ref.double()
    return HALF_ULP_BF16 * ref.abs() + 1e-5 * ref.abs().amax(dim=1, keepdim=True)


def float_mask(mask, seed=5):
    """a float mask the wrappers read as `> 0`: valid rows hold values in (0.1, 1.1), the others values in (-1, 0]"""
    r = torch.rand(mask.shape, generator=torch.Generator().manual_seed(seed))
    return torch.where(mask, r + 0.1, -r)


def byte_mask(mask):
    """a uint8 mask whose valid rows hold 1 or 200 (any non-zero byte is valid)"""
    v = torch.where(torch.arange(len(mask)) % 2 == 0, 1, 200).to(torch.uint8)
    return torch.where(mask, v, torch.zeros_like(v))


# =====================================================================================================================
# AggregatedContrastiveLoss
# =====================================================================================================================
CON_LOSS_ATOL = 1e-5                          # } the bars of test_lang_head_matches_reference
CON_GRAD_ATOL, CON_GRAD_RTOL = 2e-7, 1e-3     # }
CON_MAX_CLASSES = 256
CON_WIDTHS = (16, 48)
# label -> (valid rows, masked-out rows).  3: 99 valid of 129 rows, one short of min_count; 0 / 7 / 12 / 255: min_count, the odd
# splits 50|51 and 100|101, label 0 and label max_classes - 1; 5: large enough, every row masked out
CON_CLASSES = {3: (99, 30), 0: (100, 20), 7: (101, 0), 12: (200, 15), 255: (201, 0), 5: (0, 150)}
CON_UNLABELLED = 50                           # rows labelled -1 (valid mask true)
CON_QUALIFY = (0, 7, 12, 255)


@functools.lru_cache(maxsize=None)
def contrastive_case(C, which="full"):
    """-> namespace(pred (N, C) f32 unit rows, mask (N) bool, seg (N) int64, keys (N) f32), rows shuffled.
    'full': CON_CLASSES; class 3 (99 valid rows) points where class 0 does, so letting it in adds a column that competes with class
    0's own.  'none': no class reaches 100 valid rows.  'one': only class 7 does.  The keys of classes 7 and 12 are multiples of
    1/16: every key value repeats several times inside the class, the order among equal keys is the row index."""
    g = torch.Generator().manual_seed(4201 + C + {"full": 0, "none": 1, "one": 2}[which])
    classes = dict(CON_CLASSES)
    if which == "none":
        classes = {3: (99, 30), 0: (60, 70), 12: (1, 0), 5: (0, 150)}
    elif which == "one":
        classes = {3: (99, 30), 7: (101, 0), 0: (60, 70), 5: (0, 150)}
    centers = {lab: F.normalize(torch.randn(C, generator=g), dim=0) for lab in sorted(classes)}
    centers[3] = centers[0]
    pred, mask, seg = [], [], []
    for lab, (nv, nm) in classes.items():
        pred.append(centers[lab] + 0.5 * torch.randn(nv + nm, C, generator=g))
        mask.append(torch.cat([torch.ones(nv, dtype=torch.bool), torch.zeros(nm, dtype=torch.bool)]))
        seg.append(torch.full((nv + nm,), lab, dtype=torch.int64))
    pred.append(torch.randn(CON_UNLABELLED, C, generator=g))
    mask.append(torch.ones(CON_UNLABELLED, dtype=torch.bool))
    seg.append(torch.full((CON_UNLABELLED,), -1, dtype=torch.int64))
    pred, mask, seg = F.normalize(torch.cat(pred), dim=1), torch.cat(mask), torch.cat(seg)
    perm = torch.randperm(len(seg), generator=g)
    pred, mask, seg = pred[perm].contiguous(), mask[perm].contiguous(), seg[perm].contiguous()
    keys = torch.rand(len(seg), generator=g)
    coarse = (seg == 7) | (seg == 12)
    keys[coarse] = torch.floor(keys[coarse] * 16) / 16
    return types.SimpleNamespace(pred=pred, mask=mask, seg=seg, keys=keys)


def contrastive_reference(case, dtype=F64, reduction="mean", schedule="all", epoch_progress=None, min_count=100, loss_weight=1.0):
    """oracle.losses.aggregated_contrastive_loss(..., rand_keys=keys) in `dtype` -> (loss 0-d, dL/dpred (N, C) -- zeros when the
    loss does not depend on pred)"""
    p = case.pred.to(dtype).clone().requires_grad_(True)
    loss = olosses.aggregated_contrastive_loss(p, case.mask, case.seg, epoch_progress, 0.2, loss_weight, schedule, reduction,
                                               rand_keys=case.keys, min_count=min_count)
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), p.grad if p.grad is not None else torch.zeros_like(p)
