"""Inputs and float64 references shared by tests/test_hip_segloss_edges.py (GPU) and tests/test_segloss_host.py (CPU): the loss pair
of csrc/seg_loss.hip (cross-entropy + multiclass Lovasz-softmax) past one scan tile, one trip of the row loop and one trip of the
tile scan, the segmented sort of csrc/serialize.hip as the loss calls it, and the evaluator's counts.  Everything is built on the CPU
from seeded generators and cached; the references are torch / numpy in float64 and call nothing of the library under test."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24                                # half an ulp of a float32 in [0.5, 1): the unit of every bound below

# mirrors of csrc/seg_loss.hip (#define SL_THREADS, SL_MAX_BLOCKS, SL_ITEMS, SL_TILE, SL_MAX_CLASSES) and of csrc/serialize.hip
# (#define RS_THREADS, RS_ITEMS, RS_TILE, RS_STRIDE)
SL_THREADS, SL_MAX_BLOCKS, SL_ITEMS, SL_MAX_CLASSES = 256, 1024, 16, 256
SL_TILE = SL_THREADS * SL_ITEMS
RS_TILE = 256 * 8
NO_IGNORE = -(1 << 63)                        # what the modules hand the kernel for ignore_index=None: a label no row can carry


def scan_tiles(n):
    """grid.x of k_lovasz_tile_count / k_lovasz_scan (sl_tiles)"""
    return (max(n, 1) + SL_TILE - 1) // SL_TILE


def tile_scan_trips(n):
    """trips of the 256-tile loop in k_lovasz_tile_scan"""
    return (scan_tiles(n) + SL_THREADS - 1) // SL_THREADS


def sort_tiles(n):
    """grid.x of k_rs_hist / k_rs_scatter; RS_STRIDE pads the histogram rows to a multiple of 4 of these"""
    return (max(n, 1) + RS_TILE - 1) // RS_TILE


def row_trips(n):
    """trips of the grid-stride row loop of k_seg_softmax_ce / k_seg_loss_bwd / k_seg_iou (sl_blocks)"""
    blocks = min(max((n + SL_THREADS - 1) // SL_THREADS, 1), SL_MAX_BLOCKS)
    return max((n + blocks * SL_THREADS - 1) // (blocks * SL_THREADS), 1)


# =====================================================================================================================
# cases
# =====================================================================================================================
# scan tiles: 1, 1, 2, 2, 3, 4, 64, 64, 65, 66, 67, 256, 257, 258, 259 (one row past 66 and 17 rows past 258 full tiles open the
# 67th and 259th)
SPACED_N = (4095, 4096, 4097, 8192, 8193, 12293, 262143, 262144, 262145, 270336, 270337, 1048576, 1048577, 1056768, 1056785)
SPACED_FEW_IGNORED = 1000                     # n >= 1 000 000: exactly this many ignored rows; valid rows reach tiles 256, 257 at the two largest
# name -> (C, n, present classes, variant)
RANDOM = {"r3-8193": (3, 8193, 3, "plain"), "r20-4096": (20, 4096, 15, "plain"), "r20-12293-seen": (20, 12293, 15, "seen"),
          "r256-4097": (256, 4097, 200, "plain"), "r256-4097-ig255": (256, 4097, 200, "ig255"),
          "r20-8193-noignore": (20, 8193, 15, "noignore")}
SATURATED = "saturated"
SAT_C, SAT_N = 4, 4100
SPACED = tuple(f"spaced-{n}" for n in SPACED_N)
ALL_CASES = SPACED + tuple(RANDOM) + (SATURATED,)
NEAR_TIE_ULPS, NEAR_TIE_CAP = 4, 0.01


def _spaced(n):
    g = torch.Generator().manual_seed(7_000_003 + n)
    perm = torch.randperm(n, generator=g)
    q = (perm.double() + 0.25) / n
    logits = torch.stack([torch.log(q / (1 - q)), torch.zeros(n, dtype=F64)], 1).float()
    labels = torch.randint(0, 2, (n,), generator=g)
    if n < 1_000_000:
        labels[torch.rand(n, generator=g) < 0.1] = -1
    else:
        labels[torch.randperm(n, generator=g)[:SPACED_FEW_IGNORED]] = -1
    return types.SimpleNamespace(family="spaced", C=2, n=n, logits=logits, logits_bf16=None, labels=labels, ignore=-1, seen=None)


def _random(name):
    C, n, present, variant = RANDOM[name]
    g = torch.Generator().manual_seed(8_000_009 + 1009 * C + n + 17 * sorted(RANDOM).index(name))
    logits = torch.randn(n, C, generator=g) * 2.0
    pool = torch.randperm(C, generator=g)
    if variant == "ig255":
        pool = pool[pool != 255]
    cls = pool[:present]
    labels = cls[torch.randint(0, present, (n,), generator=g)]
    ignore, seen = -1, None
    if variant == "ig255":
        ignore = 255
    if variant == "noignore":
        ignore = None
    else:
        labels[torch.rand(n, generator=g) < 0.1] = ignore
    if variant == "seen":                     # one present class left out, one absent class let in
        seen = sorted(cls[1:].tolist() + [int(pool[present])])
    return types.SimpleNamespace(family="random", C=C, n=n, logits=logits, logits_bf16=logits.to(BF16), labels=labels, ignore=ignore,
                                 seen=seen)


def _saturated():
    """rows 3j: +-200 * one_hot (j % 4: +label, +other, -label, -other), p exactly 0 or 1 wherever the gap is 200; rows 6j + 1: ignored,
    so ignored rows precede saturated ones all along the row index; the rest random.  Logit gaps are below 20 or exactly 200."""
    C, n = SAT_C, SAT_N
    g = torch.Generator().manual_seed(9_000_011)
    logits = torch.randn(n, C, generator=g) * 2.0
    labels = torch.randint(0, C, (n,), generator=g)
    sat = torch.arange(0, n, 3)
    kind = torch.arange(len(sat)) % 4
    hot = torch.where(kind % 2 == 0, labels[sat], (labels[sat] + 1 + torch.randint(0, C - 1, (len(sat),), generator=g)) % C)
    logits[sat] = 0.0
    logits[sat, hot] = torch.where(kind < 2, 200.0, -200.0)
    labels[1::6] = -1
    c = types.SimpleNamespace(family="saturated", C=C, n=n, logits=logits, logits_bf16=logits.to(BF16), labels=labels, ignore=-1,
                              seen=None, sat_rows=sat, sat_kind=kind, sat_hot=hot)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("spaced-"):
        c = _spaced(int(name.split("-")[1]))
    elif name == SATURATED:
        c = _saturated()
    else:
        c = _random(name)
    c.name = name
    return c


def case_logits(name, dtype="f32"):
    c = case(name)
    return c.logits if dtype == "f32" else c.logits_bf16


def case_dtypes(name):
    return ("f32",) if case(name).logits_bf16 is None else ("f32", "bf16")


# =====================================================================================================================
# references
# =====================================================================================================================
def valid_mask(labels, C, ignore):
    v = (labels >= 0) & (labels < C)
    return v if ignore is None else v & (labels != ignore)


def jaccard_f64(fg_sorted, gts):
    """fg_sorted (..., m) 0/1 in descending-error order, gts (..., 1) -> the Lovasz gradient, float64"""
    fs = fg_sorted.double()
    jac = 1.0 - (gts.double() - fs.cumsum(-1)) / (gts.double() + (1.0 - fs).cumsum(-1))
    out = jac.clone()
    out[..., 1:] = jac[..., 1:] - jac[..., :-1]
    return out


def jaccard_f32(fg_sorted, gts):
    """The same in torch float32 on the CPU, written as the expression of k_lovasz_scan: J = 1 - I / U with one division, then one
    subtraction J_k - J_{k-1}.  Both cumulative sums are integers below 2^24, exact in float32."""
    fs = fg_sorted.float()
    gts = gts.float()
    jac = 1.0 - (gts - fs.cumsum(-1)) / (gts + (1.0 - fs).cumsum(-1))
    out = jac.clone()
    out[..., 1:] = jac[..., 1:] - jac[..., :-1]
    return out


def stable_descending(err, fg, rows):
    """err, fg (C, m) on the valid rows `rows` (ascending) -> (sorted errors, sorted fg, order as rows (C, m), order as positions in
    `rows`): descending errors, equal errors keep the row order"""
    es, perm = torch.sort(err, dim=1, descending=True, stable=True)
    return es, fg.gather(1, perm), rows[perm], perm


def reference(logits, labels, ignore, seen=None):
    """float64 restatement of the loss pair on (logits (n, C), labels (n)).  `seen`: list of classes or None."""
    x = logits.double()
    n, C = x.shape
    valid = valid_mask(labels, C, ignore)
    m = x.max(1).values
    ex = torch.exp(x - m[:, None])
    s = ex.sum(1)
    p = ex / s[:, None]
    rows = valid.nonzero().flatten()
    lab = labels[rows]
    ce_sum = (torch.log(s[rows]) + m[rows] - x[rows, lab]).sum()
    counts = torch.bincount(lab, minlength=C)
    present = counts > 0
    if seen is not None:
        mask = torch.zeros(C, dtype=torch.bool)
        mask[[c for c in seen if 0 <= c < C]] = True
        present = present & mask
    fg = (lab[None, :] == torch.arange(C)[:, None]).double()                  # (C, m)
    err = (fg - p[rows].t()).abs()
    es, fs, order, perm = stable_descending(err, fg, rows)
    gts = counts.double()[:, None]
    gs = jaccard_f64(fs, gts)
    lov = (es * gs).sum(1)
    g = torch.zeros(C, n, dtype=F64)
    g[:, rows] = torch.zeros_like(gs).scatter_(1, perm, gs)
    g[~present] = 0.0
    return types.SimpleNamespace(m=m, s=s, p=p, valid=valid, rows=rows, ce_sum=ce_sum, n_valid=int(valid.sum()), counts=counts,
                                 present=present, err_sorted=es, fg_sorted=fs, order=order, perm=perm, g=g, g_sorted=gs,
                                 lovasz_sum=lov[present].sum(), lovasz_per_class=lov,
                                 ce=ce_sum / max(int(valid.sum()), 1), lovasz=lov[present].sum() / max(int(present.sum()), 1))


@functools.lru_cache(maxsize=3)
def case_reference(name, dtype="f32"):
    c = case(name)
    return reference(case_logits(name, dtype).float(), c.labels, c.ignore, c.seen)


def torch_f32_pair(logits, labels, ignore, seen=None):
    """(ce, lovasz) of the reference formulas restated in torch float32 on the CPU: F.cross_entropy and the per-class loop with
    torch.sort / torch.dot (the loop of restated_pair in test_hip_semseg.py)."""
    x = logits.float()
    C = x.shape[1]
    ce = F.cross_entropy(x, labels, ignore_index=-100 if ignore is None else ignore)
    p = x.softmax(1)
    valid = valid_mask(labels, C, ignore)
    vp, vl = p[valid], labels[valid]
    losses = []
    for c in vl.unique().tolist():
        if seen is not None and c not in seen:
            continue
        fg = (vl == c).float()
        err = (fg - vp[:, c]).abs()
        es, perm = torch.sort(err, dim=0, descending=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        jac[1:] = jac[1:] - jac[:-1]
        losses.append(torch.dot(es, jac))
    lov = torch.stack(losses).mean() if losses else x.sum() * 0
    return ce, lov


@functools.lru_cache(maxsize=None)
def case_torch_f32(name, dtype="f32"):
    c = case(name)
    ce, lov = torch_f32_pair(case_logits(name, dtype).float(), c.labels, c.ignore, c.seen)
    return float(ce), float(lov)


def rel_err(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


VALUE_FLOOR = 2.0 ** -20


def value_bound(torch_err):
    """the rule of test_error_against_fp64_within_twice_torchs_own, with a floor"""
    return max(2.0 * torch_err, VALUE_FLOOR)


def near_tied(errors_sorted):
    """errors_sorted (..., m) float32 in sorted order -> bool (..., m): the element's error lies within NEAR_TIE_ULPS ulp of a sorted
    neighbour's, the ulp being that of the larger of the two.  Two float32 evaluations of the same probability that differ by an ulp
    or two may order such a pair either way."""
    e = errors_sorted.detach().cpu().numpy().astype(np.float32)
    a, b = e[..., :-1], e[..., 1:]
    close = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= NEAR_TIE_ULPS * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    out = np.zeros(e.shape, dtype=bool)
    out[..., :-1] |= close
    out[..., 1:] |= close
    return torch.from_numpy(out)


def f32_errors(p32, labels, rows):
    """|fg - p| in float32 as the kernel forms it, (C, m) on the valid rows, and fg"""
    C = p32.shape[1]
    fg = (labels[rows][None, :] == torch.arange(C)[:, None]).float()
    return (fg - p32[rows].t().float()).abs(), fg


def bwd_reference(logits, labels, rowstat, glov, present, coef, ignore):
    """float64: coef0 * (p - onehot) + coef1 * p * (v - sum_j p_j v_j), v_c = glov[c, i] * sign(p_c - fg_c) on present classes, 0 on
    the others; p from the given per-row max / sum of exponentials; ignored rows zero.  glov / present None: the CE term alone."""
    x = logits.double()
    n, C = x.shape
    valid = valid_mask(labels, C, ignore)
    p = torch.exp(x - rowstat[:, :1].double()) / rowstat[:, 1:].double()
    onehot = torch.zeros(n, C, dtype=F64)
    rows = valid.nonzero().flatten()
    onehot[rows, labels[rows]] = 1.0
    d = p - onehot
    out = float(coef[0]) * d
    if glov is not None:
        pres = present.bool()
        v = torch.where(pres[None, :], glov.double().t(), torch.zeros((), dtype=F64)) * torch.sign(d)     # NaN in absent classes: dropped
        out = out + float(coef[1]) * p * (v - (p * v).sum(1, keepdim=True))
    out[~valid] = 0.0
    return out


def bf16_bound(ref, rel_max=1e-5):
    """one rounding to bf16 of a value within rel_max * max|ref| of the reference"""
    return 2.0 ** -8 * ref.abs() + rel_max * ref.abs().max()


# =====================================================================================================================
# sort cases: keys as the loss hands them to ss_argsort_i64 (key_bits = 32, the foreground flag in bit 32)
# =====================================================================================================================
SORT_SEGMENTS = (2, 20, 256)
SORT_N = (2047, 2048, 2049, 6145, 10241)      # 1, 1, 2, 4, 6 sort tiles: RS_STRIDE pads 3, 3, 2, 0, 2 counters


@functools.lru_cache(maxsize=4)
def sort_keys(K, n):
    """(K, n) int64 = random 32 bits | random bit << 32; segment 1 draws its low words from 5 values (stability), segment K - 1 is
    sorted by its low word already"""
    g = torch.Generator().manual_seed(6_000_011 + 4099 * K + n)
    low = torch.randint(0, 1 << 32, (K, n), generator=g, dtype=torch.int64)
    five = torch.tensor([0, 1, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=torch.int64)
    low[1] = five[torch.randint(0, 5, (n,), generator=g)]
    low[K - 1] = torch.sort(low[K - 1]).values
    flag = torch.randint(0, 2, (K, n), generator=g, dtype=torch.int64)
    return low | (flag << 32)


# =====================================================================================================================
# evaluator counts
# =====================================================================================================================
IOU_N = (1, 255, 256, 257, 262401)
IOU_C = (1, 2, 20, 256)
IOU_IGNORE = (-1, 255)


def iou_counts(pred, tgt, C, ignore):
    """the formula of test_seg_iou_counts_equal_intersection_and_union's numpy restatement, (3, C) int64"""
    pred = pred.copy()
    pred[tgt == ignore] = ignore
    inter = np.bincount(pred[(pred == tgt) & (pred >= 0) & (pred < C)], minlength=C)[:C]
    out = np.bincount(pred[(pred >= 0) & (pred < C)], minlength=C)[:C]
    t = np.bincount(tgt[(tgt >= 0) & (tgt < C)], minlength=C)[:C]
    return np.stack([inter, out + t - inter, t]).astype(np.int64)


@functools.lru_cache(maxsize=8)
def iou_case(n, C, ignore):
    """-> (logits (n, C) f32 of multiples of 1/8 in [-0.5, 0.5] (exact in bf16, maxima tie often), target (n) with ignored rows and
    out-of-range values, pred (n) int32 with values >= C and negative values other than ignore)"""
    g = torch.Generator().manual_seed(5_000_011 + 1_000_003 * C + 7 * n + (ignore & 1023))
    logits = torch.randint(-4, 5, (n, C), generator=g).float() / 8
    tgt = torch.randint(0, C, (n,), generator=g)
    r = torch.rand(n, generator=g)
    tgt[r < 0.1] = ignore
    tgt[(r >= 0.1) & (r < 0.13)] = C + 3          # outside the class range, not ignore (C + 3 != 255 for every C here)
    pred = torch.randint(0, C, (n,), generator=g, dtype=torch.int32)
    r = torch.rand(n, generator=g)
    pred[r < 0.05] = C
    pred[(r >= 0.05) & (r < 0.1)] = C + 700
    pred[(r >= 0.1) & (r < 0.15)] = -7
    return logits, tgt, pred


def argmax_lowest(logits):
    """arg-max with the lowest class among equal maxima"""
    x = logits.double().numpy()
    return np.argmax(x, axis=1)               # numpy returns the first maximum
