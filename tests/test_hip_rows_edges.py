"""csrc/rows.hip -- the pooling / unpooling seam kernels -- against float64 on the CPU, in every dispatch form.

Each entry point picks its kernel from the row width in bytes and the alignment of the base pointers: 16-byte lanes, 4-byte or
2-byte lanes (gather / scatter), or one element per thread (segment reduce / broadcast, gather-add).  rows_cases.py lists the
widths and names the form each takes; test_width_list_covers_every_form keeps that list honest.

Every reference below is a plain loop (or index_add_) over the CSR in float64 on the CPU, applied to the same rounded inputs, and
calls nothing of the library.  The bounds follow from the arithmetic the kernels document -- fp32 accumulation in CSR order, one
rounding on store -- and are not measured.  With u = 2^-24 and L the segment length:

  sum,  fp32 out:  |out - ref| <= L u sum_j |x_j|             (recursive summation of L terms, Higham 4.4)
  sum,  bf16 out:  the same + 2^-8 |ref|                      (half an ulp of ONE round-to-nearest-even bf16 rounding)
  mean:            the sum bound / L + u |ref|                (one correctly rounded fp32 division)
  broadcast, gather, scatter, gather-add, min / max: bit-equal to the restated operation in the tensor's dtype.

tests/test_rows_host.py shows on the CPU that an fp32-accumulating restatement of the kernels' loop meets these bounds and a
bf16-accumulating one violates them on the 257-row and 5000-row segments."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_cases as rc  # noqa: E402
from rows_cases import BF16, F32, F64  # noqa: E402

pytestmark = pytest.mark.gpu
ORD = ("z", "z-trans", "hilbert", "hilbert-trans")
U = 2.0 ** -24                 # unit roundoff of fp32
HALF_ULP_BF16 = 2.0 ** -8      # unit roundoff of bf16 (8 significand bits)
ALL_CASES = rc.ALIGNED + rc.MISALIGNED


# =====================================================================================================================
# float64 restatements (CPU) and the bounds
# =====================================================================================================================
def ref_segment_sum(x, csr):
    """-> (sum, sum of |x|), each (n_seg, C) float64: a plain loop over the CSR; an empty segment gives 0"""
    xs = x.double()[rc.rows_in_csr_order(csr)]
    out = torch.zeros(csr.n, x.shape[1], dtype=F64)
    absum = torch.zeros_like(out)
    for s in range(csr.n):
        b, e = int(csr.ptr[s]), int(csr.ptr[s + 1])
        if e > b:
            out[s] = xs[b:e].sum(0)
            absum[s] = xs[b:e].abs().sum(0)
    return out, absum


def ref_segment_minmax(x, csr, is_max, lowest_row=False):
    """-> (value (n_seg, C) float64, arg (n_seg, C) int64): the extremum of every segment and the FIRST row in CSR order that attains
    it (lowest_row=True: the lowest row id instead).  A NaN wins (as torch.amax / amin) and arg is the first NaN row; an empty segment
    gives 0 and -1."""
    rows = rc.rows_in_csr_order(csr).numpy()
    xs = x.double().numpy()[rows]
    C = x.shape[1]
    val, arg = np.zeros((csr.n, C)), np.full((csr.n, C), -1, dtype=np.int64)
    for s in range(csr.n):
        b, e = int(csr.ptr[s]), int(csr.ptr[s + 1])
        if e == b:
            continue
        blk = xs[b:e]
        nan = np.isnan(blk)
        m = blk.max(0) if is_max else blk.min(0)                  # propagates NaN
        hit = np.where(nan.any(0)[None, :], nan, blk == m[None, :])
        if lowest_row:
            arg[s] = np.where(hit, rows[b:e, None], np.iinfo(np.int64).max).min(0)
        else:
            arg[s] = rows[b:e][hit.argmax(0)]                     # first True along the segment
        val[s] = m
    return torch.from_numpy(val), torch.from_numpy(arg)


def sum_bound(ref, absum, lens, dtype):
    b = lens.double().reshape(-1, 1) * U * absum
    return b + HALF_ULP_BF16 * ref.abs() if dtype == BF16 else b


def mean_bound(ref_sum, absum, lens, dtype):
    L = lens.clamp(min=1).double().reshape(-1, 1)
    return sum_bound(ref_sum, absum, lens, dtype) / L + U * (ref_sum / L).abs()


def round_bound(ref, dtype):
    """one rounding of an exactly known value into `dtype`"""
    return (HALF_ULP_BF16 if dtype == BF16 else U) * ref.abs()


def _within(name, got, ref, bound):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if not ref.numel():
        return
    err = (got - ref).abs()
    over = err - bound
    k = int(torch.nan_to_num(over, nan=float("inf")).argmax())
    r, c = divmod(k, ref.shape[1])
    print(f"    {name}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3g}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), \
        f"{name}: row {r} col {c}: got {got[r, c].item()!r} ref {ref[r, c].item()!r} err {err[r, c].item():.3e} bound {bound[r, c].item():.3e}"


def _same(got, ref):
    """bit-equal up to the payload of a NaN"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and torch.equal(got[~gn], ref[~rn])


# =====================================================================================================================
# device placement
# =====================================================================================================================
def place(t, align=16):
    """t on the device: a fresh allocation (16-byte aligned), or -- align = one element -- the contiguous view
    base[1 : 1 + n * C].view(n, C) of a flat allocation, which no 16-byte (and, for bf16, no 4-byte) form may touch"""
    if align == 16:
        d = t.cuda()
        assert d.numel() == 0 or d.data_ptr() % 16 == 0
        return d
    n, C = t.shape
    assert align == t.element_size()
    base = torch.empty(n * C + 8, dtype=t.dtype, device="cuda")
    v = base[1:1 + n * C].view(n, C)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and v.data_ptr() % 16 == align
    return v


@functools.lru_cache(maxsize=None)
def dev_level(permute=True, empty=True):
    csr = rc.make_csr(permute, empty)
    return types.SimpleNamespace(n=csr.n, idx_ptr=csr.idx_ptr.cuda(), cluster=csr.cluster.cuda(),
                                 indices=None if csr.indices is None else csr.indices.cuda())


@functools.lru_cache(maxsize=None)
def reduce_reference(dtype, C, permute):
    csr = rc.make_csr(permute)
    x = rc.features(csr.n_rows, C, dtype, seed=1)
    return (csr, x) + ref_segment_sum(x, csr)


def _pid(p):
    return "perm" if p else "identity"


# =====================================================================================================================
# the width list
# =====================================================================================================================
def test_width_list_covers_every_form():
    """every kernel form of every entry point has at least one width in the list, per dtype, aligned or not"""
    gather = {(dt, lane): [c for c in ALL_CASES if c[0] == dt and rc.gather_form(*c) == lane] for dt in (F32, BF16) for lane in (16, 4, 2)}
    reduce = {(dt, f): [c for c in ALL_CASES if c[0] == dt and rc.reduce_form(*c) == f] for dt in (F32, BF16) for f in ("v16", "scalar")}
    assert not gather.pop((F32, 2))                                   # an fp32 row is always a multiple of 4 bytes on a 4-byte address
    assert all(gather.values()), {k: len(v) for k, v in gather.items()}
    assert all(reduce.values()), {k: len(v) for k, v in reduce.items()}
    # by byte width: fp32 C = 1, 3, 5 -> 4-byte gather + scalar reduce; bf16 C = 1, 3 -> 2-byte gather,
    # C = 2, 4, 6 -> 4-byte gather + scalar reduce; multiples of 16 bytes -> 16-byte lanes on aligned pointers only
    assert {c[1] for c in gather[(F32, 4)] if c[2] == 16} == {1, 3, 5} and {c[1] for c in gather[(BF16, 4)]} == {2, 4, 6}
    assert {c[1] for c in gather[(BF16, 2)] if c[2] == 16} == {1, 3}
    assert {c[1] for c in reduce[(F32, "v16")]} == {4, 8, 36} and {c[1] for c in reduce[(BF16, "v16")]} == {8, 24, 72}
    for dt, C, align in rc.MISALIGNED:                                # a misaligned 16-byte-multiple row falls to the narrow forms
        assert rc.row_bytes(dt, C) % 16 == 0 and rc.reduce_form(dt, C, align) == "scalar"
        assert rc.gather_form(dt, C, align) == (4 if dt == F32 else 2)
    for C in rc.F32_WIDTHS + rc.BF16_WIDTHS:                          # the last block of every launch is partly idle
        assert (rc.N_SEG * C) % 256 and (rc.N_SEG * max(C // 8, 1)) % 256
    csr = rc.make_csr(True)
    assert set(rc.SEG_LENGTHS) <= set(csr.lens.tolist()) and int(csr.lens[rc.LONG_AT]) == rc.LONG_LEN
    assert csr.lens[0] == 0 and csr.lens[csr.n // 2] == 0 and csr.lens[-1] == 0 and csr.lens[rc.ONE_AT] == 1


# =====================================================================================================================
# ss_segment_reduce / ss_segment_bcast / ss_gather_add_rows
# =====================================================================================================================
@pytest.mark.parametrize("permute", [True, False], ids=_pid)
@pytest.mark.parametrize("case", ALL_CASES, ids=rc.case_id)
def test_segment_reduce_sum_and_mean(case, permute):
    from scenesplat_amd import native as nv
    dtype, C, align = case
    csr, x, ref, absum = reduce_reference(dtype, C, permute)
    lv = dev_level(permute)
    xd = place(x, align)
    for mean in (False, True):
        out = nv.segment_reduce(xd, lv.indices, lv.idx_ptr, lv.n, mean)
        assert out.dtype == dtype and tuple(out.shape) == (csr.n, C)
        if mean:
            _within("mean", out, ref / csr.lens.clamp(min=1).double().reshape(-1, 1), mean_bound(ref, absum, csr.lens, dtype))
        else:
            _within("sum", out, ref, sum_bound(ref, absum, csr.lens, dtype))
        assert bool((out[lv.idx_ptr[1:].long() == lv.idx_ptr[:-1].long()] == 0).all())          # empty: exactly 0, never NaN
        assert int((csr.lens == 0).sum()) >= 3
        assert torch.equal(out, nv.segment_reduce(xd, lv.indices, lv.idx_ptr, lv.n, mean))     # no atomics
    # a single-row segment is a copy in either mode
    one = int(rc.rows_in_csr_order(csr)[csr.ptr[rc.ONE_AT]])
    assert torch.equal(nv.segment_reduce(xd, lv.indices, lv.idx_ptr, lv.n, True)[rc.ONE_AT].cpu(), x[one])


@pytest.mark.parametrize("permute", [True, False], ids=_pid)
@pytest.mark.parametrize("case", ALL_CASES, ids=rc.case_id)
def test_segment_bcast(case, permute):
    from scenesplat_amd import native as nv
    dtype, C, align = case
    csr, lv = rc.make_csr(permute), dev_level(permute)
    dout = rc.cotangent(csr.n, C, dtype, seed=2)
    dd = place(dout, align)
    cl = csr.cluster.long()
    plain = nv.segment_bcast(dd, lv.cluster, lv.idx_ptr, False)
    assert plain.dtype == dtype and torch.equal(plain.cpu(), dout[cl])
    # one correctly rounded fp32 division, then (bf16) one rounding
    quot = (dout.float()[cl] / csr.lens.float()[cl].reshape(-1, 1)).to(dtype)
    scaled = nv.segment_bcast(dd, lv.cluster, lv.idx_ptr, True)
    assert torch.equal(scaled.cpu(), quot)
    # every count is the CSR's own: a row of the 5000-row segment and the row of a 1-row segment, by name
    rows = rc.rows_in_csr_order(csr)
    r_long, r_one = int(rows[csr.ptr[rc.LONG_AT] + 1234]), int(rows[csr.ptr[rc.ONE_AT]])
    assert int(cl[r_long]) == rc.LONG_AT and int(cl[r_one]) == rc.ONE_AT
    assert torch.equal(scaled[r_long].cpu(), (dout[rc.LONG_AT].float() / float(rc.LONG_LEN)).to(dtype))
    assert torch.equal(scaled[r_one].cpu(), dout[rc.ONE_AT])
    assert torch.equal(scaled, nv.segment_bcast(dd, lv.cluster, lv.idx_ptr, True))
    assert torch.equal(plain, nv.segment_bcast(dd, lv.cluster, lv.idx_ptr, False))


@pytest.mark.parametrize("case", ALL_CASES, ids=rc.case_id)
def test_gather_add_rows(case):
    """bit-equal to a + b[idx] in the tensor's dtype: both sides compute one fp32 add and one rounding"""
    from scenesplat_amd import native as nv
    dtype, C, align = case
    n, m = 1777, 301
    a, b = rc.features(n, C, dtype, seed=3), rc.cotangent(m, C, dtype, seed=4)
    idx = torch.randint(0, m, (n,), generator=torch.Generator().manual_seed(C), dtype=torch.int32)
    ref = a + b[idx.long()]
    assert ref.dtype == dtype
    for a_al, b_al in ([(16, 16)] if align == 16 else [(align, 16), (16, align), (align, align)]):
        out = nv.gather_add_rows(place(a, a_al), place(b, b_al), idx.cuda())
        assert out.dtype == dtype and torch.equal(out.cpu(), ref), (a_al, b_al)


# =====================================================================================================================
# ss_gather_rows / ss_scatter_rows
# =====================================================================================================================
@pytest.mark.parametrize("case", ALL_CASES, ids=rc.case_id)
def test_gather_and_scatter_rows(case):
    from scenesplat_amd import native as nv
    dtype, C, align = case
    m, n = 1000, 1777
    g = torch.Generator().manual_seed(100 + C)
    src = rc.cotangent(m, C, dtype, seed=5)
    idx = torch.randint(-1, m, (n,), generator=g, dtype=torch.int32)
    idx[0] = -1; idx[n - 1] = -1; idx[1] = m - 1; idx[2] = 0
    gref = torch.where((idx >= 0).unsqueeze(1), src[idx.clamp(min=0).long()], torch.zeros(1, C, dtype=dtype))
    perm = torch.randperm(m, generator=g).to(torch.int32)
    perm[::7] = -1
    fill = rc.features(m, C, dtype, seed=6, mean=-3.0)                  # rows no source lands on keep what they held
    sref = fill.clone()
    sref[perm[perm >= 0].long()] = src[perm >= 0]
    for s_al, d_al in ([(16, 16)] if align == 16 else [(align, 16), (16, align), (align, align)]):
        sd = place(src, s_al)
        out = nv.gather_rows(sd, idx.cuda(), out=place(torch.full((n, C), 7.0, dtype=dtype), d_al))
        assert torch.equal(out.cpu(), gref), ("gather", s_al, d_al)
        dst = place(fill, d_al)
        assert nv.scatter_rows(sd, perm.cuda(), dst) is dst
        assert torch.equal(dst.cpu(), sref), ("scatter", s_al, d_al)
    # the wrapper's own output, and n = 0 on both sides
    sd = place(src, align)
    assert torch.equal(nv.gather_rows(sd, idx.cuda()).cpu(), gref)
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    out0 = nv.gather_rows(sd, none)
    assert tuple(out0.shape) == (0, C) and out0.dtype == dtype
    dst = place(fill, align)
    nv.scatter_rows(torch.empty(0, C, dtype=dtype, device="cuda"), none, dst)
    assert torch.equal(dst.cpu(), fill)


# =====================================================================================================================
# autograd seams against float64 autograd of the restated operation
# =====================================================================================================================
def _f64_segment(xo, csr, mean):
    out = torch.zeros(csr.n, xo.shape[1], dtype=F64).index_add(0, csr.seg_of_pos, xo[rc.rows_in_csr_order(csr)])
    return out / csr.lens.clamp(min=1).double().reshape(-1, 1) if mean else out


def _check_segment_mean(x, cot, csr, lv, mean, dtype):
    from scenesplat_amd import functional as SF
    xg = x.cuda().requires_grad_(True)
    y = SF.segment_mean(xg, lv, mean=mean)
    xo = x.double().requires_grad_(True)
    yo = _f64_segment(xo, csr, mean)
    ref, absum = ref_segment_sum(x, csr)
    assert torch.allclose(yo.detach(), ref / csr.lens.clamp(min=1).double().reshape(-1, 1) if mean else ref, rtol=1e-12, atol=0)
    _within("y", y, yo, (mean_bound if mean else sum_bound)(ref, absum, csr.lens, dtype))
    y.backward(cot.cuda()); yo.backward(cot.double())
    assert xg.grad.dtype == dtype
    if mean:
        _within("dx", xg.grad, xo.grad, round_bound(xo.grad, dtype) + (U * xo.grad.abs() if dtype == BF16 else 0))
    else:
        assert torch.equal(xg.grad.cpu(), xo.grad.to(dtype)) and torch.equal(xo.grad.to(dtype).double(), xo.grad)


def _check_unpool_add(skip, up, cot, csr, lv, dtype):
    from scenesplat_amd import functional as SF
    sg, ug = skip.cuda().requires_grad_(True), up.cuda().requires_grad_(True)
    z = SF.unpool_add(sg, ug, lv)
    so, uo = skip.double().requires_grad_(True), up.double().requires_grad_(True)
    zo = so + uo[csr.cluster.long()]
    _within("z", z, zo, round_bound(zo.detach(), dtype))
    assert torch.equal(z.detach().cpu(), skip + up[csr.cluster.long()])
    z.backward(cot.cuda()); zo.backward(cot.double())
    assert torch.equal(sg.grad.cpu(), cot)
    ref, absum = ref_segment_sum(cot, csr)
    assert torch.allclose(uo.grad, ref, rtol=0, atol=1e-10)                 # the two float64 summation orders
    _within("dup", ug.grad, uo.grad, sum_bound(ref, absum, csr.lens, dtype))
    assert bool((ug.grad[(csr.lens == 0).cuda()] == 0).all())


@pytest.mark.parametrize("mean", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("case", rc.ALIGNED, ids=rc.case_id)
def test_segment_mean_autograd(case, mean):
    dtype, C, _ = case
    csr, lv = rc.make_csr(True), dev_level(True)
    _check_segment_mean(rc.features(csr.n_rows, C, dtype, seed=1), rc.cotangent(csr.n, C, dtype, seed=7), csr, lv, mean, dtype)


@pytest.mark.parametrize("permute", [True, False], ids=_pid)
@pytest.mark.parametrize("case", [(F32, 5, 16), (F32, 8, 16), (BF16, 6, 16), (BF16, 24, 16)], ids=rc.case_id)
def test_unpool_add_autograd(case, permute):
    dtype, C, _ = case
    csr, lv = rc.make_csr(permute), dev_level(permute)
    _check_unpool_add(rc.features(csr.n_rows, C, dtype, seed=8), rc.cotangent(csr.n, C, dtype, seed=9),
                      rc.features(csr.n_rows, C, dtype, seed=10), csr, lv, dtype)


@pytest.mark.parametrize("dtype,C", [(F32, 5), (F32, 4), (BF16, 6), (BF16, 8)], ids=lambda v: str(v).replace("torch.", ""))
def test_pool_and_unpool_on_a_planned_level(dtype, C):
    """the same two seams on the CSR build_plan lays out (clusters of at most 8 rows, none empty)"""
    from scenesplat_amd.plan import build_plan
    g = torch.Generator().manual_seed(11)
    gc = torch.unique(torch.randint(0, 24, (3000, 3), generator=g), dim=0)
    gc = gc[torch.randperm(len(gc), generator=g)]
    n = len(gc)
    fine, coarse = build_plan(gc.cuda(), torch.tensor([n // 2, n]).cuda(), ORD, (2,)).levels
    ptr = coarse.idx_ptr.cpu()[: coarse.n + 1].long()
    lens = ptr[1:] - ptr[:-1]
    csr = types.SimpleNamespace(n=coarse.n, n_rows=n, ptr=ptr, lens=lens, indices=coarse.indices.cpu(), cluster=coarse.cluster.cpu(),
                                seg_of_pos=torch.repeat_interleave(torch.arange(coarse.n), lens))
    assert int(ptr[-1]) == n and torch.equal(csr.cluster.long()[csr.indices.long()], csr.seg_of_pos) and int(lens.min()) >= 1
    _check_segment_mean(rc.features(n, C, dtype, seed=12), rc.cotangent(coarse.n, C, dtype, seed=13), csr, coarse, True, dtype)
    _check_unpool_add(rc.features(n, C, dtype, seed=14), rc.cotangent(coarse.n, C, dtype, seed=15),
                      rc.features(n, C, dtype, seed=16), csr, coarse, dtype)


@pytest.mark.parametrize("C", [5, 8])
def test_group_sum_autograd(C):
    """_GroupSum of the contrastive loss: groups of up to 5000 rows summed in fp32, rows outside every group listed behind
    ptr[-1] and mapped to the extra zero row in the backward, as AggregatedContrastiveLoss builds them"""
    from scenesplat_amd.pointcept_api.lang import _GroupSum
    csr = rc.make_csr(True)
    n_out, N = 500, csr.n_rows + 500
    g = torch.Generator().manual_seed(17)
    order = torch.randperm(N, generator=g)                                   # CSR positions [0, n_rows) are grouped, the rest is outside
    row_group = torch.full((N,), csr.n, dtype=torch.int64)
    row_group[order[:csr.n_rows]] = csr.seg_of_pos
    grouped = types.SimpleNamespace(n=csr.n, n_rows=csr.n_rows, ptr=csr.ptr, lens=csr.lens, indices=order[:csr.n_rows].to(torch.int32))
    feat = rc.features(N, C, F32, seed=18)
    cot = rc.cotangent(csr.n, C, F32, seed=19)
    fg = feat.cuda().requires_grad_(True)
    G = _GroupSum.apply(fg, order.to(torch.int32).cuda(), csr.idx_ptr.cuda(), csr.n, row_group.to(torch.int32).cuda())
    fo = feat.double().requires_grad_(True)
    Go = torch.zeros(csr.n, C, dtype=F64).index_add(0, csr.seg_of_pos, fo[order[:csr.n_rows]])
    ref, absum = ref_segment_sum(feat, grouped)
    assert torch.allclose(Go.detach(), ref, rtol=1e-12, atol=0)
    _within("G", G, Go, sum_bound(ref, absum, csr.lens, F32))
    G.backward(cot.cuda()); Go.backward(cot.double())
    assert torch.equal(fg.grad.cpu(), fo.grad.float()) and torch.equal(fo.grad.float().double(), fo.grad)
    assert int((row_group == csr.n).sum()) == n_out and bool((fg.grad.cpu()[row_group == csr.n] == 0).all())


# =====================================================================================================================
# ss_segment_minmax and its backward (one kernel form)
# =====================================================================================================================
def _minmax_data(kind, csr, C, dtype):
    n = csr.n_rows
    if kind == "ties":            # three bf16-exact values: nearly every segment has ties
        g = torch.Generator().manual_seed(23 + C)
        return torch.tensor([-0.5, 0.25, 1.0])[torch.randint(0, 3, (n, C), generator=g)].to(dtype)
    x = rc.features(n, C, dtype, seed=20)
    if kind == "normal":
        return x
    # "special": NaN and +-inf at the first / a middle / the last CSR position of segments of >= 7 rows
    nan, inf = float("nan"), float("inf")
    rows = rc.rows_in_csr_order(csr)
    segs = [s for s in range(csr.n) if csr.lens[s] >= 7 and s != rc.LONG_AT]
    for k, s in enumerate(segs):
        b, e, c = int(csr.ptr[s]), int(csr.ptr[s + 1]), k % C
        mode = k % 8
        if mode == 0:
            x[rows[b], c] = nan
        elif mode == 1:
            x[rows[e - 1], c] = nan
        elif mode == 2:           # a NaN, then larger and smaller ordered values behind it
            x[rows[b + 2], c] = nan; x[rows[b + 4], c] = inf; x[rows[b + 5], c] = -inf
        elif mode == 3:           # two NaNs: the first one stays
            x[rows[b + 1], c] = nan; x[rows[e - 1], c] = nan
        elif mode == 4:           # +inf twice: an ordinary value, first one on ties
            x[rows[b + 3], c] = inf; x[rows[e - 1], c] = inf
        elif mode == 5:
            x[rows[b + 3], c] = -inf; x[rows[e - 1], c] = -inf
        elif mode == 6:           # the extremum of an all -inf / all +inf segment is that value, at the first row
            x[rows[b:e], c] = -inf
        else:
            x[rows[b:e], c] = inf
    x[rows[csr.ptr[rc.ONE_AT]], 0] = nan                                   # a 1-row segment that is a NaN
    x[rows[csr.ptr[rc.LONG_AT] + 2500], 0] = nan                           # one NaN among 5000 rows
    x[rows[csr.ptr[rc.LONG_AT] + 4000], C - 1] = inf if C > 1 else nan
    return x


@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("kind,permute", [("normal", True), ("normal", False), ("ties", True), ("special", True)],
                         ids=["normal-perm", "normal-identity", "ties", "nan-inf"])
@pytest.mark.parametrize("dtype,C", [(dt, C) for dt in (F32, BF16) for C in (1, 5, 20)], ids=lambda v: str(v).replace("torch.", ""))
def test_segment_minmax(dtype, C, kind, permute, reduce):
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    is_max = reduce == "max"
    csr, lv = rc.make_csr(permute), dev_level(permute)
    x = _minmax_data(kind, csr, C, dtype)
    val, arg = ref_segment_minmax(x, csr, is_max)
    xd = x.cuda()
    out, garg = nv.segment_minmax(xd, lv.indices, lv.idx_ptr, lv.n, is_max)
    assert out.dtype == dtype and garg.dtype == torch.int32
    assert _same(out, val.to(dtype)) and torch.equal(val.to(dtype).double().nan_to_num(0.5), val.nan_to_num(0.5))
    assert torch.equal(garg.cpu().long(), arg)                             # the first attaining row in CSR order
    empty = csr.lens == 0
    assert int(empty.sum()) >= 3 and bool((out.cpu()[empty] == 0).all()) and bool((garg.cpu()[empty] == -1).all())
    o2, a2 = nv.segment_minmax(xd, lv.indices, lv.idx_ptr, lv.n, is_max)
    assert _same(o2, out) and torch.equal(a2, garg)
    if C == 20:                                                            # a source one element off 16-byte alignment
        o3, a3 = nv.segment_minmax(place(x, x.element_size()), lv.indices, lv.idx_ptr, lv.n, is_max)
        assert _same(o3, out) and torch.equal(a3, garg)
    if kind == "ties":
        low = ref_segment_minmax(x, csr, is_max, lowest_row=True)[1]
        tied = (arg != low)
        assert int(tied.sum()) > csr.n * C // 8, "the permutation must separate 'first in CSR order' from 'lowest row id'"
    if kind == "special":
        hasnan = torch.zeros(csr.n, C, dtype=F64).index_add_(0, csr.cluster.long(), torch.isnan(x).double()) > 0
        assert int(hasnan.sum()) >= 20 and torch.equal(torch.isnan(out.cpu()), hasnan)
        sel = garg.cpu().long()[hasnan]
        cols = torch.arange(C).expand(csr.n, C)[hasnan]
        assert bool(torch.isnan(x[sel, cols]).all()) and torch.equal(csr.cluster.long()[sel], torch.arange(csr.n).reshape(-1, 1).expand(csr.n, C)[hasnan])
        assert bool(torch.isinf(out.cpu()[~hasnan]).any())
    # backward: dout[s][c] lands on exactly that row, zeros everywhere else
    cot = rc.cotangent(csr.n, C, dtype, seed=21)
    xg = x.cuda().requires_grad_(True)
    y = SF.segment_minmax(xg, lv, is_max)
    assert _same(y, out)
    y.backward(cot.cuda())
    exp = torch.zeros(csr.n_rows, C, dtype=dtype)
    keep = arg >= 0
    exp[arg[keep], torch.arange(C).expand(csr.n, C)[keep]] = cot[keep]
    assert xg.grad.dtype == dtype and torch.equal(xg.grad.cpu(), exp)
    back = torch.zeros(csr.n, C, dtype=F64).index_add_(0, csr.cluster.long(), xg.grad.cpu().double())
    assert torch.equal(back, torch.where(empty.reshape(-1, 1), torch.zeros(1, dtype=F64), cot.double()))
    assert torch.equal(nv.segment_minmax_bwd(cot.cuda(), garg, csr.n_rows), xg.grad)
    assert torch.equal(nv.segment_minmax_bwd(place(cot, cot.element_size()), garg, csr.n_rows), xg.grad)


# =====================================================================================================================
# ss_dup_fold_rows / ss_dup_zero_rows on hand-built runs
# =====================================================================================================================
@pytest.mark.parametrize("dtype,C", [(F32, 4), (BF16, 8), (F32, 12), (BF16, 24)], ids=lambda v: str(v).replace("torch.", ""))
def test_dup_fold_and_zero_rows_on_hand_built_runs(dtype, C):
    """a run at the very first sorted positions, a run of 40 rows, a run that ends at the last sorted position"""
    from scenesplat_amd import native as nv
    keys, order, key_of_row = rc.make_runs()
    n = len(keys)
    first = torch.cat([torch.ones(1, dtype=torch.bool), keys[1:] != keys[:-1]])
    run = torch.cumsum(first, 0) - 1
    winner = torch.empty(n, dtype=torch.int64)
    winner[order.long()] = order.long()[first][run]                        # the first entry of every run
    count = torch.bincount(winner, minlength=n)
    assert int(count.max()) == 40 and int(count[winner[order[0]]]) == 3 and int(count[winner[order[-1]]]) == 2
    assert all(int(winner[r]) == int(torch.nonzero(key_of_row == key_of_row[r])[0]) for r in (int(order[0]), int(order[-1]), int(order[n // 2])))
    x = rc.features(n, C, dtype, seed=22)
    ref = torch.zeros(n, C, dtype=F64).index_add_(0, winner, x.double())
    absum = torch.zeros(n, C, dtype=F64).index_add_(0, winner, x.double().abs())
    is_w = winner == torch.arange(n)
    runs = (keys.cuda(), order.cuda())
    xd = x.cuda()
    out = nv.dup_fold_rows(xd, runs)
    assert out.dtype == dtype and bool((out.cpu()[~is_w] == 0).all())
    _within("fold", out, ref, sum_bound(ref, absum, count, dtype))
    single = is_w & (count == 1)
    assert int(single.sum()) >= 100 and torch.equal(out.cpu()[single], x[single])
    assert torch.equal(out, nv.dup_fold_rows(xd, runs)) and torch.equal(xd.cpu(), x)
    y = xd.clone()
    assert nv.dup_zero_rows_(y, runs) is y
    assert torch.equal(y.cpu(), x * is_w.unsqueeze(1).to(dtype))
    # n = 1: a run head that is also the last sorted position
    one = (torch.tensor([5], dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int32).cuda())
    assert torch.equal(nv.dup_fold_rows(xd[:1].contiguous(), one).cpu(), x[:1])
    y1 = xd[:1].clone()
    nv.dup_zero_rows_(y1, one)
    assert torch.equal(y1.cpu(), x[:1])


def test_dup_kernels_refuse_widths_and_pointers_they_cannot_move():
    """a row that is no multiple of 16 bytes, a misaligned pointer, src == dst: status 1 (bad argument), nothing written"""
    from scenesplat_amd import _lib
    from scenesplat_amd import native as nv
    keys, order, _ = rc.make_runs()
    n = len(keys)
    kd, od = keys.cuda(), order.cuda()
    lib = nv.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    for dtype, code in ((F32, nv.F32), (BF16, nv.BF16)):
        okC, badC = (4, 3) if dtype == F32 else (8, 4)
        sentinel = torch.full((n, okC), -7.0, dtype=dtype)
        x, xbad = rc.features(n, okC, dtype, seed=24), rc.features(n, badC, dtype, seed=24)
        for src, dst, C in ((place(xbad), place(sentinel[:, :badC].contiguous()), badC),           # 12- / 8-byte rows
                            (place(x, x.element_size()), place(sentinel), okC),                   # misaligned src
                            (place(x), place(sentinel, x.element_size()), okC)):                  # misaligned dst
            before = dst.cpu().clone()
            assert lib.ss_dup_fold_rows(p(src), p(kd), p(od), p(dst), n, C, code, stream) == 1
            torch.cuda.synchronize()
            assert torch.equal(dst.cpu(), before)
        xd = place(x)
        assert lib.ss_dup_fold_rows(p(xd), p(kd), p(od), p(xd), n, okC, code, stream) == 1           # in place
        for t in (place(xbad), place(x, x.element_size())):
            before = t.cpu().clone()
            assert lib.ss_dup_zero_rows(p(kd), p(od), p(t), n, t.shape[1] * t.element_size(), stream) == 1
            with pytest.raises(_lib.NativeError):
                nv.dup_zero_rows_(t, (kd, od))
            torch.cuda.synchronize()
            assert torch.equal(t.cpu(), before)
        assert torch.equal(xd.cpu(), x)
        with pytest.raises(_lib.NativeError):
            nv.dup_fold_rows(place(xbad), (kd, od))
        with pytest.raises(_lib.NativeError):
            nv.dup_fold_rows(place(x, x.element_size()), (kd, od))
