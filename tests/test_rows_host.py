"""CPU-side pin of tests/test_hip_rows_edges.py: its float64 restatements agree with the oracle's segment_csr, and its bounds
separate the arithmetic csrc/rows.hip documents (fp32 accumulation in CSR order, one rounding on store) from a bf16-accumulating
loop.  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_cases as rc  # noqa: E402
import test_hip_rows_edges as E  # noqa: E402
from rows_cases import BF16, F32, F64  # noqa: E402

from oracle import ops as oops  # noqa: E402


@pytest.mark.parametrize("permute", [True, False], ids=E._pid)
def test_restatements_agree_with_the_oracle(permute):
    """sum, mean, min, max on the generated layout without empty segments; fp32 draws widened to float64: no ties, no NaN"""
    csr = rc.make_csr(permute, empty=False)
    assert int(csr.lens.min()) >= 1 and int(csr.lens.max()) == rc.LONG_LEN and set(rc.SEG_LENGTHS[1:]) <= set(csr.lens.tolist())
    x = rc.features(csr.n_rows, 5, F32, seed=1)
    xs = x.double()[rc.rows_in_csr_order(csr)]
    ref, absum = E.ref_segment_sum(x, csr)
    assert torch.allclose(ref, oops.segment_csr(xs, csr.ptr, "sum"), rtol=1e-12, atol=0)
    assert torch.allclose(ref / csr.lens.double().reshape(-1, 1), oops.segment_csr(xs, csr.ptr, "mean"), rtol=1e-12, atol=0)
    assert torch.allclose(absum, oops.segment_csr(xs.abs(), csr.ptr, "sum"), rtol=1e-12, atol=0)
    for is_max in (False, True):
        val, arg = E.ref_segment_minmax(x, csr, is_max)
        assert torch.equal(val, oops.segment_csr(xs, csr.ptr, "max" if is_max else "min"))
        # the arg rows hold the value and lie in their segment
        cols = torch.arange(5).expand(csr.n, 5)
        assert torch.equal(x.double()[arg, cols], val) and torch.equal(csr.cluster.long()[arg], torch.arange(csr.n).reshape(-1, 1).expand(csr.n, 5))


def test_minmax_restatement_on_ties_nan_and_empty_segments():
    """what the oracle leaves open, by hand: first attaining row in CSR order, the first NaN wins, empty -> (0, -1)"""
    ptr = torch.tensor([0, 0, 4, 9, 9])
    idx = torch.tensor([8, 2, 5, 0, 7, 1, 6, 3, 4])
    csr = types.SimpleNamespace(n=4, n_rows=9, ptr=ptr, indices=idx.to(torch.int32))
    x = torch.zeros(9, 2)
    x[[8, 2, 5, 0], 0] = torch.tensor([1.0, 3.0, 3.0, 2.0])                  # max tie: rows 2 and 5 -> 2 first in CSR order AND lowest
    x[[8, 2, 5, 0], 1] = torch.tensor([4.0, 1.0, 4.0, 0.0])                  # max tie: rows 8 and 5 -> 8 first in CSR order, 5 lowest
    x[[7, 1, 6, 3, 4], 0] = torch.tensor([1.0, float("nan"), float("inf"), float("nan"), 0.0])
    x[[7, 1, 6, 3, 4], 1] = torch.tensor([-1.0, float("-inf"), 5.0, float("-inf"), float("inf")])
    val, arg = E.ref_segment_minmax(x, csr, True)
    assert arg.tolist() == [[-1, -1], [2, 8], [1, 4], [-1, -1]]
    assert val[1].tolist() == [3.0, 4.0] and bool(torch.isnan(val[2, 0])) and val[2, 1] == float("inf") and val[0].tolist() == [0.0, 0.0]
    assert E.ref_segment_minmax(x, csr, True, lowest_row=True)[1][1].tolist() == [2, 5]
    val, arg = E.ref_segment_minmax(x, csr, False)
    assert arg.tolist() == [[-1, -1], [8, 0], [1, 1], [-1, -1]] and val[2, 1] == float("-inf") and bool(torch.isnan(val[2, 0]))


# ---- the kernels' loop, restated with a chosen accumulator ---------------------------------------------------------------------
def accumulate(x, csr, acc_dtype):
    """out[s] = x[rows[b]] + x[rows[b + 1]] + ... left to right, every partial sum rounded to acc_dtype (F32: numpy float32 adds;
    BF16: an fp32 add rounded to bf16 each step); -> (n_seg, C) float32 holding the final accumulator"""
    xs = x.float()[rc.rows_in_csr_order(csr)]
    C = x.shape[1]
    acc = torch.zeros(csr.n, C, dtype=F32)
    lens, ptr = csr.lens, csr.ptr[:-1]
    for j in range(int(lens.max())):
        live = torch.nonzero(lens > j).flatten()
        nxt = acc[live].numpy() + xs[ptr[live] + j].numpy()                  # one IEEE fp32 add per element
        assert nxt.dtype == np.float32
        nxt = torch.from_numpy(nxt)
        acc[live] = nxt.to(BF16).float() if acc_dtype == BF16 else nxt
    return acc


def finish(acc, lens, mean, dtype):
    if mean:
        acc = torch.from_numpy(acc.numpy() / lens.clamp(min=1).float().reshape(-1, 1).numpy())
    return acc.to(dtype)                                                      # one rounding on store


@pytest.mark.parametrize("case", [(F32, 1), (F32, 5), (BF16, 3), (BF16, 8)], ids=lambda c: rc.case_id(c + (16,)))
def test_fp32_accumulation_meets_the_bounds_and_bf16_accumulation_does_not(case):
    dtype, C = case
    csr, x, ref, absum = E.reduce_reference(dtype, C, True)
    L = csr.lens.clamp(min=1).double().reshape(-1, 1)
    good = accumulate(x, csr, F32)
    E._within("sum", finish(good, csr.lens, False, dtype), ref, E.sum_bound(ref, absum, csr.lens, dtype))
    E._within("mean", finish(good, csr.lens, True, dtype), ref / L, E.mean_bound(ref, absum, csr.lens, dtype))
    if dtype != BF16:
        return
    bad = accumulate(x, csr, BF16)
    for mean, r, bound in ((False, ref, E.sum_bound(ref, absum, csr.lens, dtype)), (True, ref / L, E.mean_bound(ref, absum, csr.lens, dtype))):
        over = (finish(bad, csr.lens, mean, dtype).double() - r).abs() > bound
        # 5000 values near 1 stall at 256 in a bf16 accumulator: every channel of the long segment is far outside
        assert bool(over[rc.LONG_AT].all())
        assert float(finish(bad, csr.lens, False, dtype)[rc.LONG_AT].max()) <= 512
        # from 128 on the accumulator moves in whole units (from 256 in twos): the 0.1-sigma part of ~130 addends is lost, an error of
        # about one unit against a bound of 2^-8 * 257 = 1.0 -> violated in a large share of the 257-row segments' channels
        seg257 = csr.lens == 257
        assert int(seg257.sum()) >= 10 and float(over[seg257].double().mean()) > 0.2, float(over[seg257].double().mean())
        assert bool(over[seg257].any(1).double().mean() > 0.5)
        print("    bf16 accumulation: share of elements outside the bound, by length:",
              {int(l): round(float(over[csr.lens == l].double().mean()), 3) for l in csr.lens.unique() if l > 0})
