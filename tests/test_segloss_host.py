"""CPU-side pin of tests/test_hip_segloss_edges.py: the float64 restatement of the loss pair against the reference project's recorded
values, the float32 Jaccard restatement against float64, the properties the case builders promise (lattice gaps, orders, near-tie
shares, the tile / trip counts the cases reach) and the argument contract of ss_seg_loss_fwd / ss_seg_loss_bwd on the paths that
return before any launch.  No GPU needed."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_cases as sc  # noqa: E402
from segloss_cases import U  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SS_OK, SS_ERR_ARG, SS_ERR_WORKSPACE, SS_F32, SS_BF16 = 0, 1, 3, 0, 1


@pytest.fixture(scope="module")
def golden():
    spec = importlib.util.spec_from_file_location("semseg_inputs", os.path.join(GOLDEN, "semseg_inputs.py"))
    si = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(si)
    return {name: (logits, labels, seen) for name, logits, labels, seen in si.loss_cases()}, np.load(os.path.join(GOLDEN, "semseg.npz"))


@pytest.mark.parametrize("name", ["c20", "c100", "c200", "seen", "n1"])
def test_reference_reproduces_the_recorded_reference_values(golden, name):
    cases, fx = golden
    logits, labels, seen = cases[name]
    ref = sc.reference(logits, labels, -1, seen)
    ce, lov = float(fx[f"loss_{name}_ce"]), float(fx[f"loss_{name}_lov"])
    print(f"    {name}: ce {float(ref.ce):.9f} (recorded {ce:.9f}), lovasz {float(ref.lovasz):.9f} (recorded {lov:.9f})")
    assert sc.rel_err(ref.ce, ce) < 1e-6 and sc.rel_err(ref.lovasz, lov) < 1e-6


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_jaccard_f32_stays_within_three_units_of_float64(name):
    ref = sc.case_reference(name)
    gts = ref.counts.double()[:, None]
    dev = (sc.jaccard_f32(ref.fg_sorted, gts).double() - ref.g_sorted).abs()[ref.present]
    print(f"    {name}: float32 Jaccard gradient deviates from float64 by at most {float(dev.max()) / U:.2f} * 2^-24")
    assert float(dev.max()) <= 3 * U


@pytest.mark.parametrize("n", sc.SPACED_N)
def test_spaced_cases_are_ordered_unambiguously(n):
    c = sc.case(f"spaced-{n}")
    ref = sc.case_reference(f"spaced-{n}")
    gap = (ref.err_sorted[:, :-1] - ref.err_sorted[:, 1:]).min()
    # the probabilities in CPU float32, the errors formed as the kernel forms them: the same stable descending order as float64
    p32 = c.logits.softmax(1)
    e32, _ = sc.f32_errors(p32, c.labels, ref.rows)
    order32 = ref.rows[torch.sort(e32, dim=1, descending=True, stable=True).indices]
    pdev = float((p32.double() - ref.p).abs().max())
    print(f"    n={n}: least gap of the sorted errors {float(gap) / U:.2f} * 2^-24 (pitch 0.5 / n = {0.5 / n / U:.2f}), CPU float32 "
          f"probabilities deviate by {pdev / U:.2f} * 2^-24, valid rows {ref.n_valid}, scan tiles {sc.scan_tiles(n)}")
    assert float(gap) >= 7 * U and pdev <= 3 * U
    assert torch.equal(order32, ref.order)
    assert bool(ref.present.all()) and int(ref.counts.min()) > 0.4 * ref.n_valid
    if n < 1_000_000:
        assert 0.08 * n < n - ref.n_valid < 0.12 * n
    else:
        assert n - ref.n_valid == sc.SPACED_FEW_IGNORED


def test_largest_spaced_cases_put_valid_rows_past_the_tile_scan_carry():
    """the kernel sorts the ignored rows last, so a tile holds rows whose gradient is checked only below n_valid: the second trip of
    k_lovasz_tile_scan (tiles 256 ...) is seen through glov only where n_valid exceeds 256 * 4096, and through more than one of its
    tiles where it exceeds 256 * 4096 + 4096.  With 1000 ignored rows that holds from n = 1 053 673 on: for 1056768 and 1056785, not
    for 1048576 and 1048577, whose tiles past 255 hold ignored rows only (they still run the carry and the finish sum over 257)."""
    past = {n: sc.case_reference(f"spaced-{n}").n_valid for n in sc.SPACED_N if n >= 1_000_000}
    assert past == {n: n - sc.SPACED_FEW_IGNORED for n in past}
    assert [n for n, v in past.items() if v > 256 * sc.SL_TILE + sc.SL_TILE] == [1056768, 1056785]
    assert [n for n, v in past.items() if v <= 256 * sc.SL_TILE] == [1048576, 1048577]


@pytest.mark.parametrize("name", tuple(sc.RANDOM))
def test_random_cases_hold_what_they_promise_and_stay_under_the_near_tie_cap(name):
    C, n, present, variant = sc.RANDOM[name]
    c = sc.case(name)
    for dtype in sc.case_dtypes(name):
        ref = sc.case_reference(name, dtype)
        p32 = sc.case_logits(name, dtype).float().softmax(1)
        e32, _ = sc.f32_errors(p32, c.labels, ref.rows)
        es = torch.sort(e32, dim=1, descending=True, stable=True).values[ref.present]
        share = float(sc.near_tied(es).float().mean())
        print(f"    {name} {dtype}: near-tied share {100 * share:.3f} % of {es.numel()} valid elements of present classes")
        assert share <= sc.NEAR_TIE_CAP
        assert float(e32.min()) > 0 and float(e32.max()) < 1          # no saturated row: an ignored row's key is no valid row's
    assert int((ref.counts > 0).sum()) == present
    if variant == "seen":
        seen = torch.zeros(C, dtype=torch.bool)
        seen[c.seen] = True
        assert int(((ref.counts > 0) & ~seen).sum()) == 1 and int(((ref.counts == 0) & seen).sum()) == 1
        assert int(ref.present.sum()) == present - 1
    if variant == "ig255":
        assert c.ignore == 255 and int(ref.counts[255]) == 0 and 0.08 * n < int((c.labels == 255).sum()) < 0.12 * n
        assert int(c.labels.min()) >= 0
    if variant == "noignore":
        assert c.ignore is None and ref.n_valid == n
    elif variant != "ig255":
        assert 0.08 * n < int((c.labels == -1).sum()) < 0.12 * n


def test_saturated_case_holds_what_it_promises():
    c = sc.case(sc.SATURATED)
    for dtype in ("f32", "bf16"):
        x = sc.case_logits(sc.SATURATED, dtype).float()
        ref = sc.case_reference(sc.SATURATED, dtype)
        gap = (x.max(1, keepdim=True).values - x)
        assert not bool(((gap > 80) & (gap < 120)).any()) and float(gap[c.sat_rows].max()) == 200.0
        p32 = x.softmax(1)
        live = c.sat_rows[c.labels[c.sat_rows] != -1]
        assert len(c.sat_rows) == (c.n + 2) // 3 and len(live) > 0.8 * len(c.sat_rows)
        hot, kind = c.sat_hot[c.labels[c.sat_rows] != -1], c.sat_kind[c.labels[c.sat_rows] != -1]
        # +200: p is exactly 1 on the hot class and 0 elsewhere; -200: exactly 0 on the hot class
        up = kind < 2
        assert bool((p32[live[up], hot[up]] == 1).all()) and float(p32[live[up]].sum(1).max()) == 1.0
        assert bool((p32[live[~up], hot[~up]] == 0).all())
        on_label = hot == c.labels[live]
        assert abs(float(on_label.float().mean()) - 0.5) < 0.02
        # valid rows of error exactly 0 follow ignored rows of a lower row index (the same key low word, 0xFFFFFFFF)
        e32, fg = sc.f32_errors(p32, c.labels, ref.rows)
        zero = (e32 == 0)
        first_ignored = int((c.labels == -1).nonzero()[0])
        assert int(zero.sum()) > 1000 and all(int(ref.rows[zero[k]].max()) > first_ignored for k in range(c.C))
        assert bool(((fg == 1) & zero).any()) and bool(((fg == 0) & zero).any())
        # the errors of exactly 1 form one run at the head of every class, and no other error comes within 8 * 2^-24 of it
        ones = e32 == 1.0
        assert int(ones.sum()) > 500 and bool(ones.any(1).all()) and float(e32.masked_fill(ones, 0.0).max()) < 1 - 8 * U
        # what the GPU test holds to bit-equality is everything but the exact ties the saturated rows make among themselves and the
        # few random elements near them: of the elements of unsaturated rows at most the cap is near-tied
        es, perm = torch.sort(e32, dim=1, descending=True, stable=True)
        tied = torch.zeros_like(zero).scatter_(1, perm, sc.near_tied(es))
        unsat = ~torch.isin(ref.rows, c.sat_rows)
        share = float(tied[:, unsat].float().mean())
        print(f"    saturated {dtype}: {int(zero.sum())} valid elements of error 0; near-tied share of the unsaturated rows "
              f"{100 * share:.3f} %, of all rows {100 * float(tied.float().mean()):.1f} %")
        assert share <= sc.NEAR_TIE_CAP
        assert bool(torch.isfinite(ref.g).all()) and bool(ref.present.all())


def test_near_tied_flags_by_the_ulp_of_the_larger_value():
    one = np.float32(1.0)
    below = np.nextafter(one, np.float32(0))                    # 1 - 2^-24: half the ulp of 1.0 away
    vals = [float(one), float(below), 0.75, 0.75 - 5 * 2.0 ** -24, 0.25, 0.25 - 4 * 2.0 ** -26, 0.0, 0.0]
    got = sc.near_tied(torch.tensor([vals], dtype=torch.float32))[0].tolist()
    assert got == [True, True, False, False, True, True, True, True]


def test_cases_reach_every_tile_and_trip_count():
    ns = [sc.case(name).n for name in sc.ALL_CASES]
    tiles = {sc.scan_tiles(n) for n in ns}
    print("    scan tiles:", sorted(tiles))
    assert tiles >= {1, 2, 3, 64, 65, 66, 256, 257, 258} and tiles >= {4, 67, 259}
    assert {sc.tile_scan_trips(n) for n in ns} == {1, 2}
    assert {sc.sort_tiles(n) % 4 for n in ns + list(sc.SORT_N)} == {0, 1, 2, 3}
    assert [sc.sort_tiles(n) for n in sc.SORT_N] == [1, 1, 2, 4, 6]
    assert {sc.row_trips(n) for n in ns} == {1, 2, 4, 5}
    assert [sc.row_trips(n) for n in (1, 262144, 262145, 1056785)] == [1, 1, 2, 5]
    assert [sc.row_trips(n) for n in sc.IOU_N] == [1, 1, 1, 1, 2]
    assert max(sc.case(name).C * sc.case(name).n for name in sc.ALL_CASES) < 1 << 31


def test_sort_cases_hold_what_they_promise():
    for K in sc.SORT_SEGMENTS:
        keys = sc.sort_keys(K, 2049)
        low = keys & 0xFFFFFFFF
        assert int(keys.min()) >= 0 and int(keys.max()) >> 33 == 0 and len((keys >> 32).unique()) == 2
        assert len(low[1].unique()) == 5 and bool((low[K - 1][1:] >= low[K - 1][:-1]).all())
        assert not bool((keys[K - 1][1:] >= keys[K - 1][:-1]).all())         # sorted by the low word only: bit 32 must be ignored
        assert int(low[0].max()) > 0xF0000000                                # the top digit of the 32 bits is in use


def test_bwd_reference_is_the_gradient_of_the_float64_loss():
    """autograd in float64 through the restated loop (stable order) against bwd_reference fed the float64 statistics and g"""
    name = "r20-12293-seen"
    c, ref = sc.case(name), sc.case_reference(name)
    x = c.logits.double().requires_grad_(True)
    p = x.softmax(1)
    total = torch.nn.functional.cross_entropy(x, c.labels, ignore_index=-1, reduction="sum") * 0.37
    lab = c.labels[ref.rows]
    for k in ref.present.nonzero().flatten().tolist():
        fg = (lab == k).double()
        err = (fg - p[ref.rows, k]).abs()
        total = total - 1.9 * torch.dot(err[ref.perm[k]], ref.g_sorted[k])
    total.backward()
    rowstat = torch.stack([ref.m, ref.s], 1)
    got = sc.bwd_reference(c.logits, c.labels, rowstat, ref.g, ref.present.int(), (0.37, -1.9), -1)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert bool((got[~ref.valid] == 0).all()) and int((~ref.valid).sum()) > 0


def test_iou_cases_hold_ties_and_out_of_range_values():
    for C in (2, 20, 256):
        logits, tgt, pred = sc.iou_case(257, C, -1)
        assert torch.equal(logits.to(torch.bfloat16).float(), logits)
        top = logits.max(1, keepdim=True).values
        assert int(((logits == top).sum(1) > 1).sum()) > 10                 # rows with tied maxima
        assert bool((pred >= C).any()) and bool((pred == -7).any()) and bool((tgt == C + 3).any()) and bool((tgt == -1).any())
    lg = torch.tensor([[0.5, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, -1.0, 0.0]])
    assert sc.argmax_lowest(lg).tolist() == [1, 0, 0]
    got = sc.iou_counts(np.array([0, 1, 5, -7, 1]), np.array([0, 0, 1, 1, -1]), 2, -1)
    assert got.tolist() == [[1, 0], [2, 3], [2, 2]]


# =====================================================================================================================
# argument errors of the library (every call returns before a launch)
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


def fwd_call(lib, buf, n=5, C=20, dtype=SS_F32, lovasz=1, glov=True, present=True, sums=True, rowstat=True, logits=True, labels=True,
             ws=True, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ss_seg_loss_workspace_bytes(n, C)
    return lib.ss_seg_loss_fwd(buf if logits else None, dtype, buf if labels else None, n, C, -1, None, lovasz, buf if rowstat else None,
                               buf if glov else None, buf if present else None, buf if sums else None, buf if ws else None, ws_bytes, None)


def bwd_call(lib, buf, n=5, C=20, dtype=SS_F32, glov=True, present=True, coef=True, logits=True, dlogits=True):
    return lib.ss_seg_loss_bwd(buf if logits else None, dtype, buf, n, C, -1, buf, buf if glov else None, buf if present else None,
                               buf if coef else None, buf if dlogits else None, None)


def test_seg_loss_fwd_refuses_bad_arguments(lib, buf):
    for over in (dict(C=0), dict(C=257), dict(C=-1), dict(n=-1), dict(dtype=2), dict(dtype=-1), dict(sums=False), dict(glov=False),
                 dict(present=False), dict(logits=False), dict(labels=False), dict(rowstat=False),
                 dict(C=256, n=1 << 23), dict(C=2, n=1 << 30)):
        assert fwd_call(lib, buf, **over) == SS_ERR_ARG, over
    # without the Lovasz part glov / present are not needed and C * n may pass 2^31: the next check (the workspace) answers
    for over in (dict(glov=False, present=False), dict(C=256, n=1 << 23)):
        assert fwd_call(lib, buf, lovasz=0, ws=False, **over) == SS_ERR_WORKSPACE, over
    assert fwd_call(lib, buf, C=255, n=(1 << 23), ws=False) == SS_ERR_WORKSPACE          # 255 * 2^23 < 2^31: past the argument checks
    need = lib.ss_seg_loss_workspace_bytes(5, 20)
    assert need > 0 and need % 256 == 0 and lib.ss_seg_loss_workspace_bytes(5, 0) == 0 and lib.ss_seg_loss_workspace_bytes(-1, 20) == 0
    assert fwd_call(lib, buf, ws_bytes=need - 1) == SS_ERR_WORKSPACE and fwd_call(lib, buf, ws=False) == SS_ERR_WORKSPACE
    assert fwd_call(lib, buf, ws_bytes=0) == SS_ERR_WORKSPACE
    # the workspace grows with the scan tiles and the sort tiles
    assert lib.ss_seg_loss_workspace_bytes(4097, 2) > lib.ss_seg_loss_workspace_bytes(4096, 2)
    assert lib.ss_seg_loss_workspace_bytes(1056785, 2) < 128 << 20


def test_seg_loss_bwd_refuses_bad_arguments(lib, buf):
    for over in (dict(C=0), dict(C=257), dict(n=-1), dict(dtype=2), dict(coef=False), dict(present=False), dict(logits=False),
                 dict(dlogits=False)):
        assert bwd_call(lib, buf, **over) == SS_ERR_ARG, over
    assert bwd_call(lib, buf, n=0, present=False) == SS_ERR_ARG                          # glov without present, also without rows
    for over in (dict(), dict(glov=False, present=False), dict(glov=False), dict(logits=False, dlogits=False), dict(dtype=SS_BF16)):
        assert bwd_call(lib, buf, n=0, **over) == SS_OK, over                            # n = 0: no launch


def test_seg_iou_and_argsort_refuse_bad_arguments(lib, buf):
    def iou(n=5, C=20, dtype=SS_F32, pred=False, out=True):
        return lib.ss_seg_iou(buf, dtype, buf if pred else None, buf, n, C, -1, buf if out else None, None)
    for over in (dict(C=0), dict(C=257), dict(n=-1), dict(out=False), dict(dtype=2)):
        assert iou(**over) == SS_ERR_ARG, over
    for over in (dict(n=-1), dict(n=1 << 31), dict(bits=0), dict(bits=65), dict(K=0)):
        a = dict(dict(n=5, K=2, bits=32), **over)
        assert lib.ss_argsort_i64(buf, a["K"], a["n"], a["bits"], buf, None, None, buf, 1 << 40, None) == SS_ERR_ARG, over
    assert lib.ss_argsort_i64(buf, 2, 0, 32, buf, None, None, buf, 0, None) == SS_OK
    assert lib.ss_argsort_i64(buf, 2, 5, 32, buf, None, None, buf, lib.ss_argsort_workspace_bytes(5, 2) - 1, None) == SS_ERR_WORKSPACE
