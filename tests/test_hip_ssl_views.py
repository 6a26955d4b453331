"""GPU: the kernels of the self-supervised view generator (csrc/ssl_views.hip) and the transforms over them against OUTPUTS OF THE
REFERENCE'S OWN transforms (tests/golden/ssl_views.npz + ssl_views_b.npz, written by tests/golden/make_golden_ssl_views.py: draws
recorded, replayed here through apply()), and, at the sizes without a golden, against the fp64 numpy restatements of
tests/ssl_cases.py: n = 1, 255, 256, 257 (around one workgroup), 70,001 (274 reduction blocks) and 262,401 (more rows than the
1,024 x 256 threads of a full grid: the grid-stride loop).

Bounds.  Every golden stores, beside the reference's fp32 output, the same formulas evaluated in fp64 on the same draws:
  colour     max(4 x max|reference fp32 - fp64| of that case, 5e-4) on the 0..255 scale.  The stored differences are 9e-6 .. 4.3e-5
             (chain) and 1.0e-5 .. 2.8e-5 (blur), so the floor 5e-4 of test_hip_augment.py decides everywhere; sizes without a
             golden take the floor.  After NormalizeColor the bound is divided by 127.5.
  opacity, scale, quat, normal (blur)   the same rule on their own scale: max(4 x max|reference fp32 - fp64|, 5e-4 / 255 x
             max(1, max|value|)) -- the colour floor as a relative figure (1.96e-6).  Stored differences: 1.1e-8 .. 2.7e-7.
  generator  no fp64 evaluation of the whole call is stored, so every key takes its floor: colour 5e-4 / 127.5 (it comes out of
             NormalizeColor), opacity / scale / quat 5e-4 / 255 x max(1, max|value|), coord the affine bound 2^-20 M of
             test_hip_augment.py (M = 4).
  integers   grid_coord, offsets, row order and row counts are exact.
Measured maxima on an MI355X (this file, printed by every test before it asserts): see MEASURED below.
"""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssl_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
  colour chain vs the reference, n = 600       0 (brightness) .. 6.1e-5 (contrast first of four); vs fp64 9.2e-6 .. 5.1e-5
  colour chain vs fp64, n = 1 .. 262,401       <= 6.8e-5 over the eleven step lists (largest: contrast behind hue, n = 70,001)
  jitter + grayscale through Compose            1.5e-5, fused and unfused
  blur vs the reference, nine cases             colour 1.5e-5 .. 3.1e-5 (vs fp64 <= 1.0e-5); opacity / scale / quat / normal <= 2.4e-7
                                                (vs fp64 <= 1.5e-7)
  blur vs fp64, wide case and 70,001 voxels     colour 1.1e-5, the others <= 1.3e-7; peak memory growth of the wide case (205 voxels): 22,016 bytes
  generator replay (fused = unfused)            coord and grid_coord exact; colour <= 0.12, opacity / scale / quat <= 0.09 of their bounds
"""
FLOOR = 5e-4
REL_FLOOR = FLOOR / 255.0
SIZES = [1, 255, 256, 257, 70001, 262401]
CHAIN_TAGS = ["brightness", "contrast", "saturation", "hue", "gray", "cfirst", "clast", "chue", "jgray"]


def _cuda(d):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssl_views.npz")))


@pytest.fixture(scope="module")
def fb(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssl_views_b.npz")))


@pytest.fixture(scope="module")
def lists(golden_dir):
    with open(os.path.join(golden_dir, "ssl_configs.txt")) as f:
        return ast.literal_eval(f.read())


def _steps(fx, tag):
    return list(zip(fx["cc_%s_codes" % tag].tolist(), fx["cc_%s_factors" % tag].tolist()))


def _color_bound(fx, tag):
    return max(4 * float(np.abs(fx["cc_%s_ref" % tag].astype(np.float64) - fx["cc_%s_f64" % tag]).max()), FLOOR)


# ---- colour chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CHAIN_TAGS)
def test_chain_kernel_against_the_reference(fx, tag):
    from scenesplat_amd import native as nv
    base = sc.colors(int(fx["cc_n"]), int(fx["cc_seed"]))
    c = torch.from_numpy(base.copy()).cuda()
    nv.color_chain_(c, _steps(fx, tag))
    err = float(np.abs(_np(c).astype(np.float64) - fx["cc_%s_ref" % tag]).max())
    err64 = float(np.abs(_np(c).astype(np.float64) - fx["cc_%s_f64" % tag]).max())
    print("chain %s: |kernel - reference| %.3g, |kernel - fp64| %.3g, bound %.3g" % (tag, err, err64, _color_bound(fx, tag)))
    assert err <= _color_bound(fx, tag) and err64 <= _color_bound(fx, tag)


# step lists for the sizes without a golden: every step alone, contrast first / last, three orders of all four (contrast behind hue
# among them), two contrasts in one chain (two prefix means), jitter + grayscale
COMBOS = {
    "brightness": [(1, 1.4)], "contrast": [(2, 0.6)], "saturation": [(3, 1.2)], "hue": [(4, -0.1)], "hue+": [(4, 0.5)], "gray": [(5, 0.0)],
    "cfirst": [(2, 1.37), (1, 0.7), (4, 0.08), (3, 0.85)], "clast": [(3, 1.15), (4, -0.03), (1, 1.3), (2, 0.64)],
    "chue": [(1, 1.25), (4, 0.1), (2, 1.4), (3, 0.8)], "two_means": [(2, 0.7), (1, 1.4), (2, 1.3), (5, 0.0), (2, 0.9)],
    "jgray": [(4, 0.06), (2, 0.8), (3, 1.2), (1, 0.9), (5, 0.0)],
}


@pytest.mark.parametrize("n", SIZES)
def test_chain_kernel_against_fp64_at_dispatch_edges(n):
    from scenesplat_amd import native as nv
    base = sc.colors(n, 50 + n % 7)
    dev = torch.from_numpy(base).cuda()
    worst = {}
    for name, steps in COMBOS.items():
        c = dev.clone()
        nv.color_chain_(c, steps)
        worst[name] = float(np.abs(_np(c).astype(np.float64) - sc.chain64(base, steps)).max())
    print("chain n=%d: max |kernel - fp64| per step list %s" % (n, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= FLOOR, worst


def test_chain_is_deterministic_and_leaves_nothing_behind():
    from scenesplat_amd import native as nv
    base = torch.from_numpy(sc.colors(70001, 3)).cuda()
    steps = COMBOS["two_means"] + COMBOS["chue"][:3]
    assert len(steps) == 8
    a, b = base.clone(), base.clone()
    nv.color_chain_(a, steps)
    nv.color_chain_(b, steps)
    assert torch.equal(a, b) and not torch.equal(a, base)
    with pytest.raises(RuntimeError, match="at most 8"):
        nv.color_chain_(a, steps + [(5, 0.0)])
    with pytest.raises(nv._lib.NativeError):
        nv.color_chain_(a, [(4, 0.7)])                      # hue factor outside [-0.5, 0.5]
    with pytest.raises(nv._lib.NativeError):
        nv.color_chain_(a, [(6, 1.0)])
    e = torch.empty((0, 3), device="cuda")
    assert nv.color_chain_(e, steps) is e


def test_jitter_then_grayscale_fused_and_unfused(fx):
    from scenesplat_amd.pointcept_api import Compose
    cfg = [dict(type="RandomColorJitter", brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p=0.8), dict(type="RandomColorGrayScale", p=1.0)]
    f = fx["cc_jgray_jfactors"]
    pj = dict(order=fx["cc_jgray_order"].tolist(), **{k: (None if np.isnan(v) else float(v)) for k, v in zip(sc.NAMES, f)})
    assert sc.steps_of(pj, gray=True) == _steps(fx, "jgray")
    base = sc.colors(int(fx["cc_n"]), int(fx["cc_seed"]))
    out = {}
    for fuse in (True, False):
        d = Compose(cfg, fuse=fuse)(dict(color=torch.from_numpy(base.copy()).cuda()), params=[pj, dict(fired=True)])
        out[fuse] = _np(d["color"]).astype(np.float64)
        err = float(np.abs(out[fuse] - fx["cc_jgray_ref"]).max())
        print("jitter + grayscale, fuse=%s: |transform - reference| %.3g, bound %.3g" % (fuse, err, _color_bound(fx, "jgray")))
        assert err <= _color_bound(fx, "jgray")
    assert np.abs(out[True] - out[False]).max() <= _color_bound(fx, "jgray")
    assert (out[True][:, 0] == out[True][:, 1]).all() and (out[True][:, 0] == out[True][:, 2]).all()


# ---- blur -----------------------------------------------------------------------------------------------------------------------
def _blur_bound(ref, f64, key):
    if key == "color":
        return max(4 * float(np.abs(ref.astype(np.float64) - f64).max()), FLOOR)
    return max(4 * float(np.abs(ref.astype(np.float64) - f64).max()), REL_FLOOR * max(1.0, float(np.abs(f64).max())))


@pytest.mark.parametrize("tag", list(sc.BLUR_CASES))
def test_blur_transform_against_the_reference(fx, tag):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    size, sigma, occ, origin, rule, extra = sc.BLUR_CASES[tag]
    src = sc.blur_input(tag)
    d = _cuda(src)
    held = {k: d[k] for k in ("color", "opacity", "scale", "quat", "normal")}
    op = TRANSFORMS.build(dict(type="GSGaussianBlurVoxelOpc", p=1.0, sigma=[sigma, sigma, 0], extra_keys=extra))
    out = op.apply(d, dict(fired=True, sigma=sigma))
    mask = (src["opacity"] > 0.5).ravel()
    for k in ("color",) + tuple(extra):
        assert out[k] is held[k]                                                  # in place
        got, ref, f64 = _np(out[k]).astype(np.float64), fx["blur_%s_ref_%s" % (tag, k)], fx["blur_%s_f64_%s" % (tag, k)]
        bound = _blur_bound(ref, f64, k)
        err, err64 = float(np.abs(got - ref).max()), float(np.abs(got - f64).max())
        print("blur %s %s (n=%d, masked=%d): |kernel - reference| %.3g, |kernel - fp64| %.3g, bound %.3g" % (tag, k, len(mask), mask.sum(), err, err64, bound))
        assert got.shape == ref.shape and err <= bound and err64 <= bound
        if k != "quat":
            assert np.array_equal(_np(out[k])[~mask], src[k][~mask])              # rows that are not masked are not written
    for k in ("scale", "quat", "normal", "opacity"):
        if k not in extra:
            assert np.array_equal(_np(d[k]), src[k]), k                            # keys outside extra_keys are left alone
    if tag == "none":                                                             # only the quaternion normalisation acts
        assert np.array_equal(_np(out["color"]), src["color"]) and np.allclose(np.linalg.norm(_np(out["quat"]), axis=1), 1, atol=1e-6)


def test_blur_kernel_arguments_and_status():
    from scenesplat_amd import native as nv
    src = sc.blur_input("a")
    d = _cuda(src)
    # mask=None blurs every row; colour alone
    c = d["color"].clone()
    st = nv.voxel_blur_(d["grid_coord"], None, c, 1.9)
    every = dict(src, opacity=np.ones_like(src["opacity"]))
    assert int(st) == 0 and np.abs(_np(c) - sc.blur64(every, 1.9, ())["color"]).max() <= FLOOR
    # an axis of 2^21 cells or more: the status word says so, nothing is blurred, the normalisation still runs
    gc = torch.tensor([[0, 0, 0], [1 << 21, 0, 0], [5, 1, 1]], dtype=torch.int32, device="cuda")
    color, quat = torch.rand(3, 3, device="cuda") * 255, torch.randn(3, 4, device="cuda")
    c0, q0 = color.clone(), quat.clone()
    st = nv.voxel_blur_(gc, None, color, 1.0, quat=quat, normalize_quat=True)
    assert int(st) == 1 and torch.equal(color, c0) and torch.allclose(quat, q0 / q0.norm(dim=1, keepdim=True), atol=1e-6)
    gc[1, 0] = (1 << 21) - 1
    assert int(nv.voxel_blur_(gc, None, color, 1.0)) == 0 and not torch.equal(color, c0)
    with pytest.raises(nv._lib.NativeError):
        nv.voxel_blur_(gc, None, color, 4.3)                                      # r = 9 > 8
    with pytest.raises(RuntimeError, match="grid_coord"):
        nv.voxel_blur_(gc.long(), None, color, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.voxel_blur_(gc.cpu(), None, color, 1.0)
    e = torch.empty((0, 3), device="cuda")
    nv.voxel_blur_(torch.empty((0, 3), dtype=torch.int32, device="cuda"), None, e, 1.0)


def test_blur_of_a_wide_sparse_view_needs_memory_for_its_voxels_only():
    """Two clusters 2,000 cells apart on every axis: the reference's dense grid over the box would hold 2006^3 x 12 floats (hundreds
    of GB); the hash needs a few KB.  No golden can exist for this case: the fp64 restatement is the yardstick."""
    from scenesplat_amd import native as nv
    src = sc.wide_input()
    n = len(src["color"])
    assert 150 <= n <= 260 and (src["grid_coord"].max(0) - src["grid_coord"].min(0) >= 2000).all()
    d = _cuda(src)
    mask = (d["opacity"] > 0.5).reshape(-1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    st = nv.voxel_blur_(d["grid_coord"], mask, d["color"], 1.3, opacity=d["opacity"], scale=d["scale"], quat=d["quat"], normal=d["normal"],
                        normalize_quat=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print("wide blur: n=%d, peak device memory growth %d bytes" % (n, grown))
    assert int(st) == 0 and grown < 4 << 20
    want = sc.blur64(src, 1.3, ("opacity", "scale", "quat", "normal"))
    for k in ("color", "opacity", "scale", "quat", "normal"):
        err = float(np.abs(_np(d[k]).astype(np.float64) - want[k]).max())
        bound = FLOOR if k == "color" else REL_FLOOR * max(1.0, float(np.abs(want[k]).max()))
        print("wide blur %s: |kernel - fp64| %.3g, bound %.3g" % (k, err, bound))
        assert err <= bound, k


@pytest.mark.parametrize("n", [1, 257, 70001])
def test_blur_kernel_against_fp64_on_a_shell(n):
    """more than one workgroup, and the grid-stride loop of the gather: voxels on a thin random shell, sigma 0.8 (r = 2)"""
    from scenesplat_amd import native as nv
    g = np.random.RandomState(n)
    side = max(2, int(np.ceil((n / 0.22) ** (1 / 3))))
    pts = np.argwhere(g.rand(side, side, side) < 0.32)
    assert len(pts) >= n
    pts = pts[g.permutation(len(pts))[:n]]
    m = len(pts)
    src = dict(grid_coord=(pts - 11).astype(np.int32), color=(g.rand(m, 3) * 255).astype(np.float32), opacity=g.rand(m, 1).astype(np.float32),
               scale=g.rand(m, 3).astype(np.float32))
    d = _cuda(src)
    st = nv.voxel_blur_(d["grid_coord"], (d["opacity"] > 0.5).reshape(-1), d["color"], 0.8, opacity=d["opacity"], scale=d["scale"])
    want = sc.blur64(src, 0.8, ("opacity", "scale"))
    err = {k: float(np.abs(_np(d[k]).astype(np.float64) - want[k]).max()) for k in ("color", "opacity", "scale")}
    print("shell blur n=%d: |kernel - fp64| %s" % (m, err))
    assert int(st) == 0 and err["color"] <= FLOOR and err["opacity"] <= REL_FLOOR and err["scale"] <= REL_FLOOR


# ---- SphereCropRandomMaxPoints and the generator --------------------------------------------------------------------------------
def test_sphere_crop_random_max_points_replays_the_reference(fx):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    src = sc.crop_fixture(int(fx["crop_n"]), int(fx["crop_seed"]))
    op = TRANSFORMS.build(dict(type="SphereCropRandomMaxPoints", random_scale=(0.4, 1.0), point_max=1500))
    out = op.apply(_cuda(src), dict(point_max=int(fx["crop_point_max"]), center_index=int(fx["crop_center_index"])))
    idx = fx["crop_idx"]
    assert len(idx) == int(fx["crop_point_max"]) < len(src["coord"]) and set(out) == set(src)
    for k in ("coord", "grid_coord", "color", "quat", "scale", "opacity", "sh", "normal", "lang_feat", "lang_feat_64", "valid_feat_mask", "segment"):
        assert np.array_equal(_np(out[k]), src[k][idx]), k                      # same rows in the same (ascending-distance) order
    assert out["name"] == src["name"]
    small = op.apply(_cuda(src), dict(point_max=len(src["coord"]), u=0.3))      # not more points than point_max': untouched
    assert all(np.array_equal(_np(small[k]), src[k]) for k in ("coord", "sh", "segment"))
    drawn = op(_cuda(src), rng=np.random.default_rng(4))                         # a drawn call: 0.4 .. 1.0 of point_max rows
    assert 600 <= drawn["coord"].shape[0] <= 1500 and drawn["sh"].shape[0] == drawn["coord"].shape[0]


RUNS = ("global_base", "local_base", "global0", "global1", "local0", "local1", "local2")
SUB = dict(global_base="global_base_transform", local_base="local_base_transform", global0="global_transform0", global1="global_transform1",
           local0="local_transform", local1="local_transform", local2="local_transform")


def _recorded_params(fb, gcfg, run):
    out = []
    for j, c in enumerate(gcfg[SUB[run]]):
        key, t = "gen_%s_%d_" % (run, j), c["type"]
        if t == "RandomFlip":
            out.append(dict(flip_x=bool(fb[key + "flip"][0]), flip_y=bool(fb[key + "flip"][1])))
        elif t == "SphereCropRandomMaxPoints":
            out.append(dict(point_max=int(fb[key + "point_max"]), center_index=int(fb[key + "center_index"])))
        elif t == "RandomColorJitter":
            out.append(dict(order=fb[key + "order"].tolist(),
                            **{k: (None if np.isnan(v) else float(v)) for k, v in zip(sc.NAMES, fb[key + "factors"])}))
        elif t in ("RandomColorGrayScale", "RandomColorSolarize"):
            out.append(dict(fired=bool(fb[key + "fired"])))
        elif t == "GridSample":
            out.append(dict(idx=fb[key + "idx"]))
        elif t == "GSGaussianBlurVoxelOpc":
            out.append(dict(fired=bool(fb[key + "fired"]), sigma=None if np.isnan(fb[key + "sigma"]) else float(fb[key + "sigma"])))
        else:
            out.append({})
    return out


@pytest.mark.parametrize("fuse", [True, False])
def test_generator_replays_the_reference_call(fb, fuse):
    from scenesplat_amd.pointcept_api import Compose
    gcfg = ast.literal_eval(str(fb["gen_cfg"]))
    src = sc.fixture(int(fb["gen_n"]), int(fb["gen_seed"]))
    comp = Compose([gcfg], fuse=fuse)
    d = _cuda(src)
    out = comp(d, params=[dict(views=[_recorded_params(fb, gcfg, r) for r in RUNS])])
    assert set(out) == set(src) | set(fb["gen_out_keys"].tolist())
    for k, v in src.items():                                                     # every other entry is left in place, untouched
        assert (out[k] == v) if isinstance(v, str) else np.array_equal(_np(out[k]), v), k
    views = {"global_crop0": "global0", "global_crop1": "global1", "local_crop0": "local0", "local_crop1": "local1", "local_crop2": "local2"}
    worst = {}
    for view, run in views.items():
        for key in ("coord", "color", "scale", "quat", "opacity", "grid_coord"):
            got, want = _np(out[view + "_" + key]), fb["out_%s_%s" % (view, key)]
            assert got.shape == want.shape, (view, key)
            if key == "grid_coord":
                assert np.array_equal(got, want), view
                continue
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            if key == "coord":
                bound = 2.0 ** -20 * 4.0
            elif key == "color":
                bound = FLOOR / 127.5
            else:
                bound = REL_FLOOR * max(1.0, float(np.abs(want).max()))
            worst[view + "_" + key] = float((err / bound).max())
            assert (err <= bound).all(), (view, key, float(err.max()), int(np.argmax(err.max(1))))
    print("generator fuse=%s: max error / bound per output %s" % (fuse, {k: "%.3g" % v for k, v in worst.items()}))


def test_the_shipped_ssl_lists_run_on_device_tensors(lists):
    from scenesplat_amd.pointcept_api import Compose
    seen = set()
    for name, cfg in lists.items():
        if name.split("::")[0] in seen:
            continue
        seen.add(name.split("::")[0])
        out = Compose(cfg, seed=5)(_cuda(sc.fixture(3000, 35)))
        views = ["global_crop0", "global_crop1", "local_crop0", "local_crop1", "local_crop2"]
        for v in views:
            n = out[v + "_coord"].shape[0]
            assert 0 < n <= 3000 and out[v + "_offset"].tolist() == [n] and out[v + "_feat"].shape == (n, 11)
            assert out[v + "_grid_coord"].shape == (n, 3) and out[v + "_grid_coord"].dtype == torch.int32
            assert torch.isfinite(out[v + "_feat"]).all() and out[v + "_color"].abs().max() <= 1.0 + 1e-6
            assert torch.unique(out[v + "_grid_coord"], dim=0).shape[0] == n
        assert "coord" not in out and all(k.startswith(tuple(views)) for k in out)
    assert len(seen) == 3
