"""GPU: the kernels behind the transforms beyond the shipped lists (ss_aug_hsv, ss_aug_moments, ss_instance_boxes / ss_instance_scatter
in csrc/augment.hip) and the transforms over them, against OUTPUTS OF THE REFERENCE'S OWN transforms (tests/golden/augment_rest.npz,
written by tests/golden/make_golden_augment_rest.py) and against the fp64 numpy restatements of tests/test_augment_rest_host.py
(checked there, on the CPU, against the same recorded outputs) at test_hip_augment.SIZES.

Bounds:
  HSV        bit-equal: the kernel is the restatement's fp64 operations in the restatement's order, and both truncate
  moments    sums 1e-12 relative; the largest squared norm equal to numpy's fp64 value of the same expression
  coord      test_hip_augment's 2^-20 M (M = max over points and axes of sum_j |A_ij| |x_j| + |b_i| of the affine the pass applies),
             once per pass; against the reference's recorded output + the reference's own recorded distance from fp64
  scale      2^-20 relative (the same bound on a product of two factors)
  instance   dense ids, boxes and classes exact; centroids 1 ulp (fp32) from the fp64 mean, + the recorded distance against the golden
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_augment_rest_host as H  # noqa: E402
import test_hip_augment as A  # noqa: E402
from test_hip_augment import EPS20, SIZES, _cuda, _np  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "augment_rest.npz")))


@pytest.fixture(scope="module")
def base(fx):
    return H.fixture_rest(fx)


@pytest.fixture(scope="module")
def lists(golden_dir):
    import ast
    with open(os.path.join(golden_dir, "augment_configs.txt")) as f:
        return ast.literal_eval(f.read())


def _build(**cfg):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    return TRANSFORMS.build(cfg)


# ---- HueSaturationTranslation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw", [("hsa", dict(hue_max=0.2, saturation_max=0.2)), ("hsb", {})])
def test_hsv_is_bit_equal_to_the_reference(fx, base, tag, kw):
    op = _build(type="HueSaturationTranslation", **kw)
    data = _cuda({**base, "color": fx["hsv_in"]})
    out = op.apply(data, dict(hue_val=float(fx[tag + "_hue_val"]), sat_ratio=float(fx[tag + "_sat_ratio"])))
    assert out is data and np.array_equal(_np(out["color"]), fx[tag + "_color"].astype(np.float32))
    for k in ("coord", "quat", "scale", "opacity", "normal"):
        assert np.array_equal(_np(out[k]), base[k]), k


def _colors(n, seed):
    g = np.random.default_rng(seed)
    c = (g.random((n, 3)) * 255).astype(np.float32)
    k = n // 4
    c[:k] = np.floor(c[:k])                                              # whole colour values, as the datasets hand them over
    c[k:2 * k, 1] = c[k:2 * k, 0]                                        # ties of the two leading channels
    c[2 * k:2 * k + k // 2] = c[2 * k:2 * k + k // 2, :1]                # grey rows
    return c


@pytest.mark.parametrize("n", SIZES)
def test_hsv_kernel_is_bit_equal_to_fp64_numpy(n):
    from scenesplat_amd import native as nv
    c = _colors(n, n)
    for hue_val in (-0.5, 0.0, 0.5):
        for sat_ratio in (0.8, 1.2):
            got = _np(nv.aug_hsv_(torch.from_numpy(c.copy()).cuda(), hue_val, sat_ratio))
            assert np.array_equal(got, H.hsv64(c, hue_val, sat_ratio)), (n, hue_val, sat_ratio)


def test_hsv_saturates_outside_the_colour_range_and_takes_no_rows():
    from scenesplat_amd import native as nv
    c = np.array([[300.0, 0.0, 0.0], [-4.0, -4.0, -4.0], [255.0, 255.0, 255.0]], dtype=np.float32)
    assert np.array_equal(_np(nv.aug_hsv_(torch.from_numpy(c).cuda(), 0.0, 1.0)), [[255, 0, 0], [0, 0, 0], [255, 255, 255]])
    assert nv.aug_hsv_(torch.empty((0, 3), device="cuda"), 0.1, 1.0).shape == (0, 3)


def test_hsv_after_the_chromatic_trio_sees_their_flushed_output(base):
    from scenesplat_amd.pointcept_api import Compose
    trio = [dict(type="ChromaticAutoContrast", p=1.0), dict(type="ChromaticTranslation", p=1.0), dict(type="ChromaticJitter", p=1.0, std=0.05)]
    hst = dict(type="HueSaturationTranslation", hue_max=0.2, saturation_max=0.2)
    params = [dict(fired=True, blend=0.4), dict(fired=True, tr=[3.0, -5.0, 7.5]), dict(fired=True, seed=9), dict(hue_val=0.13, sat_ratio=1.1)]
    fused = Compose(trio + [hst])(_cuda(base), params=params)["color"]
    mid = Compose(trio)(_cuda(base), params=params[:3])
    want = Compose([hst], fuse=False)(dict(color=mid["color"].clone()), params=params[3:])["color"]
    assert torch.equal(fused, want) and torch.equal(fused, fused.floor())
    raw = Compose([hst])(_cuda(base), params=params[3:])["color"]
    assert not torch.equal(raw, fused)


def test_random_color_drop_and_point_clip_match_the_reference(fx, base):
    op = _build(type="RandomColorDrop", p=0.2, color_augment=0.25)
    assert np.array_equal(_np(op.apply(_cuda(base), dict(fired=True))["color"]), fx["cd_color"])
    assert np.array_equal(_np(op.apply(_cuda(base), dict(fired=False))["color"]), base["color"])
    out = _build(type="PointClip", point_cloud_range=tuple(fx["pcl_range"])).apply(_cuda(base), {})
    assert np.array_equal(_np(out["coord"]), fx["pcl_coord"])


# ---- ss_aug_moments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_moments_match_fp64_numpy_and_repeat(n):
    from scenesplat_amd import native as nv
    g = np.random.default_rng(n)
    x = (g.standard_normal((n, 3)) * [4.0, 3.0, 1.5] + [1.0, -2.0, 0.5]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    _, rot, smul, _ = A._rand_rigid(g)
    Am, b = smul[:, None] * rot, np.array([25.0, -30.0, 35.0]) + g.uniform(-1, 1, 3)     # keeps every mean away from cancellation
    x64 = x.astype(np.float64)
    for affine in (None, list(Am.reshape(-1)) + list(b)):
        p = x64
        if affine is not None:                                           # the header's order, no fused multiply-add in numpy
            p = np.stack([((Am[i, 0] * x64[:, 0] + Am[i, 1] * x64[:, 1]) + Am[i, 2] * x64[:, 2]) + b[i] for i in range(3)], 1)
        want_sum = p.sum(0)
        want_max = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).max()
        got = nv.aug_moments(xd, affine)
        assert got.dtype == torch.float64 and tuple(got.shape) == (4,)
        g64 = _np(got)
        assert (np.abs(g64[:3] - want_sum) <= 1e-12 * np.abs(want_sum)).all(), (n, g64[:3], want_sum)
        assert g64[3] == want_max, (n, g64[3], want_max)
        assert torch.equal(got, nv.aug_moments(xd, affine))              # the same bits on every run


# ---- NormalizeCoord / PositiveShift ---------------------------------------------------------------------------------------------
def _np_hooks(x):
    return dict(bbox_fn=lambda A_, b: np.concatenate([(x @ A_.T + b).min(0), (x @ A_.T + b).max(0)]),
                moments_fn=lambda A_, b: np.concatenate([(x @ A_.T + b).mean(0), [(((x @ A_.T + b) ** 2).sum(1)).max()]]))


def _host_state(ops, params, coord):
    from scenesplat_amd.pointcept_api import transform as tf
    st = tf.RigidState(**_np_hooks(coord.astype(np.float64)))
    for op, p in zip(ops, params):
        op.fold(st, dict(coord=None), p)
    return st


NC_CHAIN = [dict(type="CenterShift", apply_z=True), dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
            dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="NormalizeCoord")]


@pytest.mark.parametrize("tag", ["nc", "ncs"])
def test_normalize_coord_alone_and_folded_matches_fp64_and_the_reference(fx, base, tag):
    from scenesplat_amd.pointcept_api import Compose
    from scenesplat_amd import native as nv
    cfg = NC_CHAIN[3:] if tag == "nc" else NC_CHAIN
    params = [{}] if tag == "nc" else [{}, dict(fired=True, angle=float(fx["ncs_angle"])), dict(scale=fx["ncs_scale_draw"].tolist()), {}]
    comp = Compose(cfg)
    st = _host_state(comp.transforms, params, base["coord"])
    bound = A._affine_bound(st.A, st.b, base["coord"])
    x64 = base["coord"].astype(np.float64)
    want = x64 @ st.A.T + st.b                                           # the fp64 restatement: the host composition on numpy reductions
    if tag == "nc":
        assert np.abs(want - H.normalize64(base["coord"], 0.0)[0]).max() <= 1e-14
    assert abs(np.sqrt((want ** 2).sum(1).max()) - 1) <= 1e-14 and np.abs(want.mean(0)).max() <= 1e-14
    calls = []
    orig = nv.aug_gaussians_
    nv.aug_gaussians_ = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    try:
        out = comp(_cuda(base), params=params)
    finally:
        nv.aug_gaussians_ = orig
    assert len(calls) == 1                                               # the normalisation rides the run's one pass
    got = _np(out["coord"]).astype(np.float64)
    assert np.abs(got - want).max() <= bound, (tag, np.abs(got - want).max(), bound)
    assert np.abs(got - fx[tag + "_coord"]).max() <= bound + float(fx[tag + "_ref_err"])
    want_scale = base["scale"].astype(np.float64) * st.smul
    gs = _np(out["scale"]).astype(np.float64)
    assert np.abs(gs / want_scale - 1).max() <= EPS20
    assert np.abs(gs / fx[tag + "_scale"].astype(np.float64) - 1).max() <= EPS20 + float(fx[tag + "_scale_ref_err"])
    for k in ("color", "quat", "opacity") if tag == "nc" else ("color", "opacity"):
        assert np.array_equal(_np(out[k]), base[k]), k


def test_positive_shift_matches_the_reference_and_leaves_the_cloud(fx, base):
    data = _cuda(base)
    data["pc_coord"] = data["coord"][:50].clone()
    out = _build(type="PositiveShift").apply(data, {})
    lo = base["coord"].min(0).astype(np.float64)
    bound = A._affine_bound(np.eye(3), -lo, base["coord"])
    assert np.abs(_np(out["coord"]).astype(np.float64) - fx["ps_coord"]).max() <= bound
    assert np.array_equal(_np(out["pc_coord"]), base["coord"][:50])
    out = _build(type="NormalizeCoord").apply(out, {})
    assert np.array_equal(_np(out["pc_coord"]), base["coord"][:50])


# ---- InstanceParser -------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _run_parser(coord, segment, instance, ignore=(-1, 0, 1), inst_ignore=-1):
    op = _build(type="InstanceParser", segment_ignore_index=ignore, instance_ignore_index=inst_ignore)
    data = _cuda(dict(coord=coord, segment=segment, instance=instance))
    inst_t = data["instance"]
    out = op.apply(data, {})
    assert out["instance"] is inst_t                                     # rewritten in place
    assert out["instance_centroid"].dtype == torch.float32 and out["bbox"].dtype == torch.float32
    return out


def _check_parser(out, coord, segment, instance, ignore=(-1, 0, 1), inst_ignore=-1):
    inst, cen, box = H.instance64(coord, segment, instance, ignore, inst_ignore)
    assert np.array_equal(_np(out["instance"]).astype(np.int64), inst)
    assert tuple(out["bbox"].shape) == (len(box), 8) and np.array_equal(_np(out["bbox"]), box)
    got = _np(out["instance_centroid"]).astype(np.float64)
    assert got.shape == cen.shape and (np.abs(got - cen) <= _ulp32(cen)).all()
    assert (got[inst == inst_ignore] == inst_ignore).all()               # ignored rows: the ignore value, exactly
    return inst, cen, box


def test_instance_parser_matches_the_reference(fx, base):
    out = _run_parser(base["coord"], base["segment"], base["instance"])
    assert np.array_equal(_np(out["instance"]), fx["ip_instance"])
    assert np.array_equal(_np(out["bbox"])[:, :7], fx["ip_bbox"][:, :7]) and np.array_equal(_np(out["bbox"])[:, 7], fx["ip_bbox"][:, 7])
    _, cen, _ = _check_parser(out, base["coord"], base["segment"], base["instance"])
    got = _np(out["instance_centroid"]).astype(np.float64)
    assert (np.abs(got - fx["ip_centroid"]) <= float(fx["ip_ref_err"]) + _ulp32(cen)).all()
    again = _run_parser(base["coord"], base["segment"], base["instance"])
    for k in ("instance", "instance_centroid", "bbox"):
        assert torch.equal(out[k], again[k]), k


def _parser_case(name):
    g = np.random.default_rng(len(name))
    if name == "one_row":
        return g.random((1, 3)).astype(np.float32), np.array([5]), np.array([7])
    if name == "one_row_ignored":
        return g.random((1, 3)).astype(np.float32), np.array([1]), np.array([7])
    if name == "all_ignored":
        return g.random((65, 3)).astype(np.float32), g.choice([-1, 0, 1], 65), g.integers(0, 5, 65)
    if name == "one_instance":
        return g.random((300, 3)).astype(np.float32), g.integers(-1, 20, 300), np.full(300, 12)
    if name == "two_at_65":
        return g.random((65, 3)).astype(np.float32), g.integers(2, 20, 65), g.choice([3, 90], 65)
    if name == "minus_one_id":
        return g.random((500, 3)).astype(np.float32), g.integers(-1, 6, 500), g.choice([-1, 2, 5], 500)
    if name == "int32":
        return g.random((500, 3)).astype(np.float32), g.integers(-1, 6, 500).astype(np.int32), g.choice([-7, 2, 5], 500).astype(np.int32)
    assert name == "300_at_70001"                                        # one instance of 60,000 rows, 299 small ones
    n = 70001
    inst = np.concatenate([np.full(60000, 17), 1000 + 3 * g.integers(0, 299, n - 60000)])
    inst[60000:60299] = 1000 + 3 * np.arange(299)                        # every small id is there
    return (g.standard_normal((n, 3)) * [4.0, 3.0, 1.5]).astype(np.float32), g.integers(-1, 20, n), g.permutation(inst)


@pytest.mark.parametrize("name", ["one_row", "one_row_ignored", "all_ignored", "one_instance", "two_at_65", "minus_one_id", "int32",
                                  "300_at_70001"])
def test_instance_parser_matches_numpy_at_edge_shapes(name):
    coord, segment, instance = _parser_case(name)
    out = _run_parser(coord, segment, instance)
    inst, cen, box = _check_parser(out, coord, segment, instance)
    K = {"one_row": 1, "one_row_ignored": 0, "all_ignored": 0, "one_instance": 1, "two_at_65": 2, "minus_one_id": 3, "int32": 3,
         "300_at_70001": 300}[name]
    assert len(box) == K and out["instance"].dtype == (torch.int32 if name == "int32" else torch.int64)
    if K == 0:
        assert tuple(out["bbox"].shape) == (0, 8) and (_np(out["instance"]) == -1).all() and (_np(out["instance_centroid"]) == -1).all()
    if name == "minus_one_id":
        valid = ~np.isin(segment, (-1, 0, 1))
        assert (instance[valid] == -1).any() and (inst[valid & (instance == -1)] == 0).all()
    again = _run_parser(coord, segment, instance)
    for k in ("instance", "instance_centroid", "bbox"):
        assert torch.equal(out[k], again[k]), k


def test_instance_parser_other_ignore_indices():
    g = np.random.default_rng(4)
    coord, segment, instance = g.random((400, 3)).astype(np.float32), g.integers(0, 12, 400), g.integers(0, 9, 400)
    out = _run_parser(coord, segment, instance, ignore=(2, 7, 9), inst_ignore=-100)
    _, _, box = _check_parser(out, coord, segment, instance, ignore=(2, 7, 9), inst_ignore=-100)
    assert box[:, 7].max() <= 11 - 3 and (_np(out["instance"]) == -100).any()


# ---- ShufflePoint / CropBoundary --------------------------------------------------------------------------------------------------
ROW_KEYS = ("coord", "color", "normal", "segment", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask")


def test_shuffle_point_replays_the_reference_and_moves_every_key(fx, base):
    op = _build(type="ShufflePoint")
    perm = fx["sp_idx"]
    out = op.apply(_cuda(base), dict(idx=perm))
    for k in ROW_KEYS:                         # the reference's own keys as the reference has them; the Gaussians' rows follow their coord
        assert np.array_equal(_np(out[k]), base[k][perm]), k
    assert out["name"] == base["name"]
    n = len(perm)
    runs = [op.apply(_cuda({**base, "instance": np.arange(n)}), dict(seed=s)) for s in (5, 5, 6)]
    p0, p1, p2 = (_np(r["instance"]) for r in runs)
    assert np.array_equal(np.sort(p0), np.arange(n)) and np.array_equal(p0, p1) and not np.array_equal(p0, p2)
    assert not np.array_equal(p0, np.arange(n))
    for k in ROW_KEYS[:4] + ROW_KEYS[5:]:
        assert np.array_equal(_np(runs[0][k]), base[k][p0]), k


def test_crop_boundary_keeps_the_reference_rows_of_every_key(fx, base):
    out = _build(type="CropBoundary").apply(_cuda(base), {})
    keep = fx["cb_idx"]
    assert np.array_equal(keep, np.nonzero((base["segment"] != 0) & (base["segment"] != 1))[0])
    for k in ROW_KEYS:
        assert np.array_equal(_np(out[k]), base[k][keep]), k


def test_contrastive_views_generator_makes_two_views(base):
    from scenesplat_amd.pointcept_api import Compose
    cfg = [dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True), dict(type="NormalizeCoord")]
    gen = dict(type="ContrastiveViewsGenerator", view_keys=("coord", "color"), view_trans_cfg=cfg)
    out = Compose([gen], seed=3)(_cuda(base))
    assert np.array_equal(_np(out["coord"]), base["coord"]) and np.array_equal(_np(out["view1_color"]), base["color"])
    v1, v2 = _np(out["view1_coord"]).astype(np.float64), _np(out["view2_coord"]).astype(np.float64)
    assert not np.allclose(v1, v2, atol=1e-3)                            # the second view draws on: another angle
    for v in (v1, v2):
        assert abs(np.sqrt((v ** 2).sum(1).max()) - 1) <= 4 * EPS20 and np.abs(v.mean(0)).max() <= 4 * EPS20
    rng = np.random.default_rng(3)
    rot = Compose(cfg).transforms[0]
    angles = [rot.draw(rng, {})["angle"] for _ in range(2)]
    for v, a in zip((v1, v2), angles):
        c, s = np.cos(a), np.sin(a)
        want = H.normalize64(base["coord"].astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T, 0.0)[0]
        assert np.abs(v - want).max() <= 4 * EPS20                       # |A x| + |b| <= 2 for a normalised cloud, two roundings of slack


# ---- a shipped list with the four alternatives switched on ------------------------------------------------------------------------
def test_a_shipped_list_with_the_alternatives_runs_fused_and_unfused(lists):
    """Fused against op by op with the same draws.  GridSample makes a direct comparison of the two complete runs meaningless (a
    coordinate within rounding of a voxel face changes the set of rows, and with it NormalizeCoord's centroid), so the list is
    compared in two stretches that share their input: the head up to GridSample from the sample, the rest from the fused head's output."""
    from scenesplat_amd.pointcept_api import Compose
    cfg = H.with_alternatives(next(v for k, v in lists.items() if "lang-pretrain-scannet" in k))
    types = [e["type"] for e in cfg]
    cut = types.index("GridSample")
    n, seed = 5000, 25                                                   # this seed's draws: dropout, two rotations, both flips
    sample = A._fixture(n, 3)
    sample["segment"] = np.arange(n)                                     # a row id that travels through GridSample and Collect
    probe = Compose(cfg, seed=seed)
    params = [t.draw(probe.rng, {}) for t in probe.transforms]
    by = dict(zip(types, params))
    assert by["ChromaticJitter"]["fired"] and not by["RandomColorDrop"]["fired"] and \
        any(p.get("fired") for t, p in zip(types, params) if t == "RandomRotate"), "pick a seed whose draws exercise the list"
    # the whole list, twice: the same seed gives the same bits
    full = [Compose(cfg, seed=seed)(_cuda(sample)) for _ in range(2)]
    assert set(full[0]) == {"coord", "grid_coord", "segment", "lang_feat", "valid_feat_mask", "offset", "feat"}
    assert all(torch.equal(full[0][k], full[1][k]) for k in full[0])
    c = _np(full[0]["coord"]).astype(np.float64)
    assert abs(np.sqrt((c ** 2).sum(1).max()) - 1) <= 4 * EPS20 and np.abs(c.mean(0)).max() <= 4 * EPS20      # NormalizeCoord came last
    ids = _np(full[0]["segment"])
    assert len(np.unique(ids)) == len(ids) > 3000 and not np.array_equal(ids, np.sort(ids))                   # ShufflePoint
    # the head: seven coordinate passes op by op (CenterShift, up to three rotations, scale, flip, jitter) against one, then the
    # elastic pair on either; M <= 8 for this slab (|x| <= 4 about the centre, scaled by <= 1.1, + the distortion's 2)
    head = [Compose(cfg[:cut], fuse=f)(_cuda(sample), params=params[:cut]) for f in (True, False)]
    assert torch.equal(head[0]["segment"], head[1]["segment"])
    dc = np.abs(_np(head[0]["coord"]).astype(np.float64) - _np(head[1]["coord"])).max()
    assert dc <= (7 + 1 + 2 * 4) * EPS20 * 8.0, dc                       # the elastic pair moves a point by <= 4 x what its input differs by
    # colour: the trio is the same arithmetic fused or not, and HueSaturationTranslation truncates: whole steps, equal but for
    # rows where the two inputs straddle an integer (inputs within 5e-4 of each other: well under 1 % of the rows, one step)
    ca, cb = _np(head[0]["color"]), _np(head[1]["color"])
    assert np.array_equal(ca, np.floor(ca)) and np.abs(ca - cb).max() <= 1 and (ca != cb).any(1).mean() <= 0.01
    for k in ("quat", "scale", "normal"):                                # four passes of test_hip_augment's 2e-6 against one
        a, b = _np(head[0][k]).astype(np.float64), _np(head[1][k]).astype(np.float64)
        err = np.abs(a - b).max(1)
        if k == "quat":                                                  # the sign rule after a flip is a coin toss at its ties
            err = np.minimum(err, np.abs(a + b).max(1))
        assert err.max() <= 8e-6, k
    # the rest, from the same input: the same voxels, the same rows in the same shuffled order
    mid = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in head[0].items()}
    tail = [Compose(cfg[cut:], fuse=f)({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in mid.items()}, params=params[cut:])
            for f in (True, False)]
    assert set(tail[0]) == set(tail[1]) == set(full[0])
    for k in ("segment", "grid_coord", "lang_feat", "valid_feat_mask", "offset"):
        assert torch.equal(tail[0][k], tail[1][k]), k
    assert np.abs(_np(tail[0]["coord"]).astype(np.float64) - _np(tail[1]["coord"])).max() <= 2 * EPS20 * 2.0   # two passes, M <= 2
    assert np.abs(_np(tail[0]["feat"]).astype(np.float64) - _np(tail[1]["feat"])).max() <= 2 * EPS20 * 2.0
