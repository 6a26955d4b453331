"""CPU: the host layer of the transforms beyond the shipped lists (HueSaturationTranslation, RandomColorDrop, NormalizeCoord,
ShufflePoint -- the alternatives every shipped training list carries commented out -- and PositiveShift, PointClip, Add,
CropBoundary, ContrastiveViewsGenerator, InstanceParser): the registry, the shipped lists with the alternatives switched on, the
draws, the fold of NormalizeCoord / PositiveShift into a RigidState with host hooks, the refusal of CPU tensors -- and the fp64
numpy restatements the GPU tests of tests/test_hip_augment_rest.py measure against, checked here against the reference's recorded
outputs (tests/golden/augment_rest.npz, written by tests/golden/make_golden_augment_rest.py)."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW_OPS = {"HueSaturationTranslation": dict(hue_max=0.5, saturation_max=0.2), "RandomColorDrop": dict(p=0.2, color_augment=0.0),
           "NormalizeCoord": {}, "PositiveShift": {}, "PointClip": dict(point_cloud_range=(-80, -80, -3, 80, 80, 1)),
           "Add": dict(keys_dict={}), "ShufflePoint": {}, "CropBoundary": {},
           "ContrastiveViewsGenerator": dict(view_keys=("coord", "color", "normal", "origin_coord")),
           "InstanceParser": dict(segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)}
# the alternatives as the shipped configs spell them, and the entry each pair stands behind (commented out) in every list
ALTERNATIVES = {"ChromaticJitter": [dict(type="HueSaturationTranslation", hue_max=0.2, saturation_max=0.2),
                                    dict(type="RandomColorDrop", p=0.2, color_augment=0.0)],
                "NormalizeColor": [dict(type="NormalizeCoord"), dict(type="ShufflePoint")]}


# ---- fp64 numpy restatements (shared with the GPU tests) ------------------------------------------------------------------------
def np_mod1(a):
    """numpy's a % 1.0 spelled out: fmod, lifted by 1 when negative (may round to exactly 1.0)"""
    r = np.fmod(a, 1.0)
    return np.where(r < 0, r + 1.0, r)


def hsv64(color, hue_val, sat_ratio):
    """transform.py:1037-1100 in fp64 with ordered branches instead of np.select, truncation through uint8 included -> float32"""
    c = np.asarray(color, dtype=np.float64)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    m = maxc != minc
    d = np.where(m, maxc - minc, 1.0)
    s = np.where(m, (maxc - minc) / np.where(m, maxc, 1.0), 0.0)
    rc, gc, bc = (np.where(m, (maxc - x) / d, 0.0) for x in (r, g, b))
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, (2.0 + rc) - bc, (4.0 + gc) - rc))
    h = np_mod1(h / 6.0)
    h = np_mod1((hue_val + h) + 1.0)
    s = np.clip(sat_ratio * s, 0.0, 1.0)
    h6 = h * 6.0
    i = np.trunc(h6)
    f = h6 - i
    v = maxc
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i.astype(np.int64) % 6
    table = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v), 5: (v, p, q)}
    out = np.stack([v, v, v], 1)
    for k, cols in table.items():
        sel = (s != 0.0) & (i == k)
        for j in range(3):
            out[sel, j] = cols[j][sel]
    return np.trunc(np.clip(out, 0.0, 255.0)).astype(np.float32)


def normalize64(coord, scale):
    """NormalizeCoord (transform.py:423-434) in fp64 -> (coord, scale)"""
    c = np.asarray(coord, dtype=np.float64)
    c = c - c.mean(0)
    m = np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).max())
    return c / m, np.asarray(scale, dtype=np.float64) / m


def instance64(coord, segment, instance, segment_ignore_index, instance_ignore_index):
    """InstanceParser (transform.py:1626-1664): -> instance (n,) int64, centroid (n, 3) fp64 (an fp64 mean of the fp32 rows),
    bbox (K, 8) fp32 with the reference's fp32 arithmetic (min / max exact, (max + min) / 2, max - min)"""
    coord = np.asarray(coord, dtype=np.float32)
    segment, instance = np.asarray(segment).reshape(-1), np.asarray(instance, dtype=np.int64).copy()
    mask = ~np.isin(segment, segment_ignore_index)
    instance[~mask] = instance_ignore_index
    unique, inverse = np.unique(instance[mask], return_inverse=True)
    instance[mask] = inverse
    dense = np.full(len(coord), -1, dtype=np.int64)
    dense[mask] = inverse
    centroid = np.full((len(coord), 3), float(instance_ignore_index))
    bbox = np.zeros((len(unique), 8), dtype=np.float32)
    vacancy = np.array([v for v in segment_ignore_index if v >= 0], dtype=np.float32)
    for k in range(len(unique)):
        m = dense == k
        lo, hi = coord[m].min(0), coord[m].max(0)
        cls = np.float32(segment[m][0])
        bbox[k] = np.concatenate([(hi + lo) / np.float32(2), hi - lo, [0], [cls - np.float32((cls > vacancy).sum())]])
        centroid[m] = coord[m].astype(np.float64).mean(0)
    return instance, centroid, bbox


def with_alternatives(cfg):
    """a shipped list with the four commented alternatives put back where the configs carry them"""
    out = []
    for entry in cfg:
        out.append(entry)
        out.extend(ALTERNATIVES.get(entry["type"], []))
    return out


def fixture_rest(fx):
    """the sample the golden ran on: tests/golden/make_golden_augment.fixture(n, seed) + `instance`; HSV cases start from fx["hsv_in"]"""
    import test_hip_augment as A
    d = A._fixture(int(fx["n"]), int(fx["seed"]))
    d["instance"] = fx["instance"].copy()
    return d


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "augment_rest.npz")))


@pytest.fixture(scope="module")
def lists(golden_dir):
    with open(os.path.join(golden_dir, "augment_configs.txt")) as f:
        return ast.literal_eval(f.read())


# ---- registry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NEW_OPS))
def test_every_name_builds_with_the_reference_defaults(name):
    from scenesplat_amd import pointcept_api as api
    t = api.TRANSFORMS.build(dict(type=name))
    assert type(t) is getattr(api, name)
    for k, v in NEW_OPS[name].items():
        assert getattr(t, k) == v, (name, k)
    if name == "ContrastiveViewsGenerator":
        assert isinstance(t.view_trans, api.Compose) and t.view_trans.transforms == []
    if name == "RandomColorDrop":
        assert repr(t) == "RandomColorDrop(color_augment: 0.0, p: 0.2)"


def test_what_stays_unregistered():
    from scenesplat_amd.pointcept_api import TRANSFORMS
    with pytest.raises(KeyError):
        TRANSFORMS.build(dict(type="ClipGaussianJitter"))                # the reference's constructor cannot be called: nothing to match
    with pytest.raises(KeyError):
        TRANSFORMS.build(dict(type="GSGaussianBlurVoxelGPU"))
    with pytest.raises(NotImplementedError):
        TRANSFORMS.build(dict(type="GridSample", mode="test"))


def test_every_shipped_list_builds_with_its_alternatives_enabled(lists):
    from scenesplat_amd.pointcept_api import TRANSFORMS, Compose
    assert len(lists) >= 8
    for name, cfg in lists.items():
        full = with_alternatives(cfg)
        assert len(full) == len(cfg) + 4, name                           # every list carries all four
        comp = Compose(full)
        for entry, t in zip(full, comp.transforms):
            assert type(t) is TRANSFORMS.get(entry["type"]), (name, entry["type"])
            for k, v in entry.items():
                if k not in ("type", "offset_keys_dict") and k in vars(t):
                    assert getattr(t, k) == v, (name, entry["type"], k)
        types = [e["type"] for e in full]
        assert types.index("HueSaturationTranslation") == types.index("ChromaticJitter") + 1
        assert types[types.index("NormalizeColor") + 1:types.index("NormalizeColor") + 3] == ["NormalizeCoord", "ShufflePoint"]


# ---- draws ----------------------------------------------------------------------------------------------------------------------
def test_draws_are_deterministic_per_seed_and_stay_in_range():
    from scenesplat_amd.pointcept_api import TRANSFORMS
    ops = [TRANSFORMS.build(dict(type="HueSaturationTranslation", hue_max=0.2, saturation_max=0.3)),
           TRANSFORMS.build(dict(type="RandomColorDrop", p=0.5)), TRANSFORMS.build(dict(type="ShufflePoint")),
           TRANSFORMS.build(dict(type="NormalizeCoord")), TRANSFORMS.build(dict(type="InstanceParser"))]

    def run(seed):
        rng = np.random.default_rng(seed)
        return [[op.draw(rng, {}) for op in ops] for _ in range(50)]
    a, b, c = run(7), run(7), run(8)
    assert a == b and a != c
    hue = np.array([r[0]["hue_val"] for r in a])
    sat = np.array([r[0]["sat_ratio"] for r in a])
    assert (np.abs(hue) <= 0.2).all() and hue.min() < -0.1 and hue.max() > 0.1
    assert (np.abs(sat - 1) <= 0.3).all() and sat.min() < 0.85 and sat.max() > 1.15
    fired = [r[1]["fired"] for r in a]
    assert 10 < sum(fired) < 40 and all(isinstance(f, bool) for f in fired)
    assert len({r[2]["seed"] for r in a}) == 50 and a[0][3] == {} and a[0][4] == {}
    # HueSaturationTranslation takes exactly two uniform draws, RandomColorDrop one
    rng, ref = np.random.default_rng(3), np.random.default_rng(3)
    p = ops[0].draw(rng, {})
    assert p == dict(hue_val=(ref.random() - 0.5) * 2 * 0.2, sat_ratio=1 + (ref.random() - 0.5) * 2 * 0.3)
    assert ops[1].draw(rng, {})["fired"] == bool(ref.random() < 0.5)
    assert rng.random() == ref.random()


def test_contrastive_views_run_both_views_on_the_callers_generator():
    from scenesplat_amd.pointcept_api import Compose, TRANSFORMS
    cfg = [dict(type="RandomColorDrop", p=0.5), dict(type="HueSaturationTranslation")]
    gen = TRANSFORMS.build(dict(type="ContrastiveViewsGenerator", view_keys=("tag",), view_trans_cfg=cfg))
    seen = []
    for t in gen.view_trans.transforms:
        t.apply = lambda d, p, seen=seen: (seen.append(p), d)[1]         # record what each view drew; no device work
    comp = Compose([gen, dict(type="RandomColorDrop", p=0.5)], seed=11)
    comp.transforms[1].apply = lambda d, p: (seen.append(p), d)[1]
    out = comp(dict(tag="x", other=1))
    assert out["view1_tag"] == out["view2_tag"] == "x" and out["other"] == 1 and set(out) == {"tag", "other", "view1_tag", "view2_tag"}
    ref = np.random.default_rng(11)
    hs = TRANSFORMS.build(cfg[1])
    want = []
    for _ in range(2):                                                   # view 1, then view 2, then the parent list goes on
        want += [dict(fired=bool(ref.random() < 0.5)), hs.draw(ref, {})]
    want.append(dict(fired=bool(ref.random() < 0.5)))
    assert seen == want
    # a recorded call replays without a generator
    seen.clear()
    gen.apply(dict(tag="y"), dict(views=[want[0:2], want[2:4]]))
    assert seen == want[:4]
    with pytest.raises(ValueError, match="2 params lists"):
        gen.apply(dict(tag="y"), dict(views=[want[0:2]]))
    # set_fuse reaches the nested list
    assert gen.view_trans.fuse is True
    comp.set_fuse(False)
    assert gen.view_trans.fuse is False


def test_add_is_host_only():
    from scenesplat_amd.pointcept_api import TRANSFORMS
    out = TRANSFORMS.build(dict(type="Add", keys_dict=dict(condition="ScanNet", split=3)))(dict(coord="untouched"))
    assert out == dict(coord="untouched", condition="ScanNet", split=3)


# ---- the fold of NormalizeCoord / PositiveShift -----------------------------------------------------------------------------------
def _hooks(pts):
    def bbox(A, b):
        p = pts @ A.T + b
        return np.concatenate([p.min(0), p.max(0)])

    def moments(A, b):
        p = pts @ A.T + b
        return np.concatenate([p.mean(0), [(p * p).sum(1).max()]])
    return dict(bbox_fn=bbox, moments_fn=moments)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_normalize_coord_and_positive_shift_fold_into_the_pending_affine(seed):
    from scenesplat_amd.pointcept_api import transform as tf
    g = np.random.default_rng(seed)
    pts = g.random((200, 3)) * [4.0, 3.0, 1.5] + [7.0, -2.0, 0.5]
    ops = [tf.CenterShift(apply_z=True), tf.RandomRotate(angle=[-1, 1], axis="z", always_apply=True), tf.RandomScale(scale=[0.9, 1.1]),
           tf.NormalizeCoord(), tf.RandomShift(), tf.PositiveShift()]
    rng = np.random.default_rng(50 + seed)
    params = [op.draw(rng, {}) for op in ops]
    st = tf.RigidState(**_hooks(pts))
    data = dict(coord=None, pc_coord=None)
    x = pts - [(pts[:, 0].min() + pts[:, 0].max()) / 2, (pts[:, 1].min() + pts[:, 1].max()) / 2, pts[:, 2].min()]
    c = (x.min(0) + x.max(0)) / 2
    x = (x - c) @ tf.axis_rotation("z", params[1]["angle"]).T + c
    x = x * params[2]["scale"]
    for op, p in zip(ops[:3], params[:3]):
        op.fold(st, data, p)
    a_pc, b_pc = st.A_pc.copy(), st.b_pc.copy()                          # the cloud followed the first three ...
    assert st.pc_pending()
    ops[3].fold(st, data, params[3])
    m = np.sqrt((((x - x.mean(0)) ** 2).sum(1)).max())
    x, _ = normalize64(x, 0.0)
    assert np.abs(pts @ st.A.T + st.b - x).max() <= 1e-12
    assert abs(np.linalg.norm(pts @ st.A.T + st.b, axis=1).max() - 1) <= 1e-12 and np.abs((pts @ st.A.T + st.b).mean(0)).max() <= 1e-12
    assert st.scaled and np.allclose(st.smul, params[2]["scale"][0] / m, rtol=1e-12, atol=0)        # scale <- scale / m rides the same pass
    for op, p in zip(ops[4:], params[4:]):
        op.fold(st, data, p)
    x = x + params[4]["shift"]
    x = x - x.min(0)
    assert np.abs(pts @ st.A.T + st.b - x).max() <= 1e-12 and np.abs((pts @ st.A.T + st.b).min(0)).max() <= 1e-12
    assert np.array_equal(st.A_pc, a_pc) and np.array_equal(st.b_pc, b_pc)                              # ... and is left alone by these
    assert tf.NormalizeCoord.family == tf.PositiveShift.family == "rigid" and tf.HueSaturationTranslation.family is None


def test_normalize_coord_refuses_coincident_points():
    from scenesplat_amd.pointcept_api import transform as tf
    st = tf.RigidState(**_hooks(np.ones((5, 3))))
    with pytest.raises(ValueError, match="centroid"):
        tf.NormalizeCoord().fold(st, dict(coord=None), {})


def test_a_pending_jitter_is_flushed_before_the_moments():
    from scenesplat_amd.pointcept_api import transform as tf
    calls = []
    st = tf.RigidState(**_hooks(np.random.default_rng(0).random((10, 3))))
    st.flush = lambda data: (calls.append("flush"), tf.RigidState.reset(st))[0]
    st.add_jitter({}, 0.01, 0.05, seed=1)
    st.moments({})
    assert calls == ["flush"] and st.jitter is None


# ---- CPU tensors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["HueSaturationTranslation", "RandomColorDrop", "NormalizeCoord", "PositiveShift", "PointClip",
                                  "ShufflePoint", "CropBoundary", "InstanceParser"])
def test_cpu_tensors_are_refused(name):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    t = TRANSFORMS.build(dict(type=name))
    d = dict(coord=torch.zeros(4, 3), color=torch.zeros(4, 3), segment=torch.full((4,), 5), instance=torch.arange(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.apply(d, dict(fired=True, hue_val=0.1, sat_ratio=1.0, seed=1))


# ---- the restatements against the reference's recorded outputs --------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["hsa", "hsb"])
def test_hsv_restatement_reproduces_the_reference(fx, tag):
    got = hsv64(fx["hsv_in"], float(fx[tag + "_hue_val"]), float(fx[tag + "_sat_ratio"]))
    assert np.array_equal(got, fx[tag + "_color"].astype(np.float32))
    planted = fx["hsv_in"][:20]
    assert (planted[0] == 0).all() and (planted[1] == 255).all() and (planted[5][0] == planted[5]).all()      # black, white, a grey row
    assert np.array_equal(got[0], [0, 0, 0]) and np.array_equal(got[1], [255, 255, 255]) and (got[5] == 128).all()
    assert (fx["hsv_in"][20:] != np.floor(fx["hsv_in"][20:])).any()                                             # non-integer colours


def test_hsv_restatement_edges():
    c = np.array([[10.0, 200.0, 30.0]], dtype=np.float32)
    assert np.array_equal(hsv64(c, 0.0, 1.0), np.trunc(hsv64(c, 0.0, 1.0)))
    assert np.array_equal(np_mod1(np.array([-1e-17, -0.25, 1.5, 2.0])), [1.0, 0.75, 0.5, 0.0])   # a tiny negative rounds to exactly 1.0
    assert np.array_equal(np_mod1(np.array([-0.25])), np.array([-0.25]) % 1.0)
    assert np.array_equal(hsv64(np.array([[300.0, 0.0, 0.0]]), 0.0, 1.0)[0], [255.0, 0.0, 0.0])  # outside 0..255: saturates


def test_normalize_and_instance_restatements_sit_where_the_golden_says(fx):
    base = fixture_rest(fx)
    c, s = normalize64(base["coord"], base["scale"])
    assert np.abs(fx["nc_coord"].astype(np.float64) - c).max() == float(fx["nc_ref_err"]) < 1e-5
    inst, cen, box = instance64(base["coord"], base["segment"], base["instance"], (-1, 0, 1), -1)
    assert np.array_equal(inst, fx["ip_instance"]) and np.array_equal(box, fx["ip_bbox"])
    assert np.abs(fx["ip_centroid"].astype(np.float64) - cen).max() == float(fx["ip_ref_err"]) < 1e-5
    valid = ~np.isin(base["segment"], (-1, 0, 1))
    assert (base["instance"][valid] == -1).any() and (inst[valid] == 0).any()             # the id -1 on valid rows is instance 0
    assert len(box) == 9 and set(np.unique(base["instance"])) == {-1, 0, 3, 4, 9, 17, 40, 41, 1000}
