"""GPU: the augmentation kernels (csrc/augment.hip) and the transforms over them (pointcept_api/transform.py) against OUTPUTS OF
THE REFERENCE'S OWN transforms (tests/golden/augment.npz + augment_b.npz, written by tests/golden/make_golden_augment.py: draws recorded, replayed
here through apply()), and against an fp64 numpy restatement at the sizes without a golden: n = 1, 63, 64, 65 (around one wave),
70,001 (the multi-block reduction) and 300,001 (more rows than the 1,024 x 256 threads of a full grid: the grid-stride loop).

Bounds (M = max over points and axes of sum_j |A_ij| |x_j| + |b_i| for the affine the pass applies to its input x):
  coord / normal   2^-20 M: at most 7 roundings of 2^-24 relative to partial sums bounded by M, doubled
  quat             2e-6 absolute WITH sign (about 16 roundings on unit-scale values, doubled); rows whose two largest branch values
                   [M00, M11, M22, trace] lie within 1e-5 of each other -- the sign rule is a coin toss there -- up to sign, at most 0.5 %
  scale            1 ulp
  elastic          4 x the error of an fp32 numpy restatement against the reference's fp64 result (stored with the golden, <= 1e-5)
  colour           5e-4 on the 0..255 scale (8 roundings of 2^-24 on values <= 510, doubled), / 127.5 after NormalizeColor
"""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 70001, 300001]
EPS20 = 2.0 ** -20


def _fixture(n, seed):
    """make_golden_augment.fixture(n, seed): the sample of make_golden_transforms.py + unit normals, colours on 0..255"""
    g = np.random.RandomState(seed)
    coord = (g.rand(n, 3) * np.array([4.0, 3.0, 1.5])).astype(np.float32)
    d = dict(coord=coord, color=(g.rand(n, 3) * 2 - 1).astype(np.float32), opacity=g.rand(n, 1).astype(np.float32),
             quat=g.randn(n, 4).astype(np.float32), scale=g.rand(n, 3).astype(np.float32),
             segment=g.randint(-1, 20, n).astype(np.int64), lang_feat=g.randn(n, 16).astype(np.float32),
             valid_feat_mask=(g.rand(n) < 0.9).astype(np.int64), name="scene%d" % seed)
    g = np.random.RandomState(seed + 1000)
    d["color"] = (g.rand(n, 3) * 255).astype(np.float32)
    nrm = g.randn(n, 3)
    d["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return d


def _cuda(d):
    return {k: (torch.from_numpy(v.copy()).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return {**np.load(os.path.join(golden_dir, "augment.npz")), **np.load(os.path.join(golden_dir, "augment_b.npz"))}


@pytest.fixture(scope="module")
def base(fx):
    return _fixture(int(fx["n"]), int(fx["seed"]))


@pytest.fixture(scope="module")
def lists(golden_dir):
    with open(os.path.join(golden_dir, "augment_configs.txt")) as f:
        return ast.literal_eval(f.read())


# ---- fp64 restatements ----------------------------------------------------------------------------------------------------------
def _affine_bound(A, b, x):
    return EPS20 * float((np.abs(x).astype(np.float64) @ np.abs(A).T + np.abs(b)).max())


def _quat_mul(p, q):
    pw, px, py, pz = p
    qw, qx, qy, qz = q.T
    return np.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], 1)


def _branch_gap(q):
    q = np.asarray(q, dtype=np.float64)
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    q = q / np.where(norm > 0, norm, 1.0)
    w, x, y, z = q.T
    dec = np.stack([1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y), 3 - 4 * (x * x + y * y + z * z)], 1)
    s = np.sort(dec, axis=1)
    return s[:, 3] - s[:, 2]


def _quat64(quat, r, flip):
    """normalise, r (x) q, flip conjugation, scipy's from_matrix sign -- in fp64"""
    q = quat.astype(np.float64)
    nz = np.linalg.norm(q, axis=1) > 0
    q[nz] /= np.linalg.norm(q[nz], axis=1, keepdims=True)
    if r is not None:
        q[nz] = _quat_mul(np.asarray(r, dtype=np.float64), q[nz])
    if flip:
        s = np.array([1.0, -1.0 if flip & 2 else 1.0, -1.0 if flip & 1 else 1.0, -1.0 if flip in (1, 2) else 1.0])
        q[nz] *= s
        c = q[:, [1, 2, 3, 0]]
        lead = c[np.arange(len(q)), np.argmax(c * c, axis=1)]
        q[nz & (lead < 0)] *= -1
    return q


def _assert_quat(got, want, flipped=True, tol=2e-6):
    """with sign; after a flip, near ties of the sign rule (at most 0.5 % of the rows) up to sign"""
    tie = (_branch_gap(want) < 1e-5) & flipped
    assert tie.mean() <= 0.005 or len(want) < 200
    err = np.abs(got.astype(np.float64) - want).max(1)
    err_flip = np.abs(got.astype(np.float64) + want).max(1)
    err = np.where(tie, np.minimum(err, err_flip), err)
    assert err.max() <= tol, ("quat", float(err.max()), int(np.argmax(err)))


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def _rand_rigid(g):
    """a random rotation (quaternion + matrix), flip bits, per-axis scale, shift: what a fused run hands the kernel"""
    r = g.standard_normal(4)
    r /= np.linalg.norm(r)
    w, x, y, z = r
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    smul = g.uniform(0.9, 1.1, 3)
    return r, rot, smul, g.uniform(-2, 2, 3)


# ---- ss_aug_bbox ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [2000])
def test_bbox_is_exact_and_deterministic(n):
    from scenesplat_amd import native as nv
    g = np.random.default_rng(n)
    x = (g.standard_normal((n, 3)) * [4.0, 3.0, 1.5] + [1.0, -2.0, 0.5]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    got = _np(nv.aug_bbox(xd))
    assert np.array_equal(got, np.concatenate([x.min(0), x.max(0)]))             # min / max of the fp32 input: exact
    r, rot, smul, shift = _rand_rigid(g)
    A, b = smul[:, None] * rot, shift
    aff = list(A.reshape(-1)) + list(b)
    one, two = _np(nv.aug_bbox(xd, aff)), _np(nv.aug_bbox(xd, aff))
    assert np.array_equal(one, two)                                              # no float atomics: the same bits on every run
    y = x.astype(np.float64) @ A.T + b
    assert np.abs(one - np.concatenate([y.min(0), y.max(0)])).max() <= _affine_bound(A, b, x)
    assert np.array_equal(_np(xd), x)                                            # read only
    # the box of a pending affine IS the box of the flushed coordinates (both kernels evaluate one formula)
    nv.aug_gaussians_(coord=xd, affine=aff)
    assert np.array_equal(_np(nv.aug_bbox(xd)), one)


# ---- ss_aug_gaussians against the fp64 restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_gaussians_fused_pass_matches_fp64(n, flip):
    from scenesplat_amd import native as nv
    g = np.random.default_rng(1000 * flip + n)
    d = _fixture(n, 40 + flip)
    if n > 1:
        d["quat"][n // 2] = 0                                                   # a zero-norm row: left unchanged, no NaN
    r, rot, smul, shift = _rand_rigid(g)
    f = np.array([-1.0 if flip & 1 else 1.0, -1.0 if flip & 2 else 1.0, 1.0])
    L = f[:, None] * rot
    A, b = f[:, None] * (smul[:, None] * rot), f * smul * shift
    noise = g.standard_normal((n, 3)).astype(np.float32)
    sigma, clip = 0.005, 0.01
    want = dict(coord=d["coord"].astype(np.float64) @ A.T + b + np.clip(sigma * noise.astype(np.float64), -clip, clip),
                quat=_quat64(d["quat"], r, flip), scale=d["scale"].astype(np.float64) * smul,
                normal=d["normal"].astype(np.float64) @ L.T)
    keys = ("coord", "quat", "scale", "normal")
    for absent in (None,) + (keys if flip == 3 else ()):                       # every optional array absent, one at a time
        t = {k: torch.from_numpy(d[k].copy()).cuda() for k in keys if k != absent}
        nv.aug_gaussians_(coord=t.get("coord"), quat=t.get("quat"), scale=t.get("scale"), normal=t.get("normal"),
                          affine=list(A.reshape(-1)) + list(b), rquat=list(r), flip=flip, scale_mul=list(smul),
                          lin=list(L.reshape(-1)), jitter=(sigma, clip),
                          noise=torch.from_numpy(noise).cuda() if "coord" in t else None)
        got = {k: _np(v) for k, v in t.items()}
        assert all(np.isfinite(v).all() for v in got.values())
        if "coord" in got:
            assert np.abs(got["coord"] - want["coord"]).max() <= _affine_bound(A, b, d["coord"])
        if "normal" in got:
            assert np.abs(got["normal"] - want["normal"]).max() <= _affine_bound(L, np.zeros(3), d["normal"])
        if "scale" in got:
            assert _ulps(got["scale"], want["scale"].astype(np.float32)) <= 1
        if "quat" in got:
            _assert_quat(got["quat"], want["quat"], flipped=bool(flip))
            if n > 1:
                assert np.array_equal(got["quat"][n // 2], np.zeros(4, np.float32))


def test_gaussians_parts_that_are_off_leave_memory_untouched():
    from scenesplat_amd import native as nv
    d = _fixture(300, 9)
    t = _cuda({k: d[k] for k in ("coord", "quat", "scale", "normal")})
    nv.aug_gaussians_(coord=t["coord"], quat=t["quat"], scale=None, normal=None, affine=None, rquat=None, flip=0)
    assert all(np.array_equal(_np(t[k]), d[k]) for k in t)                       # no affine / jitter / rotation / flip: nothing written
    nv.aug_gaussians_(quat=t["quat"], flip=1)
    q = _np(t["quat"])
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 2e-6 and np.array_equal(_np(t["coord"]), d["coord"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.aug_gaussians_(coord=torch.zeros(4, 3), affine=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    from scenesplat_amd._lib import NativeError
    with pytest.raises(NativeError):
        nv.aug_gaussians_(coord=t["coord"], jitter=(0.01, 0.0))                  # clip must be positive


# ---- the ops against the reference's recorded outputs ---------------------------------------------------------------------------
def _host_affine(op, params, coord):
    """(A, b, L) the op folds for this input: the fp64 host composition with a numpy bounding box"""
    from scenesplat_amd.pointcept_api import transform as tf
    x = coord.astype(np.float64)
    st = tf.RigidState(bbox_fn=lambda A, b: np.concatenate([(x @ A.T + b).min(0), (x @ A.T + b).max(0)]))
    op.fold(st, dict(coord=None), params)
    return st.A, st.b, st.L


RIGID_CASES = {
    "cs_z": (dict(type="CenterShift", apply_z=True), lambda fx: {}),
    "cs_xy": (dict(type="CenterShift", apply_z=False), lambda fx: {}),
    "rz": (dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5), lambda fx: dict(fired=True, angle=float(fx["rz_angle"]))),
    "rx": (dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=0.5), lambda fx: dict(fired=True, angle=float(fx["rx_angle"]))),
    "ry": (dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=0.5), lambda fx: dict(fired=True, angle=float(fx["ry_angle"]))),
    "rt": (dict(type="RandomRotateTargetAngle", angle=(1 / 2, 1, 3 / 2), center=[0, 0, 0], axis="z", p=0.75),
           lambda fx: dict(fired=True, angle=float(fx["rt_angle"]))),
    "sca": (dict(type="RandomScale", scale=[0.9, 1.1], anisotropic=True), lambda fx: dict(scale=fx["sca_draw"].tolist())),
    "sh": (dict(type="RandomShift", shift=((-0.2, 0.2), (-0.2, 0.2), (-0.1, 0.1))), lambda fx: dict(shift=fx["sh_draw"].tolist())),
    "fx": (dict(type="RandomFlip", p=0.5), lambda fx: dict(flip_x=True, flip_y=False)),
    "fy": (dict(type="RandomFlip", p=0.5), lambda fx: dict(flip_x=False, flip_y=True)),
    "fxy": (dict(type="RandomFlip", p=0.5), lambda fx: dict(flip_x=True, flip_y=True)),
    "jit": (dict(type="RandomJitter", sigma=0.005, clip=0.01), lambda fx: dict(noise=fx["jit_noise"])),
}


@pytest.mark.parametrize("tag", list(RIGID_CASES))
def test_each_rigid_op_matches_the_reference(fx, base, tag):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    cfg, mk = RIGID_CASES[tag]
    op, params = TRANSFORMS.build(cfg), mk(fx)
    A, b, L = _host_affine(op, params, base["coord"])
    data = _cuda(base)
    out = op.apply(data, params)
    assert out is data
    touched = set()
    for key, bound in (("coord", _affine_bound(A, b, base["coord"])), ("normal", _affine_bound(L, np.zeros(3), base["normal"]))):
        if tag + "_" + key in fx:
            touched.add(key)
            assert np.abs(_np(out[key]).astype(np.float64) - fx[tag + "_" + key]).max() <= bound, (tag, key)
    if tag + "_quat" in fx:
        touched.add("quat")
        _assert_quat(_np(out["quat"]), fx[tag + "_quat"].astype(np.float64), flipped=tag.startswith("f"))
    if tag + "_scale" in fx:
        touched.add("scale")
        assert _ulps(_np(out["scale"]), fx[tag + "_scale"]) <= 1
    # what the reference leaves alone stays bit for bit (a flip of one axis stores its quaternions only; its coord / normal mirror)
    for key in ("coord", "quat", "scale", "normal", "color", "opacity"):
        if key in touched:
            continue
        want = base[key]
        if tag in ("fx", "fy") and key in ("coord", "normal"):
            want = want * np.array([-1 if tag == "fx" else 1, -1 if tag == "fy" else 1, 1], dtype=np.float32)
        assert np.array_equal(_np(out[key]), want), (tag, key)


def _seq(fx, lists=None):
    """the recorded head-of-list run: (config list, one params dict per op, the n = 1000 sample)"""
    cfg = [dict(type="CenterShift", apply_z=True), dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=1.0),
           dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
           dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", always_apply=True),
           dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", always_apply=True),
           dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5), dict(type="RandomJitter", sigma=0.005, clip=0.01),
           dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]), dict(type="ChromaticAutoContrast", p=1.0), dict(type="ChromaticTranslation", p=1.0, ratio=0.05),
           dict(type="ChromaticJitter", p=1.0, std=0.05)]
    a = fx["seq_angles"]
    params = [{}, dict(fired=True, idx=fx["seq_idx"]), dict(fired=True, angle=float(a[0])), dict(fired=True, angle=float(a[1])),
              dict(fired=True, angle=float(a[2])), dict(scale=fx["seq_scale"].tolist()),
              dict(flip_x=bool(fx["seq_flips"][0]), flip_y=bool(fx["seq_flips"][1])), dict(noise=fx["seq_noise"]),
              dict(fired=True, noise=[fx["seq_el_raw0"], fx["seq_el_raw1"]]), dict(fired=True, blend=float(fx["seq_blend"])), dict(fired=True, tr=fx["seq_tr"].tolist()),
              dict(fired=True, noise=fx["seq_cnoise"])]
    return cfg, params, _fixture(int(fx["seq_n"]), int(fx["seq_seed"]))


@pytest.mark.parametrize("fuse", [True, False])
def test_head_of_the_shipped_list_matches_the_reference(fx, fuse):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import Compose, transform as tf
    cfg, params, sample = _seq(fx)
    comp = Compose(cfg, fuse=fuse)
    calls = []
    orig = nv.aug_gaussians_
    nv.aug_gaussians_ = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        mid = Compose(cfg[:8], fuse=fuse)(_cuda(sample), params=params[:8])        # the checkpoint after RandomJitter
        del calls[:]
        out = comp(_cuda(sample), params=params)
    finally:
        nv.aug_gaussians_ = orig
    # CenterShift | dropout | three rotations + scale + flip + jitter | elastic: two rigid passes fused, seven op by op
    assert len(calls) == (2 if fuse else 7)
    # the bound of the composed affine on the run's input
    x = sample["coord"].astype(np.float64)
    st = tf.RigidState(bbox_fn=lambda A, b: np.concatenate([(x @ A.T + b).min(0), (x @ A.T + b).max(0)]))
    for op, p in zip(comp.transforms[:8], params[:8]):
        if op.family == "rigid" and "noise" not in p:
            op.fold(st, dict(coord=None), p)
    assert st.flip == 3 and st.q is not None
    idx = fx["seq_idx"]
    rigid = _affine_bound(st.A, st.b, sample["coord"])
    assert np.abs(_np(mid["coord"]) - fx["seq_coord"]).max() <= rigid
    # ElasticDistortion inside the run: its input is what the rigid pass left (within `rigid` of the reference's), its grids are the
    # recorded ones (apply() refuses them unless the box of the fp32 coordinates asks for the same shapes).  An input error e comes
    # out of a pair as at most (1 + 2 lip) e, lip = magnitude / granularity * sum over the axes of the largest step between neighbouring
    # nodes of the smoothed grid (the trilinear field's Lipschitz constant in the max norm; twice, because the grid's origin is the box
    # minimum of the same coordinates and is off by up to e as well); on top of that the pairs' own fp32 error,
    # 4 x what the fp32 numpy restatement of both pairs shows against the reference (stored, <= 1e-5).
    gain = 1.0
    for raw, (gran, mag) in zip((fx["seq_el_raw0"], fx["seq_el_raw1"]), comp.transforms[8].distortion_params):
        sm = tf.box_blur3(torch.from_numpy(raw)).numpy().astype(np.float64)
        gain *= 1 + 2 * mag / gran * sum(np.abs(np.diff(sm, axis=a)).max() for a in range(3))
    assert float(fx["seq_el_f32_err"]) <= 1e-5
    err = np.abs(_np(out["coord"]) - fx["seq_el_coord"]).max()
    assert 1e-3 < np.abs(fx["seq_el_coord"] - fx["seq_coord"]).max() and err <= gain * rigid + 4 * float(fx["seq_el_f32_err"]), (err, gain, rigid)
    assert np.abs(_np(out["normal"]) - fx["seq_normal"]).max() <= _affine_bound(st.L, np.zeros(3), sample["normal"])
    _assert_quat(_np(out["quat"]), fx["seq_quat"])
    assert _ulps(_np(out["scale"]), fx["seq_scale_out"]) <= 1
    assert np.abs(_np(out["color"]) - fx["seq_color"]).max() <= 5e-4
    for k in ("segment", "lang_feat", "opacity", "valid_feat_mask"):
        assert np.array_equal(_np(out[k]), sample[k][idx]), k


# ---- jitter with the kernel's own draws -------------------------------------------------------------------------------------------
def test_jitter_draws_are_seeded_clipped_and_normal():
    from scenesplat_amd.pointcept_api import TRANSFORMS
    n, sigma = 70001, 0.01
    op = TRANSFORMS.build(dict(type="RandomJitter", sigma=sigma, clip=100 * sigma))

    def run(seed, op=op):
        return _np(op.apply(dict(coord=torch.zeros(n, 3, device="cuda")), dict(seed=seed))["coord"]).astype(np.float64)
    a, b, c = run(123456789012345), run(123456789012345), run(123456789012346)
    assert np.array_equal(a, b) and (a != c).mean() > 0.99
    assert abs(a.mean()) <= 5 * sigma / np.sqrt(3 * n)
    assert abs(a.var() / sigma ** 2 - 1) <= 0.05
    assert abs(np.corrcoef(a[:, 0], a[:, 1])[0, 1]) <= 5 / np.sqrt(n) and abs(np.corrcoef(a[:-1, 2], a[1:, 2])[0, 1]) <= 5 / np.sqrt(n)
    tight = TRANSFORMS.build(dict(type="RandomJitter", sigma=0.005, clip=0.01))       # the shipped pair: clips at 2 sigma
    t = run(7, tight)
    assert np.abs(t).max() == np.float32(0.01) and (np.abs(t) == np.float32(0.01)).mean() > 0.03


# ---- ss_aug_elastic ---------------------------------------------------------------------------------------------------------------
def _elastic64(coord, noise, origin, gran, mag):
    """coord + trilinear(noise, coord) * mag in fp64; node i at origin + i * gran, 0 outside (transform.py:1156-1168)"""
    c = coord.astype(np.float64)
    d = np.array(noise.shape[:3])
    t = (c - np.asarray(origin, dtype=np.float64)) / gran
    inside = np.all((t >= 0) & (t <= d - 1), axis=1)
    i0 = np.clip(np.floor(t).astype(int), 0, d - 2)
    f = t - i0
    acc = np.zeros((len(c), 3))
    for k in range(8):
        o = np.array([k >> 2, (k >> 1) & 1, k & 1])
        j = i0 + o
        acc += np.prod(np.where(o, f, 1 - f), axis=1)[:, None] * noise[j[:, 0], j[:, 1], j[:, 2]].astype(np.float64)
    return np.where(inside[:, None], c + acc * mag, c)


@pytest.mark.parametrize("k", [0, 1])
def test_elastic_pass_matches_the_reference(fx, base, k):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    gran, mag = [[0.2, 0.4], [0.8, 1.6]][k]
    stored = float(fx["el%d_f32_err" % k])
    assert stored <= 1e-5, "ill-conditioned elastic fixture"
    cin = base["coord"] if k == 0 else fx["el0_out"].astype(np.float32)
    op = TRANSFORMS.build(dict(type="ElasticDistortion", distortion_params=[[gran, mag]]))
    out = op.apply(dict(coord=torch.from_numpy(cin.copy()).cuda()), dict(fired=True, noise=[fx["el%d_raw" % k]]))
    err = np.abs(_np(out["coord"]).astype(np.float64) - fx["el%d_out" % k]).max()
    assert err <= 4 * stored, (err, stored)
    with pytest.raises(ValueError, match="does not fit"):
        op.apply(dict(coord=torch.from_numpy(cin.copy()).cuda()), dict(fired=True, noise=[fx["el%d_raw" % k][1:]]))


def test_elastic_two_passes_equal_one_after_the_other_and_own_grids_are_seeded(fx, base):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    both = TRANSFORMS.build(dict(type="ElasticDistortion"))
    assert both.distortion_params == [[0.2, 0.4], [0.8, 1.6]]
    grids = [fx["el0_raw"], fx["el1_raw"]]
    a = _np(both.apply(dict(coord=torch.from_numpy(base["coord"].copy()).cuda()), dict(fired=True, noise=grids))["coord"])
    d = dict(coord=torch.from_numpy(base["coord"].copy()).cuda())
    for p, gr in zip(both.distortion_params, grids):
        d = TRANSFORMS.build(dict(type="ElasticDistortion", distortion_params=[p])).apply(d, dict(fired=True, noise=[gr]))
    assert np.array_equal(a, _np(d["coord"]))
    own = [_np(both.apply(dict(coord=torch.from_numpy(base["coord"].copy()).cuda()), dict(fired=True, seed=s))["coord"]) for s in (5, 5, 6)]
    assert np.array_equal(own[0], own[1]) and not np.array_equal(own[0], own[2])
    assert 1e-3 < np.abs(own[0] - base["coord"]).max() < 1.6
    off = both.apply(dict(coord=torch.from_numpy(base["coord"].copy()).cuda()), dict(fired=False, seed=5))
    assert np.array_equal(_np(off["coord"]), base["coord"])


def test_elastic_edges_one_point_corner_and_outside():
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import TRANSFORMS, transform as tf
    g = np.random.default_rng(3)
    # n = 1: the reference's grid is 3 x 3 x 3 around the point, which sits on the middle node
    p = np.array([[1.25, -0.5, 2.0]], dtype=np.float32)
    raw = g.standard_normal((3, 3, 3, 3)).astype(np.float32)
    op = TRANSFORMS.build(dict(type="ElasticDistortion", distortion_params=[[0.25, 0.5]]))
    got = _np(op.apply(dict(coord=torch.from_numpy(p.copy()).cuda()), dict(fired=True, noise=[raw]))["coord"])
    sm = tf.box_blur3(torch.from_numpy(raw)).numpy()
    want = _elastic64(p, sm, p[0] - 0.25, 0.25, 0.5)
    assert np.array_equal(want, p + sm[1, 1, 1].astype(np.float64) * 0.5)
    tol = EPS20 * (np.abs(p).max() + 0.5 * np.abs(sm).max())       # exact weights: 8 fma roundings on |noise|, one on the sum, doubled
    assert np.abs(got - want).max() <= tol
    # five points through the op: point 0 is the maximum corner of the extent (coordinates on a 1/16 lattice: t is exact)
    pts = np.array([[2.0, 1.5, 1.0], [0.0, 0.0, 0.0], [0.5, 1.5, 0.25], [2.0, 0.0, 0.5], [1.0625, 0.8125, 1.0]], dtype=np.float32)
    dim, origin = tf.ElasticDistortion.grid_geometry(np.concatenate([pts.min(0), pts.max(0)]), 0.25)
    assert tuple(dim) == (11, 9, 7)
    raw = g.standard_normal((11, 9, 7, 3)).astype(np.float32)
    got = _np(op.apply(dict(coord=torch.from_numpy(pts.copy()).cuda()), dict(fired=True, noise=[raw]))["coord"])
    sm = tf.box_blur3(torch.from_numpy(raw)).numpy()
    want = _elastic64(pts, sm, origin, 0.25, 0.5)
    assert np.abs(want[0] - pts[0]).max() > 1e-3
    assert np.abs(got - want).max() <= EPS20 * (np.abs(pts).max() + 0.5 * np.abs(sm).max())
    # the kernel alone: the grid's own last node is inside (value = the node), anything beyond or below it gets no displacement
    noise = g.standard_normal((4, 3, 5, 3)).astype(np.float32)
    origin = [-0.25, 0.5, 1.0]
    last = np.array([-0.25 + 3 * 0.25, 0.5 + 2 * 0.25, 1.0 + 4 * 0.25], dtype=np.float32)
    q = np.stack([last, last + [0.0625, 0, 0], last + [0, 0, 0.0625], [-0.3125, 0.75, 1.5], [0.0, 0.4375, 1.5], [0.0, 0.75, 0.9375],
                  [1e6, 0.75, 1.5], [0.0, 0.75, 1.5]]).astype(np.float32)
    t = torch.from_numpy(q.copy()).cuda()
    nv.aug_elastic_(t, torch.from_numpy(noise).cuda(), origin, 0.25, 2.0)
    got = _np(t)
    assert np.array_equal(got[1:7], q[1:7])                                    # outside: bit for bit unchanged
    want = _elastic64(q, noise, origin, 0.25, 2.0)
    assert np.array_equal(want[0], last + noise[3, 2, 4].astype(np.float64) * 2.0)
    assert np.abs(got - want).max() <= EPS20 * (np.abs(q[[0, 7]]).max() + 2.0 * np.abs(noise).max())
    assert np.abs(got[7] - q[7]).max() > 1e-3


# ---- ss_aug_color -----------------------------------------------------------------------------------------------------------------
def _color64(c, lo, hi, flags, blend, tr, noise, std, normalize):
    c = c.astype(np.float64)
    if flags & 1:
        c = (1 - blend) * c + blend * ((c - lo) * (255 / (hi - lo)))
    if flags & 2:
        c = np.clip(c + tr, 0, 255)
    if flags & 4:
        c = np.clip(c + noise.astype(np.float64) * std * 255, 0, 255)
    return c / 127.5 - 1 if normalize else c


COLOR_CASES = {
    "cac": ([dict(type="ChromaticAutoContrast", p=1.0, blend_factor=None)], lambda fx: [dict(fired=True, blend=float(fx["cac_blend"]))]),
    "ctr": ([dict(type="ChromaticTranslation", p=1.0, ratio=0.05)], lambda fx: [dict(fired=True, tr=fx["ctr_tr"].tolist())]),
    "cji": ([dict(type="ChromaticJitter", p=1.0, std=0.05)], lambda fx: [dict(fired=True, noise=fx["cji_noise"])]),
    "call": ([dict(type="ChromaticAutoContrast", p=1.0), dict(type="ChromaticTranslation", p=1.0, ratio=0.05),
              dict(type="ChromaticJitter", p=1.0, std=0.05)],
             lambda fx: [dict(fired=True, blend=float(fx["call_blend"])), dict(fired=True, tr=fx["call_tr"].tolist()),
                         dict(fired=True, noise=fx["call_noise"])]),
}


@pytest.mark.parametrize("tag", list(COLOR_CASES))
@pytest.mark.parametrize("fuse", [True, False])
def test_colour_ops_match_the_reference(fx, base, tag, fuse):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import Compose
    assert (base["color"].max(0) > base["color"].min(0)).all()                   # no fixture channel is constant
    cfg, mk = COLOR_CASES[tag]
    calls = []
    orig = nv.aug_color_
    nv.aug_color_ = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        got = _np(Compose(cfg, fuse=fuse)(_cuda(base), params=mk(fx))["color"])
        assert len(calls) == (1 if fuse else len(cfg))
        assert np.abs(got - fx[tag + "_color"]).max() <= 5e-4
        assert tag == "cac" or (got.min() >= 0 and got.max() <= 255)
        if tag == "ctr":                                                         # values that clip are 0 or 255 exactly
            pre = base["color"].astype(np.float64) + fx["ctr_tr"]
            assert (pre < -5e-4).any() and (pre > 255 + 5e-4).any()
            assert (got[pre < -5e-4] == 0).all() and (got[pre > 255 + 5e-4] == 255).all()
        if tag != "cac":
            assert (got == 0).any() and (got == 255).any()
        if tag == "call":
            del calls[:]
            got = _np(Compose(cfg + [dict(type="NormalizeColor")], fuse=fuse)(_cuda(base), params=mk(fx) + [{}])["color"])
            assert len(calls) == (1 if fuse else 4)
            assert np.abs(got - fx["call_norm_color"]).max() <= 5e-4 / 127.5
    finally:
        nv.aug_color_ = orig


def test_auto_contrast_refuses_a_constant_channel(base):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    c = base["color"].copy()
    c[:, 1] = 17.0
    with pytest.raises(ValueError, match="constant"):
        TRANSFORMS.build(dict(type="ChromaticAutoContrast", p=1.0)).apply(dict(color=torch.from_numpy(c).cuda()), dict(fired=True, blend=0.5))


@pytest.mark.parametrize("n", SIZES)
def test_colour_kernel_matches_fp64(n):
    from scenesplat_amd import native as nv
    g = np.random.default_rng(n)
    c = (g.random((n, 3)) * 255).astype(np.float32)
    noise = g.standard_normal((n, 3)).astype(np.float32)
    tr, blend, std = g.uniform(-12, 12, 3), 0.37, 0.05
    lo, hi = (c.min(0), c.max(0)) if n > 1 else (np.zeros(3, np.float32), np.full(3, 255, np.float32))
    for flags, normalize in ((1, False), (2, False), (4, False), (7, False), (7, True), (0, True)):
        t = torch.from_numpy(c.copy()).cuda()
        nv.aug_color_(t, flags, lo.tolist(), hi.tolist(), blend, tr.tolist(), std, torch.from_numpy(noise).cuda(), 0, normalize)
        want = _color64(c, lo.astype(np.float64), hi.astype(np.float64), flags, blend, tr, noise, std, normalize)
        assert np.abs(_np(t) - want).max() <= (5e-4 / 127.5 if normalize else 5e-4), (flags, normalize)
    own = []
    for seed in (11, 11, 12):                                                    # the kernel's own draws: seeded
        t = torch.from_numpy(c.copy()).cuda()
        nv.aug_color_(t, 4, jitter_std=std, seed=seed)
        own.append(_np(t))
    assert np.array_equal(own[0], own[1]) and (n == 1 or not np.array_equal(own[0], own[2]))
    if n == 70001:
        z = (own[0].astype(np.float64) - c) / (std * 255)
        z = z[(own[0] > 0) & (own[0] < 255)]
        assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05


# ---- RandomDropout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["do", "dos"])
def test_dropout_replays_the_reference_index(fx, base, tag):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    from scenesplat_amd.pointcept_api.transform import DROPOUT_KEYS
    op = TRANSFORMS.build(dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=1.0))
    data = _cuda(base)
    data["untouched"] = torch.arange(len(base["coord"]), device="cuda")
    idx = fx["do_idx"]
    if tag == "dos":
        data["sampled_index"] = torch.from_numpy(fx["dos_sampled_in"]).cuda()
    out = op.apply(data, dict(fired=True, idx=idx))
    if tag == "dos":
        assert np.array_equal(_np(out["sampled_index"]), fx["dos_sampled_out"])
        idx = fx["dos_idx"]                                                      # unique(idx + sampled_index), as the reference
    checked = 0
    for k in DROPOUT_KEYS:
        if k in base:
            assert np.array_equal(_np(out[k]), base[k][idx]), k
            checked += 1
    assert checked == 9 and out["untouched"].shape[0] == len(base["coord"])
    own = [_np(op.apply(_cuda(base), dict(fired=True, seed=s))["coord"]) for s in (3, 3, 4)]
    assert own[0].shape == (1600, 3) and np.array_equal(own[0], own[1]) and not np.array_equal(own[0], own[2])
    rows = {r.tobytes() for r in base["coord"]}
    assert len({r.tobytes() for r in own[0]}) == 1600 and all(r.tobytes() in rows for r in own[0])
    assert op.apply(data, dict(fired=False, seed=1)) is data


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_compose_runs_a_shipped_train_list_end_to_end(lists):
    from scenesplat_amd.pointcept_api import Compose
    cfg = next(v for k, v in lists.items() if "lang-pretrain-scannet" in k)
    sample = _fixture(5000, 3)
    seed = 2024
    probe = Compose(cfg, seed=seed)
    params = [t.draw(probe.rng, {}) for t in probe.transforms]
    assert any(p.get("fired") for t, p in zip(probe.transforms, params) if type(t).__name__ == "RandomRotate")
    runs = [Compose(cfg, seed=seed)(_cuda(sample)), Compose(cfg, seed=seed)(_cuda(sample)),
            Compose(cfg, seed=seed, fuse=False)(_cuda(sample), params=params)]
    out = runs[0]
    assert set(out) == {"coord", "grid_coord", "segment", "lang_feat", "valid_feat_mask", "offset", "feat"}
    n = out["coord"].shape[0]
    assert 3000 < n <= 5000 and _np(out["offset"]).tolist() == [n]
    assert tuple(out["feat"].shape) == (n, 11) and out["feat"].dtype == torch.float32
    assert all(out[k].shape[0] == n for k in ("grid_coord", "segment", "lang_feat", "valid_feat_mask"))
    gc = _np(out["grid_coord"])
    assert gc.dtype.kind == "i" and gc.min() >= 0 and (gc.min(0) == 0).all()
    assert len(np.unique(gc, axis=0)) == n                                        # one Gaussian per voxel
    feat = _np(out["feat"]).astype(np.float64)
    assert np.isfinite(feat).all() and np.abs(np.linalg.norm(feat[:, 4:8], axis=1) - 1).max() <= 2e-6
    assert feat[:, :3].min() >= -1 - 1e-6 and feat[:, :3].max() <= 1 + 1e-6       # NormalizeColor
    c = _np(out["coord"])
    assert abs(c[:, 0].min() + c[:, 0].max()) < 1e-5 and abs(c[:, 1].min() + c[:, 1].max()) < 1e-5    # the second CenterShift
    for k in out:                                                                 # the same seed: the same bits
        assert torch.equal(out[k], runs[1][k]), k
    # op by op with the same draws: the voxel set can differ where a coordinate sits within rounding of a voxel face
    assert abs(runs[2]["coord"].shape[0] - n) <= 0.01 * n and set(runs[2]) == set(out)
