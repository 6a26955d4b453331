"""CPU: the host side of `pc_coord` / `pc_segment` (the point cloud some lists carry beside the Gaussians) in
scenesplat_amd/pointcept_api/transform.py -- the second pending affine of RigidState against the cloud the REFERENCE's transforms
produced (tests/golden/augment_pc.npz, written by tests/golden/make_golden_pc.py with the draws of augment_b.npz), which ops fold
into it and which do not, the shipped val / test lists that name pc_coord (tests/golden/pc_configs.txt), and the argument
contract of ss_voxel_pick_labelled on the paths that return before a launch.

Bound of the affine check: 2^-20 max(|x| |A|^T + |b|), the one tests/test_hip_augment.py applies to `coord`; the reference itself
shifts the cloud in fp32 (CenterShift works in place on the fp32 array), so an fp64 composition cannot be held tighter."""
import ast
import os

import numpy as np
import pytest
import torch

EPS20 = 2.0 ** -20


def _affine_bound(A, b, x):
    return EPS20 * float((np.abs(x).astype(np.float64) @ np.abs(A).T + np.abs(b)).max())


def _coord(n, seed):
    """the coordinates of make_golden_augment.fixture(n, seed)"""
    return (np.random.RandomState(seed).rand(n, 3) * np.array([4.0, 3.0, 1.5])).astype(np.float32)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return {**np.load(os.path.join(golden_dir, "augment_b.npz")), **np.load(os.path.join(golden_dir, "augment_pc.npz"))}


@pytest.fixture(scope="module")
def lists(golden_dir):
    with open(os.path.join(golden_dir, "pc_configs.txt")) as f:
        return ast.literal_eval(f.read())


def _box(pts):
    return lambda A, b: np.concatenate([(pts[0] @ A.T + b).min(0), (pts[0] @ A.T + b).max(0)])


BOTH = dict(coord=None, pc_coord=None)                     # the keys are all fold() looks at with a bbox_fn


def _head_ops(fx):
    """the rigid ops of the recorded head of the shipped list (RandomDropout sits between the first two) and their draws"""
    from scenesplat_amd.pointcept_api import transform as tf
    a = fx["seq_angles"]
    return [(tf.CenterShift(apply_z=True), {}),
            (tf.RandomRotate(angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True), dict(fired=True, angle=float(a[0]))),
            (tf.RandomRotate(angle=[-1 / 64, 1 / 64], axis="x", always_apply=True), dict(fired=True, angle=float(a[1]))),
            (tf.RandomRotate(angle=[-1 / 64, 1 / 64], axis="y", always_apply=True), dict(fired=True, angle=float(a[2]))),
            (tf.RandomScale(scale=[0.9, 1.1]), dict(scale=fx["seq_scale"].tolist())),
            (tf.RandomFlip(p=0.5), dict(flip_x=bool(fx["seq_flips"][0]), flip_y=bool(fx["seq_flips"][1])))]


def test_cloud_affine_of_the_recorded_head_matches_the_reference(fx):
    from scenesplat_amd.pointcept_api import transform as tf
    x = _coord(int(fx["seq_n"]), int(fx["seq_seed"])).astype(np.float64)
    pts = [x]
    st = tf.RigidState(bbox_fn=_box(pts))
    for i, (op, p) in enumerate(_head_ops(fx)):
        op.fold(st, BOTH, p)
        if i == 0:
            pts[0] = x[fx["seq_idx"]]                      # RandomDropout: the rotations about the box centre see the kept Gaussians
    assert st.pc_pending() and st.coord_pending() and st.flip == 3
    x_pc = fx["pc_coord"].astype(np.float64)
    got = x_pc @ st.A_pc.T + st.b_pc
    assert got.shape == fx["seq_pc"].shape
    assert np.abs(got - fx["seq_pc"]).max() <= _affine_bound(st.A_pc, st.b_pc, fx["pc_coord"])
    assert np.abs(fx["seq_pc"] - x_pc).max() > 0.1          # the cloud did move
    assert np.array_equal(st.A_pc, st.A) and np.array_equal(st.b_pc, st.b)     # no shift / jitter yet: one affine for both
    a12 = st.affine12_pc()
    assert len(a12) == 12 and np.array_equal(a12[:9], st.A_pc.reshape(-1)) and np.array_equal(a12[9:], st.b_pc)
    st.reset()
    assert not st.pc_pending() and st.affine12_pc() is None and np.array_equal(st.A_pc, np.eye(3)) and not st.b_pc.any()


def test_shift_and_jitter_leave_the_cloud_affine_alone(fx):
    from scenesplat_amd.pointcept_api import transform as tf
    pts = [_coord(100, 3).astype(np.float64)]
    st = tf.RigidState(bbox_fn=_box(pts))
    for op, p in _head_ops(fx)[:5]:
        op.fold(st, BOTH, p)
    A_pc, b_pc, b = st.A_pc.copy(), st.b_pc.copy(), st.b.copy()
    tf.RandomShift().fold(st, BOTH, dict(shift=[0.1, -0.15, 0.05]))
    assert np.array_equal(st.A_pc, A_pc) and np.array_equal(st.b_pc, b_pc) and not np.array_equal(st.b, b)
    tf.RandomJitter(sigma=0.005, clip=0.01).fold(st, BOTH, dict(seed=5))
    assert np.array_equal(st.A_pc, A_pc) and np.array_equal(st.b_pc, b_pc) and st.jitter is not None
    # alone, neither makes the cloud pending: their flush does not launch a pass over it
    st = tf.RigidState(bbox_fn=_box(pts))
    tf.RandomShift().fold(st, BOTH, dict(shift=[0.1, -0.15, 0.05]))
    tf.RandomJitter(sigma=0.005, clip=0.01).fold(st, BOTH, dict(seed=5))
    assert st.coord_pending() and not st.pc_pending()


def test_without_a_cloud_nothing_is_pending_for_it(fx):
    from scenesplat_amd.pointcept_api import transform as tf
    pts = [_coord(100, 3).astype(np.float64)]
    for data in (dict(coord=None), dict(pc_coord=None)):                      # the reference treats the cloud under `"coord" in data`
        st = tf.RigidState(bbox_fn=_box(pts))
        for op, p in _head_ops(fx):
            op.fold(st, data, p)
        assert not st.pc_pending() and st.affine12_pc() is None


@pytest.mark.parametrize("apply_z", [True, False])
def test_center_shift_moves_the_cloud_by_the_gaussians_shift(apply_z):
    from scenesplat_amd.pointcept_api import transform as tf
    x = _coord(200, 4).astype(np.float64) + [3.0, -1.0, 0.25]
    st = tf.RigidState(bbox_fn=_box([x]))
    tf.CenterShift(apply_z=apply_z).fold(st, BOTH, {})
    want = -np.array([(x[:, 0].min() + x[:, 0].max()) / 2, (x[:, 1].min() + x[:, 1].max()) / 2, x[:, 2].min() if apply_z else 0.0])
    assert np.array_equal(st.b, want) and np.array_equal(st.b_pc, st.b) and np.array_equal(st.A_pc, np.eye(3))


def test_rotation_without_a_centre_turns_the_cloud_about_the_gaussians_box():
    from scenesplat_amd.pointcept_api import transform as tf
    x = _coord(200, 5).astype(np.float64) + [3.0, -1.0, 0.25]
    c = (x.min(0) + x.max(0)) / 2
    for cls, kw in ((tf.RandomRotate, dict(axis="x", center=None)), (tf.RandomRotateTargetAngle, dict(axis="z", center=None))):
        st = tf.RigidState(bbox_fn=_box([x]))
        cls(**kw).fold(st, BOTH, dict(fired=True, angle=0.7))
        rot = tf.axis_rotation(kw["axis"], 0.7)
        assert np.array_equal(st.A_pc, rot) and np.array_equal(st.b_pc, rot @ (-c) + c)
        assert np.array_equal(st.A, st.A_pc) and np.array_equal(st.b, st.b_pc)
        # a cloud far from the Gaussians still turns about THEIR centre, not its own
        far = x + 10.0
        assert np.abs((far @ st.A_pc.T + st.b_pc) - ((far - c) @ rot.T + c)).max() <= 1e-12


def test_flush_refuses_a_cloud_that_is_not_on_the_device():
    from scenesplat_amd.pointcept_api import transform as tf
    data = dict(coord=torch.rand(8, 3), pc_coord=torch.rand(5, 3))
    with pytest.raises(RuntimeError, match="pc_coord.*no CPU fallback"):
        tf.RandomScale().apply(data, dict(scale=[1.05]))


def test_every_shipped_list_that_names_the_cloud_builds(lists):
    from scenesplat_amd.pointcept_api import TRANSFORMS, Compose
    assert len(lists) >= 10
    assert sum("::val" in k for k in lists) >= 4 and sum("::test" in k and k.endswith("::transform") for k in lists) >= 5
    for cfgname in ("matterport3d", "holicity", "concat_dataset"):
        assert any(cfgname in k for k in lists), cfgname
    named, samplers = 0, {True: 0, False: 0}
    for name, cfg in lists.items():
        comp = Compose(cfg)
        assert len(comp.transforms) == len(cfg) >= 3, name
        named += "pc_coord" in repr(cfg)
        for entry, t in zip(cfg, comp.transforms):
            assert type(t) is TRANSFORMS.get(entry["type"]), (name, entry["type"])
            if entry["type"] == "GridSample":
                assert t.apply_to_pc is entry.get("apply_to_pc", True), name     # the config's value, the reference's default
                assert t.mode == "train"
                samplers[t.apply_to_pc] += 1
    assert named >= 10 and samplers[True] >= 4 and samplers[False] >= 5
    # every test dataset comes as a pair: the list in front of the fragments and the one behind them, which collects the cloud
    for k in lists:
        if "::test" in k and k.endswith("::transform"):
            post = lists[k[:-len("transform")] + "post_transform"]
            assert post[-1]["type"] == "Collect" and {"pc_coord", "pc_segment"} <= set(post[-1]["keys"]), k


def test_voxel_pick_entry_point_checks_its_arguments():
    import ctypes
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    SS_OK, SS_ERR_ARG = 0, 1
    buf = (ctypes.c_int32 * 4)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ss_voxel_pick_labelled(ptr, ptr, -1, None, -1, ptr, None) == SS_ERR_ARG
    assert lib.ss_voxel_pick_labelled(None, ptr, 3, None, -1, ptr, None) == SS_ERR_ARG           # NULL order
    assert lib.ss_voxel_pick_labelled(ptr, None, 3, None, -1, ptr, None) == SS_ERR_ARG
    assert lib.ss_voxel_pick_labelled(ptr, ptr, 3, None, -1, None, None) == SS_ERR_ARG
    assert lib.ss_voxel_pick_labelled(None, None, 0, None, -1, None, None) == SS_OK              # nothing to do: no launch
