"""Golden vectors of the transforms beyond the shipped lists, from the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment_rest.py

The recipe of make_golden_augment.py: pointcept/datasets/transform.py is imported through the stub loader, `random` / `np.random`
are seeded, what the transform will draw is drawn once in advance, the generators are re-seeded and the transform runs ->
tests/golden/augment_rest.npz (data only; no reference source).

  fixture   fixture(2000, seed) of make_golden_augment.py, with
            `hsv_in`    its colours with planted rows in front: black, (255, 255, 255), the three pure primaries, grey rows, rows
                        with r == g == max and with g == b == max (and r == b == max); the rest stay non-integer colours
            `instance`  ids with gaps (-1, 0, 3, 4, 9, 17, 40, 41, 1000), -1 on valid segments included; the fixture's segments
                        already hold the ignored 0 / 1 / -1
  per op    HueSaturationTranslation (shipped 0.2 / 0.2 and the default 0.5 / 0.2: draws + output), RandomColorDrop, NormalizeCoord
            (alone, and behind CenterShift -> RandomRotate z -> RandomScale with their draws), PositiveShift, PointClip, ShufflePoint
            (its permutation), CropBoundary (its kept rows), InstanceParser
  distances the reference sums NormalizeCoord's centroid and InstanceParser's centroids sequentially in fp32; `*_ref_err` is the
            reference's own distance from the fp64 numpy restatement of tests/test_augment_rest_host.py, which the tests add to
            their bound when they compare with the reference's output
"""
import importlib
import os
import random
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
R = "/root/reference/"
N = 2000
SEED = 21


def planted_colors(color):
    """the fixture's colours with the HSV edge rows planted in front"""
    rows = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 128, 128), (1, 1, 1), (37.5, 37.5, 37.5),
            (200, 200, 10), (200, 200, 199.5), (10, 200, 200), (3.25, 77.5, 77.5), (200, 10, 200), (90, 90, 0), (0, 17, 17),
            (255, 255, 0), (0, 255, 255), (255, 0, 255), (254.99, 255, 254.99), (1e-3, 0, 0)]
    out = color.copy()
    out[:len(rows)] = np.asarray(rows, dtype=np.float32)
    return out


def instance_ids(n, seed):
    g = np.random.RandomState(seed + 2000)
    return g.choice(np.array([-1, 0, 3, 4, 9, 17, 40, 41, 1000], dtype=np.int64), n)


def main():
    import make_golden as mg
    from make_golden_augment import fixture
    import test_augment_rest_host as H
    mg.stubpkg("pointcept", R + "pointcept")
    mg.stubpkg("pointcept.utils", R + "pointcept/utils")
    mg.stubpkg("pointcept.datasets", R + "pointcept/datasets")
    T = importlib.import_module("pointcept.datasets.transform")
    fx = {"n": np.int64(N), "seed": np.int64(SEED)}
    base = fixture(N, SEED)
    base["instance"] = instance_ids(N, SEED)
    fx["instance"] = base["instance"]
    fx["hsv_in"] = planted_colors(base["color"])

    def fresh():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}

    def seed(s):
        random.seed(s)
        np.random.seed(s)

    # ---- HueSaturationTranslation ----
    for tag, s, kw in (("hsa", 200, dict(hue_max=0.2, saturation_max=0.2)), ("hsb", 201, dict())):
        op = T.HueSaturationTranslation(**kw)
        seed(s)
        hue_val = (np.random.rand() - 0.5) * 2 * op.hue_max
        sat_ratio = 1 + (np.random.rand() - 0.5) * 2 * op.saturation_max
        seed(s)
        d = fresh()
        d["color"] = fx["hsv_in"].copy()
        out = op(d)["color"]
        assert out.dtype == np.float32 and np.array_equal(out, np.floor(out))
        assert np.array_equal(H.hsv64(fx["hsv_in"], hue_val, sat_ratio), out), "the fp64 restatement misses the reference"
        fx[tag + "_hue_val"], fx[tag + "_sat_ratio"], fx[tag + "_color"] = np.float64(hue_val), np.float64(sat_ratio), out.astype(np.uint8)
    assert not np.array_equal(fx["hsa_color"], fx["hsb_color"])

    # ---- RandomColorDrop (a seed for which it fires) ----
    s = 210
    while True:
        seed(s)
        if np.random.rand() < 0.2:
            break
        s += 1
    seed(s)
    fx["cd_color"] = T.RandomColorDrop(p=0.2, color_augment=0.25)(fresh())["color"]
    assert np.array_equal(fx["cd_color"], base["color"] * np.float32(0.25))

    # ---- NormalizeCoord alone, and behind CenterShift -> RandomRotate z -> RandomScale ----
    out = T.NormalizeCoord()(fresh())
    want_c, want_s = H.normalize64(base["coord"], base["scale"])
    fx["nc_coord"], fx["nc_scale"] = out["coord"], out["scale"]
    fx["nc_ref_err"] = np.float64(np.abs(out["coord"].astype(np.float64) - want_c).max())
    fx["nc_scale_ref_err"] = np.float64(np.abs(out["scale"].astype(np.float64) / want_s - 1).max())
    assert out["coord"].dtype == np.float32 and fx["nc_ref_err"] < 1e-5
    ops = [T.CenterShift(apply_z=True), T.RandomRotate(angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
           T.RandomScale(scale=[0.9, 1.1]), T.NormalizeCoord()]
    seed(220)
    random.random()
    angle = np.random.uniform(-1, 1) * np.pi
    sc = np.random.uniform(0.9, 1.1, 1)
    seed(220)
    d = fresh()
    for op in ops:
        d = op(d)
    fx["ncs_angle"], fx["ncs_scale_draw"] = np.float64(angle), sc
    fx["ncs_coord"], fx["ncs_scale"] = d["coord"], d["scale"]
    c64 = base["coord"].astype(np.float64)
    shift = np.array([(c64[:, 0].min() + c64[:, 0].max()) / 2, (c64[:, 1].min() + c64[:, 1].max()) / 2, c64[:, 2].min()])
    ca, sa = np.cos(angle), np.sin(angle)
    rot = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    pre = ((c64 - shift) @ rot.T) * sc
    want_c, want_s = H.normalize64(pre, base["scale"].astype(np.float64) * sc)
    fx["ncs_ref_err"] = np.float64(np.abs(np.asarray(d["coord"], dtype=np.float64) - want_c).max())
    fx["ncs_scale_ref_err"] = np.float64(np.abs(np.asarray(d["scale"], dtype=np.float64) / want_s - 1).max())
    assert fx["ncs_ref_err"] < 1e-5, fx["ncs_ref_err"]

    # ---- PositiveShift, PointClip ----
    fx["ps_coord"] = T.PositiveShift()(fresh())["coord"]
    fx["pcl_range"] = np.array([0.5, 0.25, 0.1, 3.0, 2.5, 1.0])
    fx["pcl_coord"] = T.PointClip(point_cloud_range=tuple(fx["pcl_range"]))(fresh())["coord"].astype(np.float32)
    assert (fx["pcl_coord"] != base["coord"]).any(0).all()

    # ---- ShufflePoint: the permutation it draws; every key it moves is checked against it here ----
    seed(230)
    perm = np.arange(N)
    np.random.shuffle(perm)
    seed(230)
    out = T.ShufflePoint()(fresh())
    for k in ("coord", "color", "normal", "segment", "instance"):
        assert np.array_equal(out[k], base[k][perm]), k
    assert np.array_equal(out["quat"], base["quat"]), "the reference moves quat after all?"
    fx["sp_idx"] = perm.astype(np.int64)

    # ---- CropBoundary: the rows it keeps ----
    out = T.CropBoundary()(fresh())
    keep = np.nonzero((base["segment"] != 0) & (base["segment"] != 1))[0]
    for k in ("coord", "color", "normal", "segment", "instance"):
        assert np.array_equal(out[k], base[k][keep]), k
    fx["cb_idx"] = keep.astype(np.int64)
    assert 0 < len(keep) < N

    # ---- InstanceParser ----
    out = T.InstanceParser(segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)(fresh())
    inst64, cen64, box64 = H.instance64(base["coord"], base["segment"], base["instance"], (-1, 0, 1), -1)
    assert np.array_equal(out["instance"], inst64) and np.array_equal(out["bbox"].astype(np.float32), box64)
    valid = ~np.isin(base["segment"], (-1, 0, 1))
    assert (base["instance"][valid] == -1).any(), "no id of -1 on a valid segment"
    fx["ip_instance"] = out["instance"].astype(np.int64)
    fx["ip_bbox"] = out["bbox"].astype(np.float32)
    assert np.array_equal(fx["ip_bbox"].astype(np.float64), out["bbox"]), "the reference's boxes hold more than fp32"
    fx["ip_centroid"] = out["instance_centroid"].astype(np.float32)
    assert np.array_equal(fx["ip_centroid"].astype(np.float64), out["instance_centroid"])
    fx["ip_ref_err"] = np.float64(np.abs(out["instance_centroid"] - cen64).max())
    assert fx["ip_ref_err"] < 1e-5

    path = os.path.join(HERE, "augment_rest.npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < (1 << 20)
    print("augment_rest.npz", os.path.getsize(path) // 1024, "KiB;", int(fx["ip_bbox"].shape[0]), "instances; reference distances",
          {k: float(v) for k, v in fx.items() if k.endswith("_ref_err")})


if __name__ == "__main__":
    main()
