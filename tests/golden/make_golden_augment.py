"""Golden vectors of the per-sample augmentations from the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

Same recipe as make_golden_transforms.py: pointcept/datasets/transform.py is imported through the stub loader, `random` /
`np.random` are seeded, what the transform will draw is drawn once in advance, the generators are re-seeded and the transform
runs -> tests/golden/augment.npz holds inputs' seeds, the draws and the outputs (data only; no reference source), and
tests/golden/augment_configs.txt the `data.train.transform` lists of the shipped lang-pretrain / semseg-gs configs.

  fixture   sample(n, seed) of make_golden_transforms.py with a unit `normal` added and colours on 0..255 (`fixture()` below; the
            tests rebuild it from the seed)
  per op    n = 2000: CenterShift, RandomRotate z / x / y, RandomRotateTargetAngle, RandomScale, RandomShift, RandomFlip (x, y,
            both), RandomJitter, ElasticDistortion (both passes, raw noise grids), the three chromatic ops alone and in sequence,
            NormalizeColor, RandomDropout (with and without sampled_index)
  sequence  the head of the shipped list in one run: CenterShift -> RandomDropout -> RandomRotate z / x / y -> RandomScale ->
            RandomFlip -> RandomJitter (checkpoint `seq_*`) -> ElasticDistortion (`seq_el_*`: raw grids, fp64 coordinates) -> the
            three chromatic ops (`seq_color`)

Size: a committed file stays under 1 MiB and random fp64 mantissas do not compress, so the vectors are split over two files:
augment.npz (CenterShift, the rotations, scale, shift) and augment_b.npz (everything else); the tests read both as one table.
What is fp64 in the reference is stored in fp64; draws the device replays in fp32 (noise) are stored in fp32.  A flip of one axis
stores its quaternions only (coord / normal come with the flip of both); the sequence runs on n = 1000.
"""
import ast
import glob
import importlib
import os
import pprint
import random
import sys
import textwrap

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
R = "/root/reference/"
N = 2000


def fixture(n, seed):
    """make_golden_transforms.sample(n, seed) + unit normals, colours on 0..255."""
    from make_golden_transforms import sample
    d = sample(n, seed)
    g = np.random.RandomState(seed + 1000)
    d["color"] = (g.rand(n, 3) * 255).astype(np.float32)
    nrm = g.randn(n, 3)
    d["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return d


def branch_gap(quat_wxyz):
    """Gap between the two largest of [M00, M11, M22, trace] of the rotation a (unit) quaternion stands for: scipy's from_matrix
    picks its branch -- and with it the sign of the result -- by that arg-max, so a small gap means the sign is a coin toss."""
    q = np.asarray(quat_wxyz, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    dec = np.stack([1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y), 3 - 4 * (x * x + y * y + z * z)], 1)
    s = np.sort(dec, axis=1)
    return s[:, 3] - s[:, 2]


def blur2(raw):
    """what the reference does to a raw noise grid before it interpolates: the 3-tap mean along x, y, z, twice, zeros outside"""
    import scipy.ndimage
    sm = raw
    for _ in range(2):
        for shape in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)):
            sm = scipy.ndimage.convolve(sm, np.ones(shape, np.float32) / 3, mode="constant", cval=0)
    return sm


def elastic_f32(coord, noise, origin, gran, mag):
    """The kernel's formula restated in fp32 numpy: the yardstick for what fp32 can reach against the reference's fp64 result."""
    f32 = np.float32
    c = coord.astype(f32)
    d = np.array(noise.shape[:3])
    t = (c - origin.astype(f32)) / f32(gran)
    inside = np.all((t >= 0) & (t <= (d - 1).astype(f32)), axis=1)
    i0 = np.clip(np.floor(t).astype(int), 0, d - 2)
    f = t - i0.astype(f32)
    acc = np.zeros((len(c), 3), f32)
    for k in range(8):
        o = np.array([k >> 2, (k >> 1) & 1, k & 1])
        w = np.prod(np.where(o, f, f32(1) - f), axis=1, dtype=f32)
        j = i0 + o
        acc += w[:, None] * noise[j[:, 0], j[:, 1], j[:, 2]]
    return np.where(inside[:, None], c + acc * f32(mag), c)


def transform_lists(ref):
    """{config path[::dataset index]: data.train.transform} of every shipped lang-pretrain-* / semseg-gs-* config, as data."""
    import make_golden_configs as mc
    import make_golden_semseg as ms
    out, skipped = {}, []
    for p in sorted(glob.glob(ref + "configs/*/lang-pretrain-*.py") + glob.glob(ref + "configs/*/semseg-gs-*.py")):
        rel = os.path.relpath(p, ref)
        try:
            cfg = mc.load_config(ref, rel)
        except AssertionError:                       # the ScanNet semseg configs import their class-name constants
            cfg = ms.load_config(ref, rel)
        except NameError as err:                     # one shipped concat config names an undefined data root: not loadable as shipped
            skipped.append((rel, str(err)))
            continue

        def walk(d, tag):
            if "transform" in d:
                out[tag] = d["transform"]
            for i, sub in enumerate(d.get("datasets", [])):
                walk(sub, "%s::datasets[%d]" % (rel, i))
        walk(cfg["data"]["train"], rel)
    txt = "{\n" + "".join("%r:\n%s,\n" % (k, textwrap.indent(pprint.pformat(v, width=116, sort_dicts=False), "    "))
                          for k, v in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(os.path.join(HERE, "augment_configs.txt"), "w") as f:
        f.write(txt + "\n")
    return out, skipped


def main():
    import make_golden as mg
    mg.stubpkg("pointcept", R + "pointcept")
    mg.stubpkg("pointcept.utils", R + "pointcept/utils")
    mg.stubpkg("pointcept.datasets", R + "pointcept/datasets")
    T = importlib.import_module("pointcept.datasets.transform")
    fx = {"n": np.int64(N), "seed": np.int64(21)}
    base = fixture(N, 21)

    def fresh():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}

    def seed(s):
        random.seed(s)
        np.random.seed(s)

    # ---- CenterShift ----
    fx["cs_z_coord"] = T.CenterShift(apply_z=True)(fresh())["coord"]
    fx["cs_xy_coord"] = T.CenterShift(apply_z=False)(fresh())["coord"]

    # ---- rotations: the angle the op will draw, then the op ----
    for tag, kw in (("rz", dict(angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5)),
                    ("rx", dict(angle=[-1 / 64, 1 / 64], axis="x", p=0.5)),
                    ("ry", dict(angle=[-1 / 64, 1 / 64], axis="y", p=0.5))):
        s = 30
        while True:                                    # a seed for which the op fires
            seed(s)
            if not random.random() > kw["p"]:
                break
            s += 1
        angle = np.random.uniform(kw["angle"][0], kw["angle"][1]) * np.pi
        seed(s)
        out = T.RandomRotate(**kw)(fresh())
        fx[tag + "_angle"] = np.float64(angle)
        fx[tag + "_coord"], fx[tag + "_quat"], fx[tag + "_normal"] = out["coord"], out["quat"], out["normal"]
        assert out["coord"].dtype == np.float64 and not np.allclose(out["coord"], base["coord"])
    s = 40
    while True:
        seed(s)
        if not random.random() > 0.75:
            break
        s += 1
    angle = np.random.choice((1 / 2, 1, 3 / 2)) * np.pi
    seed(s)
    out = T.RandomRotateTargetAngle(angle=(1 / 2, 1, 3 / 2), center=[0, 0, 0], axis="z", p=0.75)(fresh())
    fx["rt_angle"] = np.float64(angle)
    fx["rt_coord"], fx["rt_quat"], fx["rt_normal"] = out["coord"], out["quat"], out["normal"]

    # ---- RandomScale (isotropic as shipped, and anisotropic), RandomShift ----
    seed(50)                                           # anisotropic: three factors (the sequence below has the shipped isotropic one)
    draw = np.random.uniform(0.9, 1.1, 3)
    seed(50)
    out = T.RandomScale(scale=[0.9, 1.1], anisotropic=True)(fresh())
    fx["sca_draw"], fx["sca_coord"], fx["sca_scale"] = draw, out["coord"], out["scale"]
    seed(51)
    sh = [np.random.uniform(-0.2, 0.2), np.random.uniform(-0.2, 0.2), np.random.uniform(-0.1, 0.1)]
    seed(51)
    fx["sh_draw"] = np.array(sh)
    fx["sh_coord"] = T.RandomShift(shift=((-0.2, 0.2), (-0.2, 0.2), (-0.1, 0.1)))(fresh())["coord"]

    # ---- RandomFlip: seeds that give x only, y only, both ----
    want = {(True, False): "fx", (False, True): "fy", (True, True): "fxy"}
    s = 60
    while want:
        seed(s)
        got = (bool(np.random.rand() < 0.5), bool(np.random.rand() < 0.5))
        if got in want:
            tag = want.pop(got)
            seed(s)
            out = T.RandomFlip(p=0.5)(fresh())
            fx[tag + "_quat"] = out["quat"]
            if tag == "fxy":
                fx["fxy_coord"], fx["fxy_normal"] = out["coord"], out["normal"]
            gap = branch_gap(out["quat"])
            assert (gap < 1e-5).mean() <= 0.005, "fixture has too many near ties of the sign rule"
            assert (out["coord"][:, 0] == -base["coord"][:, 0]).all() == got[0]
        s += 1

    # ---- RandomJitter (shipped sigma / clip: clips at 2 sigma, so clipping is exercised) ----
    seed(70)
    noise = np.random.randn(N, 3)
    seed(70)
    out = T.RandomJitter(sigma=0.005, clip=0.01)(fresh())
    fx["jit_noise"] = noise.astype(np.float32)
    fx["jit_coord"] = out["coord"]
    assert (np.abs(0.005 * noise) > 0.01).any()

    # ---- ElasticDistortion: pass by pass, fp64 in / fp64 out, raw grids recorded ----
    cur = base["coord"].copy()
    worst = 0.0
    for k, (gran, mag) in enumerate([[0.2, 0.4], [0.8, 1.6]]):
        dim = ((cur - cur.min(0)).max(0) // gran).astype(int) + 3                  # on the fp32 coordinates, as the datasets hand them over
        seed(80 + k)
        raw = np.random.randn(*dim, 3).astype(np.float32)
        seed(80 + k)
        out64 = T.ElasticDistortion.elastic_distortion(cur.astype(np.float64), gran, mag)
        seed(80 + k)
        out32 = T.ElasticDistortion.elastic_distortion(cur.copy(), gran, mag)      # the fp32 path draws the same grid (same noise_dim)
        assert np.abs(out32 - out64).max() < 1e-5
        err = np.abs(elastic_f32(cur, blur2(raw), cur.min(0) - np.float32(gran), gran, mag).astype(np.float64) - out64).max()
        worst = max(worst, err)
        # input of pass 0: the fixture's coord; of pass 1: el0_out rounded to fp32
        fx["el%d_raw" % k], fx["el%d_out" % k], fx["el%d_f32_err" % k] = raw, out64, np.float64(err)
        assert np.abs(out64 - cur).max() > 1e-3
        cur = out64.astype(np.float32)
    assert worst < 1e-5, "ill-conditioned elastic fixture"

    # ---- the blur alone: a (7,5,4,3) grid and the smallest grid the reference can produce ----
    g = np.random.RandomState(90)
    for tag, shape in (("blur_a", (7, 5, 4, 3)), ("blur_b", (3, 3, 3, 3))):
        raw = g.randn(*shape).astype(np.float32)
        fx[tag + "_in"], fx[tag + "_out"] = raw, blur2(raw)

    # ---- chromatic ops: alone (p = 1 so that they fire) and in sequence; NormalizeColor ----
    assert (base["color"].max(0) > base["color"].min(0)).all()
    seed(100)
    np.random.rand()
    blend = np.random.rand()
    seed(100)
    fx["cac_blend"] = np.float64(blend)
    fx["cac_color"] = T.ChromaticAutoContrast(p=1.0, blend_factor=None)(fresh())["color"]
    seed(101)
    np.random.rand()
    tr = (np.random.rand(1, 3) - 0.5) * 255 * 2 * 0.05
    seed(101)
    fx["ctr_tr"] = tr[0]
    fx["ctr_color"] = T.ChromaticTranslation(p=1.0, ratio=0.05)(fresh())["color"]
    seed(102)
    np.random.rand()
    cn = np.random.randn(N, 3)
    seed(102)
    fx["cji_noise"] = cn.astype(np.float32)
    fx["cji_color"] = T.ChromaticJitter(p=1.0, std=0.05)(fresh())["color"]
    for k in ("ctr_color", "cji_color"):
        assert (fx[k] == 0).any() and (fx[k] == 255).any(), "no clipped value in the fixture"
    seed(103)
    np.random.rand(); b3 = np.random.rand()
    np.random.rand(); t3 = (np.random.rand(1, 3) - 0.5) * 255 * 2 * 0.05
    np.random.rand(); n3 = np.random.randn(N, 3)
    seed(103)
    d = fresh()
    for op in (T.ChromaticAutoContrast(p=1.0), T.ChromaticTranslation(p=1.0, ratio=0.05), T.ChromaticJitter(p=1.0, std=0.05)):
        d = op(d)
    fx["call_blend"], fx["call_tr"], fx["call_noise"], fx["call_color"] = np.float64(b3), t3[0], n3.astype(np.float32), d["color"]
    fx["call_norm_color"] = T.NormalizeColor()(dict(color=d["color"].copy()))["color"]

    # ---- RandomDropout: the index the op draws; every subset key is checked against it here, the index is what gets stored ----
    for tag, with_si in (("do", False), ("dos", True)):
        d = fresh()
        if with_si:
            d["sampled_index"] = np.sort(np.random.RandomState(5).choice(N, 40, replace=False))
            fx["dos_sampled_in"] = d["sampled_index"]
        seed(110)
        random.random()
        idx = np.random.choice(N, int(N * (1 - 0.2)), replace=False)
        seed(110)
        out = T.RandomDropout(dropout_ratio=0.2, dropout_application_ratio=1.0)(d)
        if with_si:
            idx = np.unique(np.append(idx, fx["dos_sampled_in"]))
            fx["dos_sampled_out"] = out["sampled_index"]
        for k in ("coord", "color", "normal", "segment", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask"):
            assert np.array_equal(out[k], base[k][idx]), k
        fx[tag + "_idx"] = idx.astype(np.int64)

    # ---- the head of the shipped list as one run ----
    ops = [T.CenterShift(apply_z=True), T.RandomDropout(dropout_ratio=0.2, dropout_application_ratio=1.0),
           T.RandomRotate(angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
           T.RandomRotate(angle=[-1 / 64, 1 / 64], axis="x", always_apply=True),
           T.RandomRotate(angle=[-1 / 64, 1 / 64], axis="y", always_apply=True),
           T.RandomScale(scale=[0.9, 1.1]), T.RandomFlip(p=0.5), T.RandomJitter(sigma=0.005, clip=0.01)]
    NS = 1000
    sbase = fixture(NS, 22)
    fx["seq_n"], fx["seq_seed"] = np.int64(NS), np.int64(22)

    def sfresh():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sbase.items()}
    s = 120
    while True:                                        # a seed whose RandomFlip mirrors at least one axis
        seed(s)
        random.random()                                                   # dropout fires?
        idx = np.random.choice(NS, int(NS * (1 - 0.2)), replace=False)
        angles = []
        for rng_ in ([-1, 1], [-1 / 64, 1 / 64], [-1 / 64, 1 / 64]):
            random.random()
            angles.append(np.random.uniform(rng_[0], rng_[1]) * np.pi)
        sc = np.random.uniform(0.9, 1.1, 1)
        flips = (bool(np.random.rand() < 0.5), bool(np.random.rand() < 0.5))
        noise = np.random.randn(len(idx), 3)
        if flips[0] and flips[1] and random.random() < 0.95:              # ... and whose ElasticDistortion fires
            break
        s += 1
    seed(s)
    d = sfresh()
    for op in ops:
        d = op(d)
    assert (branch_gap(d["quat"]) < 1e-5).mean() <= 0.005
    fx["seq_idx"], fx["seq_angles"], fx["seq_scale"], fx["seq_flips"] = idx.astype(np.int64), np.array(angles), sc, np.array(flips)
    fx["seq_noise"] = noise.astype(np.float32)
    fx["seq_coord"], fx["seq_quat"], fx["seq_normal"], fx["seq_scale_out"] = d["coord"], d["quat"], d["normal"].astype(np.float32), d["scale"]
    assert len(d["coord"]) == len(idx) and np.array_equal(d["segment"], sbase["segment"][idx])
    assert d["coord"].dtype == np.float64 and d["quat"].dtype == np.float64
    # ElasticDistortion continues on the running stream: per pair the grid it is about to draw (its shape follows from the
    # coordinates that pair sees) is drawn first, the stream is put back, and the reference's own pass runs
    cur = d["coord"].copy()
    ops_el = T.ElasticDistortion(distortion_params=[[0.2, 0.4], [0.8, 1.6]])
    c32 = cur.astype(np.float32)
    for k, (gran, mag) in enumerate(ops_el.distortion_params):
        dim = ((cur - cur.min(0)).max(0) // gran).astype(int) + 3
        dim32 = np.floor_divide(c32.max(0) - c32.min(0), np.float32(gran)).astype(int) + 3
        assert np.array_equal(dim, dim32), "the fp32 coordinates would ask for another grid"
        state = np.random.get_state()
        raw = np.random.randn(*dim, 3).astype(np.float32)
        np.random.set_state(state)
        cur = T.ElasticDistortion.elastic_distortion(cur, gran, mag)
        c32 = elastic_f32(c32, blur2(raw), c32.min(0) - np.float32(gran), gran, mag)
        fx["seq_el_raw%d" % k] = raw
    fx["seq_el_coord"] = cur.copy()
    fx["seq_el_f32_err"] = np.float64(np.abs(c32.astype(np.float64) - cur).max())      # both pairs in fp32, from the rounded input
    assert cur.dtype == np.float64 and fx["seq_el_f32_err"] < 1e-5 and np.abs(cur - d["coord"]).max() > 1e-3
    np.random.rand(); b3 = np.random.rand()                              # the chromatic draws follow on the same stream
    np.random.rand(); t3 = (np.random.rand(1, 3) - 0.5) * 255 * 2 * 0.05
    np.random.rand(); n3 = np.random.randn(len(idx), 3)
    seed(s)
    d = sfresh()
    for op in ops + [ops_el, T.ChromaticAutoContrast(p=1.0), T.ChromaticTranslation(p=1.0, ratio=0.05), T.ChromaticJitter(p=1.0, std=0.05)]:
        d = op(d)
    fx["seq_blend"], fx["seq_tr"], fx["seq_cnoise"], fx["seq_color"] = np.float64(b3), t3[0], n3.astype(np.float32), d["color"]
    assert np.array_equal(d["coord"], fx["seq_el_coord"]), "the op drew other grids than the ones recorded"

    lists, skipped = transform_lists(R)
    first = ("n", "seed", "cs_", "rz_", "rx_", "ry_", "rt_", "sca_", "sh_")
    parts = {"augment.npz": {k: v for k, v in fx.items() if k.startswith(first)},
             "augment_b.npz": {k: v for k, v in fx.items() if not k.startswith(first)}}
    for name, part in parts.items():
        np.savez_compressed(os.path.join(HERE, name), **part)
        assert os.path.getsize(os.path.join(HERE, name)) < (1 << 20), name
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")
    print(len(lists), "transform lists; skipped", skipped, "; elastic fp32 restatement error",
          [float(fx["el%d_f32_err" % k]) for k in range(2)], "sequence", float(fx["seq_el_f32_err"]))

if __name__ == "__main__":
    main()
