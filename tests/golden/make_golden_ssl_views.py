"""Golden vectors of the self-supervised view transforms from the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ssl_views.py

The recipe of make_golden_augment.py: pointcept/datasets/transform.py is imported through the stub loader; `random`, `np.random`
AND torch are seeded (RandomColorJitter.get_params calls torch.randperm); what a transform will draw is drawn once in advance, the
generators are put back and the transform runs.  Data only, no reference source:

  ssl_views.npz      colour chain (n = 600: tests/ssl_cases.colors): every step alone, contrast first / last, all four steps fired in
                     three drawn orders (one with contrast behind hue), jitter + grayscale.  Per case the (code, factor) steps, the
                     reference's fp32 output `_ref` and `_f64`, the same formulas in fp64 (ssl_cases.chain64) on the same draws.
                     blur (ssl_cases.BLUR_CASES): the reference's output per blurred key `_ref_<key>` and `_f64_<key>` (ssl_cases.blur64).
                     SphereCropRandomMaxPoints on fixture(2000, 31) + `sh` / `lang_feat_64`: the drawn point_max, centre and the crop's
                     row index (every cropped key is checked against it here).
                     The reference's timings of the ops profiles/ssl_views.md quotes (`time_*`, seconds, this container's CPU), one
                     full generator call on 800,000 Gaussians among them.
  ssl_views_b.npz    one ContrastiveViewsGenerator_SSL call (the scannet ssl-pretrain list's generator with point_max 1500 and a 0.1 m
                     grid, on fixture(2000, 33)): the draws of every sub-list run as `gen_<run>_*` (GridSample's kept rows read off
                     the op's own output) and the output dict `out_<key>`.
  ssl_configs.txt    the evaluated `data.train.transform` lists of the three ssl-pretrain configs, as literals.
"""
import ast
import glob
import importlib
import os
import pprint
import random
import sys
import textwrap
import time

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
R = "/root/reference/"
NC = 600

import ssl_cases as sc  # noqa: E402
from make_golden_augment import branch_gap, fixture  # noqa: E402

assert all(np.array_equal(v, sc.fixture(50, 3)[k]) for k, v in fixture(50, 3).items())      # the tests rebuild the fixture from ssl_cases


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def get_state():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def set_state(st):
    random.setstate(st[0])
    np.random.set_state(st[1])
    torch.set_rng_state(st[2])


def jitter_draws(op):
    """what RandomColorJitter.__call__ is about to draw -> the params dict of the device transform (the streams are put back)"""
    st = get_state()
    order = torch.randperm(4).tolist()
    fac = [None if r is None else float(np.random.uniform(r[0], r[1])) for r in (op.brightness, op.contrast, op.saturation, op.hue)]
    for i in order:
        if fac[i] is not None and not np.random.rand() < op.p:
            fac[i] = None
    set_state(st)
    return dict(order=order, **dict(zip(sc.NAMES, fac)))


def kept_rows(before, after):
    """the input row of every output row of GridSample, from the op's own output: coordinates are distinct, so a row is its key"""
    rows = {c.tobytes(): i for i, c in enumerate(np.ascontiguousarray(before))}
    assert len(rows) == len(before), "two Gaussians share a coordinate"
    return np.array([rows[c.tobytes()] for c in np.ascontiguousarray(after)], dtype=np.int64)


def crop_draws(op, n):
    st = get_state()
    pm = int(np.random.uniform(op.random_scale[0], op.random_scale[1]) * op.point_max)
    ci = int(np.random.randint(n))
    set_state(st)
    return pm, ci


def distance_gaps_ok(coord, ci, pm):
    """the crop keeps rows in distance order: no two of the distances it sorts may be closer than 4 ulp (argsort is not stable, and
    the device sums the squares in another order)"""
    d = np.sort(np.sum(np.square(coord.astype(np.float64) - coord[ci].astype(np.float64)), 1))
    k = min(pm + 1, len(d))
    return bool((np.diff(d[:k]) > 4 * np.spacing(d[1:k].astype(np.float32)).astype(np.float64)).all())


def run_list(ops, d, tag, fx):
    """one sub-list of the generator, op by op: record what each op draws, then let the reference's op run"""
    for j, op in enumerate(ops):
        name, key = type(op).__name__, "gen_%s_%d_" % (tag, j)
        if name == "RandomFlip":
            st = get_state()
            fx[key + "flip"] = np.array([np.random.rand() < op.p, np.random.rand() < op.p])
            set_state(st)
        elif name == "SphereCropRandomMaxPoints":
            pm, ci = crop_draws(op, len(d["coord"]))
            assert distance_gaps_ok(d["coord"], ci, pm), "near tie in the crop's distances"
            fx[key + "point_max"], fx[key + "center_index"] = np.int64(pm), np.int64(ci)
        elif name == "RandomColorJitter":
            p = jitter_draws(op)
            fx[key + "order"] = np.array(p["order"])
            fx[key + "factors"] = np.array([np.nan if p[k] is None else p[k] for k in sc.NAMES])
        elif name in ("RandomColorGrayScale", "RandomColorSolarize"):
            st = get_state()
            fx[key + "fired"] = np.bool_(np.random.rand() < op.p)
            set_state(st)
        elif name == "GridSample":
            before = d["coord"].copy()
            g64, g32 = np.floor(before / np.array(op.grid_size)), np.floor(before / np.float32(op.grid_size))
            assert np.array_equal(g64, g32), "a coordinate sits on a cell border: fp32 and fp64 voxelise it differently"
        elif name == "GSGaussianBlurVoxelOpc":
            st = get_state()
            fired = np.random.rand() < op.p
            fx[key + "fired"] = np.bool_(fired)
            fx[key + "sigma"] = np.float64(np.random.uniform(op.sigma[0], op.sigma[1]) if fired else np.nan)
            set_state(st)
        else:
            assert name in ("CenterShift", "NormalizeColor", "ToTensor"), name
        if name == "RandomFlip" and fx[key + "flip"].any():
            assert (branch_gap(d["quat"]) > 1e-5).all(), "near tie of scipy's sign rule in the fixture"
        d = op(d)
        if name == "GridSample":
            fx[key + "idx"] = kept_rows(before, d["coord"])
    return d


def transform_lists(ref):
    import make_golden_configs as mc
    out = {}
    for p in sorted(glob.glob(ref + "configs/*/ssl-pretrain-*.py")):
        rel = os.path.relpath(p, ref)
        cfg = mc.load_config(ref, rel)

        def walk(d, tag):
            if "transform" in d:
                out[tag] = d["transform"]
            for i, sub in enumerate(d.get("datasets", [])):
                walk(sub, "%s::datasets[%d]" % (rel, i))
        walk(cfg["data"]["train"], rel)
    txt = "{\n" + "".join("%r:\n%s,\n" % (k, textwrap.indent(pprint.pformat(v, width=116, sort_dicts=False), "    "))
                          for k, v in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(os.path.join(HERE, "ssl_configs.txt"), "w") as f:
        f.write(txt + "\n")
    return out


def main():
    import make_golden as mg
    mg.stubpkg("pointcept", R + "pointcept")
    mg.stubpkg("pointcept.utils", R + "pointcept/utils")
    mg.stubpkg("pointcept.datasets", R + "pointcept/datasets")
    T = importlib.import_module("pointcept.datasets.transform")
    fx, fb = {"cc_n": np.int64(NC), "cc_seed": np.int64(41)}, {}
    base_color = sc.colors(NC, 41)

    # ---- colour chain -------------------------------------------------------------------------------------------------------------
    def record(tag, steps, ref):
        assert ref.dtype == np.float32
        fx["cc_%s_codes" % tag] = np.array([c for c, _ in steps], dtype=np.int64)
        fx["cc_%s_factors" % tag] = np.array([f for _, f in steps], dtype=np.float64)
        fx["cc_%s_ref" % tag] = ref
        fx["cc_%s_f64" % tag] = sc.chain64(base_color, steps)
        err = np.abs(ref.astype(np.float64) - fx["cc_%s_f64" % tag]).max()
        assert err < 1e-3, (tag, err)
        return err

    worst = {}
    # each step alone: only that range is set and p = 1, so the op draws the permutation, one factor and one coin
    for k, (name, rng_) in enumerate(zip(sc.NAMES, ([1.4, 1.4], [0.6, 1.4], [0.8, 1.2], [-0.1, 0.1]))):
        op = T.RandomColorJitter(**{name: rng_}, p=1.0)
        seed(200 + k)
        p = jitter_draws(op)
        out = op(dict(color=base_color.copy()))["color"]
        worst[name] = record(name, sc.steps_of(p), out)
    assert (fx["cc_brightness_ref"] == 255).any() and (fx["cc_brightness_ref"] == 0).any()
    seed(210)
    out = T.RandomColorGrayScale(p=1.0)(dict(color=base_color.copy()))["color"]
    worst["gray"] = record("gray", [(sc.GRAY, 0.0)], np.ascontiguousarray(out))
    # all four fired (p = 0.8 as shipped): three drawn orders -- contrast first, contrast last, contrast right behind hue
    want = {"cfirst": lambda o: o[0] == 1, "clast": lambda o: o[3] == 1, "chue": lambda o: o.index(1) == o.index(3) + 1 and o[0] != 1 and o[3] != 1}
    op = T.RandomColorJitter(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p=0.8)
    s = 220
    while want:
        seed(s)
        p = jitter_draws(op)
        for tag, cond in list(want.items()):
            if all(p[k] is not None for k in sc.NAMES) and cond(p["order"]):
                out = op(dict(color=base_color.copy()))["color"]
                worst[tag] = record(tag, sc.steps_of(p), out)
                fx["cc_%s_order" % tag] = np.array(p["order"])
                del want[tag]
                break
        s += 1
    # jitter then grayscale, as the shipped view lists have them
    seed(s)
    while True:
        seed(s)
        p = jitter_draws(op)
        if sum(p[k] is not None for k in sc.NAMES) >= 3 and p["contrast"] is not None:
            break
        s += 1
    d = T.RandomColorGrayScale(p=1.0)(op(dict(color=base_color.copy())))
    worst["jgray"] = record("jgray", sc.steps_of(p, gray=True), np.ascontiguousarray(d["color"]))
    fx["cc_jgray_order"] = np.array(p["order"])
    fx["cc_jgray_jfactors"] = np.array([np.nan if p[k] is None else p[k] for k in sc.NAMES])

    # ---- blur ---------------------------------------------------------------------------------------------------------------------
    for tag, (size, sigma, occ, origin, rule, extra) in sc.BLUR_CASES.items():
        d = sc.blur_input(tag)
        assert len(np.unique(d["grid_coord"], axis=0)) == len(d["grid_coord"])
        seed(400)
        out = T.GSGaussianBlurVoxelOpc(p=1.0, sigma=[sigma, sigma, 0], extra_keys=extra)({k: v.copy() for k, v in d.items()})
        f64 = sc.blur64(d, sigma, extra)
        for k in ("color",) + tuple(extra):
            assert out[k].dtype == np.float32 and out[k].shape == d[k].shape, (tag, k, out[k].dtype)
            fx["blur_%s_ref_%s" % (tag, k)], fx["blur_%s_f64_%s" % (tag, k)] = out[k], f64[k]
            err = np.abs(out[k].astype(np.float64) - f64[k]).max()
            worst["blur_%s_%s" % (tag, k)] = err
            assert err < (1e-3 if k == "color" else 1e-5), (tag, k, err)
        fx["blur_%s_n" % tag], fx["blur_%s_masked" % tag] = np.int64(len(d["color"])), np.int64((d["opacity"] > 0.5).sum())

    # ---- SphereCropRandomMaxPoints ------------------------------------------------------------------------------------------------
    N = 2000
    base = sc.crop_fixture(N, 31)
    op = T.SphereCropRandomMaxPoints(random_scale=(0.4, 1.0), point_max=1500)
    s = 500
    while True:
        seed(s)
        pm, ci = crop_draws(op, N)
        if pm < N and distance_gaps_ok(base["coord"], ci, pm):
            break
        s += 1
    out = op({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()})
    idx = np.argsort(np.sum(np.square(base["coord"] - base["coord"][ci]), 1), kind="stable")[:pm]
    for k in ("coord", "grid_coord", "color", "quat", "scale", "opacity", "sh", "normal", "lang_feat", "lang_feat_64", "valid_feat_mask",
              "segment"):
        assert np.array_equal(out[k], base[k][idx]), k
    fx["crop_n"], fx["crop_seed"], fx["crop_point_max"], fx["crop_center_index"], fx["crop_idx"] = \
        np.int64(N), np.int64(31), np.int64(pm), np.int64(ci), idx.astype(np.int64)

    # ---- one full generator call --------------------------------------------------------------------------------------------------
    lists = transform_lists(R)
    gcfg = [c for c in lists["configs/scannet/ssl-pretrain-scannet-all-base.py"] if c["type"] == "ContrastiveViewsGenerator_SSL"][0]
    gcfg = ast.literal_eval(repr(gcfg))

    def shrink(cfgs):
        for c in cfgs:
            if c["type"] == "SphereCropRandomMaxPoints":
                c["point_max"] = 1500
            if c["type"] == "GridSample":
                c["grid_size"] = 0.1
            if c["type"] == "GSGaussianBlurVoxelOpc":
                c["p"] = 1.0 if c["p"] == 1.0 else 0.7
    for k in ("global_base_transform", "local_base_transform", "global_transform0", "global_transform1", "local_transform"):
        shrink(gcfg[k])
    fb["gen_cfg"] = np.array(repr(gcfg))
    NG = 2000
    gbase = fixture(NG, 33)
    fb["gen_n"], fb["gen_seed"] = np.int64(NG), np.int64(33)
    keys = gcfg["view_keys"]

    def gfresh():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in gbase.items()}
    s = 600
    while True:
        gen = T.TRANSFORMS.build(ast.literal_eval(repr(gcfg)))
        seed(s)
        rec = {}
        try:
            d = gfresh()
            gb = run_list(gen.global_base_transform.transforms, {k: d[k].copy() for k in keys}, "global_base", rec)
            g0 = run_list(gen.global_transform0.transforms, {k: gb[k].copy() for k in keys}, "global0", rec)
            g1 = run_list(gen.global_transform1.transforms, {k: gb[k].copy() for k in keys}, "global1", rec)
            lb = run_list(gen.local_base_transform.transforms, {k: d[k].copy() for k in keys}, "local_base", rec)
            loc = [run_list(gen.local_transform.transforms, {k: lb[k].copy() for k in keys}, "local%d" % i, rec)
                   for i in range(gen.local_crop_num)]
            blurred = sum(bool(v) for k, v in rec.items() if k.endswith("fired") and (k[:-5] + "sigma") in rec)
            flipped = any(v.any() for k, v in rec.items() if k.endswith("flip"))
            if blurred >= 3 and flipped:
                break
        except AssertionError as err:
            print("seed", s, "skipped:", err)
        s += 1
    seed(s)
    out = gen(gfresh())
    stepped = dict(global_crop0=g0, global_crop1=g1, **{"local_crop%d" % i: v for i, v in enumerate(loc)})
    for pre, dd in stepped.items():
        for k, v in dd.items():
            assert np.array_equal(np.asarray(out[pre + "_" + k]), np.asarray(v)), (pre, k)
    fb.update(rec)
    new_keys = sorted(k for k in out if k not in gbase)
    fb["gen_out_keys"] = np.array(new_keys)
    for k in new_keys:
        v = np.asarray(out[k])
        fb["out_" + k] = v.astype(np.int32) if v.dtype.kind == "i" else v.astype(np.float32) if k.endswith(("color", "opacity", "scale", "coord")) else v
    for k in gbase:
        assert out[k] is not None and (not isinstance(gbase[k], np.ndarray) or np.array_equal(out[k], gbase[k])), k

    # ---- what the reference's ops cost on this CPU (profiles/ssl_views.md) ----------------------------------------------------------
    big = (np.random.RandomState(7).rand(300000, 3) * 255).astype(np.float32)
    op = T.RandomColorJitter(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p=1.0)
    t = []
    for rep in range(3):
        seed(700 + rep)
        t0 = time.perf_counter()
        op(dict(color=big.copy()))
        t.append(time.perf_counter() - t0)
    fx["time_jitter_300k"] = np.float64(min(t))
    # 300 k occupied voxels of a 2 cm grid over a room-like shell (the walls, floor and ceiling of a 6 x 5 x 2.6 m box, two cells thick)
    gsz = np.array([300, 250, 130])
    gg = np.random.RandomState(8)
    pts = np.zeros((0, 3), dtype=np.int64)
    while len(pts) < 300000:
        p = (gg.rand(200000, 3) * gsz).astype(np.int64)
        ax = gg.randint(0, 3, len(p))
        p[np.arange(len(p)), ax] = np.where(gg.rand(len(p)) < 0.5, gg.randint(0, 2, len(p)), gsz[ax] - 1 - gg.randint(0, 2, len(p)))
        pts = np.unique(np.concatenate([pts, p]), axis=0)
    pts = pts[gg.permutation(len(pts))[:300000]]
    nb = len(pts)
    bd = dict(coord=pts.astype(np.float32), grid_coord=pts, color=(gg.rand(nb, 3) * 255).astype(np.float32),
              opacity=gg.rand(nb, 1).astype(np.float32), scale=gg.rand(nb, 3).astype(np.float32), quat=gg.randn(nb, 4).astype(np.float32))
    fx["time_blur_n"] = np.int64(nb)
    fx["time_blur_grid"] = gsz
    for sg in (0.5, 1.0, 2.0):
        seed(710)
        t0 = time.perf_counter()
        T.GSGaussianBlurVoxelOpc(p=1.0, sigma=[sg, sg, 0], extra_keys=("scale", "quat", "opacity"))({k: v.copy() for k, v in bd.items()})
        fx["time_blur_sigma_%s" % sg] = np.float64(time.perf_counter() - t0)

    # one call of the scannet list's generator as shipped, 800 k Gaussians on the surfaces of an 8 x 6 x 3 m room (4 cm thick): the
    # sample scripts/bench_ssl_views.py builds on the device, drawn here with numpy
    ng = 800000
    box = np.array([8.0, 6.0, 3.0])
    coord = gg.rand(ng, 3) * box
    ax = gg.randint(0, 3, ng)
    depth = gg.rand(ng) * 0.04
    coord[np.arange(ng), ax] = np.where(gg.rand(ng) < 0.5, depth, box[ax] - depth)
    big = dict(coord=coord.astype(np.float32), color=(gg.rand(ng, 3) * 255).astype(np.float32), opacity=gg.rand(ng, 1).astype(np.float32),
               quat=gg.randn(ng, 4).astype(np.float32), scale=(gg.rand(ng, 3) * 0.05).astype(np.float32))
    shipped = [c for c in lists["configs/scannet/ssl-pretrain-scannet-all-base.py"] if c["type"] == "ContrastiveViewsGenerator_SSL"][0]
    gen = T.TRANSFORMS.build(ast.literal_eval(repr(shipped)))
    seed(720)
    t0 = time.perf_counter()
    out = gen(big)
    fx["time_generator_800k"] = np.float64(time.perf_counter() - t0)
    fx["time_generator_800k_rows"] = np.array([len(out["%s_coord" % v]) for v in ("global_crop0", "global_crop1", "local_crop0", "local_crop1",
                                                                                 "local_crop2")])
    del out, big

    for name, part in (("ssl_views.npz", fx), ("ssl_views_b.npz", fb)):
        np.savez_compressed(os.path.join(HERE, name), **part)
        assert os.path.getsize(os.path.join(HERE, name)) < (1 << 20), name
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")
    print("seed of the generator run", s, "; max |reference fp32 - fp64| per case:")
    for k, v in worst.items():
        print("  %-24s %.3g" % (k, v))
    print({k: np.asarray(v).tolist() for k, v in fx.items() if k.startswith("time_")})


if __name__ == "__main__":
    main()
