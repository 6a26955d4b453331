"""Golden vectors of the transforms on a sample that carries a point cloud beside its Gaussians (`pc_coord` / `pc_segment`),
from the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pc.py

Same recipe as make_golden_augment.py, and the same seeds: every op draws what it drew there, which is asserted (the Gaussians'
outputs must equal the ones augment.npz / augment_b.npz hold), so tests/golden/augment_pc.npz only adds the cloud's side (data
only; no reference source):

  cloud     pc_coord (m = 1000, fp32, in the box of the n = 2000 fixture) and pc_segment in [-1, 6), with four planted cells at the
            cloud grid size `gp_grid`: all members -1 | lowest row -1 and a later one labelled | 100 members of which the first 70
            are -1 (a run longer than a wave) | single-member cells (they occur by themselves; asserted)
  per op    `<tag>_pc`: pc_coord after CenterShift (cs_z, cs_xy), RandomRotate (rz, rx, ry), RandomRotateTargetAngle (rt),
            RandomScale (sca), RandomFlip (fx, fy, fxy); RandomShift and RandomJitter leave it bit for bit (asserted here)
  sequence  `seq_pc`: the cloud after the recorded head of the shipped list (the n = 1000 sample of augment_b.npz + the cloud)
  gp_*      GridSample(apply_to_pc=True): the rows it keeps of the cloud with and without pc_segment (recovered from the
            coordinates it returns: the cloud has no duplicate point)
  gsi_*     GridSample with `sampled_index` on the Gaussians: the per-voxel pick it drew, the merged idx_unique, the remapped
            sampled_index and grid_coord

Conditions asserted here (the seed of the cloud advances until they hold): no FNV collision on the cloud's grid; every scaled
cloud coordinate is at least 2^-10 of a cell away from an integer and below 2^9, so an fp32 floor and the reference's fp64 floor
agree.  The Gaussians of gsi_* are the fixed fixture: their grid size is a power of two (the fp32 quotient is exact), and the
equality of the two floors and the absence of an FNV collision are asserted directly.

tests/golden/pc_configs.txt: every `val` / `test` transform list (and `test_cfg.post_transform` list) of the shipped
lang-pretrain configs whose dataset collects `pc_coord`, as literals.
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
N, M = 2000, 1000
GP_GRID = 0.25            # the cloud's grid: 16 x 12 x 6 cells for 1000 points, so empty, single and shared cells all occur
GSI_GRID = 0.25
PLANT_ALL_IGNORED, PLANT_LATE_LABEL, PLANT_LONG = (10, 2, 1), (7, 7, 2), (3, 3, 3)


def cloud(seed):
    """(pc_coord (M, 3) f32, pc_segment (M,) i64) in the box of make_golden_augment.fixture, with the planted cells"""
    g = np.random.RandomState(seed)
    pc = (g.rand(M, 3) * np.array([4.0, 3.0, 1.5])).astype(np.float32)
    seg = g.randint(-1, 6, M).astype(np.int64)

    def put(rows, cell):
        pc[rows] = ((np.array(cell) + 0.1 + 0.8 * g.rand(len(rows), 3)) * GP_GRID).astype(np.float32)
    long_rows = np.arange(5, 1000, 10)                      # 100 rows spread over the whole array
    put(long_rows, PLANT_LONG)
    put(np.array([17, 333, 801]), PLANT_ALL_IGNORED)
    put(np.array([42, 444, 902]), PLANT_LATE_LABEL)
    cells = np.floor(pc.astype(np.float64) / GP_GRID).astype(int)
    for cell, kind in ((PLANT_LONG, "long"), (PLANT_ALL_IGNORED, "all"), (PLANT_LATE_LABEL, "late")):
        rows = np.nonzero((cells == np.array(cell)).all(1))[0]           # the planted rows and whoever else fell into the cell
        if kind == "all":
            seg[rows] = -1
        elif kind == "late":
            seg[rows] = -1
            seg[rows[-1]] = 4
        else:
            seg[rows[:70]] = -1
            seg[rows[70:]] = g.randint(0, 6, len(rows) - 70)
    return pc, seg


def grid_ok(T, x, grid):
    """the fixture conditions for x / grid: no FNV collision, floor is safe in fp32"""
    s = x.astype(np.float64) / grid
    if np.abs(s).max() >= 2.0 ** 9 or np.abs(s - np.round(s)).min() < 2.0 ** -10:
        return False
    gc = np.floor(s).astype(int)
    gc -= gc.min(0)
    return len(np.unique(T.GridSample.fnv_hash_vec(gc))) == len(np.unique(gc, axis=0))


def rows_of(sub, full):
    """indices i with full[i] == sub[k], for a `full` without duplicate rows"""
    table = {r.tobytes(): i for i, r in enumerate(full)}
    assert len(table) == len(full), "duplicate points in the cloud"
    return np.array([table[r.tobytes()] for r in sub], dtype=np.int64)


def pc_lists(ref):
    """{config::val | config::test[i]::transform | config::test[i]::post_transform: list} of the datasets that collect pc_coord"""
    import make_golden_configs as mc
    out, skipped = {}, []
    for p in sorted(glob.glob(ref + "configs/*/lang-pretrain-*.py")):
        rel = os.path.relpath(p, ref)
        try:
            cfg = mc.load_config(ref, rel)
        except NameError as err:                     # one shipped concat config names an undefined data root: not loadable as shipped
            skipped.append((rel, str(err)))
            continue
        for split in ("val", "test"):
            part = cfg["data"].get(split)
            if part is None:
                continue
            many = isinstance(part, (list, tuple))
            for i, d in enumerate(part if many else [part]):
                tag = "%s::%s" % (rel, split) + ("[%d]" % i if many else "")
                post = (d.get("test_cfg") or {}).get("post_transform")
                if "pc_coord" not in repr(d["transform"]) and "pc_coord" not in repr(post):
                    continue
                out[tag + "::transform"] = d["transform"]
                if post is not None:
                    out[tag + "::post_transform"] = post
    txt = "{\n" + "".join("%r:\n%s,\n" % (k, textwrap.indent(pprint.pformat(v, width=116, sort_dicts=False), "    "))
                          for k, v in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(os.path.join(HERE, "pc_configs.txt"), "w") as f:
        f.write(txt + "\n")
    return out, skipped


def main():
    import make_golden as mg
    from make_golden_augment import fixture
    mg.stubpkg("pointcept", R + "pointcept")
    mg.stubpkg("pointcept.utils", R + "pointcept/utils")
    mg.stubpkg("pointcept.datasets", R + "pointcept/datasets")
    T = importlib.import_module("pointcept.datasets.transform")
    old = {**np.load(os.path.join(HERE, "augment.npz")), **np.load(os.path.join(HERE, "augment_b.npz"))}
    assert int(old["n"]) == N and int(old["seed"]) == 21
    base = fixture(N, 21)

    # ---- the cloud: advance the seed until the fixture conditions hold ----
    cseed = 300
    while True:
        pc, seg = cloud(cseed)
        if grid_ok(T, pc, GP_GRID) and len(np.unique(pc, axis=0)) == M:
            break
        cseed += 1
    cells = np.floor(pc.astype(np.float64) / GP_GRID).astype(int)
    _, inv, cnt = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert (cnt == 1).sum() >= 50 and cnt.max() >= 100
    fx = {"pc_seed": np.int64(cseed), "pc_coord": pc, "pc_segment": seg, "gp_grid": np.float64(GP_GRID),
          "gp_plant_cells": np.array([PLANT_ALL_IGNORED, PLANT_LATE_LABEL, PLANT_LONG])}
    base["pc_coord"], base["pc_segment"] = pc, seg

    def fresh():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}

    def seed(s):
        random.seed(s)
        np.random.seed(s)

    def same(out, tag, keys):
        for k in keys:
            assert np.array_equal(out[k], old[tag + "_" + k]), (tag, k, "the op drew other numbers than in augment.npz")

    # ---- CenterShift ----
    for tag, z in (("cs_z", True), ("cs_xy", False)):
        out = T.CenterShift(apply_z=z)(fresh())
        same(out, tag, ["coord"])
        fx[tag + "_pc"] = out["pc_coord"]
        assert out["pc_coord"].dtype == np.float32                       # the reference shifts the cloud in fp32

    # ---- rotations (the seeds of make_golden_augment.py) ----
    for tag, kw in (("rz", dict(angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5)),
                    ("rx", dict(angle=[-1 / 64, 1 / 64], axis="x", p=0.5)),
                    ("ry", dict(angle=[-1 / 64, 1 / 64], axis="y", p=0.5))):
        s = 30
        while True:
            seed(s)
            if not random.random() > kw["p"]:
                break
            s += 1
        seed(s)
        out = T.RandomRotate(**kw)(fresh())
        same(out, tag, ["coord", "quat", "normal"])
        fx[tag + "_pc"] = out["pc_coord"]
    s = 40
    while True:
        seed(s)
        if not random.random() > 0.75:
            break
        s += 1
    seed(s)
    out = T.RandomRotateTargetAngle(angle=(1 / 2, 1, 3 / 2), center=[0, 0, 0], axis="z", p=0.75)(fresh())
    same(out, "rt", ["coord", "quat", "normal"])
    fx["rt_pc"] = out["pc_coord"]

    # ---- RandomScale; RandomShift leaves the cloud alone ----
    seed(50)
    out = T.RandomScale(scale=[0.9, 1.1], anisotropic=True)(fresh())
    same(out, "sca", ["coord", "scale"])
    fx["sca_pc"] = out["pc_coord"]
    seed(51)
    out = T.RandomShift(shift=((-0.2, 0.2), (-0.2, 0.2), (-0.1, 0.1)))(fresh())
    same(out, "sh", ["coord"])
    assert np.array_equal(out["pc_coord"], pc)

    # ---- RandomFlip ----
    want = {(True, False): "fx", (False, True): "fy", (True, True): "fxy"}
    s = 60
    while want:
        seed(s)
        got = (bool(np.random.rand() < 0.5), bool(np.random.rand() < 0.5))
        if got in want:
            tag = want.pop(got)
            seed(s)
            out = T.RandomFlip(p=0.5)(fresh())
            same(out, tag, ["quat"] + (["coord", "normal"] if tag == "fxy" else []))
            fx[tag + "_pc"] = out["pc_coord"]
        s += 1

    # ---- RandomJitter leaves the cloud alone ----
    seed(70)
    out = T.RandomJitter(sigma=0.005, clip=0.01)(fresh())
    same(out, "jit", ["coord"])
    assert np.array_equal(out["pc_coord"], pc)

    # ---- the head of the shipped list with the cloud ----
    ops = [T.CenterShift(apply_z=True), T.RandomDropout(dropout_ratio=0.2, dropout_application_ratio=1.0),
           T.RandomRotate(angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
           T.RandomRotate(angle=[-1 / 64, 1 / 64], axis="x", always_apply=True),
           T.RandomRotate(angle=[-1 / 64, 1 / 64], axis="y", always_apply=True),
           T.RandomScale(scale=[0.9, 1.1]), T.RandomFlip(p=0.5), T.RandomJitter(sigma=0.005, clip=0.01)]
    NS = int(old["seq_n"])
    sbase = fixture(NS, int(old["seq_seed"]))
    sbase["pc_coord"], sbase["pc_segment"] = pc, seg
    s = 120
    while True:                                        # the seed make_golden_augment.py settled on: its recorded draws come back
        seed(s)
        random.random()
        idx = np.random.choice(NS, int(NS * (1 - 0.2)), replace=False)
        if np.array_equal(idx, old["seq_idx"]):
            break
        s += 1
        assert s < 1000
    seed(s)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sbase.items()}
    for op in ops:
        d = op(d)
    assert np.array_equal(d["coord"], old["seq_coord"]) and np.array_equal(d["quat"], old["seq_quat"])
    assert np.array_equal(d["pc_segment"], seg) and len(d["pc_coord"]) == M
    fx["seq_pc"] = d["pc_coord"]

    # ---- GridSample(apply_to_pc=True): the rows of the cloud it keeps ----
    keys = ("coord", "color", "opacity", "quat", "scale", "segment", "lang_feat", "valid_feat_mask")
    for tag, with_seg in (("gp_chosen", True), ("gp_chosen_noseg", False)):
        d = fresh()
        if not with_seg:
            del d["pc_segment"]
        seed(200)
        out = T.GridSample(grid_size=GP_GRID, hash_type="fnv", mode="train", keys=keys, apply_to_pc=True)(d)
        chosen = rows_of(out["pc_coord"], pc)
        assert len(chosen) == len(cnt) and len(np.unique(inv[chosen])) == len(cnt)          # one row per occupied cell
        if with_seg:
            assert np.array_equal(out["pc_segment"], seg[chosen])
        fx[tag] = chosen
    # the planted cells resolve as planned
    by_cell = {tuple(c): r for c, r in zip(map(tuple, cells[fx["gp_chosen"]]), fx["gp_chosen"])}
    rows = lambda cell: np.nonzero((cells == np.array(cell)).all(1))[0]
    assert by_cell[PLANT_ALL_IGNORED] == rows(PLANT_ALL_IGNORED)[0] and (seg[rows(PLANT_ALL_IGNORED)] == -1).all()
    late = rows(PLANT_LATE_LABEL)
    assert seg[late[0]] == -1 and by_cell[PLANT_LATE_LABEL] == late[-1] and len(late) >= 3
    lng = rows(PLANT_LONG)
    assert len(lng) >= 100 and by_cell[PLANT_LONG] == lng[70] and (seg[lng[:70]] == -1).all()
    assert (fx["gp_chosen"] != fx["gp_chosen_noseg"]).sum() >= 3
    d = fresh()
    out = T.GridSample(grid_size=GP_GRID, keys=keys, apply_to_pc=False)(d)
    assert out["pc_coord"] is base["pc_coord"] or np.array_equal(out["pc_coord"], pc)

    # ---- GridSample with sampled_index on the Gaussians ----
    # (the Gaussians are the fixed fixture, so no seed can be advanced: the grid size is a power of two, which makes the fp32
    # quotient exact, and the two things that matter are asserted directly)
    si = np.sort(np.random.RandomState(6).choice(N, 60, replace=False))
    gc = np.floor(base["coord"] / np.array(GSI_GRID)).astype(int)
    assert np.array_equal(gc, np.floor(base["coord"] / np.float32(GSI_GRID)).astype(int)) and base["coord"].dtype == np.float32
    gc -= gc.min(0)
    key = T.GridSample.fnv_hash_vec(gc)
    assert len(np.unique(key)) == len(np.unique(gc, axis=0))
    idx_sort = np.argsort(key)
    _, _, count = np.unique(key[idx_sort], return_inverse=True, return_counts=True)
    seed(210)
    pick = idx_sort[np.cumsum(np.insert(count, 0, 0)[0:-1]) + np.random.randint(0, count.max(), count.size) % count]
    seed(210)
    d = fresh()
    del d["pc_coord"], d["pc_segment"]
    d["sampled_index"] = si.copy()
    out = T.GridSample(grid_size=GSI_GRID, hash_type="fnv", mode="train", keys=keys, return_grid_coord=True)(d)
    merged = np.unique(np.append(pick, si))
    assert np.array_equal(out["coord"], base["coord"][merged]) and np.array_equal(out["segment"], base["segment"][merged])
    assert len(merged) > len(pick) and np.array_equal(merged[out["sampled_index"]], si)
    fx["gsi_grid"], fx["gsi_sampled_in"], fx["gsi_pick"] = np.float64(GSI_GRID), si.astype(np.int64), pick.astype(np.int64)
    fx["gsi_idx_unique"], fx["gsi_sampled_out"] = merged.astype(np.int64), out["sampled_index"].astype(np.int64)
    fx["gsi_grid_coord"] = out["grid_coord"].astype(np.int32)

    lists, skipped = pc_lists(R)
    path = os.path.join(HERE, "augment_pc.npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < (1 << 20)
    print("augment_pc.npz", os.path.getsize(path) // 1024, "KiB; cloud seed", cseed, "; cells", len(cnt), "; single-member", int((cnt == 1).sum()),
          "; longest", int(cnt.max()), ";", len(lists), "lists; skipped", skipped)


if __name__ == "__main__":
    main()
