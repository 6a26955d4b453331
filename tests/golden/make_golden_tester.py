"""Generator of tests/golden/tester.npz and tests/golden/tester_configs.txt: the open-vocabulary test stage against the
reference's OWN helper functions.

    python tests/golden/make_golden_tester.py <path of the reference tree>

tester.npz: two small scenes (inputs drawn here from the recorded seeds) and the recorded OUTPUTS of the reference's
`neighbor_voting`, `clustering_voting` and `intersection_and_union` (pointcept/utils/misc.py, loaded by file path; numba is
replaced by a stand-in whose `njit` returns the function unchanged, so the voting loop runs as plain Python) on the chain of
engines/test.py:372-510: top-k / threshold -> pred[inverse] -> pred_label_mapping -> neighbour voting -> per-instance voting ->
counts.  Only data is written; no reference source.

A scene: n Gaussians (`origin_*`), a grid-sampled subset of n_grid points reached through `inverse`, and per grid point three
distinct classes (a, b, c) from which the test builds features whose ranks are unambiguous.  Fragment 0 holds every grid point,
fragment 1 about half of them; with the threshold between one and two fragments' worth of probability, the points seen once fall
to ignore_index in the arg-max form.

One condition is asserted (and the seed advanced until it holds): for every query the relative gap between the k-th and the
(k+1)-th neighbour distance is >= 1e-5, two orders above fp32 rounding of a squared distance on unit-box coordinates, so an exact
kNN in fp32 and cKDTree in fp64 choose the same neighbours and the comparison can be exact.

tester_configs.txt: the `test` and `data["test"]` dicts of the two shipped configs tests/test_reference_configs.py uses, evaluated
as literals by make_golden_configs.load_config (plain assignments, a handful of builtins, nothing imported)."""
import ast
import importlib.util
import os
import pprint
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tester.npz")
OUT_CFG = os.path.join(HERE, "tester_configs.txt")
VOTE_K = 5
IGNORE = -1
THRESHOLD = 1.0
SCENES = [dict(n=600, classes=6, seed=1, pc=0, mapping={4: 1, 5: 2}),
          dict(n=257, classes=12, seed=2, pc=150, mapping={7: 3, 3: 9, 40: 0})]      # chained, and a key outside the domain
INSTANCE_IDS = np.array([-1, 3, 7, 20, 41, 1000])


def load_misc(ref):
    numba = types.ModuleType("numba")
    numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    numba.prange = range
    sys.modules["numba"] = numba
    spec = importlib.util.spec_from_file_location("ref_misc", os.path.join(ref, "pointcept", "utils", "misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw_scene(n, classes, seed, pc):
    """the scene's inputs from its seed (the test reads them from the file; the seed is recorded for the record)"""
    g = np.random.RandomState(seed)
    n_grid = (2 * n) // 3
    d = dict(origin_coord=g.rand(n, 3).astype(np.float32), origin_feat_mask=g.rand(n) < 0.9,
             origin_instance=INSTANCE_IDS[g.randint(0, len(INSTANCE_IDS), n)].astype(np.int64),
             origin_segment=g.randint(-1, classes, n).astype(np.int64))
    inverse = np.concatenate([g.permutation(n_grid), g.randint(0, n_grid, n - n_grid)]).astype(np.int64)
    d["inverse"] = inverse[g.permutation(n)]
    d["abc"] = np.stack([g.permutation(classes)[:3] for _ in range(n_grid)]).astype(np.int64)
    d["frag0"] = g.permutation(n_grid).astype(np.int64)
    d["frag1"] = np.sort(g.permutation(n_grid)[:n_grid // 2]).astype(np.int64)
    d["grid_coord_pts"] = g.rand(n_grid, 3).astype(np.float32)
    if pc:
        d["pc_coord"] = g.rand(pc, 3).astype(np.float32)
        d["pc_segment"] = g.randint(-1, classes, pc).astype(np.int64)
    return d


def knn_gap(d):
    from scipy.spatial import cKDTree
    used = d["origin_coord"][d["origin_feat_mask"]].astype(np.float64)
    q = (d["pc_coord"] if "pc_coord" in d else d["origin_coord"]).astype(np.float64)
    dist, _ = cKDTree(used).query(q, k=VOTE_K + 1)
    d2 = dist ** 2
    return float(np.min((d2[:, VOTE_K] - d2[:, VOTE_K - 1]) / d2[:, VOTE_K]))


def run_chain(misc, d, classes, mapping, topk):
    """engines/test.py:372-510 with the reference's helpers -> dict of recorded results"""
    seen = np.zeros(len(d["abc"]), np.int64)
    seen[d["frag0"]] += 1
    seen[d["frag1"]] += 1
    if topk:
        pred = d["abc"].copy()
    else:
        pred = d["abc"][:, 0].copy()
        pred[seen < 2] = IGNORE                     # one fragment's maximum is below THRESHOLD, two fragments' above (asserted in the test)
    pred = pred[d["inverse"]]
    for key, item in mapping.items():
        pred[pred == key] = item
    table = pred.copy()
    pred = pred[:, 0] if topk else pred
    base = pred.copy()
    if "pc_coord" in d:
        pred = misc.neighbor_voting(d["origin_coord"], pred, VOTE_K, IGNORE, classes, valid_mask=d["origin_feat_mask"],
                                    query_coords=d["pc_coord"])
        segment = d["pc_segment"]
    else:
        pred = misc.neighbor_voting(d["origin_coord"], pred, VOTE_K, IGNORE, classes, valid_mask=d["origin_feat_mask"])
        segment = d["origin_segment"]
    voted = pred.copy()
    pred = misc.clustering_voting(pred, d["origin_instance"], IGNORE)        # returns pred unchanged on a shape mismatch (pc query set)
    inter, union, target = misc.intersection_and_union(pred, segment, classes, IGNORE)
    return dict(table=table.astype(np.int32), base=base.astype(np.int32), voted=voted.astype(np.int32), final=pred.astype(np.int32),
                inter=inter.astype(np.int64), union=union.astype(np.int64), target=target.astype(np.int64))


def main_scenes(ref):
    misc = load_misc(ref)
    out = dict(vote_k=VOTE_K, ignore_index=IGNORE, threshold=THRESHOLD, num_scenes=len(SCENES))
    for s, sc in enumerate(SCENES):
        seed = sc["seed"]
        while True:
            d = draw_scene(sc["n"], sc["classes"], seed, sc["pc"])
            gap = knn_gap(d)
            if gap >= 1e-5:
                break
            seed += 100
        print("scene %d: seed %d, min relative kNN gap %.3g" % (s, seed, gap))
        out.update({"s%d_%s" % (s, k): v for k, v in d.items()})
        out.update({"s%d_seed" % s: seed, "s%d_classes" % s: sc["classes"], "s%d_knn_gap" % s: gap,
                    "s%d_map_keys" % s: np.array(list(sc["mapping"].keys())), "s%d_map_items" % s: np.array(list(sc["mapping"].values()))})
        for form, topk in (("k1", False), ("k3", True)):
            r = run_chain(misc, d, sc["classes"], sc["mapping"], topk)
            out.update({"s%d_%s_%s" % (s, form, k): v for k, v in r.items()})
        # clustering_voting on its own: the un-voted origin-level prediction of the arg-max form
        cv_in = out["s%d_k1_base" % s]
        out["s%d_cv_out" % s] = misc.clustering_voting(cv_in.copy(), d["origin_instance"], IGNORE).astype(np.int32)
        assert (cv_in != out["s%d_cv_out" % s]).any()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def main_configs(ref):
    sys.path.insert(0, HERE)
    from make_golden_configs import CONFIGS, load_config
    out = {}
    for rel in CONFIGS:
        cfg = load_config(ref, rel)
        out[rel] = {"test": cfg["test"], "data": {"test": cfg["data"]["test"]}}
    txt = "{\n" + "".join("%r:\n%s,\n" % (rel, textwrap.indent(pprint.pformat(cfg, width=116, sort_dicts=False), "    "))
                          for rel, cfg in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(OUT_CFG, "w") as f:
        f.write(txt + "\n")
    print("wrote", OUT_CFG, os.path.getsize(OUT_CFG), "bytes")


if __name__ == "__main__":
    main_scenes(sys.argv[1])
    main_configs(sys.argv[1])
