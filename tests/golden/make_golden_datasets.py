"""Generator of tests/golden/datasets.npz and tests/golden/dataset_configs.txt: the dataset layer against the reference's OWN
dataset classes.

    python tests/golden/make_golden_datasets.py <path of the reference tree>

datasets.npz: two tiny scenes (n = 257 and n = 96 Gaussians, a cloud of m = 130 points, lang_feat 768 wide in fp16) per dataset
family, stored in deliberately mixed dtypes, and what `get_data()` of every reference class returned for them with `is_train`
both ways.  The reference's `pointcept.datasets` is imported with stand-ins for the packages it names but does not need here
(termcolor, SharedArray, numba).  Only data is written; no reference source.

Layout of the file: equal arrays are stored once.  `index` is a JSON object {logical name: blob id}, the arrays are `blob_<id>`.
Logical names: `raw/<family>/<scene>/<asset>` (what the test writes to <root>/<split>/<scene>/<asset>.npy) and
`out/<class>/<train|eval>/<scene>/<key>` (the reference's returned dict without `name`).

Scene 0 has every label asset; scene 1 has no segment / instance assets (the -1 fills) and the other stored dtypes.  Stored forms:
f64 coord, u8 colour, f32 / f64 scale with values outside both clip ranges plus NaN, +-inf and -0.0, f32 opacity (n,), i64 / u8
masks with values whose low byte is zero, i64 segment20 (n, 1), i16 ScanNet++ segment (n, 3).  No stored dtype needs a host
conversion (no f64 lang_feat, no float labels): the fixture scenes run through the kernel alone.

dataset_configs.txt: the `data` dicts and batch_size* / mix_prob / seed / train of the shipped configs, evaluated as literals by
make_golden_configs.load_config (plain assignments, a handful of builtins, nothing imported)."""
import ast
import hashlib
import json
import os
import pprint
import sys
import tempfile
import textwrap
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "datasets.npz")
OUT_CFG = os.path.join(HERE, "dataset_configs.txt")
SCENES = [("scene0000_00", 257), ("scene0001_00", 96)]
M = 130
LANG = 768
CONFIGS = ["configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py",
           "configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py",
           "configs/scannet/semseg-gs-scannet-all-w-normal-fixed-xyz.py",
           "configs/scannet/semseg-gs-scannet200-all-w-normal-fixed-xyz.py",
           "configs/scannet/ssl-pretrain-scannet-all-base.py"]
CFG_KEYS = ("data", "batch_size", "batch_size_val", "batch_size_test", "num_worker", "mix_prob", "seed", "train")
# class -> family (the folder the class is pointed at)
CLASSES = {"DefaultDataset": "generic", "ScanNetGSDataset": "scannet", "ScanNet200GSDataset": "scannet", "ScanNetPPGSDataset": "scannetpp",
           "Matterport3DGSDataset": "generic", "Matterport3D_160_GSDataset": "generic", "HoliCityGSDataset": "generic",
           "KITTI360GSDataset": "generic", "GenericGSDataset": "generic"}


def stand_ins():
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules["termcolor"] = tc
    sys.modules["SharedArray"] = types.ModuleType("SharedArray")
    numba = types.ModuleType("numba")
    numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    numba.prange = range
    sys.modules.setdefault("numba", numba)


def base_scene(s, n):
    """the assets every family shares"""
    g = np.random.RandomState(100 + s)
    scale = g.rand(n, 3) * 2.0 - 0.2                       # below 0 / 1e-4 and above 1.0 / 1.5
    scale[:8, 0] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-4, 1.5, 1.0]
    scale[8:12, 1] = [5e-5, 1.5000001, 0.01, 10.0]
    opacity = g.rand(n)
    opacity[:5] = [0.0, 0.001, 0.0005, -0.0, 1.0]
    mask = (g.rand(n) < 0.8).astype(np.int64)
    mask[:6] = [256, 0, 512, 1, 65536, -256]               # low byte zero: truthy all the same
    d = dict(coord=(g.rand(n, 3) * 4.0 - 1.0).astype(np.float64), color=g.randint(0, 256, (n, 3)).astype(np.uint8),
             scale=scale.astype(np.float32 if s == 0 else np.float64), opacity=opacity.astype(np.float32),
             quat=g.randn(n, 4).astype(np.float32), normal=g.randn(n, 3).astype(np.float32 if s == 0 else np.float64),
             lang_feat=g.randn(n, LANG).astype(np.float16),
             valid_feat_mask=mask if s == 0 else (mask != 0).astype(np.uint8) * np.uint8(3),
             pc_coord=(g.rand(M, 3) * 4.0 - 1.0).astype(np.float64 if s == 0 else np.float32))
    return d, g


def families(s, n):
    d, g = base_scene(s, n)
    labels = s == 0                                        # scene 1: no segment / instance assets among the Gaussians
    scannet = dict(d, pc_segment20=g.randint(-1, 20, M).astype(np.int64), pc_segment200=g.randint(-1, 200, (M, 1)).astype(np.int16),
                   pc_instance=g.randint(-1, 30, M).astype(np.int64))
    scannetpp = dict(d, pc_segment=g.randint(-1, 100, (M, 2)).astype(np.int16), pc_instance=g.randint(-1, 30, (M, 1)).astype(np.int32))
    generic = dict(d, pc_segment=g.randint(-1, 21, (M, 1)).astype(np.int64), pc_segment_nyu_160=g.randint(-1, 160, M).astype(np.int16),
                   pc_instance=g.randint(-1, 30, M).astype(np.int32), strength=g.rand(n, 1).astype(np.float32),
                   pose=g.randn(4, 4).astype(np.float64))
    if labels:
        wide = g.randint(-1, 20, (n, 1)).astype(np.int64)
        wide[:2, 0] = [2 ** 31, -2 ** 31 - 1]               # wrap-around, as astype(int32)
        scannet.update(segment20=wide, segment200=g.randint(-1, 200, n).astype(np.int32), instance=g.randint(-1, 40, n).astype(np.int64))
        scannetpp.update(segment=g.randint(-1, 100, (n, 3)).astype(np.int16), instance=g.randint(-1, 40, (n, 2)).astype(np.int32))
        generic.update(segment=g.randint(-1, 21, n).astype(np.uint8), segment_nyu_160=g.randint(-1, 160, (n, 1)).astype(np.int16),
                       instance=g.randint(-1, 40, n).astype(np.int8))
    else:
        scannetpp.update(segment200=g.randint(-1, 200, n).astype(np.int64), instance=g.randint(-1, 40, n).astype(np.int16))
    return dict(scannet=scannet, scannetpp=scannetpp, generic=generic)


class Blobs:
    def __init__(self):
        self.index, self.blobs = {}, {}

    def add(self, name, arr):
        arr = np.ascontiguousarray(arr)
        key = hashlib.sha1(repr((arr.dtype.str, arr.shape)).encode() + arr.tobytes()).hexdigest()[:16]
        self.blobs.setdefault(key, arr)
        self.index[name] = key

    def save(self, path):
        np.savez_compressed(path, index=np.array(json.dumps(self.index, sort_keys=True)), **{"blob_" + k: v for k, v in self.blobs.items()})


def main_scenes(ref):
    stand_ins()
    sys.path.insert(0, ref)
    import pointcept.datasets as pd                        # noqa: F401  (registers the classes)
    import pointcept.datasets.kitti360_gs                  # noqa: F401  (not imported by the package itself)
    from pointcept.datasets.builder import DATASETS
    blobs = Blobs()
    with tempfile.TemporaryDirectory() as root:
        for s, (scene, n) in enumerate(SCENES):
            for fam, assets in families(s, n).items():
                folder = os.path.join(root, fam, "val", scene)
                os.makedirs(folder)
                for k, v in assets.items():
                    np.save(os.path.join(folder, k + ".npy"), v)
                    blobs.add("raw/%s/%s/%s" % (fam, scene, k), v)
        for cls, fam in CLASSES.items():
            for is_train in (True, False):
                kw = {} if cls == "DefaultDataset" else dict(is_train=is_train)
                if cls == "DefaultDataset" and not is_train:
                    continue
                ds = DATASETS.get(cls)(split="val", data_root=os.path.join(root, fam), **kw)
                assert len(ds) == len(SCENES)
                for i in range(len(ds)):
                    d = ds.get_data(i)
                    scene = d.pop("name")
                    assert scene == ds.get_data_name(i)
                    for k, v in d.items():
                        blobs.add("out/%s/%s/%s/%s" % (cls, "train" if is_train else "eval", scene, k), np.asarray(v))
    blobs.save(OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(blobs.index), "names,", len(blobs.blobs), "arrays")


def main_configs(ref):
    sys.path.insert(0, HERE)
    from make_golden_configs import load_config
    from make_golden_semseg import load_config as load_config_semseg      # (serves the semseg configs' one import, the class names)
    out = {}
    for rel in CONFIGS:
        cfg = (load_config_semseg if "semseg" in rel else load_config)(ref, rel)
        out[rel] = {k: cfg[k] for k in CFG_KEYS if k in cfg}
    txt = "{\n" + "".join("%r:\n%s,\n" % (rel, textwrap.indent(pprint.pformat(cfg, width=116, sort_dicts=False), "    "))
                          for rel, cfg in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(OUT_CFG, "w") as f:
        f.write(txt + "\n")
    print("wrote", OUT_CFG, os.path.getsize(OUT_CFG), "bytes")


if __name__ == "__main__":
    main_scenes(sys.argv[1])
    main_configs(sys.argv[1])
