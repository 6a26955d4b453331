"""CPU: the host side of the dataset layer (scenesplat_amd/pointcept_api/datasets.py): the DATASETS registry, the shipped `data`
dicts (tests/golden/dataset_configs.txt) building datasets, the scene lists, the ingest plan (native.ingest_plan) of every class on
the fixture scenes (tests/golden/datasets.npz, written by tests/golden/make_golden_datasets.py from the reference's own classes)
and the loaders' index logic.  Nothing is launched."""
import ast
import json
import os

import numpy as np
import pytest
import torch

NAMES = ["DefaultDataset", "ConcatDataset", "ScanNetGSDataset", "ScanNet200GSDataset", "ScanNetPPGSDataset", "Matterport3DGSDataset",
         "Matterport3D_160_GSDataset", "HoliCityGSDataset", "KITTI360GSDataset", "GenericGSDataset"]
FAMILY = {"DefaultDataset": "generic", "ScanNetGSDataset": "scannet", "ScanNet200GSDataset": "scannet", "ScanNetPPGSDataset": "scannetpp",
          "Matterport3DGSDataset": "generic", "Matterport3D_160_GSDataset": "generic", "HoliCityGSDataset": "generic",
          "KITTI360GSDataset": "generic", "GenericGSDataset": "generic"}
SCENES = ["scene0000_00", "scene0001_00"]
CONCAT = "configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py"
F32_BITS = lambda v: int(np.float32(v).view(np.uint32))      # noqa: E731


class Fixture:
    def __init__(self, golden_dir):
        z = np.load(os.path.join(golden_dir, "datasets.npz"))
        self.z, self.index = z, json.loads(str(z["index"]))

    def names(self, prefix):
        return sorted(k[len(prefix):] for k in self.index if k.startswith(prefix))

    def get(self, name):
        return self.z["blob_" + self.index[name]]

    def write(self, root, family, split="val", scenes=SCENES):
        """the scene folders of one family under root/<split>/"""
        for scene in scenes:
            folder = os.path.join(root, split, scene)
            os.makedirs(folder, exist_ok=True)
            for asset in self.names("raw/%s/%s/" % (family, scene)):
                np.save(os.path.join(folder, asset + ".npy"), self.get("raw/%s/%s/%s" % (family, scene, asset)))
        return root


@pytest.fixture(scope="module")
def fx(golden_dir):
    return Fixture(golden_dir)


def load_configs(golden_dir):
    with open(os.path.join(golden_dir, "dataset_configs.txt")) as f:
        return ast.literal_eval(f.read())


def pointed(d, root, **extra):
    """a shipped dataset dict with data_root pointed at `root` (recursively for a ConcatDataset)"""
    d = dict(d)
    if d["type"] == "ConcatDataset":
        d["datasets"] = [pointed(x, root, **extra) for x in d["datasets"]]
    else:
        d.update(data_root=root, **extra)
    return d


def test_registry_names_and_exports():
    from scenesplat_amd import pointcept_api as api
    assert sorted(api.DATASETS.module_dict) == sorted(NAMES)
    for n in NAMES:
        assert api.DATASETS.get(n) is getattr(api, n)
    for f in ("build_dataset", "build_train_loader", "build_val_loader", "build_test_loader", "DeviceLoader"):
        assert callable(getattr(api, f))
    with pytest.raises(KeyError):
        api.build_dataset(dict(type="SemanticKITTIDataset"))


def test_existing_pins_still_hold(tmp_path):
    from scenesplat_amd.pointcept_api import HOOKS, TESTERS, TRANSFORMS, Trainer  # noqa: F401
    for name in ("PreciseEvaluator", "BeginningEvaluator", "LangPretrainZeroShotSemSegEval", "LangPretrainZeroShotSemSegEvalMulti"):
        assert name not in HOOKS.module_dict
    with pytest.raises(NotImplementedError):
        TRANSFORMS.build(dict(type="GridSample", mode="test"))
    assert "GSGaussianBlurVoxelGPU" not in TRANSFORMS.module_dict
    with pytest.raises(ValueError):
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=dict(save_path=str(tmp_path), device="cpu", test={}, data=dict(test={})),
                           model=object()))


def test_every_shipped_data_dict_builds(golden_dir, tmp_path):
    from scenesplat_amd.pointcept_api import build_dataset
    built = 0
    for rel, cfg in load_configs(golden_dir).items():
        for part in ("train", "val", "test"):
            v = cfg["data"].get(part)
            if v is None:
                continue
            for d in (v if isinstance(v, list) else [v]):
                ds = build_dataset(pointed(d, str(tmp_path), device="cpu"))
                assert type(ds).__name__ == d["type"] and len(ds) == 0
                subs = ds.datasets if d["type"] == "ConcatDataset" else [ds]
                for sub, sd in zip(subs, d["datasets"] if d["type"] == "ConcatDataset" else [d]):
                    assert sub.test_mode == bool(sd.get("test_mode", False)) and sub.is_train == sd.get("is_train", True)
                    assert sub.loop == (1 if sub.test_mode else sd.get("loop", 1))
                    assert len(sub.transform.transforms) == len(sd.get("transform") or [])
                    if sub.test_mode:
                        assert len(sub.aug_transform) == len(sd["test_cfg"]["aug_transform"]) and sub.test_voxelize["mode"] == "test"
                built += 1
    assert built == 19          # 1 + 3 + 5 (concat), 3 x 3 (the single-dataset configs), 1 (ssl: train only)


def test_refusals(tmp_path):
    from scenesplat_amd.pointcept_api import build_dataset
    root = str(tmp_path)
    with pytest.raises(NotImplementedError, match="cache_bytes"):
        build_dataset(dict(type="ScanNetGSDataset", data_root=root, cache=True, device="cpu"))
    with pytest.raises(ValueError, match="tail_classes"):
        build_dataset(dict(type="ScanNetPPGSDataset", data_root=root, sample_tail_classes=True, device="cpu"))
    ds = build_dataset(dict(type="ScanNetPPGSDataset", data_root=root, sample_tail_classes=True, tail_classes=[82, 74], device="cpu"))
    assert ds.tail_classes.tolist() == [82, 74] and not hasattr(ds, "class2id")
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n40\n")
    assert build_dataset(dict(type="ScanNetGSDataset", data_root=root, class2id=str(ids), device="cpu")).class2id.tolist() == [1, 2, 40]
    assert build_dataset(dict(type="ScanNetGSDataset", data_root=root, class2id=[3, 4], device="cpu")).class2id.tolist() == [3, 4]
    tc = dict(voxelize=None, crop=dict(type="SphereCrop"), post_transform=[], aug_transform=[[]])
    with pytest.raises(NotImplementedError, match="crop"):
        build_dataset(dict(type="ScanNetGSDataset", data_root=root, test_mode=True, test_cfg=tc, device="cpu"))


def test_get_data_list_and_names(fx, tmp_path):
    import glob
    from scenesplat_amd.pointcept_api import build_dataset
    root = fx.write(str(tmp_path), "scannet", "val")
    fx.write(root, "scannet", "train", scenes=SCENES[:1])
    kw = dict(data_root=root, device="cpu")
    ds = build_dataset(dict(type="ScanNetGSDataset", split="val", loop=3, **kw))
    assert ds.data_list == glob.glob(os.path.join(root, "val", "*")) and len(ds) == 6
    assert sorted(ds.get_data_name(i) for i in range(2)) == SCENES and ds.get_data_name(5) == ds.get_data_name(1)
    seq = build_dataset(dict(type="DefaultDataset", split=("val", "train"), **kw))
    assert seq.data_list == glob.glob(os.path.join(root, "val", "*")) + glob.glob(os.path.join(root, "train", "*"))
    flt = build_dataset(dict(type="Matterport3DGSDataset", split="val", filtered_scene=["scene0001"], **kw))
    assert [os.path.basename(p) for p in flt.data_list] == ["scene0000_00"]
    lr = tmp_path / "lr.txt"
    lr.write_text("scene0000_00\nscene0042_00\n")
    ds = build_dataset(dict(type="ScanNet200GSDataset", split="val", lr_file=str(lr), **kw))
    assert ds.data_list == [os.path.join(root, "train", "scene0000_00"), os.path.join(root, "train", "scene0042_00")]
    # test mode forces loop = 1
    tc = dict(voxelize=dict(type="GridSample", mode="test", grid_size=0.02, keys=("coord",)), crop=None, post_transform=[], aug_transform=[[]])
    assert len(build_dataset(dict(type="ScanNetGSDataset", split="val", loop=5, test_mode=True, test_cfg=tc, **kw))) == 2
    with pytest.raises(RuntimeError, match="CPU"):
        ds.get_data(0)
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type="ScanNetPPGSDataset", split="val", multilabel=True, **kw)).get_data(0)


def test_concat_dataset_list_and_loop(fx, tmp_path):
    from scenesplat_amd.pointcept_api import build_dataset
    root = fx.write(str(tmp_path), "generic")
    sub = dict(split="val", data_root=root, device="cpu")
    cat = build_dataset(dict(type="ConcatDataset", loop=2, datasets=[dict(type="HoliCityGSDataset", loop=2, **sub), dict(type="GenericGSDataset", **sub)]))
    assert [(int(a), int(b)) for a, b in cat.data_list] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)] and len(cat) == 12
    assert cat.get_data_name(7) == cat.datasets[0].get_data_name(1) and cat.get_data_name(4) == cat.datasets[1].get_data_name(0)


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def plan_of(fx, cls, scene, is_train, tmp_path):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import build_dataset
    root = fx.write(str(tmp_path / cls), FAMILY[cls])
    kw = {} if cls == "DefaultDataset" else dict(is_train=is_train)
    ds = build_dataset(dict(type=cls, split="val", data_root=root, device="cpu", **kw))
    path = os.path.join(root, "val", scene)
    arrays = {n: np.load(os.path.join(path, n + ".npy")) for n in ds.asset_names(path)}
    return arrays, nv.ingest_plan(arrays, ds.rules(arrays)), ds


@pytest.mark.parametrize("cls", [n for n in NAMES if n != "ConcatDataset"])
def test_plan_matches_the_reference_dicts(fx, tmp_path, cls):
    """keys, dtypes and shapes of the planned outputs (plus the -1 fills) are the recorded dict's; offsets are aligned; nothing on
    the fixture scenes needs the host fallback"""
    from scenesplat_amd import native as nv
    for is_train in ((True,) if cls == "DefaultDataset" else (True, False)):
        for scene in SCENES:
            arrays, (desc, offsets, specs, fallback), ds = plan_of(fx, cls, scene, is_train, tmp_path)
            prefix = "out/%s/%s/%s/" % (cls, "train" if is_train else "eval", scene)
            want = {k: fx.get(prefix + k) for k in fx.names(prefix)}
            got = {s["name"]: s for s in specs}
            assert fallback == [] and desc.shape == (len(arrays), 8) and desc.dtype == np.int64
            fills = [k for k in ds.FILL if k not in got]
            assert set(got) | set(fills) == set(want), (sorted(got), fills, sorted(want))
            for k in fills:
                assert want[k].dtype == np.int32 and (want[k] == -1).all() and want[k].shape == (len(want["coord"]),)
            # (scene 1 of the ScanNet++ family stores segment200 and a 1-d instance instead: the class's two fall-back branches)
            assert bool(fills) == (scene == SCENES[1] and bool(ds.FILL) and cls != "ScanNetPPGSDataset")
            for j, s in enumerate(specs):
                w = want[s["name"]]
                assert s["dtype"] == w.dtype.name and tuple(s["shape"]) == w.shape, (s["name"], s["dtype"], s["shape"], w.dtype, w.shape)
                assert desc[j, 2] == w.size and desc[j, 0] == offsets[s["stored"]] and desc[j, 0] % nv.INGEST_ALIGN == 0 and desc[j, 1] == 0
                word = int(desc[j, 3])
                assert word & 0xff == nv.INGEST_CODES[arrays[s["stored"]].dtype.name] and (word >> 8) & 0xff == nv.INGEST_CODES[w.dtype.name]
            ends = sorted((offsets[s["stored"]], offsets[s["stored"]] + s["array"].nbytes) for s in specs)
            assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= offsets[""] and offsets[""] % nv.INGEST_ALIGN == 0


def test_plan_rows_flags_and_clip_bits(fx, tmp_path):
    from scenesplat_amd import native as nv
    LO, HI, PICK = nv.INGEST_HAS_LO, nv.INGEST_HAS_HI, nv.INGEST_PICK

    def row(cls, scene, stored, is_train=False):
        arrays, (desc, offsets, specs, fallback), _ = plan_of(fx, cls, scene, is_train, tmp_path)
        j = [s["stored"] for s in specs].index(stored)
        return desc[j], specs[j]
    # the scale clip per class; opacity as a column, with its floor where the reference has one
    for cls, lo, hi, olo in (("ScanNetGSDataset", 0.0, 1.5, None), ("ScanNetPPGSDataset", 0.0, 1.5, None), ("Matterport3DGSDataset", 0.0, 1.5, None),
                             ("HoliCityGSDataset", 1e-4, 1.0, 0.001), ("GenericGSDataset", 1e-4, 1.0, 0.001)):
        d, s = row(cls, SCENES[0], "scale")
        assert (d[3] >> 16) == LO | HI and d[6] == F32_BITS(lo) and d[7] == F32_BITS(hi) and not s["alias"]
        d, s = row(cls, SCENES[0], "opacity")
        assert s["shape"] == (257, 1) and (d[3] >> 16) == (LO if olo is not None else 0) and (olo is None or d[6] == F32_BITS(olo))
        assert s["alias"] == (olo is None)                      # stored f32, no clip: a view of the arena
    d, s = row("KITTI360GSDataset", SCENES[0], "scale")        # (divided by 10 before its clip: two torch ops after the launch)
    assert (d[3] >> 16) == 0
    # renamed keys, flattening, the column pick
    d, s = row("ScanNetGSDataset", SCENES[0], "segment20")
    assert s["name"] == "segment" and s["shape"] == (257,) and (d[3] >> 16) == 0 and d[3] & 0xffff == 7 | (6 << 8)
    d, s = row("ScanNet200GSDataset", SCENES[0], "pc_segment200")
    assert s["name"] == "pc_segment" and s["shape"] == (130,) and d[3] & 0xffff == 5 | (6 << 8)
    d, s = row("Matterport3D_160_GSDataset", SCENES[0], "segment_nyu_160")
    assert s["name"] == "segment" and s["shape"] == (257,)
    d, s = row("ScanNetPPGSDataset", SCENES[0], "segment")
    assert (d[3] >> 16) == PICK and (d[4], d[5], d[2]) == (3, 0, 257) and s["shape"] == (257,)
    d, s = row("ScanNetPPGSDataset", SCENES[0], "instance")
    assert (d[3] >> 16) == PICK and (d[4], d[5]) == (2, 0)
    d, s = row("ScanNetPPGSDataset", SCENES[1], "instance")    # stored 1-d: the reference's except branch flattens
    assert (d[3] >> 16) == 0 and s["shape"] == (96,)
    d, s = row("ScanNetPPGSDataset", SCENES[1], "segment200")
    assert s["name"] == "segment"
    d, s = row("HoliCityGSDataset", SCENES[0], "pc_segment")
    assert s["shape"] == (130, 1) and s["dtype"] == "int32"
    d, s = row("ScanNetGSDataset", SCENES[0], "lang_feat")
    assert s["alias"] and s["dtype"] == "float16" and s["shape"] == (257, 768)
    d, s = row("ScanNetGSDataset", SCENES[0], "valid_feat_mask")
    assert d[3] & 0xffff == 7 | (8 << 8) and not s["alias"]
    d, s = row("ScanNetGSDataset", SCENES[0], "pc_instance")   # no rule: as stored
    assert s["alias"] and s["dtype"] == "int64"
    # is_train decides whether the cloud is read at all
    arrays, _, _ = plan_of(fx, "ScanNetGSDataset", SCENES[0], True, tmp_path)
    assert not any(k.startswith("pc_c") or k.startswith("pc_s") for k in arrays) and "pc_instance" in arrays


def test_plan_host_fallback():
    from scenesplat_amd import native as nv
    g = np.random.RandomState(0)
    arrays = dict(lang_feat=g.randn(5, 8), segment=g.rand(5) * 4, mask=g.rand(5) - 0.5, coord=g.rand(5, 3), big=np.arange(5, dtype=">i4"))
    rules = dict(lang_feat=dict(dtype="float16"), segment=dict(dtype="int32", shape="flat"), mask=dict(dtype="bool"), coord=dict(dtype="float32"),
                 big=dict(dtype="float32"))
    desc, offsets, specs, fallback = nv.ingest_plan(arrays, rules)
    assert fallback == ["lang_feat", "segment", "mask"]         # f64 -> f16 would round twice; float -> int / bool is numpy's
    by = {s["stored"]: s for s in specs}
    assert by["lang_feat"]["array"].dtype == np.float16 and np.array_equal(by["lang_feat"]["array"], arrays["lang_feat"].astype(np.float16))
    assert by["segment"]["array"].dtype == np.int32 and by["mask"]["array"].dtype == bool and by["coord"]["array"].dtype == np.float64
    assert by["big"]["array"].dtype == np.dtype("<i4") and np.array_equal(by["big"]["array"], np.arange(5))
    assert [int(w) & 0xffff for w in desc[:, 3]] == [2 | (2 << 8), 6 | (6 << 8), 8 | (8 << 8), 0 | (1 << 8), 6 | (1 << 8)]
    with pytest.raises(ValueError, match="float32"):
        nv.ingest_plan(dict(a=np.zeros(3)), dict(a=dict(dtype="int32", lo=0.0)))
    with pytest.raises(IndexError):
        nv.ingest_plan(dict(a=np.zeros(3, np.int16)), dict(a=dict(dtype="int32", shape="column")))
    with pytest.raises(RuntimeError, match="no device conversion"):
        nv.ingest_group(np.array([[256, 256, 4, 0 | (2 << 8), 0, 0, 0, 0]], dtype=np.int64), "cpu")
    for s, d, ok in (("float64", "float32", True), ("float64", "float16", False), ("float32", "float16", True), ("float32", "int32", False),
                     ("int64", "int32", True), ("int16", "bool", True), ("bool", "int32", True), ("int64", "int64", True), ("float16", "bool", False)):
        assert nv.ingest_pair_on_device(s, d) is ok


# ---- the loaders ------------------------------------------------------------------------------------------------------------
class Counted:
    """a dataset of n integers that records the order it was read in"""

    def __init__(self, n):
        self.n, self.seen, self.hints = n, [], []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        self.seen.append(i)
        return i

    def set_next(self, i):
        self.hints.append(i)


def test_device_loader_len_and_order():
    from scenesplat_amd.pointcept_api import DeviceLoader
    for n, bs in ((10, 3), (9, 3), (2, 3), (0, 2)):
        ds = Counted(n)
        for drop in (False, True):
            dl = DeviceLoader(ds, bs, drop_last=drop, collate=list)
            ref = torch.utils.data.DataLoader(range(n), batch_size=bs, drop_last=drop)
            assert len(dl) == len(ref) and [b for b in dl] == [b.tolist() for b in ref]
            assert dl.dataset is ds and dl.batch_size == bs and len(dl.sampler) == n
    # the hint is the next index of the sampler's order, None at the end
    ds = Counted(5)
    dl = DeviceLoader(ds, 2, shuffle=True, seed=7, collate=list)
    e0 = [i for b in dl for i in b]
    assert ds.seen == e0 and ds.hints == e0[1:] + [None] and sorted(e0) == list(range(5))
    e1 = [i for b in dl for i in b]
    again = [i for b in DeviceLoader(Counted(5), 2, shuffle=True, seed=7, collate=list) for i in b]
    assert again == e0 and e1 != e0 and sorted(e1) == list(range(5))      # seeded, and a new permutation per epoch


def test_device_loader_shards_like_distributed_sampler(monkeypatch):
    from torch.utils.data import DistributedSampler
    from scenesplat_amd.pointcept_api import DeviceLoader, datasets
    ds = Counted(11)
    for rank in (0, 1):
        monkeypatch.setattr(datasets, "get_world_size", lambda: 2)
        monkeypatch.setattr(datasets, "get_rank", lambda r=rank: r)
        dl = DeviceLoader(ds, 2, shuffle=True, seed=5, drop_last=True, collate=list)
        ref = DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True, seed=5)
        assert isinstance(dl.sampler, DistributedSampler) and len(dl) == len(ref) // 2
        for epoch in (0, 1):
            dl.sampler.set_epoch(epoch)
            ref.set_epoch(epoch)
            want = list(ref)
            assert [i for b in dl for i in b] == want[:len(want) // 2 * 2]


def test_multi_dataset_loader_follows_the_reference_formula(golden_dir, fx, tmp_path):
    from scenesplat_amd.pointcept_api import build_train_loader, engine
    cfg = load_configs(golden_dir)[CONCAT]
    root = fx.write(str(tmp_path), "generic", "train")
    fx.write(root, "scannet", "train")
    fx.write(root, "scannetpp", "train")
    data = dict(cfg["data"], train=pointed(cfg["data"]["train"], root, device="cpu", split="train"))
    assert cfg["train"]["type"] == "MultiDatasetTrainer"
    loader = build_train_loader(dict(cfg, data=data, batch_size_per_gpu=1, seed=3))
    assert isinstance(loader, engine.MultiDatasetLoader)
    shipped = [d["loop"] for d in cfg["data"]["train"]["datasets"]]
    assert loader.ratios == shipped == [3, 2, 2]
    subs = [dl.dataset for dl in loader.dataloaders]
    assert [d.loop for d in subs] == [cfg["data"]["train"].get("loop", 1), 1, 1] and [len(dl) for dl in loader.dataloaders] == [2, 2, 2]
    main = len(loader.dataloaders[0])
    assert len(loader) == main // shipped[0] * sum(shipped) + main % shipped[0]
    # per-dataset transform seeds: num_datasets * rank + dataset_id + seed (rank 0 here)
    assert [d.seed for d in subs] == [3, 4, 5]
    assert all(dl.drop_last and dl.batch_size == 1 for dl in loader.dataloaders)
    # not under MultiDatasetTrainer: one loader over the concat set
    one = build_train_loader(dict(cfg, data=data, train=dict(type="DefaultTrainer"), batch_size_per_gpu=4, seed=None))
    assert type(one).__name__ == "DeviceLoader" and type(one.dataset).__name__ == "ConcatDataset" and len(one) == (2 * 3 + 2 * 2 + 2 * 2) // 4


def test_val_and_test_loader_builders(golden_dir, fx, tmp_path):
    from scenesplat_amd.pointcept_api import build_test_loader, build_val_loader
    from scenesplat_amd.pointcept_api.tester import TesterBase
    cfg = load_configs(golden_dir)[CONCAT]
    root = fx.write(str(tmp_path), "scannet")
    data = dict(cfg["data"], val=[pointed(d, root, device="cpu", split="val") for d in cfg["data"]["val"]],
                test=[pointed(d, root, device="cpu", split="val") for d in cfg["data"]["test"]])
    vals = build_val_loader(dict(cfg, data=data, batch_size_val_per_gpu=2))
    assert isinstance(vals, list) and len(vals) == 3 and all(v.batch_size == 2 and not v.drop_last and len(v) == 1 for v in vals)
    one = build_val_loader(dict(cfg, data=dict(data, val=data["val"][1])))
    assert type(one).__name__ == "DeviceLoader" and type(one.dataset).__name__ == "ScanNet200GSDataset"
    t = build_test_loader(dict(cfg, data=data, batch_size_test_per_gpu=1), index=1)
    assert t.batch_size == 1 and len(t) == 2 and t.dataset.test_mode and type(t.dataset).__name__ == "ScanNet200GSDataset"
    assert t.collate(["x"]) == TesterBase.collate_fn(["x"]) == ["x"]


def test_prefetch_does_not_change_the_order(fx, tmp_path, monkeypatch):
    """The worker thread reads and packs ahead, the consumer decides: samples come in the sampler's order with prefetch on and
    off, and what was packed for them is the same.  The stager's three GPU steps are replaced by host stand-ins; its reads, plans,
    slots, hints and the worker thread run as they are."""
    from scenesplat_amd.pointcept_api import DeviceLoader, build_dataset
    root = fx.write(str(tmp_path), "scannet")
    runs = {}
    for prefetch in (False, True):
        ds = build_dataset(dict(type="ScanNetGSDataset", split="val", data_root=root, loop=3, prefetch=prefetch, is_train=False, device="cpu"))
        st = ds.stager
        packed = []

        def grow(slot, total, st=st):
            st.slots[slot] = torch.empty(total + 64, dtype=torch.uint8)

        def upload(slot, total, st=st):
            return st.slots[slot][:total].clone()

        def launch(arena, plan, views, packed=packed):
            packed.append(bytes(arena.numpy()[:plan[1][""]][plan[1]["coord"]:plan[1]["coord"] + 64]))
            return dict({s["name"]: torch.zeros(1) for s in plan[2]}, segment=torch.zeros(1), instance=torch.zeros(1))   # (no -1 fills)
        monkeypatch.setattr(st, "_grow", grow)
        monkeypatch.setattr(st, "_upload", upload)
        monkeypatch.setattr(st, "_launch", launch)
        ds.device = st.device = torch.device("cuda")           # (only the type is looked at; nothing below touches a GPU)
        dl = DeviceLoader(ds, 2, shuffle=True, seed=1, collate=lambda s: [d["name"] for d in s])
        names = [n for b in dl for n in b]
        st.close()
        runs[prefetch] = (names, packed, ds.stats["np_load"])
        assert ds.stats["prefetched"] == (5 if prefetch else 0) and ds.stats["uploads"] == 6 and st.pending is None
    assert runs[True] == runs[False] and len(runs[True][0]) == 6 and sorted(set(runs[True][0])) == SCENES
    coord = {s: fx.get("raw/scannet/%s/coord" % s).tobytes()[:64] for s in SCENES}
    assert runs[True][1] == [coord[n] for n in runs[True][0]]   # every sample was packed from its own files
