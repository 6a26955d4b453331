"""The dataset layer the shipped configs name first: `data = dict(train=dict(type="ScanNetGSDataset", ...), ...)`.

Mirror of pointcept/datasets (defaults.py, scannetgs.py, scannetppgs.py, matterport3dgs.py, holicitygs.py, kitti360_gs.py,
generic_gs.py, dataloader.py, builder.py) whose samples are DEVICE tensors.  The per-asset `astype` / `clip` / `reshape` / `[:, 0]`
block of the reference's `get_data` is one packed upload and ONE grouped launch per scene (csrc/ingest.hip):

    .npy files --np.load--> stored dtypes --pack at 256-byte offsets--> pinned slot --one copy--> device arena --ss_ingest_group--> dict

* two pinned slots, grown on demand; a slot is rewritten only after the event behind its copy has passed; with prefetch=True ONE
  worker thread reads and packs the sample the loader announced as next while the device works (the worker touches no GPU API:
  copy and launch are issued by the consuming thread, so the order of samples never depends on thread timing);
* an asset stored in its target dtype (lang_feat in fp16) is a VIEW of the arena: no pass over it at all;
* cache_bytes > 0 keeps the raw arenas of the most recently used scenes on the device (LRU); a hit is one launch that copies
  every asset out of the cached arena (the transforms update tensors in place, so a hit hands out no views).

Loaders: DeviceLoader (a sized iterable with .dataset / .sampler / .batch_size) and build_train_loader / build_val_loader /
build_test_loader.  There are no worker processes: `num_worker_per_gpu` is accepted and ignored."""
import glob
import os
import threading
from collections import OrderedDict
from collections.abc import Sequence
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import gpu_transforms as gt
from .. import native as nv
from .engine import MultiDatasetLoader, get_rank, get_world_size
from .registry import Registry
from .transform import Compose

DATASETS = Registry("datasets")


def build_dataset(cfg):
    """builder.py:13-15"""
    return DATASETS.build(cfg)


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


_TORCH_DTYPES = {"float64": torch.float64, "float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8, "int8": torch.int8,
                 "int16": torch.int16, "int32": torch.int32, "int64": torch.int64, "bool": torch.bool}
_F32 = dict(dtype="float32")
_I32_FLAT = dict(dtype="int32", shape="flat")


# ---- staging: pinned slots, the worker thread, the scene cache -----------------------------------------------------------------------
class _Packed:
    """One scene read from disk and planned: the plan of native.ingest_plan, and the slot its payload sits in (None: not packed yet,
    because the slot has to grow, which only the consuming thread may do)."""

    def __init__(self, path, plan, slot):
        self.path, self.plan, self.slot = path, plan, slot


class SceneStager:
    """Reads, packs, uploads and converts the scenes of one dataset (module docstring)."""

    def __init__(self, device, cache_bytes=0, prefetch=True, stats=None):
        self.device = torch.device(device)
        self.cache_bytes, self.prefetch = int(cache_bytes), bool(prefetch)
        self.stats = stats if stats is not None else {}
        for k in ("np_load", "host_fallback", "cache_hit", "cache_miss", "launches", "uploads", "prefetched"):
            self.stats.setdefault(k, 0)
        self.slots, self.events, self.next_slot = [None, None], [None, None], 0
        self.cache, self.cache_used = OrderedDict(), 0       # path -> (arena, plan)
        self.pending = None                                  # (path, future -> _Packed, slot)
        self.pool = None
        self.lock = threading.Lock()

    # -- host side (also run by the worker: no GPU API below this line until `fetch`) --------------------------------------------
    def _read(self, path, names, rules_of):
        arrays = OrderedDict()
        for name in names:
            arrays[name] = np.load(os.path.join(path, name + ".npy"))
            with self.lock:
                self.stats["np_load"] += 1
        return nv.ingest_plan(arrays, rules_of(arrays))

    def _pack(self, plan, slot):
        desc, offsets, specs, _ = plan
        buf = self.slots[slot]
        if buf is None or buf.numel() < offsets[""]:
            return False
        host = buf.numpy()
        for spec in specs:
            a, off = spec["array"], offsets[spec["stored"]]
            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        return True

    def _read_and_pack(self, path, names, rules_of, slot):
        plan = self._read(path, names, rules_of)
        return _Packed(path, plan, slot if self._pack(plan, slot) else None)

    # -- consuming thread ----------------------------------------------------------------------------------------------------
    def _free_slot(self):
        """the slot to write next, once the copy that last read it has completed"""
        slot = self.next_slot
        self.next_slot = 1 - slot
        if self.events[slot] is not None:
            self.events[slot].synchronize()
            self.events[slot] = None
        return slot

    def announce(self, path, names, rules_of):
        """the loader's hint: `path` is the next scene of the sampler's order"""
        if not self.prefetch or self.device.type != "cuda" or path in self.cache:
            return
        if self.pending is not None:
            if self.pending[0] == path:
                return
            self._drop_pending()
        if self.pool is None:
            self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="scene-ingest")
        slot = self._free_slot()
        self.pending = (path, self.pool.submit(self._read_and_pack, path, names, rules_of, slot), slot)

    def _drop_pending(self):
        path, fut, slot = self.pending
        self.pending = None
        fut.result()                 # (the worker owns the slot until it is done)
        self.next_slot = slot        # nothing was copied out of it: it is free again

    def fetch(self, path, names, rules_of):
        """-> {output key: device tensor} of one scene"""
        if self.device.type != "cuda":
            raise RuntimeError("datasets: samples are built on the GPU (device='cuda'); there is no CPU fallback")
        hit = self.cache.get(path)
        if hit is not None:
            self.cache.move_to_end(path)
            self.stats["cache_hit"] += 1
            return self._launch(hit[0], hit[1], views=False)
        if self.pending is not None and self.pending[0] != path:
            self._drop_pending()
        if self.pending is not None:
            _, fut, slot = self.pending
            self.pending = None
            packed = fut.result()
            self.stats["prefetched"] += 1
        else:
            slot = self._free_slot()
            packed = self._read_and_pack(path, names, rules_of, slot)
        plan = packed.plan
        total = plan[1][""]
        if packed.slot is None:                  # the slot has to grow: pinned memory is allocated by this thread only
            self._grow(slot, total)
            self._pack(plan, slot)
        self.stats["host_fallback"] += len(plan[3])
        if self.cache_bytes > 0:
            self.stats["cache_miss"] += 1
        arena = self._upload(slot, total)
        self.stats["uploads"] += 1
        cached = 0 < total <= self.cache_bytes
        if cached:
            light = (plan[0], plan[1], [dict(s, array=None) for s in plan[2]], plan[3])     # (the host arrays are not kept)
            self.cache[path] = (arena, light)
            self.cache_used += total
            while self.cache_used > self.cache_bytes:
                _, (old, old_plan) = self.cache.popitem(last=False)
                self.cache_used -= old_plan[1][""]
        return self._launch(arena, plan, views=not cached)

    # -- the three steps that touch the GPU --------------------------------------------------------------------------------------
    def _grow(self, slot, total):
        self.slots[slot] = torch.empty(max(total + total // 4, 1 << 20), dtype=torch.uint8).pin_memory()

    def _upload(self, slot, total):
        """ONE copy of the packed slot into a fresh device arena; the event behind it guards the slot's next rewrite"""
        arena = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        arena[:total].copy_(self.slots[slot][:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        return arena

    def _launch(self, arena, plan, views):
        desc, offsets, specs, _ = plan
        base = arena.data_ptr()
        out, rows = {}, []
        for j, spec in enumerate(specs):
            dt = _TORCH_DTYPES[spec["dtype"]]
            n_out = int(desc[j, 2])
            if views and spec["alias"]:
                off = offsets[spec["stored"]]
                out[spec["name"]] = arena[off:off + n_out * np.dtype(spec["dtype"]).itemsize].view(dt).view(spec["shape"])
                continue
            t = torch.empty(spec["shape"], dtype=dt, device=self.device)
            out[spec["name"]] = t
            row = desc[j].copy()
            row[0] += base
            row[1] = t.data_ptr()
            rows.append(row)
        if rows:
            nv.ingest_group(np.stack(rows), self.device)
            self.stats["launches"] += 1
        return out

    def close(self):
        if self.pending is not None:
            self._drop_pending()
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None


class FragmentList(Sequence):
    """The `fragment_list` of prepare_test_data (defaults.py:160-182) built lazily: fragment p is gathered and post-transformed on
    access and not kept (the shipped lists collect the 768-wide lang_feat per fragment: all fragments of a large scene at once would
    not fit).  Order: aug 0's fragments, then aug 1's, ..."""

    def __init__(self, parts, keys, return_grid_coord, post_transform):
        self.parts, self.keys, self.return_grid_coord, self.post = parts, tuple(keys), return_grid_coord, post_transform
        self.bounds = np.cumsum([0] + [p[1]["index"].shape[0] for p in parts])

    def __len__(self):
        return int(self.bounds[-1])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        a = int(np.searchsorted(self.bounds, i, side="right")) - 1
        data, vox = self.parts[a]
        idx = vox["index"][i - int(self.bounds[a])]
        idx32 = idx.to(torch.int32).contiguous()
        part = dict(index=idx)
        if self.return_grid_coord:
            part["grid_coord"] = vox["grid_coord"]       # (members of a voxel share it: the same rows for every fragment)
        for k, v in data.items():
            part[k] = gt.take_rows(v, idx32) if k in self.keys else v
        return self.post(part)


# ---- the dataset classes -------------------------------------------------------------------------------------------------------------
@DATASETS.register_module()
class DefaultDataset:
    """defaults.py:15-192 with device samples.  Extension keywords: device, seed (of this package's Compose), cache_bytes, prefetch,
    tail_classes (the ids `sample_tail_classes` selects), class2id (an array or a text file of ids; set only when given)."""
    VALID_ASSETS = ["coord", "color", "normal", "strength", "segment", "instance", "pose"]
    EVAL_PC_ASSETS = []
    FILL = ("segment", "instance")       # keys filled with -1 over coord's rows when absent
    MULTILABEL_RAISES = False            # (only ScanNet++ looks at `multilabel`, and refuses it)
    _next = None

    def __init__(self, split="train", data_root="data/dataset", transform=None, test_mode=False, test_cfg=None, cache=False,
                 ignore_index=-1, loop=1, sample_tail_classes=False, filtered_scene=None, device="cuda", seed=None, cache_bytes=0,
                 prefetch=True, tail_classes=None, class2id=None, is_train=True, multilabel=False):
        if cache:
            raise NotImplementedError("cache=True (the reference's shared_dict) is not supported: use cache_bytes=<device bytes> for the scene cache")
        self.data_root, self.split = data_root, split
        self.seed = seed
        self.transform = Compose(transform, seed=seed)
        self.cache = False
        self.ignore_index = ignore_index
        self.loop = loop if not test_mode else 1
        self.test_mode = test_mode
        self.test_cfg = test_cfg if test_mode else None
        self.sample_tail = sample_tail_classes
        self.is_train, self.multilabel = is_train, multilabel
        if sample_tail_classes and tail_classes is None:
            raise ValueError("sample_tail_classes=True needs tail_classes=<ids> (the id tables are not part of this package)")
        self.tail_classes = None if tail_classes is None else np.asarray(tail_classes).reshape(-1)
        if class2id is not None:
            self.class2id = np.loadtxt(class2id, dtype=np.int64).reshape(-1) if isinstance(class2id, (str, os.PathLike)) else np.asarray(class2id)
        self.device = torch.device(device)
        self.stats = {}
        self.stager = SceneStager(self.device, cache_bytes=cache_bytes, prefetch=prefetch, stats=self.stats)
        if test_mode:
            vox = _cfg_get(self.test_cfg, "voxelize")
            if vox is not None:
                if _cfg_get(vox, "type", "GridSample") != "GridSample" or _cfg_get(vox, "mode", "test") != "test":
                    raise NotImplementedError("test_cfg.voxelize: GridSample(mode='test')")
                for k in ("return_min_coord", "return_displacement", "project_displacement", "return_inverse"):
                    if _cfg_get(vox, k):
                        raise NotImplementedError(f"test_cfg.voxelize: {k} has no device form")
            self.test_voxelize = vox          # read by prepare_test_data: mode "test" stays unregistered in TRANSFORMS
            if _cfg_get(self.test_cfg, "crop") is not None:
                raise NotImplementedError("test_cfg.crop is not supported (no shipped config sets it)")
            self.test_crop = None
            self.post_transform = Compose(_cfg_get(self.test_cfg, "post_transform"), seed=seed)
            self.aug_transform = [Compose(aug, seed=seed) for aug in _cfg_get(self.test_cfg, "aug_transform")]
        self.data_list = self.get_data_list(filtered_scene=filtered_scene)

    # -- the list --------------------------------------------------------------------------------------------------------------
    def get_data_list(self, filtered_scene=None):
        if isinstance(self.split, str):
            data_list = glob.glob(os.path.join(self.data_root, self.split, "*"))
        elif isinstance(self.split, Sequence):
            data_list = []
            for split in self.split:
                data_list += glob.glob(os.path.join(self.data_root, split, "*"))
        else:
            raise NotImplementedError
        if filtered_scene is not None:
            data_list = [d for d in data_list if os.path.basename(d).split("_")[0] not in filtered_scene]
        return data_list

    def get_data_name(self, idx):
        return os.path.basename(self.data_list[idx % len(self.data_list)])

    def __len__(self):
        return len(self.data_list) * self.loop

    # -- one scene -------------------------------------------------------------------------------------------------------------
    def asset_names(self, path):
        keep = set(self.VALID_ASSETS) | (set() if self.is_train else set(self.EVAL_PC_ASSETS))
        return [a[:-4] for a in sorted(os.listdir(path)) if a.endswith(".npy") and a[:-4] in keep]

    def rules(self, arrays):
        """{stored name: rule of native.ingest_plan} for the assets at hand (defaults.py:103-124)"""
        return dict(coord=_F32, color=_F32, normal=_F32, segment=_I32_FLAT, instance=_I32_FLAT)

    def finish(self, data_dict, idx):
        """what the reference does after the casts (fills, la_file, tail classes)"""
        for k in self.FILL:
            if k not in data_dict:
                data_dict[k] = torch.full((data_dict["coord"].shape[0],), -1, dtype=torch.int32, device=self.device)
        return data_dict

    def _path(self, idx):
        return self.data_list[idx % len(self.data_list)]

    def prefetch(self, idx):
        """hint from the loader: sample idx is the next one of the sampler's order (read and packed by the worker thread)"""
        path = self._path(idx)
        if self.device.type == "cuda" and self.stager.prefetch:
            self.stager.announce(path, self.asset_names(path), self.rules)

    def set_next(self, idx):
        """the sample to prefetch as soon as the coming get_data has taken its own out of the staging slot (None: nothing)"""
        self._next = idx

    def get_data(self, idx):
        if self.multilabel and self.MULTILABEL_RAISES:
            raise NotImplementedError
        if self.device.type != "cuda":
            raise RuntimeError("datasets: samples are built on the GPU (device='cuda'); there is no CPU fallback")
        path = self._path(idx)
        data_dict = self.stager.fetch(path, self.asset_names(path), self.rules)
        nxt, self._next = self._next, None
        if nxt is not None:
            self.prefetch(nxt)                         # the worker reads while this sample's transforms run
        data_dict["name"] = self.get_data_name(idx)
        return self.finish(data_dict, idx)

    # -- modes -----------------------------------------------------------------------------------------------------------------
    def prepare_train_data(self, idx):
        return self.transform(self.get_data(idx))

    def prepare_test_data(self, idx):
        """defaults.py:136-183"""
        data_dict = self.transform(self.get_data(idx))
        result_dict = dict(segment=data_dict.pop("segment", None), name=data_dict.pop("name", None))
        for k in ("coord", "pc_coord", "pc_segment"):
            if k in data_dict:
                result_dict[k] = data_dict[k]
        for k in ("origin_coord", "origin_feat_mask", "origin_instance"):
            if k in data_dict:
                result_dict[k] = data_dict.pop(k)
        if "origin_segment" in data_dict:
            assert "inverse" in data_dict
            result_dict["origin_segment"] = data_dict.pop("origin_segment")
            result_dict["inverse"] = data_dict.pop("inverse")
        parts = []
        vox = self.test_voxelize
        for aug in self.aug_transform:
            # the reference deep-copies the dict per aug; here only what an op may update in place is cloned, the float32 tensors
            # (transform.py's contract): labels, masks and the fp16 lang_feat -- the bulk of a scene -- are shared between the augs
            data = aug({k: (v.clone() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in data_dict.items()})
            if vox is not None:
                if "pc_coord" in data and _cfg_get(vox, "apply_to_pc", True):       # transform.py:1224-1260
                    chosen = gt.grid_sample_pc(data["pc_coord"], _cfg_get(vox, "grid_size", 0.05), data.get("pc_segment"))
                    data["pc_coord"] = data["pc_coord"][chosen]
                    if "pc_segment" in data:
                        data["pc_segment"] = data["pc_segment"][chosen]
                frag = gt.grid_sample_test(data["coord"], _cfg_get(vox, "grid_size", 0.05))
            else:
                n = data["coord"].shape[0]
                frag = dict(index=torch.arange(n, device=self.device).unsqueeze(0), grid_coord=None)
            parts.append((data, frag))
        keys = _cfg_get(vox, "keys", ("coord", "color", "normal", "segment")) if vox is not None else ()
        result_dict["fragment_list"] = FragmentList(parts, keys, bool(vox is not None and _cfg_get(vox, "return_grid_coord", False)),
                                                    self.post_transform)
        return result_dict

    def __getitem__(self, idx):
        return self.prepare_test_data(idx) if self.test_mode else self.prepare_train_data(idx)


class _GSDataset(DefaultDataset):
    """what the Gaussian-splat classes share: the float assets, opacity as a column, the scale clip, lang_feat / valid_feat_mask"""
    SCALE_CLIP = (0.0, 1.5)
    OPACITY_LO = None
    FILL = ()

    def rules(self, arrays):
        r = {k: _F32 for k in ("coord", "pc_coord", "color", "normal", "quat", "sh")}
        r["opacity"] = dict(dtype="float32", shape="col1", lo=self.OPACITY_LO)
        r["scale"] = dict(dtype="float32", lo=self.SCALE_CLIP[0], hi=self.SCALE_CLIP[1])
        r["lang_feat"] = dict(dtype="float16")
        r["valid_feat_mask"] = dict(dtype="bool")
        return r


@DATASETS.register_module()
class ScanNetGSDataset(_GSDataset):
    """scannetgs.py:18-167"""
    VALID_ASSETS = ["coord", "color", "normal", "segment20", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask",
                    "pc_instance"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment20"]
    FILL = ("segment", "instance")

    def __init__(self, lr_file=None, la_file=None, sample_tail=False, is_train=True, **kwargs):
        self.lr = np.loadtxt(lr_file, dtype=str).reshape(-1) if lr_file is not None else None
        self.la = torch.load(la_file, weights_only=False) if la_file is not None else None
        super().__init__(is_train=is_train, **kwargs)       # (sample_tail is accepted and, as in the reference, overwritten by
        #                                                      sample_tail_classes; this class never reads either)

    def get_data_list(self, filtered_scene=None):
        if self.lr is None:
            return super().get_data_list(filtered_scene=filtered_scene)
        return [os.path.join(self.data_root, "train", str(name)) for name in self.lr]

    def rules(self, arrays):
        r = super().rules(arrays)
        seg = "segment20" if "segment20" in arrays else "segment200"
        r[seg] = dict(_I32_FLAT, name="segment")
        pc = "pc_segment20" if "pc_segment20" in arrays else "pc_segment200"
        r[pc] = dict(_I32_FLAT, name="pc_segment")
        r["instance"] = _I32_FLAT
        return r

    def finish(self, data_dict, idx):
        data_dict = super().finish(data_dict, idx)
        if self.la:                                    # scannetgs.py:155-160 (a rare path: plain torch ops)
            sampled_index = torch.as_tensor(np.asarray(self.la[self.get_data_name(idx)])).to(self.device)
            mask = torch.ones_like(data_dict["segment"], dtype=torch.bool)
            mask[sampled_index.long()] = False
            data_dict["segment"][mask] = self.ignore_index
            data_dict["sampled_index"] = sampled_index
        return data_dict


@DATASETS.register_module()
class ScanNet200GSDataset(ScanNetGSDataset):
    VALID_ASSETS = ["coord", "color", "normal", "segment200", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask",
                    "pc_instance"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment200"]


@DATASETS.register_module()
class ScanNetPPGSDataset(_GSDataset):
    """scannetppgs.py:10-165"""
    VALID_ASSETS = ["coord", "color", "segment", "segment200", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask",
                    "normal"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment", "pc_instance"]
    FILL = ("segment", "instance")
    MULTILABEL_RAISES = True

    def __init__(self, multilabel=False, is_train=True, **kwargs):
        super().__init__(multilabel=multilabel, is_train=is_train, **kwargs)

    def rules(self, arrays):
        r = super().rules(arrays)
        r["pc_segment"] = dict(dtype="int32", shape="column", column=0)
        if "segment" in arrays:
            r["segment"] = dict(dtype="int32", shape="column", column=0)      # (segment200, if stored as well, stays as stored)
        else:
            r["segment200"] = dict(_I32_FLAT, name="segment")
        r["instance"] = dict(dtype="int32", shape="column_or_flat", column=0)
        return r

    def finish(self, data_dict, idx):
        data_dict = super().finish(data_dict, idx)
        if self.sample_tail:                           # scannetppgs.py:161-164
            tail = torch.as_tensor(self.tail_classes, device=self.device).to(data_dict["segment"].dtype)
            data_dict["sampled_index"] = torch.nonzero(torch.isin(data_dict["segment"], tail)).reshape(-1)
        return data_dict


@DATASETS.register_module()
class Matterport3DGSDataset(_GSDataset):
    """matterport3dgs.py:10-121"""
    VALID_ASSETS = ["coord", "color", "segment", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask", "normal"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment"]
    FILL = ("segment",)

    def __init__(self, multilabel=False, is_train=True, **kwargs):
        super().__init__(multilabel=multilabel, is_train=is_train, **kwargs)

    def rules(self, arrays):
        r = super().rules(arrays)
        r["segment" if "segment" in arrays else "segment_nyu_160"] = dict(_I32_FLAT, name="segment")
        r["pc_segment" if "pc_segment" in arrays else "pc_segment_nyu_160"] = dict(_I32_FLAT, name="pc_segment")
        return r


@DATASETS.register_module()
class Matterport3D_160_GSDataset(Matterport3DGSDataset):
    VALID_ASSETS = ["coord", "color", "segment_nyu_160", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask", "normal"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment_nyu_160"]


@DATASETS.register_module()
class HoliCityGSDataset(_GSDataset):
    """holicitygs.py:10-102"""
    VALID_ASSETS = ["coord", "color", "segment", "instance", "quat", "scale", "opacity", "lang_feat", "valid_feat_mask", "normal"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment", "pc_instance"]
    SCALE_CLIP = (1e-4, 1.0)
    OPACITY_LO = 0.001

    def __init__(self, multilabel=False, is_train=True, **kwargs):
        super().__init__(multilabel=multilabel, is_train=is_train, **kwargs)

    def rules(self, arrays):
        r = super().rules(arrays)
        r["pc_segment"] = dict(dtype="int32")
        r["segment"] = _I32_FLAT
        return r


@DATASETS.register_module()
class KITTI360GSDataset(HoliCityGSDataset):
    """kitti360_gs.py:10-104: coord and scale are divided by 10 after the cast and before the clip (two small torch ops)"""
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment"]
    SCALE_CLIP = (None, None)

    def finish(self, data_dict, idx):
        # a device divisor: a Python scalar would turn the division into a multiplication by 0.1, one ulp off numpy's quotient
        ten = torch.full((), 10.0, dtype=torch.float32, device=self.device)
        if "coord" in data_dict:
            data_dict["coord"].div_(ten)
        if "scale" in data_dict:
            data_dict["scale"] = data_dict["scale"].div_(ten).clamp_(0.01, 10.0)
        return super().finish(data_dict, idx)


@DATASETS.register_module()
class GenericGSDataset(HoliCityGSDataset):
    """generic_gs.py:10-85"""
    VALID_ASSETS = ["coord", "color", "segment", "quat", "scale", "opacity"]
    EVAL_PC_ASSETS = ["pc_coord", "pc_segment", "pc_instance"]


@DATASETS.register_module()
class ConcatDataset:
    """defaults.py:195-235"""
    _next = None

    def __init__(self, datasets, loop=1):
        self.datasets = [build_dataset(d) if isinstance(d, dict) else d for d in datasets]
        self.loop = loop
        self.data_list = self.get_data_list()

    def get_data_list(self):
        return [(i, j) for i, d in enumerate(self.datasets) for j in range(len(d))]

    def _where(self, idx):
        dataset_idx, data_idx = self.data_list[idx % len(self.data_list)]
        return int(dataset_idx), int(data_idx)

    def get_data(self, idx):
        i, j = self._where(idx)
        out = self.datasets[i][j]
        nxt, self._next = self._next, None
        if nxt is not None:
            self.prefetch(nxt)
        return out

    def get_data_name(self, idx):
        i, j = self._where(idx)
        return self.datasets[i].get_data_name(j)

    def prefetch(self, idx):
        i, j = self._where(idx)
        if hasattr(self.datasets[i], "prefetch"):
            self.datasets[i].prefetch(j)

    def set_next(self, idx):
        self._next = idx

    def __getitem__(self, idx):
        return self.get_data(idx)

    def __len__(self):
        return len(self.data_list) * self.loop


# ---- loaders -------------------------------------------------------------------------------------------------------------------------
class _EpochSampler:
    """range(len) or, with shuffle, a seeded torch.Generator permutation per epoch (the single-process sampler)"""

    def __init__(self, n, shuffle, seed):
        self.n, self.shuffle, self.seed, self.epoch = n, shuffle, 0 if seed is None else int(seed), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n

    def __iter__(self):
        if not self.shuffle:
            return iter(range(self.n))
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        return iter(torch.randperm(self.n, generator=g).tolist())


class DeviceLoader:
    """A sized iterable of batches of device samples.  sampler: any iterable of indices with a length; default:
    torch.utils.data.DistributedSampler when get_world_size() > 1 (the reference's indices; set_epoch as Trainer.train calls it),
    else range / a seeded permutation that advances with every epoch.  collate: list of samples -> batch (default: point_collate)."""

    def __init__(self, dataset, batch_size=1, sampler=None, shuffle=False, drop_last=False, collate=None, seed=None):
        self.dataset, self.batch_size, self.drop_last = dataset, int(batch_size), bool(drop_last)
        self.collate = collate if collate is not None else gt.point_collate
        self._auto_epoch = False
        if sampler is None:
            if get_world_size() > 1:
                from torch.utils.data import DistributedSampler
                sampler = DistributedSampler(dataset, num_replicas=get_world_size(), rank=get_rank(), shuffle=shuffle,
                                             seed=0 if seed is None else int(seed))
            else:
                sampler = _EpochSampler(len(dataset), shuffle, seed)
                self._auto_epoch = shuffle
        self.sampler = sampler

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def indices(self):
        """the sample indices of the coming epoch, batch by batch"""
        order = list(iter(self.sampler))
        batches = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        if self.drop_last and batches and len(batches[-1]) < self.batch_size:
            batches.pop()
        return batches

    def __iter__(self):
        batches = self.indices()
        if self._auto_epoch:
            self.sampler.set_epoch(self.sampler.epoch + 1)     # (under DDP Trainer.train sets the epoch itself)
        # the dataset is told which sample follows: it hands that index to its worker thread as soon as the current sample has left
        # the staging slot.  The order of samples is the sampler's, whatever the worker does.
        flat = [i for b in batches for i in b]
        set_next = getattr(self.dataset, "set_next", None)
        pos = 0
        for b in batches:
            samples = []
            for i in b:
                pos += 1
                if set_next is not None:
                    set_next(flat[pos] if pos < len(flat) else None)
                samples.append(self.dataset[i])
            yield self.collate(samples)


def _identity_collate(batch):
    return batch


def _mix_collate(mix_prob):
    def collate(samples):
        return gt.point_collate(samples, mix_prob)
    return collate


def _seeded(dcfg, seed):
    """the dataset dict with the transform seed of its loader, unless it names one"""
    dcfg = dict(dcfg)
    if seed is None:
        return dcfg
    if dcfg.get("type") == "ConcatDataset":
        dcfg["datasets"] = [_seeded(d, seed) if isinstance(d, dict) else d for d in dcfg["datasets"]]
    else:
        dcfg.setdefault("seed", int(seed))
    return dcfg


def build_train_loader(cfg):
    """cfg: the config mapping (data["train"], batch_size_per_gpu, mix_prob, seed [, train["type"], num_worker_per_gpu: ignored]).
    A ConcatDataset under train.type == "MultiDatasetTrainer" -> engine.MultiDatasetLoader with the semantics of
    datasets/dataloader.py:23-102; anything else -> one shuffling DeviceLoader with drop_last."""
    dcfg = cfg["data"]["train"]
    bs = int(cfg.get("batch_size_per_gpu", cfg.get("batch_size", 1)))
    mix_prob, seed = cfg.get("mix_prob", 0), cfg.get("seed")
    multi = _cfg_get(cfg.get("train"), "type") == "MultiDatasetTrainer" and dcfg.get("type") == "ConcatDataset"
    if not multi:
        worker_seed = None if seed is None else get_rank() + int(seed)         # _worker_init_fn with one worker and one dataset
        return DeviceLoader(build_dataset(_seeded(dcfg, worker_seed)), bs, shuffle=True, drop_last=True, collate=_mix_collate(mix_prob),
                            seed=seed)
    subs = list(dcfg["datasets"])
    nd = len(subs)
    concat = ConcatDataset([build_dataset(_seeded(d, None if seed is None else nd * get_rank() + j + int(seed))) for j, d in enumerate(subs)],
                           loop=dcfg.get("loop", 1))
    ratios = [int(d.loop) for d in concat.datasets]
    for d in concat.datasets:
        d.loop = 1                                     # the original loops serve as ratios
    concat.datasets[0].loop = concat.loop              # the main dataset defines the epoch
    loaders = [DeviceLoader(d, bs, shuffle=True, drop_last=True, collate=_mix_collate(mix_prob), seed=seed) for d in concat.datasets]
    return MultiDatasetLoader(loaders, ratios)


def build_val_loader(cfg):
    """data["val"]: one dict -> one loader, a list -> a list (batch_size_val_per_gpu, no shuffle, point_collate without Mix3D)"""
    dval = cfg["data"]["val"]
    bs = int(cfg.get("batch_size_val_per_gpu", cfg.get("batch_size_val", 1)))
    seed = cfg.get("seed")

    def one(d):
        return DeviceLoader(build_dataset(_seeded(d, seed)), bs, shuffle=False, drop_last=False, collate=_mix_collate(0))
    return [one(d) for d in dval] if isinstance(dval, (list, tuple)) else one(dval)


def build_test_loader(cfg, index=None):
    """data["test"] (entry `index` of a list) -> a loader with the tester's identity collate (batch_size_test_per_gpu)"""
    dtest = cfg["data"]["test"]
    if index is not None:
        dtest = dtest[index]
    bs = int(cfg.get("batch_size_test_per_gpu", cfg.get("batch_size_test", 1)))
    return DeviceLoader(build_dataset(_seeded(dtest, cfg.get("seed"))), bs, shuffle=False, drop_last=False, collate=_identity_collate)
