"""The labelled point cloud of the original scene, attached to the GS scene folders and chunk folders: the files the dataset classes
list as EVAL_PC_ASSETS (`pc_coord.npy`, `pc_segment*.npy`, `pc_instance.npy`) and the validation / test lists of the lang-pretrain
configs collect.  It is the step between `chunk_split` and the loaders.

Mirror of pointcept/datasets/preprocessing/adding_pc_label_to_gs_chunk.py: `copy_scene_level`, `build_chunks`, `SceneCache.slice`
(the cloud rows that are among the k nearest of some Gaussian of the chunk AND within `dist_limit` of it, in ascending row order)
and `semseg_label_slice` (per Gaussian the label of its nearest cloud row, -1 beyond the limit), with the same file names.

    chunk coord.npy x nc --concatenate--> q (m, 3), q_offset        scene coord.npy + segment*.npy --one packed upload--> arena
      -> ONE pointops.knn_query(k, pc, [M], q, [m]) per batch       (the grid over the cloud is built once per batch; a scene that
                                                                     fits one batch builds it once: the reference's one tree per scene)
      -> ss_pc_mark: fp64 distance test, bitmap (nc, ceil(M / 32)) by integer OR, nearest row per Gaussian
      -> ss_pc_compact_scan / ss_pc_compact: the set bits in ascending order = np.unique without a sort; ONE (nc) counts read per batch
      -> grouped gather of (chunk, asset) problems into a staging buffer --one download per batch--> views / np.save

Deviations from the reference:
* the neighbours are SELECTED with this package's fp32 distance and the smaller-index tie rule of `knn_query`; scipy's cKDTree
  selects in fp64 with an unspecified tie order.  The two differ only where two candidates lie within fp32 rounding of each other
  across the k-th place (or, for the nearest label, the first);
* the `dist_limit` DECISION is made in fp64 from the fp32 coordinates, as numpy makes it: d = sqrt(dx * dx + dy * dy + dz * dz) with
  dx = (double)qx - (double)px, the squares added in x, y, z order, no fused multiply-add;
* the reference edits constants in the file; here they are arguments (and a command line);
* `coord` arrays must be (n, 3) float32 (what every converter writes); every other asset keeps its dtype and trailing shape.
There is no CPU path: the search, the distance test, the compaction and the gather run on the GPU."""
import argparse
import glob
import os
import shutil
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

from .. import native as nv
from .. import pointops
from . import preprocessing as pre

SCENE_SPLITS = ("train", "val", "test")
PROFILE = None          # a dict while scripts/bench_pc_attach.py measures: seconds per stage (each stage then ends with a synchronize)


class _Stage:
    def __init__(self, key, device_work=True):
        self.key, self.device_work = key, device_work

    def __enter__(self):
        if PROFILE is not None:
            if self.device_work:
                torch.cuda.synchronize()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if PROFILE is not None:
            if self.device_work:
                torch.cuda.synchronize()
            PROFILE[self.key] = PROFILE.get(self.key, 0.0) + time.perf_counter() - self.t0


# ---- names (pure host: tests/test_pc_attach_host.py) ------------------------------------------------------------------------------------
def is_chunk_subdir(name):
    """a chunked split folder of gs_root (`val_grid1.0cm_chunk6x6_stride3x3`), not a filtered copy of one"""
    return "chunk" in name and "filtered" not in name


def split_from_subdir(name):
    for s in SCENE_SPLITS:
        if name.startswith(s):
            return s
    raise ValueError(f"cannot infer the split (train / val / test) from '{name}'")


def scene_and_chunk(dir_name):
    """`<scene>_<chunk number>` -> (scene, chunk number); scene names contain underscores themselves"""
    scene, chunk = dir_name.rsplit("_", 1)
    return scene, chunk


def segment_files(scene_dir):
    """{stem: path} of the segment*.npy of an original scene folder, sorted by name"""
    return OrderedDict((os.path.basename(p)[:-4], p) for p in sorted(glob.glob(os.path.join(scene_dir, "segment*.npy"))))


def _report_missing(path):
    print(f"original scene missing: {path}", file=sys.stderr)


# ---- the slice ----------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes):
    return -(-nbytes // pre.STAGE_ALIGN) * pre.STAGE_ALIGN


def _as_rows(a, name):
    """a numpy array, or a device tensor; a tensor that is not on the GPU is refused"""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise RuntimeError(f"{name}: slice_point_cloud needs a GPU tensor or a numpy array (no CPU fallback)")
        return a.contiguous()
    return np.ascontiguousarray(a)


def _check_coord(a, name):
    dt = a.dtype
    if a.ndim != 2 or a.shape[1] != 3 or dt not in (np.float32, torch.float32):
        raise ValueError(f"{name}: must be (n, 3) float32, got {tuple(a.shape)} {dt}")


def _numpy_dtype(t):
    return np.dtype(str(t.dtype).replace("torch.", ""))


def _cloud_arena(pc_coord, pc_assets, dev):
    """-> (keep-alive list, coord tensor (M, 3) f32 on dev, [(name, device address, numpy dtype, trailing shape, row_bytes)] with
    "pc_coord" first).  numpy inputs travel in ONE packed upload; device tensors are used where they lie."""
    M = pc_coord.shape[0]
    entries, keep, host = [], [], OrderedDict()
    for name, a in [("pc_coord", pc_coord)] + list(pc_assets.items()):
        if isinstance(a, torch.Tensor):
            a = a.to(dev)
            keep.append(a)
            entries.append([name, a.data_ptr(), _numpy_dtype(a), tuple(a.shape[1:]), a.numel() * a.element_size() // M])
        else:
            host[name] = a
            entries.append([name, None, a.dtype, tuple(a.shape[1:]), a.nbytes // M])
    if host:
        arena, offsets, _ = pre._upload(host, M, dev)
        keep.append(arena)
        for e in entries:
            if e[1] is None:
                e[1] = arena.data_ptr() + offsets[e[0]]
    coord = keep[0] if isinstance(pc_coord, torch.Tensor) else pre._typed(arena, offsets["pc_coord"], M * 12, torch.float32, (M, 3))
    return keep, coord, [tuple(e) for e in entries]


def chunk_batches(rows_per_chunk, M, k, assets, nearest, workspace_bytes):
    """[[chunk numbers]] in order: a batch's bitmap, idx / dist, query rows, nearest rows and staging buffer (bounded by
    min(M, rows * k) cloud rows per chunk) stay within workspace_bytes, and within the int32 limits of the kernels."""
    words = -(-M // 32)
    row_bytes = sum(a[4] for a in assets)
    near_bytes = sum(a[4] for a in assets if a[0] in nearest)
    batches, cur, used, pairs = [], [], 0, 0
    for c, m_c in enumerate(rows_per_chunk):
        stage = sum(_aligned(min(M, m_c * k) * a[4]) for a in assets) + sum(_aligned(m_c * a[4]) for a in assets if a[0] in nearest)
        cost = words * 4 + m_c * (8 * k + 12 + 4) + stage
        if cost > workspace_bytes:
            raise ValueError(f"slice_point_cloud: workspace_bytes={workspace_bytes} is smaller than one chunk needs ({cost} bytes: "
                             f"{m_c} Gaussians, k={k}, {row_bytes} + {near_bytes} bytes per row)")
        if cur and (used + cost > workspace_bytes or (pairs + m_c * k) >= 2 ** 31 or (len(cur) + 1) * words * 32 >= 2 ** 31):
            batches.append(cur)
            cur, used, pairs = [], 0, 0
        cur.append(c)
        used += cost
        pairs += m_c * k
    if cur:
        batches.append(cur)
    return batches


def slice_point_cloud(chunk_coords, pc_coord, pc_assets, k_neighbors=16, dist_limit=0.25, nearest_assets=(), workspace_bytes=1 << 30,
                      device=None):
    """SceneCache.slice (and semseg_label_slice) of the reference for all chunks of one scene (module docstring).
    chunk_coords: a list of (m_c, 3) float32 Gaussian centres; pc_coord (M, 3) float32; pc_assets {name: (M, ...) array of any dtype};
    numpy arrays or GPU tensors.  nearest_assets: names of pc_assets (signed integer dtypes) whose per-Gaussian nearest label is wanted.
    -> (slices, labels): slices[c] = (pc_coord rows (r_c, 3) float32, {name: rows}) with the cloud rows ascending; labels[c] =
    {name: (m_c, ...) labels of the nearest cloud row, -1 beyond dist_limit} for nearest_assets.  numpy arrays in the assets' dtypes.
    The arrays of one batch are views of that batch's pinned download buffer (np.save writes straight from it): the buffer lives as
    long as any of them, so `.copy()` a slice that is to outlive the rest.
    The result does not depend on workspace_bytes (how the chunks fall into batches)."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("slice_point_cloud: the point cloud is sliced on the GPU (device='cuda'); there is no CPU fallback")
    chunk_coords = [_as_rows(c, f"chunk_coords[{i}]") for i, c in enumerate(chunk_coords)]
    pc_coord = _as_rows(pc_coord, "pc_coord")
    pc_assets = OrderedDict((n, _as_rows(a, n)) for n, a in pc_assets.items())
    _check_coord(pc_coord, "pc_coord")
    for i, c in enumerate(chunk_coords):
        _check_coord(c, f"chunk_coords[{i}]")
    M = pc_coord.shape[0]
    if M < 1:
        raise ValueError("slice_point_cloud: pc_coord has no rows")
    if "pc_coord" in pc_assets:
        raise ValueError("slice_point_cloud: 'pc_coord' is the cloud itself, not an asset")
    for n, a in pc_assets.items():
        if a.ndim == 0 or a.shape[0] != M:
            raise ValueError(f"slice_point_cloud: asset '{n}' has leading dimension {a.shape[0] if a.ndim else None}, pc_coord has {M}")
    nearest_assets = tuple(nearest_assets)
    for n in nearest_assets:
        if n not in pc_assets:
            raise ValueError(f"slice_point_cloud: nearest asset '{n}' is not among pc_assets")
        dt = np.dtype(_numpy_dtype(pc_assets[n]) if isinstance(pc_assets[n], torch.Tensor) else pc_assets[n].dtype)
        if dt.kind != "i":
            raise ValueError(f"slice_point_cloud: nearest asset '{n}' must have a signed integer dtype (-1 marks no label), got {dt}")
    k = min(int(k_neighbors), M)
    if k < 1:
        raise ValueError("slice_point_cloud: k_neighbors must be at least 1")
    slices, labels = [None] * len(chunk_coords), [None] * len(chunk_coords)
    with torch.cuda.device(dev):
        dev = torch.device("cuda", torch.cuda.current_device())
        with _Stage("upload"):
            keep, cloud, assets = _cloud_arena(pc_coord, pc_assets, dev)
        cloud_off = torch.tensor([M], dtype=torch.int32, device=dev)
        for batch in chunk_batches([c.shape[0] for c in chunk_coords], M, k, assets, nearest_assets, int(workspace_bytes)):
            _slice_batch(batch, chunk_coords, cloud, cloud_off, assets, k, float(dist_limit), nearest_assets, dev, slices, labels)
    return slices, labels


def _slice_batch(batch, chunk_coords, cloud, cloud_off, assets, k, dist_limit, nearest_assets, dev, slices, labels):
    M, nc = cloud.shape[0], len(batch)
    q_off = np.zeros(nc + 1, dtype=np.int64)
    q_off[1:] = np.cumsum([chunk_coords[c].shape[0] for c in batch])
    m = int(q_off[-1])
    with _Stage("upload"):
        parts = [chunk_coords[c] for c in batch]
        if all(isinstance(p, np.ndarray) for p in parts):
            q = torch.from_numpy(np.concatenate(parts, axis=0) if parts else np.empty((0, 3), np.float32)).to(dev)
        else:
            q = torch.cat([p.to(dev) if isinstance(p, torch.Tensor) else torch.from_numpy(p).to(dev) for p in parts], dim=0)
        q = q.contiguous()
        q_offset = torch.from_numpy(q_off.astype(np.int32)).to(dev)
    with _Stage("search"):
        if m > 0:
            idx, _ = pointops.knn_query(k, cloud, cloud_off, q, q_offset[-1:])
        else:
            idx = torch.empty((0, k), dtype=torch.int32, device=dev)
    with _Stage("mark_compact"):
        bitmap, nearest, status = nv.pc_mark(cloud, q, q_offset, idx, dist_limit)
        tile_base, counts_d = nv.pc_compact_scan(bitmap, M)
        host = torch.cat([counts_d, status]).cpu().numpy()                 # the one read of the batch
        if host[-1]:
            raise nv._lib.NativeError("slice_point_cloud: the neighbour search returned a row index outside the cloud")
        counts = host[:nc].astype(np.int64)
        row_off = np.zeros(nc + 1, dtype=np.int64)
        row_off[1:] = np.cumsum(counts)
        rows = nv.pc_compact(bitmap, M, tile_base, int(row_off[-1]))
    with _Stage("gather"):
        # the staging buffer: per chunk its assets through `rows`, then the nearest labels of its Gaussians (prefilled with -1: the
        # grouped gather leaves the row of an index outside the table, here -1, unwritten)
        plan, used = [], 0                                                 # (chunk slot, asset, offset, rows, index address, fill)
        for s in range(nc):
            for a in assets:
                plan.append((s, a, used, int(counts[s]), rows.data_ptr() + 4 * int(row_off[s]), False))
                used += _aligned(int(counts[s]) * a[4])
        near_start = used
        for s in range(nc):
            m_s = int(q_off[s + 1] - q_off[s])
            for a in assets:
                if a[0] in nearest_assets:
                    plan.append((s, a, used, m_s, nearest.data_ptr() + 4 * int(q_off[s]), True))
                    used += _aligned(m_s * a[4])
        stage_d = torch.empty(max(used, 1), dtype=torch.uint8, device=dev)
        if used > near_start:
            stage_d[near_start:used].fill_(255)
        desc = np.array([(a[1], stage_d.data_ptr() + off, ip, n, a[4], 0, M, M) for _, a, off, n, ip, _ in plan if n > 0 and a[4] > 0],
                        dtype=np.int64).reshape(-1, 8)
        nv.chunk_gather_group(desc, dev)
    with _Stage("download"):
        stage_h = torch.empty(max(used, 1), dtype=torch.uint8).pin_memory()
        stage_h[:used].copy_(stage_d[:used], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        host_bytes = stage_h.numpy()
    out = [[None, OrderedDict(), OrderedDict()] for _ in range(nc)]
    for s, (name, _, dtype, trailing, row_bytes), off, n, _, is_label in plan:
        arr = host_bytes[off:off + n * row_bytes].view(dtype).reshape((n,) + tuple(trailing))
        if is_label:
            out[s][2][name] = arr
        elif name == "pc_coord":
            out[s][0] = arr
        else:
            out[s][1][name] = arr
    for s, c in enumerate(batch):
        slices[c], labels[c] = (out[s][0], out[s][1]), out[s][2]


# ---- folders -------------------------------------------------------------------------------------------------------------------------------
def copy_scene_level(gs_root, pc_root, splits=("val", "test")):
    """coord.npy -> pc_coord.npy, segment*.npy -> pc_segment*.npy (neither overwrites) and instance.npy -> pc_instance.npy for every
    scene folder of gs_root/<split>.  -> the scene folders written to"""
    done = []
    for split in splits:
        gs_split = os.path.join(gs_root, split)
        if not os.path.isdir(gs_split):
            continue
        for scene in sorted(os.listdir(gs_split)):
            scene_dir = os.path.join(gs_split, scene)
            if not os.path.isdir(scene_dir):
                continue
            src = os.path.join(pc_root, split, scene)
            if not os.path.isdir(src):
                _report_missing(src)
                continue
            pairs = [(os.path.join(src, "coord.npy"), os.path.join(scene_dir, "pc_coord.npy"))]
            pairs += [(p, os.path.join(scene_dir, f"pc_{stem}.npy")) for stem, p in segment_files(src).items()]
            for s, d in pairs:
                if not os.path.exists(d):
                    shutil.copy2(s, d)
            if os.path.exists(os.path.join(src, "instance.npy")):
                shutil.copy2(os.path.join(src, "instance.npy"), os.path.join(scene_dir, "pc_instance.npy"))
            done.append(scene_dir)
    return done


def chunk_dirs_by_scene(subdir):
    """{scene: [chunk directories of it, by chunk number]} of one chunked split folder"""
    scenes = {}
    for d in os.listdir(subdir):
        path = os.path.join(subdir, d)
        if os.path.isdir(path) and "_" in d:
            scene, chunk = scene_and_chunk(d)
            scenes.setdefault(scene, []).append(((0, int(chunk), "") if chunk.isdigit() else (1, 0, chunk), path))
    return OrderedDict((s, [p for _, p in sorted(scenes[s])]) for s in sorted(scenes))


def _load(path):
    with _Stage("read", device_work=False):
        return np.load(path)


def _save(path, arr):
    with _Stage("write", device_work=False):
        np.save(path, arr)


def attach_point_cloud(gs_root, pc_root, k_neighbors=16, dist_limit=0.25, write_semseg_label=False, scene_level=("val", "test"),
                       device=None, workspace_bytes=1 << 30):
    """build_chunks and copy_scene_level of the reference (module docstring).  gs_root: the preprocessed GS dataset (scene splits and
    chunked splits); pc_root: the original dataset, pc_root/<split>/<scene>/{coord, segment*, instance}.npy.  Every chunk directory
    gets pc_coord.npy and pc_<segment name>.npy; with write_semseg_label also <name>.npy (the label of each Gaussian's nearest cloud
    point) for the segment arrays whose name contains "nyu".  -> {scene: [chunk directories written]}"""
    written = OrderedDict()
    for sub in sorted(d for d in os.listdir(gs_root) if os.path.isdir(os.path.join(gs_root, d)) and is_chunk_subdir(d)):
        split = split_from_subdir(sub)
        for scene, dirs in chunk_dirs_by_scene(os.path.join(gs_root, sub)).items():
            src = os.path.join(pc_root, split, scene)
            if not os.path.isdir(src):
                _report_missing(src)
                continue
            pc_coord = _load(os.path.join(src, "coord.npy"))
            segments = OrderedDict((stem, _load(p)) for stem, p in segment_files(src).items())
            nearest = tuple(n for n in segments if "nyu" in n) if write_semseg_label else ()
            chunk_coords = [_load(os.path.join(d, "coord.npy")) for d in dirs]
            slices, labels = slice_point_cloud(chunk_coords, pc_coord, segments, k_neighbors, dist_limit, nearest, workspace_bytes, device)
            for d, (coord, segs), lab in zip(dirs, slices, labels):
                _save(os.path.join(d, "pc_coord.npy"), coord)
                for name, arr in segs.items():
                    _save(os.path.join(d, f"pc_{name}.npy"), arr)
                for name, arr in lab.items():
                    _save(os.path.join(d, f"{name}.npy"), arr)
            written.setdefault(scene, []).extend(dirs)
    copy_scene_level(gs_root, pc_root, tuple(scene_level or ()))
    return written


# ---- command line --------------------------------------------------------------------------------------------------------------------------
def build_parser():
    parser = argparse.ArgumentParser(description="Attach the labelled point cloud of the original scenes to GS scene and chunk folders "
                                                 "on the GPU (adding_pc_label_to_gs_chunk.py)")
    parser.add_argument("--gs_root", required=True, help="the preprocessed GS dataset: scene splits and chunked splits")
    parser.add_argument("--pc_root", required=True, help="the original dataset: <split>/<scene>/{coord, segment*, instance}.npy")
    parser.add_argument("--k_neighbors", default=16, type=int, help="neighbours of every Gaussian that are looked at")
    parser.add_argument("--dist_limit", default=0.25, type=float, help="largest distance (metres) of a kept neighbour")
    parser.add_argument("--write_semseg_label", action="store_true", help="also write the nearest-point label of every Gaussian (nyu segments)")
    parser.add_argument("--no_scene_level", action="store_true", help="skip the copy into the val / test scene folders")
    return parser


def main(argv=None):
    cfg = build_parser().parse_args(argv)
    done = attach_point_cloud(cfg.gs_root, cfg.pc_root, k_neighbors=cfg.k_neighbors, dist_limit=cfg.dist_limit,
                              write_semseg_label=cfg.write_semseg_label, scene_level=() if cfg.no_scene_level else ("val", "test"))
    for scene, dirs in done.items():
        print(f"{scene}: {len(dirs)} chunks")


if __name__ == "__main__":
    main()
