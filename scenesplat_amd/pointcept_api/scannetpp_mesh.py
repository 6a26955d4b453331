"""The ScanNet++ converter on the device: a raw scan (`scans/mesh_aligned_0.05.ply`, `segments.json`, `segments_anno.json`) -> the labelled
point-cloud folder (`coord`, `color`, `normal`, and for train / val `segment`, `instance`, both (n, 3) int16), and together with a 3DGS
checkpoint -> the GS scene folder the `configs/scannetpp/*` configs and `ScanNetPPGSDataset` read.

Mirror of pointcept/datasets/preprocessing/scannetpp/preprocess_scannetpp.py (`parse_scene` and its command line) and of
preprocess_scannetpp_gs.py (the Gaussians of a checkpoint: normals and labels of the nearest vertex of the point-cloud folder, the
language features with the half-valid rule): the same file names, dtypes, shapes and bytes.

    header (host) -> vertex and face blocks -> ss_mesh_decode_vertices / ss_mesh_decode_faces: `load_ply_mesh` of scannet_mesh.py, which
         takes the 15-byte `x y z red green blue` records as any other stride                                       (csrc/mesh.hip)
      -> ss_mesh_face_cross_f64, the stable radix argsort of the 3F corner entries by vertex, ss_pool_partition,
         ss_mesh_vertex_normals_f64: Open3D's `compute_vertex_normals(normalized=True)` as a sort and a walk       (csrc/scannetpp.hip)
      -> first_groups (host: the parsed json is host data) -> ss_spp_segment_hist -> ss_spp_group_sizes -> ss_spp_labels: the reference's
         sequential loop over `segGroups` (one `np.isin` pass over all vertices per object) as three launches, nothing read in between
      -> (GS) load_gaussian_ply, the hash-grid 1-NN, ss_gather_rows -> np.save

Values against the reference: `coord`, `color` (Open3D holds c / 255.0; `(c / 255.0 * 255).astype(uint8)` gives every byte back),
`segment` and `instance` are bit for bit the reference's.  `normal` is bit for bit the DEFINITION Open3D implements (fp64 vertices, the
unnormalised cross products of the incident faces added in face order, once per corner, a division by the fp64 norm where it is above
zero, one rounding to fp32), restated in numpy by tests/golden/make_golden_scannetpp.py: Open3D itself is not part of this package's
tests.  Deviations:
* the oriented-bounding-box pruning of preprocess_scannetpp_gs.py (open3d's `get_minimal_oriented_bounding_box` plus 25 cm) is the
  keyword `prune_box=0.25` (oriented_box.py): the box of least volume among the frames of ALL edges of the hull's triangles, where
  Open3D tries one edge per triangle in Qhull's vertex order; never larger than Open3D's.  The default None writes every Gaussian.
* the checkpoint arrays are `load_gaussian_ply`'s: the reference's ScanNet++ script computes `quat` and `color` through fp64
  intermediates, so last-bit differences are possible (counted on the fixture: profiles/scannetpp.md), and `scale` / `opacity` are what
  gaussian_ply.py documents.
* the nearest vertex is the fp32 hash-grid search's (equal distances: the lower row), the reference's an fp64 KD-tree's.
* `filter_map_classes` / `map_benchmark.csv` are left out: the reference computes the remapped label and never writes it; the label
  index is `class2idx.get(<the original label>, ignore_index)`.
* the checkpoint folder is the first in sorted order among the folders under gs_root whose name ends with the scene name (the
  reference: the first in listing order).
* a scene that cannot be read is reported and skipped without leaving a folder; `feat_only` reads no checkpoint.
* Open3D turns a NaN normal into (0, 0, 1); coordinates that are not finite are kept as they come out of the arithmetic.

Only triangle meshes whose `x`, `y`, `z` are float32 at 4-byte offsets and whose colours are uchar have a device form; anything else is a
ValueError, never a host fallback."""
import argparse
import json
import os
import warnings
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from .. import native as nv
from .gaussian_ply import GS_ASSETS, _gather_byte_rows, _load_features, _nearest_rows, load_gaussian_ply, prune_gaussians, scan_box
from .scannet_mesh import _save, load_ply_mesh, mesh_columns, read_mesh_header  # noqa: F401  (the mesh reader is shared)

MESH_FILE = "mesh_aligned_0.05.ply"
SEGMENTS_FILE = "segments.json"
ANNO_FILE = "segments_anno.json"
CHECKPOINT = os.path.join("ckpts", "point_cloud_30000.ply")
SPLIT_FILES = OrderedDict([("train", "nvs_sem_train.txt"), ("val", "nvs_sem_val.txt"), ("test", "sem_test.txt")])
TOP100 = os.path.join("metadata", "semantic_benchmark", "top100.txt")


def _device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("scannetpp_mesh: scans are converted on the GPU (device='cuda'); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


# ---- host side: the label tables (pure numpy: what tests/test_scannetpp_host.py checks) -------------------------------------------------
def scannetpp_classes(top100_txt):
    """`metadata/semantic_benchmark/top100.txt` -> (names, class2idx), read with the reference's own call (one name per line; the dummy
    delimiter keeps the blanks inside a name)"""
    names = np.loadtxt(os.fspath(top100_txt), dtype=str, delimiter=".")
    return names, {name: idx for idx, name in enumerate(names)}


def first_groups(seg_groups, class2idx, ignore_index=-1):
    """`segGroups` of a segments_anno.json -> dict(first3 (max segment + 1, 3) int32, table_label (n_groups,) int32, table_object
    (n_groups,) int32, ignore_index).  first3[s] = the first three groups, in file order, whose label index
    `class2idx.get(label, ignore_index)` is not ignore_index and that list segment s (a repeat inside one list counts once); -1 = an
    empty slot.  Every vertex of a segment meets the same groups in the reference's loop, so these are the slots of all its vertices.
    ValueError: a negative segment id, or an `objectId` of a labelled group outside int16 (the dtype of the reference's arrays)."""
    groups = list(seg_groups)
    G = len(groups)
    table_label = np.full(G, ignore_index, dtype=np.int32)
    table_object = np.full(G, ignore_index, dtype=np.int32)
    seg_parts, group_parts = [], []
    for k, g in enumerate(groups):
        index = class2idx.get(g["label"], ignore_index)
        if index == ignore_index:
            continue                                                     # takes no slot
        object_id = int(g["objectId"])
        if not -2 ** 15 <= object_id < 2 ** 15 or not -2 ** 15 <= int(index) < 2 ** 15:
            raise ValueError(f"group {k}: objectId {object_id} / label index {index} outside int16")
        table_label[k], table_object[k] = index, object_id
        segs = np.asarray(g["segments"], dtype=np.int64).reshape(-1)
        if segs.size and segs.min() < 0:
            raise ValueError(f"group {k} (objectId {object_id}): negative segment id")
        seg_parts.append(segs)
        group_parts.append(np.full(segs.size, k, dtype=np.int64))
    segs = np.concatenate(seg_parts) if seg_parts else np.zeros(0, dtype=np.int64)
    owners = np.concatenate(group_parts) if group_parts else np.zeros(0, dtype=np.int64)
    if segs.size and segs.max() >= 2 ** 31 - 1:
        raise ValueError("a segment id outside int32")
    first3 = np.full((int(segs.max()) + 1 if segs.size else 0, 3), -1, dtype=np.int32)
    if segs.size:
        pairs = np.unique(segs * G + owners)                             # sorted by segment, then by group; a repeat drops out
        seg, owner = pairs // G, pairs % G
        starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        rank = np.arange(len(seg)) - np.repeat(starts, np.diff(np.r_[starts, len(seg)]))
        keep = rank < 3
        first3[seg[keep], rank[keep]] = owner[keep]
    return dict(first3=first3, table_label=table_label, table_object=table_object, ignore_index=int(ignore_index))


# ---- device side -------------------------------------------------------------------------------------------------------------------------
def mesh_vertex_normals_o3d(coord, faces):
    """coord (n, 3) f32, faces (F, 3) int32, on the device -> (n, 3) f32 vertex normals in the definition of Open3D's
    `compute_vertex_normals(normalized=True)` (fp64 sums of the unnormalised face cross products in face order), bit for bit."""
    for t in (coord, faces):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError("scannetpp_mesh: normals are computed on the GPU; there is no CPU fallback")
    with torch.cuda.device(coord.device):
        return nv.mesh_vertex_normals_o3d(coord, faces)


def multilabels(seg_indices, groups, device, src=None):
    """seg_indices (n,) integers (host), groups = first_groups(...) -> (segment, instance) device int16 (n, 3): per vertex, or per row of
    src (device int32 vertex rows), up to three labels in `segGroups` order, column 0 swapped to the smallest instance."""
    seg = np.asarray(seg_indices).reshape(-1)
    if seg.size and (seg.min() < 0 or seg.max() >= 2 ** 31):
        raise ValueError("segIndices outside [0, 2^31)")
    dev = _device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    with torch.cuda.device(dev):
        seg, first3, table_label, table_object = up(seg), up(groups["first3"]), up(groups["table_label"]), up(groups["table_object"])
        count = nv.spp_segment_hist(seg, first3.shape[0])
        size = nv.spp_group_sizes(first3, count, table_label.numel())
        return nv.spp_labels(seg, first3, table_label, table_object, size, src=src, empty=groups.get("ignore_index", -1))


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------------
def _names(path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                     # (numpy reports an empty list)
        return np.loadtxt(os.fspath(path), dtype=str, ndmin=1)


def _scenes_and_splits(dataset_root, scenes=None):
    """-> [(scene name, split)]: the three split lists of the download in the reference's order; `scenes` (a sequence of names or a text
    file of them) keeps the listed ones, as the reference's `--scenes_list` does (np.intersect1d: sorted)."""
    lists = OrderedDict((split, _names(os.path.join(os.fspath(dataset_root), "splits", name))) for split, name in SPLIT_FILES.items())
    if scenes is not None:
        wanted = _names(scenes) if isinstance(scenes, (str, os.PathLike)) else np.asarray(list(scenes), dtype=str)
        lists = OrderedDict((split, np.intersect1d(names, wanted)) for split, names in lists.items())
    return [(str(name), split) for split, names in lists.items() for name in names]


def _scans(dataset_root, name, split):
    return os.path.join(os.fspath(dataset_root), "sem_test" if split == "test" else "data", name, "scans")


def preprocess_scannetpp(dataset_root, output_root, ignore_index=-1, scenes=None, device=None):
    """preprocess_scannetpp.py on the device: every scene of `splits/nvs_sem_train.txt`, `nvs_sem_val.txt` (under `data/`) and
    `sem_test.txt` (under `sem_test/`) -> output_root/train|val|test/<scene>/ with coord.npy (f32), color.npy (u8), normal.npy (f32)
    and, for train and val, segment.npy and instance.npy ((n, 3) int16).  A scene that cannot be read is reported and skipped.
    -> the directories written."""
    dev = _device(device)
    _, class2idx = scannetpp_classes(os.path.join(os.fspath(dataset_root), TOP100))
    written = []
    for name, split in _scenes_and_splits(dataset_root, scenes):
        print(f"Parsing scene {name} in {split} split")
        scans = _scans(dataset_root, name, split)
        try:
            mesh = load_ply_mesh(os.path.join(scans, MESH_FILE), dev)
            n = mesh["coord"].shape[0]
            arrays = OrderedDict(coord=mesh["coord"].cpu().numpy(), color=mesh["color"].cpu().numpy(),
                                 normal=mesh_vertex_normals_o3d(mesh["coord"], mesh["faces"]).cpu().numpy())
            if split != "test":
                with open(os.path.join(scans, SEGMENTS_FILE)) as f:
                    seg_indices = np.array(json.load(f)["segIndices"])
                with open(os.path.join(scans, ANNO_FILE)) as f:
                    seg_groups = json.load(f)["segGroups"]
                if seg_indices.shape != (n,):
                    raise ValueError(f"{name}: {seg_indices.shape[0] if seg_indices.ndim else 0} segIndices for {n} vertices")
                segment, instance = multilabels(seg_indices, first_groups(seg_groups, class2idx, ignore_index), dev)
                arrays["segment"], arrays["instance"] = segment.cpu().numpy(), instance.cpu().numpy()
        except (ValueError, KeyError, OSError) as e:
            print(f"  skipped, it could not be read: {e!r}")
            continue
        out_dir = os.path.join(os.fspath(output_root), split, name)
        _save(out_dir, arrays)
        written.append(out_dir)
    return written


def _checkpoint(gs_root, name):
    folders = sorted(p for p in Path(gs_root).rglob("*") if p.is_dir() and p.name.endswith(name))
    if not folders:
        raise ValueError(f"no folder with suffix {name} found in {gs_root}")
    return os.path.join(folders[0], CHECKPOINT)


def _too_few(valid):
    with np.errstate(invalid="ignore"):
        return bool(np.float64(valid.sum()) / np.float64(valid.size) < 0.5)


def _features(feat_root, name):
    """-> (lang_feat float16, valid_feat_mask int64, whether under half of the rows hold a feature)"""
    lang = _load_features(os.path.join(os.fspath(feat_root), name, "langfeat.pth"))
    valid = np.any(lang != 0.0, axis=1).astype(int)
    return lang, valid, _too_few(valid)


def preprocess_scannetpp_gs(dataset_root, gs_root, pc_root, output_root, feat_root=None, feat_only=False, skip_feat=False, scenes_list=None,
                            device=None, prune_box=None):
    """preprocess_scannetpp_gs.py on the device: per scene the checkpoint <gs_root>/**/<*scene>/ckpts/point_cloud_30000.ply through
    load_gaussian_ply, the nearest row of pc_root/<split>/<scene>/coord.npy per Gaussian (hash-grid 1-NN; equal distances: the lower
    row), and into output_root/<split>/<scene>/ the five Gaussian assets, normal.npy and, for train and val, segment.npy and
    instance.npy: the rows of the point-cloud folder's arrays, gathered.  With feat_root (and not skip_feat) lang_feat.npy (fp16) and
    valid_feat_mask.npy (int64), unless under half of the rows hold a feature: the scene is then reported among the skipped and gets no
    feature files.  feat_only writes the feature files alone.  prune_box = m (the reference's 0.25): only the Gaussians inside the
    minimal oriented box of the point-cloud folder's coord.npy grown by m are kept, in file order, before the nearest-row search; every
    array written holds the kept rows, and the half-valid rule looks at the kept rows (the reference's order).  feat_only never prunes,
    as in the reference.  None writes all.  A cloud that spans no volume: the scene is skipped.
    -> (the directories written, the scene names skipped for their features)."""
    dev = _device(device)
    written, skipped = [], []
    for name, split in _scenes_and_splits(dataset_root, scenes_list):
        print(f"Parsing scene {name} in {split} split")
        out_dir = os.path.join(os.fspath(output_root), split, name)
        pc_dir = os.path.join(os.fspath(pc_root), split, name)
        try:
            arrays, feats = OrderedDict(), None
            pruning = prune_box is not None and not feat_only

            def take_features(lang, valid, too_few):
                if too_few:
                    print(f"  valid language feature percent too low, skipping the features of scene {name}")
                    skipped.append(name)
                else:
                    arrays["valid_feat_mask"], arrays["lang_feat"] = valid, lang

            if feat_root is not None and (feat_only or not skip_feat):
                feats = _features(feat_root, name)
                if not pruning:
                    take_features(*feats)
            if not feat_only:
                gs = load_gaussian_ply(_checkpoint(gs_root, name), dev)
                n = gs["coord"].shape[0]
                have = arrays["lang_feat"] if "lang_feat" in arrays else feats[0] if pruning and feats is not None else None
                if have is not None and have.shape[0] != n:
                    raise ValueError(f"{name}: {n} Gaussians, but the features hold {have.shape[0]} rows")
                pc_coord = np.load(os.path.join(pc_dir, "coord.npy"))
                if pruning:
                    gs, kept = prune_gaussians(gs, scan_box(pc_coord, prune_box, dev))
                    n = kept.numel()
                    if feats is not None:                                # the half-valid rule on the kept rows
                        rows = kept.cpu().numpy()
                        take_features(feats[0][rows], feats[1][rows], _too_few(feats[1][rows]))
                arrays.update((k, gs[k].cpu().numpy()) for k in GS_ASSETS)
                pc = OrderedDict(normal=np.load(os.path.join(pc_dir, "normal.npy")))
                if split != "test":
                    pc["instance"] = np.load(os.path.join(pc_dir, "instance.npy"))
                    pc["segment"] = np.load(os.path.join(pc_dir, "segment.npy"))
                with torch.cuda.device(dev):
                    nearest, m = _nearest_rows(gs["coord"], pc_coord)
                    for k, a in pc.items():
                        if a.shape[0] != m:
                            raise ValueError(f"{name}: {k}.npy has {a.shape[0]} rows, coord.npy has {m}")
                        a = np.ascontiguousarray(a)
                        rows = torch.from_numpy(a.reshape(m, -1).view(np.uint8)).to(dev)
                        got = _gather_byte_rows(rows, nearest).cpu().numpy()
                        arrays[k] = got.view(a.dtype).reshape((n,) + a.shape[1:])
        except (ValueError, KeyError, OSError) as e:
            print(f"  skipped, it could not be read: {e!r}")
            continue
        if not arrays:
            continue                                                     # feat_only without features to write
        _save(out_dir, arrays)
        written.append(out_dir)
    print(f"Skipped the following scenes for lang_feat: {skipped}")
    return written, skipped


def build_parser():
    parser = argparse.ArgumentParser(description="ScanNet++ scans to scene folders of .npy assets on the GPU (the arguments of "
                                                 "preprocess_scannetpp.py and preprocess_scannetpp_gs.py)")
    parser.add_argument("--dataset_root", required=True, help="the ScanNet++ download: holds data, sem_test, metadata and splits")
    parser.add_argument("--output_root", required=True, help="where the train / val / test folders go")
    parser.add_argument("--ignore_index", default=-1, type=int, help="the ignore index")
    parser.add_argument("--num_workers", default=1, type=int, help="accepted and ignored: the device does the work")
    parser.add_argument("--gs_root", default=None, help="the ScanNet++ Gaussian checkpoints: convert the Gaussians instead of the vertices")
    parser.add_argument("--pc_root", default=None, help="the point-cloud folders this module wrote without --gs_root (required with it)")
    parser.add_argument("--feat_root", default=None, help="folder with <scene>/langfeat.pth language features (with --gs_root)")
    parser.add_argument("--feat_only", action="store_true", help="write the language features only")
    parser.add_argument("--skip_feat", action="store_true", help="do not write the language features")
    parser.add_argument("--scenes_list", default=None, help="text file of the scenes to process")
    parser.add_argument("--prune_box", nargs="?", const=0.25, default=None, type=float,
                        help="with --gs_root: keep only the Gaussians inside the minimal oriented box of the point cloud grown by this margin (0.25 when no value is given)")
    return parser


def main(argv=None):
    parser = build_parser()
    cfg = parser.parse_args(argv)
    if cfg.gs_root is not None:
        if cfg.pc_root is None:
            parser.error("--gs_root needs --pc_root")
        done, _ = preprocess_scannetpp_gs(cfg.dataset_root, cfg.gs_root, cfg.pc_root, cfg.output_root, feat_root=cfg.feat_root,
                                          feat_only=cfg.feat_only, skip_feat=cfg.skip_feat, scenes_list=cfg.scenes_list,
                                          **({} if cfg.prune_box is None else dict(prune_box=cfg.prune_box)))
    else:
        done = preprocess_scannetpp(cfg.dataset_root, cfg.output_root, ignore_index=cfg.ignore_index, scenes=cfg.scenes_list)
    print(f"{len(done)} scene folder(s) written")
    return 0 if done else 1


if __name__ == "__main__":
    raise SystemExit(main())
