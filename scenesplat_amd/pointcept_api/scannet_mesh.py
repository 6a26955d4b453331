"""The ScanNet converter on the device: a raw scan (`<scene>_vh_clean_2.ply`, `.0.010000.segs.json`, `.aggregation.json`) -> the labelled
point-cloud folder (`coord`, `color`, `normal`, `segment20`, `segment200`, `instance`), and together with a 3DGS checkpoint -> the GS scene
folder the `semseg-gs-scannet*` configs and `ScanNetGSDataset` read.

Mirror of pointcept/datasets/preprocessing/scannet/preprocess_scannet.py (`read_plymesh`, `vertex_normal`, `point_indices_from_group`,
`handle_process` and its command line) and of preprocess_scannet_gs.py (the same for the Gaussians of a checkpoint: labels and normals of
the nearest mesh vertex): the same file names, dtypes, shapes and bytes.

    header (host, no plyfile) -> vertex and face blocks --readinto--> pinned --pieces of whole records--> device
      -> ss_mesh_decode_vertices / ss_mesh_decode_faces: one pass each over the interleaved records                  (csrc/mesh.hip)
      -> ss_mesh_face_terms, stable radix argsort of the 3F corner entries by vertex, ss_pool_partition, ss_mesh_vertex_normals:
         the reference's Python loop over the faces (`nv[face[i]] += nf[i]`) as a sort and a walk, bit-equal to it
      -> ss_mesh_labels: the per-object `np.isin` passes as one lookup through seg_to_group
      -> (GS) load_gaussian_ply, the hash-grid 1-NN, ss_gather_rows -> np.save

Values against the reference: every array is bit for bit the reference's, except what `load_gaussian_ply` documents for `scale` and
`opacity` of the checkpoint.  Deviations:
* the oriented-bounding-box pruning of preprocess_scannet_gs.py (open3d's `get_minimal_oriented_bounding_box` plus 25 cm) is the
  keyword `prune_box=0.25` (oriented_box.py): the box of least volume among the frames of ALL edges of the hull's triangles, where
  Open3D tries one edge per triangle in Qhull's vertex order; never larger than Open3D's.  The default None writes every Gaussian.
* the label table, the two valid-id lists and the split lists are arguments: the reference reads them from its `meta_data` folder, this
  package ships none of them (they come with the ScanNet download).
* `gs_root/<scene>/ckpts/*.ply`: the first in sorted order (the reference: the first in listing order).
* a scene that cannot be read is reported and skipped without leaving a folder (the GS script creates the folder first).
* the nearest vertex is the fp32 hash-grid search's (equal distances: the lower row), the reference's an fp64 KD-tree's.

Only triangle meshes whose `x`, `y`, `z` are float32 at 4-byte offsets and whose colours are uchar have a device form; anything else is a
ValueError, never a host fallback."""
import argparse
import csv
import glob
import json
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from .. import native as nv
from .gaussian_ply import GS_ASSETS, MAX_HEADER, PLY_TYPES, _load_features, _nearest_rows, load_gaussian_ply, prune_gaussians, scan_box

CLOUD_FILE_PFIX = "_vh_clean_2"
SEGMENTS_FILE_PFIX = ".0.010000.segs.json"
AGGREGATIONS_FILE_PFIX = ".aggregation.json"
IGNORE_INDEX = -1
FACE_BYTES = nv.MESH_FACE_BYTES
# the strings pandas.read_csv reads as a missing value: such a raw_category never equals a label
PANDAS_NA = frozenset(["", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
                       "NULL", "NaN", "None", "n/a", "nan", "null"])

MeshHeader = namedtuple("MeshHeader", "n_vertices vertex_stride vertex_offset properties n_faces face_offset index_type")
MeshHeader.__doc__ = """n_vertices, vertex_stride (bytes of a vertex record), vertex_offset (file offset of the vertex block), properties
(OrderedDict name -> (numpy dtype, byte offset inside a record)), n_faces, face_offset (file offset of the face block: records of 13
bytes), index_type ('int' or 'uint')"""


# ---- host side: the header (pure python: what tests/test_scannet_mesh_host.py checks) ---------------------------------------------------
def read_mesh_header(path):
    """-> MeshHeader of a binary little-endian .ply whose first element is `vertex` and whose second is `face` with the single property
    `list uchar int|uint vertex_indices`.  ValueError names the cause otherwise."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        head = f.read(MAX_HEADER)
    if head[:3] != b"ply" or head[3:4] not in (b"\n", b"\r"):
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic)")
    end = head.find(b"end_header")
    nl = head.find(b"\n", end) if end >= 0 else -1
    if nl < 0:
        raise ValueError(f"{path}: no end_header line in the first {MAX_HEADER} bytes")
    fmt, elements, props, stride, face_props = None, [], OrderedDict(), 0, []
    for raw in head[:nl].split(b"\n")[1:]:
        words = raw.decode("ascii", "replace").rstrip("\r").split()
        if not words or words[0] in ("comment", "obj_info", "end_header"):
            continue
        if words[0] == "format":
            fmt = " ".join(words[1:])
            if fmt != "binary_little_endian 1.0":
                raise ValueError(f"{path}: format '{fmt}' is not supported (binary_little_endian 1.0 only)")
        elif words[0] == "element":
            if len(words) != 3:
                raise ValueError(f"{path}: malformed element line '{' '.join(words)}'")
            expected = ("vertex", "face")
            if len(elements) < 2 and words[1] != expected[len(elements)]:
                raise ValueError(f"{path}: element {len(elements) + 1} is '{words[1]}', not '{expected[len(elements)]}'")
            elements.append((words[1], int(words[2])))
        elif words[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property before any element")
            if len(elements) > 2:
                continue                                              # elements after face are not read
            if len(elements) == 2:
                face_props.append(words[1:])
                continue
            if len(words) >= 2 and words[1] == "list":
                raise ValueError(f"{path}: list property '{words[-1]}' inside the vertex element")
            if len(words) != 3:
                raise ValueError(f"{path}: malformed property line '{' '.join(words)}'")
            if words[1] not in PLY_TYPES:
                raise ValueError(f"{path}: unknown property type '{words[1]}' of '{words[2]}'")
            dtype = np.dtype("<" + PLY_TYPES[words[1]])
            props.setdefault(words[2], (dtype, stride))
            stride += dtype.itemsize
        else:
            raise ValueError(f"{path}: unknown header line '{' '.join(words)}'")
    if fmt is None:
        raise ValueError(f"{path}: no format line")
    if not elements:
        raise ValueError(f"{path}: no vertex element")
    if len(elements) < 2:
        raise ValueError(f"{path}: no face element after the vertex element")
    (_, n), (_, n_faces) = elements[:2]
    if n < 0 or n_faces < 0:
        raise ValueError(f"{path}: negative element count ({n} vertices, {n_faces} faces)")
    if len(face_props) != 1 or len(face_props[0]) != 4 or face_props[0][0] != "list":
        raise ValueError(f"{path}: the face element must hold one list property, got {[' '.join(p) for p in face_props]}")
    _, count_type, index_type, _ = face_props[0]
    if PLY_TYPES.get(count_type) != "u1":
        raise ValueError(f"{path}: the face list counts with '{count_type}', not uchar")
    if PLY_TYPES.get(index_type) not in ("i4", "u4"):
        raise ValueError(f"{path}: the face list indexes with '{index_type}', not int or uint")
    vertex_offset = nl + 1
    face_offset = vertex_offset + n * stride
    size = os.path.getsize(path)
    if size < face_offset + n_faces * FACE_BYTES:
        raise ValueError(f"{path}: the file holds {size} bytes, shorter than header {vertex_offset} + {n} vertices x {stride} bytes + "
                         f"{n_faces} faces x {FACE_BYTES} bytes")
    return MeshHeader(n, stride, vertex_offset, props, n_faces, face_offset, "int" if PLY_TYPES[index_type] == "i4" else "uint")


def mesh_columns(header):
    """-> byte offsets [x, y, z, red, green, blue] inside a vertex record.  KeyError: a missing property; ValueError: no device form."""
    offsets = []
    for name in ("x", "y", "z", "red", "green", "blue"):
        if name not in header.properties:
            raise KeyError(name)
        dtype, off = header.properties[name]
        if name in "xyz":
            if dtype != np.dtype("<f4"):
                raise ValueError(f"no device form: property '{name}' is {dtype.name}, not float32")
            if off % 4:
                raise ValueError(f"no device form: property '{name}' sits at byte offset {off}, not a multiple of 4")
        elif dtype != np.dtype("u1"):
            raise ValueError(f"no device form: property '{name}' is {dtype.name}, not uchar")
        offsets.append(off)
    return offsets


def _device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("scannet_mesh: meshes are converted on the GPU (device='cuda'); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


# ---- host side: the label tables ---------------------------------------------------------------------------------------------------------
def _id_list(ids, name):
    """a sequence of ids, or a text file of them (as `class2id=` of the datasets) -> list of int"""
    if ids is None:
        raise ValueError(f"{name} is required: the valid class ids come with the ScanNet download, not with this package")
    if isinstance(ids, (str, os.PathLike)):
        ids = np.loadtxt(ids, dtype=np.int64)
    return [int(i) for i in np.asarray(ids).reshape(-1)]


class LabelTables:
    """raw_category -> (segment20 label, segment200 label), as `point_indices_from_group` maps a group's label"""

    def __init__(self, rows, class_ids20, class_ids200):
        self.class_ids20, self.class_ids200 = list(class_ids20), list(class_ids200)
        self.rows = OrderedDict()
        for raw_category, id200, nyu40id in rows:
            self.rows.setdefault(raw_category, (nyu40id, id200))         # the first matching row wins (`.iloc[0]`)

    @staticmethod
    def _index(ids, value):
        return ids.index(value) if value in ids else IGNORE_INDEX

    def lookup(self, label):
        id20, id200 = self.rows.get(label, (0, 0)) if isinstance(label, str) else (0, 0)      # no row: id 0
        return self._index(self.class_ids20, id20), self._index(self.class_ids200, id200)


def scannet_label_tables(labels_tsv, class_ids20, class_ids200):
    """`scannetv2-labels.combined.tsv` (columns raw_category, id, nyu40id among others) and the two valid-id lists (each a sequence or a
    text file of ids) -> LabelTables."""
    ids20, ids200 = _id_list(class_ids20, "class_ids20"), _id_list(class_ids200, "class_ids200")
    rows = []
    with open(os.fspath(labels_tsv), newline="", encoding="utf-8") as f:
        reader = csv.reader(f, delimiter="\t")
        names = next(reader, None)
        if names is None or any(c not in names for c in ("raw_category", "id", "nyu40id")):
            raise ValueError(f"{labels_tsv}: no header line with the columns raw_category, id and nyu40id")
        col = [names.index(c) for c in ("raw_category", "id", "nyu40id")]
        for line in reader:
            if not line:
                continue                                              # (pandas skips blank lines)
            cells = [line[c] if c < len(line) else "" for c in col]
            if cells[0] in PANDAS_NA:
                continue                                              # read as missing: equal to no label
            rows.append((cells[0], int(float(cells[1])), int(float(cells[2]))))
    return LabelTables(rows, ids20, ids200)


def group_tables(seg_groups, tables):
    """`segGroups` of an aggregation file -> dict(seg_to_group (max segment + 1,) int32 with -1 = no group, table20 / table200 /
    table_instance (n_groups,) int32).  seg_to_group is filled group after group: a segment in several groups belongs to the last, the
    order in which the reference's loop overwrites."""
    groups = list(seg_groups)
    top = -1
    for g in groups:
        segs = np.asarray(g["segments"], dtype=np.int64).reshape(-1)
        if segs.size:
            if segs.min() < 0:
                raise ValueError(f"group {g.get('id')}: negative segment id")
            top = max(top, int(segs.max()))
    seg_to_group = np.full(top + 1, -1, dtype=np.int32)
    t20, t200, tinst = (np.empty(len(groups), dtype=np.int32) for _ in range(3))
    for k, g in enumerate(groups):
        seg_to_group[np.asarray(g["segments"], dtype=np.int64).reshape(-1)] = k
        t20[k], t200[k] = tables.lookup(g["label"])
        tinst[k] = int(g["id"])
    return dict(seg_to_group=seg_to_group, table20=t20, table200=t200, table_instance=tinst)


# ---- device side ---------------------------------------------------------------------------------------------------------------------------
def load_ply_mesh(path, device=None, staging_bytes=256 << 20):
    """-> {coord (n, 3) f32, color (n, 3) u8, faces (F, 3) int32} on the device.  Both blocks are read into pinned memory and uploaded in
    pieces of whole records of at most staging_bytes (at least one record); one decode launch per piece writes at the piece's row
    offset.  A piece keeps its file offset modulo 4 in the staging buffer, as it would in a mapping of the whole file: the kernels take
    records at any byte.  ValueError: a face that is no triangle, or an index outside [0, n)."""
    header = read_mesh_header(path)
    offsets = mesh_columns(header)                                       # (every refusal that needs only the file: before the device)
    dev = _device(device)
    n, stride, F = header.n_vertices, header.vertex_stride, header.n_faces
    with torch.cuda.device(dev):
        out = OrderedDict(coord=torch.empty((n, 3), dtype=torch.float32, device=dev), color=torch.empty((n, 3), dtype=torch.uint8, device=dev),
                          faces=torch.empty((F, 3), dtype=torch.int32, device=dev))
        if n == 0 and F == 0:
            return out
        per_v = max(1, min(n, int(staging_bytes) // stride))
        per_f = max(1, min(F, int(staging_bytes) // FACE_BYTES))
        cap = max(per_v * stride, per_f * FACE_BYTES) + 4
        host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        stage = torch.empty(cap, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream()

        def pieces(f, what, file_offset, count, rec_bytes, per, decode):
            f.seek(file_offset)
            for row in range(0, count, per):
                rows = min(per, count - row)
                at = (file_offset + row * rec_bytes) & 3
                got = f.readinto(memoryview(view[at:at + rows * rec_bytes]))
                if got != rows * rec_bytes:
                    raise ValueError(f"{path}: the {what} block ends after {row * rec_bytes + (got or 0)} of {count * rec_bytes} bytes")
                stage[at:at + rows * rec_bytes].copy_(host[at:at + rows * rec_bytes], non_blocking=True)
                stream.synchronize()                                     # the pinned buffer is free for the next read
                decode(rows, row, at)

        with open(os.fspath(path), "rb", buffering=0) as f:
            pieces(f, "vertex", header.vertex_offset, n, stride, per_v,
                   lambda rows, row, at: nv.mesh_decode_vertices(stage, rows, stride, offsets, out["coord"], out["color"], row=row, start=at))
            pieces(f, "face", header.face_offset, F, FACE_BYTES, per_f,
                   lambda rows, row, at: nv.mesh_decode_faces(stage, rows, n, out["faces"], status, row=row, start=at))
        nv.mesh_check_status(status, os.fspath(path))
    return out


def mesh_vertex_normals(coord, faces, form="pc"):
    """coord (n, 3) f32, faces (F, 3) int32, on the device -> (n, 3) f32 area-weighted vertex normals: `vertex_normal` of
    preprocess_scannet.py (form='pc') or of preprocess_scannet_gs.py (form='gs'), bit for bit."""
    for t in (coord, faces):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError("scannet_mesh: normals are computed on the GPU; there is no CPU fallback")
    with torch.cuda.device(coord.device):
        return nv.mesh_vertex_normals(coord, faces, form)


def mesh_labels(seg_indices, groups, dtype, device, src=None):
    """seg_indices (n,) integers (host), groups = group_tables(...) -> (segment20, segment200, instance) device tensors of `dtype`, one
    row per vertex, or per row of src (device int32 vertex rows)."""
    seg = np.asarray(seg_indices).reshape(-1)
    if seg.size and (seg.min() < -2 ** 31 or seg.max() >= 2 ** 31):
        raise ValueError("segIndices outside int32")
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    return nv.mesh_labels(up(seg), up(groups["seg_to_group"]), up(groups["table20"]), up(groups["table200"]), up(groups["table_instance"]),
                          dtype, src=src)


# ---- the scripts -----------------------------------------------------------------------------------------------------------------------------
def _scene_list(names):
    """a sequence of scene names, or a text file with one per line"""
    if names is None:
        return []
    if isinstance(names, (str, os.PathLike)):
        with open(names) as f:
            return f.read().splitlines()
    return list(names)


def _split_of(scene_id, train_scenes, val_scenes):
    return "train" if scene_id in train_scenes else "val" if scene_id in val_scenes else "test"


def _scene_files(scene_path):
    scene_id = os.path.basename(os.path.normpath(scene_path))
    return (scene_id, os.path.join(scene_path, f"{scene_id}{CLOUD_FILE_PFIX}.ply"),
            os.path.join(scene_path, f"{scene_id}{CLOUD_FILE_PFIX}{SEGMENTS_FILE_PFIX}"),
            os.path.join(scene_path, f"{scene_id}{AGGREGATIONS_FILE_PFIX}"))


def _scene_labels(segments_file, aggregations_file, tables, n):
    """-> (segIndices array, group_tables) of a scene's two json files"""
    with open(segments_file) as f:
        seg_indices = np.array(json.load(f)["segIndices"])
    with open(aggregations_file) as f:
        seg_groups = json.load(f)["segGroups"]
    if seg_indices.shape != (n,):
        raise ValueError(f"{segments_file}: {seg_indices.shape[0] if seg_indices.ndim else 0} segIndices for {n} vertices")
    return seg_indices, group_tables(seg_groups, tables)


def _save(out_dir, arrays):
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _scene_paths(dataset_root):
    return sorted(glob.glob(os.fspath(dataset_root) + "/scans*/scene*"))


def preprocess_scannet(dataset_root, output_root, labels_tsv, class_ids20, class_ids200, train_list, val_list, parse_normals=True,
                       device=None):
    """preprocess_scannet.py on the device: every `scans*/scene*` of dataset_root -> output_root/train|val|test/<scene>/ with coord.npy
    (f32), color.npy (u8), normal.npy (f32, the 'pc' form) and, for a scene of the train or val list, segment20 / segment200 /
    instance .npy (int64).  A scene that cannot be read is reported and skipped.  -> the directories written."""
    tables = scannet_label_tables(labels_tsv, class_ids20, class_ids200)
    train_scenes, val_scenes = _scene_list(train_list), _scene_list(val_list)
    dev = _device(device)
    written = []
    for scene_path in _scene_paths(dataset_root):
        scene_id, mesh_path, segments_file, aggregations_file = _scene_files(scene_path)
        split = _split_of(scene_id, train_scenes, val_scenes)
        print(f"Processing: {scene_id} in {split}")
        try:
            mesh = load_ply_mesh(mesh_path, dev)
            n = mesh["coord"].shape[0]
            arrays = OrderedDict(coord=mesh["coord"].cpu().numpy(), color=mesh["color"].cpu().numpy())
            if parse_normals:
                arrays["normal"] = mesh_vertex_normals(mesh["coord"], mesh["faces"], "pc").cpu().numpy()
            if split != "test":
                seg_indices, groups = _scene_labels(segments_file, aggregations_file, tables, n)
                for name, t in zip(("segment20", "segment200", "instance"), mesh_labels(seg_indices, groups, torch.int64, dev)):
                    arrays[name] = t.cpu().numpy()
        except (ValueError, KeyError, OSError) as e:
            print(f"  skipped, it could not be read: {e!r}")
            continue
        out_dir = os.path.join(os.fspath(output_root), split, scene_id)
        _save(out_dir, arrays)
        written.append(out_dir)
    return written


def preprocess_scannet_gs(dataset_root, output_root, gs_root, labels_tsv, class_ids20, class_ids200, train_list, val_list, feat_root=None,
                          feat_only=False, skip_feat=False, device=None, prune_box=None):
    """preprocess_scannet_gs.py on the device: per scene the checkpoint gs_root/<scene>/ckpts/*.ply through load_gaussian_ply, the nearest
    mesh vertex per Gaussian (hash-grid 1-NN; equal distances: the lower row), and into output_root/train|val|test/<scene>/ the five
    Gaussian assets, normal.npy (the 'gs' form normals of the nearest vertex), for a train or val scene segment20 / segment200 /
    instance .npy (int16), and with feat_root lang_feat.npy (fp16) and valid_feat_mask.npy (int64).  feat_only is accepted and ignored,
    as in the reference.  prune_box = m (the reference's 0.25): only the Gaussians inside the minimal oriented box of the scan's
    vertices grown by m are kept, in file order, before the nearest-vertex search; every array written holds the kept rows.  None
    writes all.  A scan whose vertices span no volume is skipped.  -> the directories written."""
    tables = scannet_label_tables(labels_tsv, class_ids20, class_ids200)
    train_scenes, val_scenes = _scene_list(train_list), _scene_list(val_list)
    dev = _device(device)
    written = []
    for scene_path in _scene_paths(dataset_root):
        scene_id, mesh_path, segments_file, aggregations_file = _scene_files(scene_path)
        split = _split_of(scene_id, train_scenes, val_scenes)
        print(f"Processing scene: {scene_id} in {split}")
        candidates = sorted(glob.glob(os.path.join(os.fspath(gs_root), scene_id, "ckpts", "*.ply")))
        if not candidates:
            print(f"  skipped: no Gaussian .ply under {os.path.join(os.fspath(gs_root), scene_id, 'ckpts')}")
            continue
        try:
            mesh = load_ply_mesh(mesh_path, dev)
            if mesh["coord"].shape[0] == 0:
                raise ValueError(f"{mesh_path}: no vertices")
            gs = load_gaussian_ply(candidates[0], dev)
            n_file = gs["coord"].shape[0]
            kept = None
            if prune_box is not None:
                gs, kept = prune_gaussians(gs, scan_box(mesh["coord"], prune_box, dev))
            n = gs["coord"].shape[0]
            arrays = OrderedDict((k, gs[k].cpu().numpy()) for k in GS_ASSETS)
            with torch.cuda.device(dev):
                normals = mesh_vertex_normals(mesh["coord"], mesh["faces"], "gs")
                nearest, _ = _nearest_rows(gs["coord"], mesh["coord"])
                arrays["normal"] = nv.gather_rows(normals, nearest).cpu().numpy() if n else np.empty((0, 3), dtype=np.float32)
                if split != "test":
                    seg_indices, groups = _scene_labels(segments_file, aggregations_file, tables, mesh["coord"].shape[0])
                    for name, t in zip(("segment20", "segment200", "instance"), mesh_labels(seg_indices, groups, torch.int16, dev, src=nearest)):
                        arrays[name] = t.cpu().numpy()
            if feat_root is not None and not skip_feat:
                lang = _load_features(os.path.join(os.fspath(feat_root), scene_id, "langfeat.pth"))
                if lang.shape[0] != n_file:
                    raise ValueError(f"{scene_id}: {n_file} Gaussians, but the features hold {lang.shape[0]} rows")
                if kept is not None:
                    lang = lang[kept.cpu().numpy()]
                arrays["valid_feat_mask"] = np.any(lang != 0.0, axis=1).astype(np.int64)
                arrays["lang_feat"] = lang
        except (ValueError, KeyError, OSError) as e:
            print(f"  skipped, it could not be read: {e!r}")
            continue
        out_dir = os.path.join(os.fspath(output_root), split, scene_id)
        _save(out_dir, arrays)
        print(f"  {n} Gaussians -> {out_dir} ({', '.join(arrays)})")
        written.append(out_dir)
    return written


def build_parser():
    parser = argparse.ArgumentParser(description="ScanNet scans to scene folders of .npy assets on the GPU (the arguments of preprocess_scannet.py and "
                                                 "preprocess_scannet_gs.py, and the files those read from their meta_data folder)")
    parser.add_argument("--dataset_root", required=True, help="the ScanNet download: holds scans*/scene*")
    parser.add_argument("--output_root", required=True, help="where the train / val / test folders go")
    parser.add_argument("--gs_root", default=None, help="folder with <scene>/ckpts/*.ply 3DGS checkpoints: convert the Gaussians instead of the vertices")
    parser.add_argument("--feat_root", default=None, help="folder with <scene>/langfeat.pth language features (with --gs_root)")
    parser.add_argument("--feat_only", action="store_true", help="accepted and ignored, as in the reference")
    parser.add_argument("--skip_feat", action="store_true", help="do not write the language features")
    parser.add_argument("--prune_box", nargs="?", const=0.25, default=None, type=float,
                        help="with --gs_root: keep only the Gaussians inside the scan's minimal oriented box grown by this margin (0.25 when no value is given)")
    parser.add_argument("--parse_normals", default=True, type=bool, help="whether to write normal.npy (point-cloud form)")
    parser.add_argument("--num_workers", default=1, type=int, help="accepted and ignored: the device does the work")
    parser.add_argument("--labels_tsv", required=True, help="scannetv2-labels.combined.tsv")
    parser.add_argument("--class_ids20", required=True, help="text file of the 20 valid nyu40 ids")
    parser.add_argument("--class_ids200", required=True, help="text file of the 200 valid ScanNet200 ids")
    parser.add_argument("--train_list", required=True, help="scannetv2_train.txt")
    parser.add_argument("--val_list", required=True, help="scannetv2_val.txt")
    return parser


def main(argv=None):
    cfg = build_parser().parse_args(argv)
    common = dict(labels_tsv=cfg.labels_tsv, class_ids20=cfg.class_ids20, class_ids200=cfg.class_ids200, train_list=cfg.train_list,
                  val_list=cfg.val_list)
    if cfg.gs_root is not None:
        done = preprocess_scannet_gs(cfg.dataset_root, cfg.output_root, cfg.gs_root, feat_root=cfg.feat_root, feat_only=cfg.feat_only,
                                     skip_feat=cfg.skip_feat, **({} if cfg.prune_box is None else dict(prune_box=cfg.prune_box)), **common)
    else:
        done = preprocess_scannet(cfg.dataset_root, cfg.output_root, parse_normals=cfg.parse_normals, **common)
    print(f"{len(done)} scene folder(s) written")
    return 0 if done else 1


if __name__ == "__main__":
    raise SystemExit(main())
