"""3DGS checkpoints on the device: `point_cloud.ply` -> the scene folder (`coord.npy`, `color.npy`, `opacity.npy`, `scale.npy`,
`quat.npy`, optionally `segment` / `normal` / `instance` / `lang_feat` / `valid_feat_mask`) that the datasets, `chunk_split` and the
loaders start from.

Mirror of scripts/preprocess_gs.py (`read_gaussian_attributes`, `process_ply_file` and its command line) and of the Gaussian part of
pointcept/datasets/preprocessing/holicity/preprocess_holicity_gs.py (`read_gaussian_attribute`, the 1-nearest-neighbour label transfer,
`lang_feat.npy` / `valid_feat_mask.npy`): the same file names, dtypes and shapes.

    header (host, no plyfile) -> vertex block --readinto--> pinned --pieces of whole records--> device
      -> ss_ply_decode: ONE pass over the interleaved records writes coord / color / opacity / scale / quat   (csrc/ply.hip)
      -> transfer_labels: pointops.knn_query(k = 1) on the labelled cloud, ss_gather_rows of every asset
      -> np.save

Values against the reference:
* `coord`, `color`, `quat`: bit for bit (every fp32 step rounded on its own, in numpy's order).
* `scale` = exp(x) and `opacity` = 1 / (1 + exp(-x)) are evaluated in fp64 and rounded ONCE to fp32.  numpy's fp32 `exp` is not
  correctly rounded (up to 2.4 fp32 ulp from the fp64 value for exp, 3.2 for the sigmoid over the ranges checkpoints hold:
  profiles/ply_ingest.md), so these two arrays are NOT bit-equal to the reference's; they are the closer ones.  A logit of -100 gives
  the denormal 3.8e-44 the fp64 expression rounds to, where the reference's fp32 sigmoid gives 0.
* a vertex with `rot_0 == 0` yields an all-zero quaternion, as in the reference (sign(0) = 0); kept, not repaired.
* the oriented-bounding-box pruning of the ScanNet / HoliCity scripts is a keyword, `prune_box=0.25` (oriented_box.py: the minimal
  oriented box of the labelled cloud, grown by 25 cm, keeps the Gaussians inside; every edge of a hull triangle is a candidate frame,
  Open3D tries one per triangle).  The default None writes every Gaussian (the HoliCity script computes the mask and then replaces
  it by all ones).
* directory mode processes the files in sorted order (the reference: listing order).

Only float32 properties at 4-byte offsets have a device form; anything else is a ValueError ("no device form"), never a host fallback."""
import argparse
import os
from collections import OrderedDict, namedtuple
from pathlib import Path

import numpy as np
import torch

from .. import native as nv
from .. import pointops
from . import oriented_box

PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
             "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
REQUIRED = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity")
GS_ASSETS = ("coord", "color", "opacity", "scale", "quat")
PC_ASSETS = ("segment", "normal", "instance")
MAX_HEADER = 1 << 20

PlyHeader = namedtuple("PlyHeader", "count stride data_offset properties")
PlyHeader.__doc__ = """count: vertices; stride: bytes of a vertex record; data_offset: file offset of the vertex block;
properties: OrderedDict name -> (numpy dtype, byte offset inside a record), in file order"""


# ---- host side: the header and the column choice (pure python: what tests/test_gaussian_ply_host.py checks) -----------------------------
def read_ply_header(path):
    """-> PlyHeader of a binary little-endian .ply whose first element is `vertex`.  ValueError names the cause otherwise."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        head = f.read(MAX_HEADER)
    if head[:3] != b"ply" or head[3:4] not in (b"\n", b"\r"):
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic)")
    end = head.find(b"end_header")
    nl = head.find(b"\n", end) if end >= 0 else -1
    if nl < 0:
        raise ValueError(f"{path}: no end_header line in the first {MAX_HEADER} bytes")
    data_offset = nl + 1
    fmt, count, props, stride, element = None, None, OrderedDict(), 0, None
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
            if element is None and words[1] != "vertex":
                raise ValueError(f"{path}: the first element is '{words[1]}', not 'vertex'")
            element = words[1] if element is None else "<after vertex>"
            if element == "vertex":
                count = int(words[2])
        elif words[0] == "property":
            if element is None:
                raise ValueError(f"{path}: a property before any element")
            if element != "vertex":
                continue                                              # elements after vertex are ignored
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
    if count is None:
        raise ValueError(f"{path}: no vertex element")
    if count < 0:
        raise ValueError(f"{path}: negative vertex count {count}")
    size = os.path.getsize(path)
    if size < data_offset + count * stride:
        raise ValueError(f"{path}: the file holds {size} bytes, shorter than header {data_offset} + {count} vertices x {stride} bytes")
    return PlyHeader(count, stride, data_offset, props)


def gaussian_columns(header):
    """-> (byte offsets [x, y, z, f_dc_0..2, opacity, scale_*, rot*], n_scale, n_rot) of the columns read_gaussian_attributes selects:
    `scale_` / `rot` prefix matches sorted by their numeric suffix.  KeyError: a missing property; ValueError: no or more than four
    scale / rot columns, or a column without a device form."""
    props = header.properties
    for name in REQUIRED:
        if name not in props:
            raise KeyError(name)
    scale_names = sorted([p for p in props if p.startswith("scale_")], key=lambda s: int(s.split("_")[-1]))
    rot_names = sorted([p for p in props if p.startswith("rot")], key=lambda s: int(s.split("_")[-1]))
    for kind, names in (("scale_*", scale_names), ("rot*", rot_names)):
        if not 1 <= len(names) <= 4:
            raise ValueError(f"{len(names)} {kind} properties: 1 to 4 expected")
    names = list(REQUIRED) + scale_names + rot_names
    if header.stride % 4:
        raise ValueError(f"no device form: the record stride {header.stride} is not a multiple of 4")
    for name in names:
        dtype, off = props[name]
        if dtype != np.dtype("<f4"):
            raise ValueError(f"no device form: property '{name}' is {dtype.name}, not float32")
        if off % 4:
            raise ValueError(f"no device form: property '{name}' sits at byte offset {off}, not a multiple of 4")
    return [props[name][1] for name in names], len(scale_names), len(rot_names)


def _device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("gaussian_ply: checkpoints are decoded on the GPU (device='cuda'); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


# ---- device side -----------------------------------------------------------------------------------------------------------------------
def load_gaussian_ply(path, device=None, staging_bytes=256 << 20):
    """-> {coord (n, 3) f32, color (n, 3) u8, opacity (n,) f32, scale (n, k) f32, quat (n, r) f32} on the device.  The vertex block is
    read into pinned memory and uploaded in pieces of whole records of at most staging_bytes (at least one record); one ss_ply_decode
    launch per piece writes at the piece's row offset."""
    header = read_ply_header(path)
    offsets, n_scale, n_rot = gaussian_columns(header)                   # (every refusal happens before the device is touched)
    dev = _device(device)
    n, stride = header.count, header.stride
    with torch.cuda.device(dev):
        out = OrderedDict(coord=torch.empty((n, 3), dtype=torch.float32, device=dev), color=torch.empty((n, 3), dtype=torch.uint8, device=dev),
                          opacity=torch.empty(n, dtype=torch.float32, device=dev), scale=torch.empty((n, n_scale), dtype=torch.float32, device=dev),
                          quat=torch.empty((n, n_rot), dtype=torch.float32, device=dev))
        if n == 0:
            return out
        per = min(n, max(1, int(staging_bytes) // stride))
        host = torch.empty(per * stride, dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        stage = torch.empty(per * stride, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream()
        with open(os.fspath(path), "rb", buffering=0) as f:
            f.seek(header.data_offset)
            for row in range(0, n, per):
                rows = min(per, n - row)
                got = f.readinto(memoryview(view[:rows * stride]))
                if got != rows * stride:
                    raise ValueError(f"{path}: the vertex block ends after {row * stride + (got or 0)} of {n * stride} bytes")
                stage[:rows * stride].copy_(host[:rows * stride], non_blocking=True)
                stream.synchronize()                                     # the pinned buffer is free for the next read; the decode of
                                                                         # this piece then runs beside that read
                nv.ply_decode(stage, rows, stride, offsets, n_scale, n_rot, out["coord"], out["color"], out["opacity"], out["scale"],
                              out["quat"], row=row)
        stream.synchronize()
    return out


def _rows_as_bytes(asset, dev):
    """an asset of any dtype and trailing shape -> ((m, row_bytes) uint8 device tensor, numpy dtype, trailing shape)"""
    if isinstance(asset, torch.Tensor):
        t = asset.detach().to(dev).contiguous()
        dtype = np.dtype(str(t.dtype).replace("torch.", ""))
        shape = tuple(t.shape)
        flat = t.view(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8, device=dev)
    else:
        a = np.ascontiguousarray(asset)
        dtype, shape = a.dtype, a.shape
        flat = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(dev)
    m = shape[0]
    return flat.view(m, flat.numel() // m if m else 0), dtype, shape[1:]


def _nearest_rows(coord, pc_coord):
    """(n,) int32: per Gaussian the nearest row of the cloud (equal fp32 distances: the lower row)"""
    pc = pc_coord if isinstance(pc_coord, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc_coord))
    if pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError(f"transfer_labels: pc_coord must be (m, 3), got {tuple(pc.shape)}")
    if pc.shape[0] == 0:
        raise ValueError("transfer_labels: the point cloud is empty")
    nv._req(coord, torch.float32, "coord")
    if coord.dim() != 2 or coord.shape[1] != 3:
        raise ValueError(f"transfer_labels: coord must be (n, 3), got {tuple(coord.shape)}")
    dev = coord.device
    pc = pc.to(dev).to(torch.float32).contiguous()
    n, m = coord.shape[0], pc.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), m
    idx, _ = pointops.knn_query(1, pc, torch.tensor([m], dtype=torch.int32, device=dev), coord, torch.tensor([n], dtype=torch.int32, device=dev))
    return idx.view(n), m


def _gather_byte_rows(src, idx):
    """dst[i] = src[idx[i]] for rows of bytes (m, row_bytes).  ss_gather_rows moves lanes of 2 bytes at least, so a row of an odd
    width (a uint8 / int8 / bool label, a uint8 (m, 3) colour) goes through the grouped gather of csrc/chunking.hip, which has a byte lane."""
    n, row_bytes = idx.numel(), src.shape[1]
    if n == 0 or row_bytes == 0:
        return torch.empty((n, row_bytes), dtype=torch.uint8, device=src.device)
    if row_bytes % 2 == 0:
        return nv.gather_rows(src, idx)
    dst = torch.empty((n, row_bytes), dtype=torch.uint8, device=src.device)
    m = src.shape[0]
    nv.chunk_gather_group(np.array([[src.data_ptr(), dst.data_ptr(), idx.data_ptr(), n, row_bytes, 0, m, m]], dtype=np.int64), src.device)
    return dst


def scan_box(points, margin, device):
    """the minimal oriented box of a scan's points ((m, 3) float32, numpy or device) grown by margin.  ValueError: no volume."""
    return oriented_box.minimal_oriented_box(points, device).enlarged(margin)


def prune_gaussians(gs, box):
    """load_gaussian_ply's result without the Gaussians outside `box` (an OrientedBox): -> (the kept Gaussians, still in file order;
    the kept rows, ascending int32 on the device).  Prints the reference's line."""
    kept = oriented_box.points_within_box(box, gs["coord"])
    n = gs["coord"].shape[0]
    print(f"  Pruned {n - kept.numel()} gaussians by init bounding box.")
    out = OrderedDict()
    for k, t in gs.items():
        rows = _gather_byte_rows(t.reshape(n, int(np.prod(t.shape[1:]))).view(torch.uint8), kept)
        out[k] = rows.view(t.dtype).view((kept.numel(),) + tuple(t.shape[1:]))
    return out, kept


def _transfer(coord, pc_coord, pc_assets):
    """-> {name: ((n, row_bytes) uint8 device tensor, numpy dtype, trailing shape)}"""
    idx, m = _nearest_rows(coord, pc_coord)
    out = OrderedDict()
    for name, asset in pc_assets.items():
        src, dtype, trailing = _rows_as_bytes(asset, coord.device)
        if src.shape[0] != m:
            raise ValueError(f"transfer_labels: asset '{name}' has {src.shape[0]} rows, the cloud has {m}")
        if name == "segment" and trailing == (1,):
            trailing = ()                                                # the reference squeezes an (m, 1) segment
        out[name] = (_gather_byte_rows(src, idx), dtype, trailing)
    return out


def transfer_labels(coord, pc_coord, pc_assets):
    """For every Gaussian of coord (n, 3) f32 (device) the nearest point of pc_coord (m, 3) (numpy or tensor), and every asset of
    pc_assets {name: (m, ...) array of any dtype} gathered by it: -> {name: (n, ...) device tensor of the asset's dtype}."""
    out = OrderedDict()
    for name, (rows, dtype, trailing) in _transfer(coord, pc_coord, pc_assets).items():
        try:
            tdtype = torch.from_numpy(np.empty(0, dtype=dtype)).dtype
        except TypeError:
            raise ValueError(f"no device form: asset '{name}' of dtype {dtype} has no torch dtype") from None
        out[name] = rows.view(-1).view(tdtype).view((rows.shape[0],) + tuple(trailing)) if rows.numel() else torch.empty(
            (rows.shape[0],) + tuple(trailing), dtype=tdtype, device=rows.device)
    return out


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------------
def collect_ply_files(input, output, recursive=False):
    """-> [(ply path, output directory)] by the rule of the reference's command line: a single file writes into `output` itself, a
    directory into output / relative parent / stem"""
    input, output = Path(input), Path(output)
    if input.is_file() and input.suffix == ".ply":
        return [(input, output)]
    if input.is_dir():
        files = sorted(input.rglob("*.ply") if recursive else input.glob("*.ply"))
        return [(f, output / f.relative_to(input).parent / f.stem) for f in files]
    raise ValueError(f"{input}: neither a .ply file nor a directory")


def _load_features(feat):
    """-> lang_feat (n, width) float16 of a langfeat.pth (holding (features, _)) or a .npy"""
    feat = os.fspath(feat)
    if feat.endswith(".npy"):
        return np.load(feat).astype(np.float16)
    features, _ = torch.load(feat, map_location="cpu")
    return features.to(torch.float16).numpy()


def preprocess_gs(input, output, recursive=False, pc_dir=None, feat=None, device=None, prune_box=None):
    """scripts/preprocess_gs.py on the device; with pc_dir (coord.npy + any of segment / normal / instance .npy) the nearest-neighbour
    label transfer of preprocess_holicity_gs.py, with feat its lang_feat.npy (float16) and valid_feat_mask.npy (int64).  prune_box = m
    (the reference's 0.25; needs pc_dir): only the Gaussians inside the minimal oriented box of pc_dir's coord.npy grown by m are
    written, in file order, and the labels are transferred to those alone; None writes all.  A file that does not parse, or a cloud
    without a box, is reported and skipped.  -> the directories written."""
    if prune_box is not None and pc_dir is None:
        raise ValueError("preprocess_gs: prune_box needs pc_dir (the box is the labelled cloud's)")
    files = collect_ply_files(input, output, recursive)
    if not files:
        print(f"{input}: no .ply file in it")
        return []
    print(f"{len(files)} checkpoint(s) to convert")
    cloud = None
    if pc_dir is not None:
        pc_coord = np.load(os.path.join(pc_dir, "coord.npy"))
        cloud = (pc_coord, OrderedDict((a, np.load(os.path.join(pc_dir, a + ".npy"))) for a in PC_ASSETS
                                       if os.path.exists(os.path.join(pc_dir, a + ".npy"))))
    all_lang = _load_features(feat) if feat is not None else None
    written, box = [], None
    for ply_path, out_dir in files:
        print(f"{ply_path}:")
        try:
            gs = load_gaussian_ply(ply_path, device)
        except (ValueError, KeyError, OSError) as e:
            print(f"  skipped, it could not be read: {e!r}")
            continue
        n = gs["coord"].shape[0]
        lang = all_lang
        if lang is not None and lang.shape[0] != n:
            raise ValueError(f"{ply_path}: {n} Gaussians, but {feat} holds {lang.shape[0]} feature rows")
        if prune_box is not None:
            try:
                if box is None:                                           # one cloud, one box
                    box = scan_box(cloud[0], prune_box, gs["coord"].device)
            except ValueError as e:
                print(f"  skipped, it could not be read: {e!r}")
                continue
            gs, kept = prune_gaussians(gs, box)
            n = kept.numel()
            if lang is not None:
                lang = lang[kept.cpu().numpy()]
        arrays = OrderedDict((k, gs[k].cpu().numpy()) for k in GS_ASSETS)
        if cloud is not None:
            for name, (rows, dtype, trailing) in _transfer(gs["coord"], *cloud).items():
                arrays[name] = rows.cpu().numpy().reshape(-1).view(dtype).reshape((n,) + tuple(trailing))
        if lang is not None:
            arrays["lang_feat"] = lang
            arrays["valid_feat_mask"] = np.any(lang != 0.0, axis=1).astype(np.int64)
        out_dir.mkdir(parents=True, exist_ok=True)
        for name, a in arrays.items():
            np.save(out_dir / (name + ".npy"), a)
        print(f"  {n} Gaussians -> {out_dir} ({', '.join(arrays)})")
        written.append(str(out_dir))
    return written


def build_parser():
    parser = argparse.ArgumentParser(description="3DGS checkpoints (.ply) to scene folders of .npy assets, decoded on the GPU (the arguments of scripts/preprocess_gs.py)")
    parser.add_argument("--input", required=True, help="one checkpoint (.ply), or a folder of them")
    parser.add_argument("--output", required=True, help="where the scene folder(s) go: the folder itself for one file, one sub-folder per checkpoint for a folder")
    parser.add_argument("--recursive", action="store_true", help="with a folder: take the checkpoints of its sub-folders too")
    parser.add_argument("--pc_dir", default=None, help="labelled point cloud folder (coord.npy + segment / normal / instance .npy) to transfer from")
    parser.add_argument("--feat", default=None, help="language features of the Gaussians: langfeat.pth holding (features, _), or a .npy")
    parser.add_argument("--prune_box", nargs="?", const=0.25, default=None, type=float,
                        help="keep only the Gaussians inside the minimal oriented box of --pc_dir's cloud grown by this margin (0.25 when no value is given)")
    return parser


def main(argv=None):
    cfg = build_parser().parse_args(argv)
    done = preprocess_gs(cfg.input, cfg.output, recursive=cfg.recursive, pc_dir=cfg.pc_dir, feat=cfg.feat,
                         **({} if cfg.prune_box is None else dict(prune_box=cfg.prune_box)))
    print(f"{len(done)} scene folder(s) written")
    return 0 if done else 1


if __name__ == "__main__":
    raise SystemExit(main())
