"""Scene chunking on the device: the step between a preprocessed scene folder and the chunked splits the shipped configs read
(`train_grid1.0cm_chunk6x6_stride3x3`, ...).

Mirror of pointcept/datasets/preprocessing/sampling_chunking_data_gs.py (`chunking_scene` and its command line): the same positional
arguments, the same directory and file names, and, wherever the reference is deterministic, the same bytes in every file.

    *.npy --np.load--> stored dtypes --pack (native.ingest_plan)--> pinned --one copy--> device arena
      -> extent, recentred coord                    (membership only: the saved coord is the original)
      -> lang_feat[valid_feat_mask == 1] /= norm    (in place in the arena, before any subsampling)
      -> grid subsample: one row per occupied cell  (cells in first-occurrence order; `pick`, never a subsampled copy of the scene)
      -> membership of every row in ALL chunks, row lists in ascending row order, counts  --one read--> minimum size, max_chunk_num
      -> grouped gather of (chunk, asset) problems into a staging buffer of at most `staging_bytes` --one download per batch--> np.save

Differences from the reference, all of them where it is not deterministic itself:
* with `grid_size` and a `valid_feat_mask`, the reference draws the kept row of a cell from numpy's global generator, one draw per
  cell in a host loop.  Here the kept row is the cell's valid row number Philox4x32-10(seed, smallest row of the cell) mod n_valid,
  counted in ascending row order (a cell without a valid row keeps its first row, as there);
* `max_chunk_num`: the reference orders the chunks by `argsort(counts)[::-1]` with numpy's default (unstable) sort, so the order
  among equal counts is unspecified.  Here: descending count, equal counts in descending origin index;
* lang_feat rows are normalised with fp32 sums and ONE rounding to the storage dtype (numpy's fp16 arithmetic rounds after every
  operation and lies up to 2 fp16 ulp from the exact quotient: profiles/chunking.md).

`coord` must be (n, 3) float32 (what every converter of the reference writes); every other asset keeps its dtype and trailing shape.
There are no worker processes: one process per GPU (`--num_workers` / `--single_process` are accepted and ignored)."""
import argparse
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from .. import native as nv

STAGE_ALIGN = 64        # offsets of the (chunk, asset) blocks in the staging buffer: the 16-byte path of the gather, whole cache lines
_VALID = "<valid>"      # the arena's name for (valid_feat_mask == 1) as bytes (no file can have it: the assets are *.npy stems)
PROFILE = None          # a dict while scripts/bench_chunking.py measures: seconds spent in np.load ("read") and np.save ("write")


def _timed(key, fn, *args):
    if PROFILE is None:
        return fn(*args)
    t0 = time.perf_counter()
    out = fn(*args)
    PROFILE[key] = PROFILE.get(key, 0.0) + time.perf_counter() - t0
    return out


# ---- host side: names, origins, selection (pure numpy: what tests/test_chunking_host.py checks) ------------------------------------
def split_dir_name(split, grid_size, chunk_range, chunk_stride):
    """sampling_chunking_data_gs.py:131-143"""
    grid = f"grid{grid_size * 100:.1f}cm_" if grid_size is not None else ""
    return f"{split}_{grid}chunk{chunk_range[0]}x{chunk_range[1]}_stride{chunk_stride[0]}x{chunk_stride[1]}"


def chunk_origins(bev_max, chunk_range, chunk_stride):
    """The reference's own expression (sampling_chunking_data_gs.py:84-92), so the end points of `arange` agree bit for bit.
    bev_max: the x and y maxima of the recentred (and subsampled) coord as np.float32.  -> (xs (nx,), ys (ny,)) float64; chunk
    ix * ny + iy starts at (xs[ix], ys[iy]).  A room smaller than range - stride has no origin."""
    bx, by = np.float32(bev_max[0]), np.float32(bev_max[1])
    xs = np.arange(0, bx + chunk_stride[0] - chunk_range[0], chunk_stride[0])
    ys = np.arange(0, by + chunk_stride[1] - chunk_range[1], chunk_stride[1])
    return xs.astype(np.float64), ys.astype(np.float64)


def origin_table(xs, ys):
    """(nx * ny, 2): the reference's `chunks` array (meshgrid with indexing="ij")"""
    x, y = np.meshgrid(xs, ys, indexing="ij")
    return np.concatenate([x.reshape([-1, 1]), y.reshape([-1, 1])], axis=-1)


def select_chunks(counts, chunk_minimum_size, max_chunk_num=None):
    """-> the origin indices that are written, in chunk-number order (sampling_chunking_data_gs.py:95-128).  With max_chunk_num below
    the number of origins: the max_chunk_num fullest chunks, descending count, equal counts in descending origin index (module
    docstring).  A chunk below chunk_minimum_size is skipped and takes no number."""
    counts = np.asarray(counts).reshape(-1)
    order = np.arange(counts.shape[0])
    if max_chunk_num is not None and counts.shape[0] > max_chunk_num:
        order = np.argsort(counts, kind="stable")[::-1][:max_chunk_num]
    return [int(c) for c in order if counts[c] >= chunk_minimum_size]


def slots_per_row(chunk_range, chunk_stride):
    """the most chunks one row can lie in: ceil(range / stride) per axis"""
    return int(-(-chunk_range[0] // chunk_stride[0])) * int(-(-chunk_range[1] // chunk_stride[1]))


def load_scene(scene_path):
    """every *.npy of the folder, in listing order, whatever its dtype and trailing shape"""
    arrays = OrderedDict()
    for asset in os.listdir(scene_path):
        if asset.endswith(".npy"):
            arrays[asset[:-4]] = _timed("read", np.load, os.path.join(scene_path, asset))
    return arrays


def check_assets(arrays):
    """-> n = coord's rows; ValueError names an asset whose leading dimension differs"""
    if "coord" not in arrays:
        raise ValueError("chunk_scene: the scene has no coord.npy")
    coord = arrays["coord"]
    if coord.ndim != 2 or coord.shape[1] != 3 or coord.dtype != np.float32:
        raise ValueError(f"chunk_scene: 'coord' must be (n, 3) float32, got {coord.shape} {coord.dtype}")
    n = coord.shape[0]
    if n == 0:
        raise ValueError("chunk_scene: 'coord' has no rows")
    for name, a in arrays.items():
        if a.ndim == 0 or a.shape[0] != n:
            raise ValueError(f"chunk_scene: asset '{name}' has leading dimension {a.shape[0] if a.ndim else None}, coord has {n}")
    if "lang_feat" in arrays:
        if "valid_feat_mask" not in arrays:
            raise ValueError("chunk_scene: 'lang_feat' needs 'valid_feat_mask'")
        lf = arrays["lang_feat"]
        if lf.ndim != 2 or lf.dtype not in (np.float16, np.float32):
            raise ValueError(f"chunk_scene: 'lang_feat' must be (n, width) float16 | float32, got {lf.shape} {lf.dtype}")
    if "valid_feat_mask" in arrays and arrays["valid_feat_mask"].size != n:
        raise ValueError(f"chunk_scene: asset 'valid_feat_mask' has {arrays['valid_feat_mask'].size} elements, coord has {n} rows")
    return n


# ---- device side -----------------------------------------------------------------------------------------------------------------------
def _upload(arrays, n, dev):
    """One packed upload.  Every asset travels as its (n, row_bytes) bytes, so any stored dtype has a device form and none is converted.
    -> (arena, {name: byte offset}, [(name, dtype, trailing shape, row_bytes)])"""
    packed, assets = OrderedDict(), []
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        row_bytes = a.nbytes // n
        assets.append((name, a.dtype, a.shape[1:], row_bytes))
        packed[name] = a.reshape(-1).view(np.uint8)
    if "valid_feat_mask" in arrays:
        packed[_VALID] = (arrays["valid_feat_mask"].reshape(-1) == 1).astype(np.uint8)
    _, offsets, specs, _ = nv.ingest_plan(packed, {})
    total = offsets[""]
    host = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
    view = host.numpy()
    for spec in specs:
        off = offsets[spec["stored"]]
        view[off:off + spec["array"].nbytes] = spec["array"]
    arena = host.to(dev, non_blocking=True)
    torch.cuda.current_stream().synchronize()          # (the pinned source is released when this function returns)
    return arena, offsets, assets


def _typed(arena, off, nbytes, dtype, shape):
    return arena[off:off + nbytes].view(dtype).view(shape)


def subsample_rows(rec, grid_size, extent_max, valid, seed):
    """One row per occupied cell of floor(rec / grid_size), the cells in first-occurrence order.  rec (n, 3) f32 recentred; extent_max:
    its column maxima (np.float32 x 3, the host's copy); valid (n) uint8 | None.  -> pick (m,) int32 rows of the scene."""
    n = rec.shape[0]
    cell_max = np.floor(np.asarray(extent_max, dtype=np.float32) / np.float32(grid_size))
    if not np.isfinite(cell_max).all():
        raise ValueError("chunk_scene: grid_size is too small for the extent of the scene")
    bits = [max(1, int(c).bit_length()) for c in cell_max]
    if sum(bits) > 63:
        raise ValueError(f"chunk_scene: the cells of grid_size={grid_size} need {bits} bits per axis, more than one int64 key packs")
    status = torch.zeros(1, dtype=torch.int32, device=rec.device)
    keys = nv.chunk_cell_keys(rec, grid_size, bits, status)
    order = nv.argsort_i64(keys.view(1, n), sum(bits), want_inverse=False, want_sorted=False)[0][0]
    _, idx_ptr, _, n_out = nv.pool_partition(keys, order, 0)
    flags = torch.stack([n_out[0], status[0]]).cpu()
    m = int(flags[0])
    if int(flags[1]):
        raise ValueError("chunk_scene: a coordinate is NaN or outside the extent of the scene")
    first, pick = nv.chunk_cell_pick(order, idx_ptr, m, valid, seed)
    by_first = nv.argsort_i64(first.view(1, m), max(1, int(n).bit_length()), want_inverse=False, want_sorted=False)[0][0]
    return nv.gather_rows(pick.view(m, 1), by_first).view(m)


def chunk_rows(rec, pick, xs, ys, chunk_range, chunk_stride):
    """Membership of every (picked) row in every chunk at once.  -> (counts (nchunk,) and offsets (nchunk + 1,) as numpy, rows: device
    int32, chunk c's rows of the (subsampled) scene, ascending, at rows[offsets[c]:offsets[c + 1]])."""
    nx, ny, slots = len(xs), len(ys), slots_per_row(chunk_range, chunk_stride)
    bounds = np.concatenate([xs, xs + chunk_range[0], ys, ys + chunk_range[1]]).astype(np.float64)
    bounds = torch.from_numpy(bounds).to(rec.device)
    status = torch.zeros(1, dtype=torch.int32, device=rec.device)
    slot_keys, counts = nv.chunk_membership(rec, pick, bounds, nx, ny, slots, status)
    offsets = nv.chunk_offsets(counts)
    m = slot_keys.shape[0]
    slot_order = nv.argsort_i64(slot_keys.view(1, m * slots), max(1, int(nx * ny).bit_length()), want_inverse=False, want_sorted=False)[0][0]
    host = torch.cat([offsets, counts.to(torch.int64), status.to(torch.int64)]).cpu().numpy()      # the one read of the counts
    offsets_h, counts_h = host[:nx * ny + 1], host[nx * ny + 1:-1]
    if host[-1]:
        raise RuntimeError("chunk_scene: a row lies in more chunks than ceil(range / stride) per axis allows")
    rows = nv.chunk_slot_rows(slot_order, int(offsets_h[-1]), slots)
    return counts_h, offsets_h, rows


def chunk_scene(name, dataset_root, output_dir, split, grid_size=None, chunk_range=(6, 6), chunk_stride=(3, 3), chunk_minimum_size=10000,
                max_chunk_num=None, *, seed=0, device="cuda", staging_bytes=1 << 30):
    """chunking_scene of the reference on the device (module docstring).  -> the chunk directories written, in chunk order."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("chunk_scene: scenes are chunked on the GPU (device='cuda'); there is no CPU fallback")
    arrays = load_scene(os.path.join(dataset_root, split, name))
    n = check_assets(arrays)
    root = os.path.join(output_dir if output_dir is not None else dataset_root, split_dir_name(split, grid_size, chunk_range, chunk_stride))
    with torch.cuda.device(dev):
        dev = torch.device("cuda", torch.cuda.current_device())
        arena, offsets, assets = _upload(arrays, n, dev)
        del arrays
        coord = _typed(arena, offsets["coord"], n * 12, torch.float32, (n, 3))
        valid = arena[offsets[_VALID]:offsets[_VALID] + n] if _VALID in offsets else None
        extent = nv.chunk_extent(coord)
        rec = nv.chunk_recentre(coord, extent)
        for a_name, dtype, trailing, row_bytes in assets:
            if a_name == "lang_feat" and row_bytes:
                lang = _typed(arena, offsets[a_name], n * row_bytes, torch.float16 if dtype == np.float16 else torch.float32, (n, trailing[0]))
                nv.chunk_lang_normalize_(lang, valid)
        ext = extent.cpu().numpy()                         # the small read of the extent
        ext_max = ext[3:] - ext[:3]                        # fp32: rounding is monotonic, so this is the maximum of the recentred copy
        pick = None
        if grid_size is not None:
            pick = subsample_rows(rec, grid_size, ext_max, valid, seed)
            ext = nv.chunk_extent(rec, pick).cpu().numpy()
            ext_max = ext[3:]
        xs, ys = chunk_origins(ext_max[:2], chunk_range, chunk_stride)
        if len(xs) == 0 or len(ys) == 0:
            return []
        counts, row_off, rows = chunk_rows(rec, pick, xs, ys, chunk_range, chunk_stride)
        kept = select_chunks(counts, chunk_minimum_size, max_chunk_num)
        return _write_chunks(root, name, kept, counts, row_off, rows, pick, arena, offsets, assets, n, dev, int(staging_bytes))


def _write_chunks(root, name, kept, counts, row_off, rows, pick, arena, offsets, assets, n, dev, staging_bytes):
    """Gather the kept chunks batch by batch into the staging buffer, download each batch once and np.save views of it."""
    def aligned(nbytes):
        return -(-nbytes // STAGE_ALIGN) * STAGE_ALIGN

    problems = [(k, c, a) for k, c in enumerate(kept) for a in assets]         # (chunk number, origin index, asset)
    sizes = [aligned(int(counts[c]) * a[3]) for _, c, a in problems]
    if sizes and max(sizes) > staging_bytes:
        raise ValueError(f"chunk_scene: staging_bytes={staging_bytes} is smaller than one asset of one chunk ({max(sizes)} bytes)")
    batches, cur, used = [], [], 0                                             # a batch: [(problem, offset in the staging buffer)], its bytes
    for prob, size in zip(problems, sizes):
        if cur and used + size > staging_bytes:
            batches.append((cur, used))
            cur, used = [], 0
        cur.append((prob, used))
        used += size
    if cur:
        batches.append((cur, used))
    capacity = max([end for _, end in batches], default=0)
    stage_d = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
    stage_h = torch.empty(max(capacity, 1), dtype=torch.uint8).pin_memory()
    host = stage_h.numpy()
    base, stage, rows_ptr = arena.data_ptr(), stage_d.data_ptr(), rows.data_ptr()
    pick_ptr, pick_rows = (pick.data_ptr(), pick.numel()) if pick is not None else (0, n)
    dirs = []
    for batch, end in batches:
        desc = np.array([(base + offsets[a[0]], stage + off, rows_ptr + 4 * int(row_off[c]), int(counts[c]), a[3], pick_ptr, n, pick_rows)
                         for (_, c, a), off in batch if a[3] > 0], dtype=np.int64).reshape(-1, 8)      # (empty rows: nothing to move)
        nv.chunk_gather_group(desc, dev)
        stage_h[:end].copy_(stage_d[:end], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        for (k, c, (a_name, dtype, trailing, row_bytes)), off in batch:
            path = os.path.join(root, f"{name}_{k}")
            if not dirs or dirs[-1] != path:
                os.makedirs(path, exist_ok=True)
                dirs.append(path)
            cnt = int(counts[c])
            _timed("write", np.save, os.path.join(path, a_name + ".npy"), host[off:off + cnt * row_bytes].view(dtype).reshape((cnt,) + tuple(trailing)))
    return dirs


def chunk_split(dataset_root, split, output_dir=None, subset_list=None, **kwargs):
    """chunk_scene over the scenes of dataset_root/split (the reference's command-line loop).  subset_list: a text file with one scene
    name per line, or an iterable of names; None: every scene.  -> {scene name: its chunk directories}"""
    names = sorted(os.listdir(os.path.join(dataset_root, split)))
    if subset_list is not None:
        if isinstance(subset_list, (str, os.PathLike)):
            with open(subset_list) as f:
                subset_list = {line.strip() for line in f if line.strip()}
        keep = set(subset_list)
        names = [s for s in names if s in keep]
    return {s: chunk_scene(s, dataset_root, output_dir, split, **kwargs) for s in names}


# ---- command line: the reference's argument names ---------------------------------------------------------------------------------------
def build_parser():
    parser = argparse.ArgumentParser(description="Chunk the scenes of a split on the GPU (sampling_chunking_data_gs.py)")
    parser.add_argument("--dataset_root", required=True, help="the preprocessed dataset (split folders of scene folders of .npy assets)")
    parser.add_argument("--output_dir", default=None, help="where the chunked split goes (default: dataset_root)")
    parser.add_argument("--split", required=True, type=str, help="the split to process")
    parser.add_argument("--grid_size", default=None, type=float, help="grid size of the initial grid sampling")
    parser.add_argument("--chunk_range", default=[6, 6], type=int, nargs="+", help="range of a chunk, e.g. --chunk_range 6 6")
    parser.add_argument("--chunk_stride", default=[3, 3], type=int, nargs="+", help="stride between chunks, e.g. --chunk_stride 3 3")
    parser.add_argument("--chunk_minimum_size", default=10000, type=int, help="fewest rows of a chunk that is written")
    parser.add_argument("--num_workers", default=1, type=int, help="accepted and ignored: one process per GPU")
    parser.add_argument("--subset_list", type=str, default=None, help="text file of the scene names to process (default: all)")
    parser.add_argument("--max_chunk_num", type=int, default=None, help="keep only this many chunks of a scene, the fullest first")
    parser.add_argument("--single_process", action="store_true", help="accepted and ignored")
    parser.add_argument("--seed", type=int, default=0, help="seed of the per-cell pick among valid rows")
    return parser


def main(argv=None):
    cfg = build_parser().parse_args(argv)
    done = chunk_split(cfg.dataset_root, cfg.split, cfg.output_dir, cfg.subset_list, grid_size=cfg.grid_size, chunk_range=cfg.chunk_range,
                       chunk_stride=cfg.chunk_stride, chunk_minimum_size=cfg.chunk_minimum_size, max_chunk_num=cfg.max_chunk_num,
                       seed=cfg.seed)
    for scene, dirs in done.items():
        print(f"{scene}: {len(dirs)} chunks")


if __name__ == "__main__":
    main()
