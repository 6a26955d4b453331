"""Text queries on saved scene features, on the device (the reference's roadmap task "Text-based Scene Query" and its documented
tools/text_to_geometry.py; the reference carries no program for it: the definition is DESIGN.md 8t).

    from scenesplat_amd.pointcept_api import query_scene, load_text_queries, extract_geometry
    emb = load_text_queries("scannet20_text_embeddings_siglip2.pt", "scannet20_labels.txt", ["chair", "table"])
    out = query_scene(features, emb, method="threshold", threshold=0.15, max_points=30000)
    out["indices"][0]                          # ascending int32 rows of the Gaussians that answer "chair", on the device
    extract_geometry("scene0011_00", out, "out", ["chair", "table"])

One pass over the (N, D) features scores every Gaussian against all the queries (csrc/text_query.hip: cosine scores on the fp32 MFMA),
an exact radix select cuts a selection to its best rows, and the bitmaps become ascending row lists through the compaction kernels of
csrc/pc_attach.hip.  The features never leave the device.  Two small host reads per call: the (Q, 3) statistics after the score pass
(the adaptive threshold is worked out from them in fp64) and the Q counts and thresholds after the select pass.

Free text is not encoded here: that needs the SigLIP text tower, whose weights this project does not carry.  The queries are rows of an
embeddings file (the reference's *_text_embeddings_*.pt) looked up by class name.

    python -m scenesplat_amd.pointcept_api.text_query SCENE_DIR --features scene_feat.pth --embeddings E.pt --class-names names.txt \\
        --queries chair table --threshold 0.15 --max-points 30000 --save-individual --output out
"""
import argparse
import os

import numpy as np
import torch

from .. import _lib

MAX_DIM = _lib.CONSTANTS["SS_QUERY_MAX_DIM"]
MAX_QUERIES = _lib.CONSTANTS["SS_QUERY_MAX_QUERIES"]
METHODS = ("threshold", "topk", "adaptive")
SCENE_ARRAYS = ("coord", "color", "opacity", "scale", "quat", "normal")
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# the reference's documented example
DEFAULT_THRESHOLD = 0.15
PALETTE = ((0.90, 0.10, 0.10), (0.10, 0.60, 0.90), (0.10, 0.75, 0.20), (0.95, 0.75, 0.10), (0.60, 0.20, 0.80), (0.95, 0.45, 0.10),
           (0.10, 0.80, 0.75), (0.85, 0.25, 0.60))


# ---- the definition's host steps ----------------------------------------------------------------------------------------------------
def unit_rows(text_embeddings):
    """step 1 on the host: T (Q, D) -> T / max(|T|, 1e-12) per row in fp64, rounded to fp32 once"""
    t = np.asarray(text_embeddings, dtype=np.float64)
    norm = np.sqrt((t * t).sum(axis=1, keepdims=True))
    return (t / np.maximum(norm, 1e-12)).astype(np.float32)


def adaptive_threshold(stats, kappa=2.0, floor=0.0):
    """step 3: stats (Q, 3) = {L, sum s, sum s^2} -> fp32 max(mu + kappa sigma, floor) per query; +inf where L == 0"""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 3)
    tau = np.full(stats.shape[0], np.inf, dtype=np.float32)
    for q, (L, s1, s2) in enumerate(stats):
        if L > 0:
            mu = s1 / L
            sigma = np.sqrt(max(s2 / L - mu * mu, 0.0))
            tau[q] = np.float32(max(mu + kappa * sigma, floor))
    return tau


def _as_embeddings(text_embeddings):
    if isinstance(text_embeddings, torch.Tensor):
        text_embeddings = text_embeddings.detach().to("cpu", torch.float64).numpy()
    t = np.asarray(text_embeddings, dtype=np.float64)
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2:
        raise ValueError(f"text_embeddings must be (Q, D) or (D,), got {t.shape}")
    return t


def _validate(shape, t, method, threshold, k, kappa, floor, max_points, valid_mask):
    if len(shape) != 2:
        raise ValueError(f"features must be (N, D), got {tuple(shape)}")
    n, D = shape
    if n < 1:
        raise ValueError("features has no rows")
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"D = {D} is outside 1..SS_QUERY_MAX_DIM = {MAX_DIM}")
    if t.shape[1] != D:
        raise ValueError(f"text_embeddings have {t.shape[1]} columns, features have {D}")
    if not 1 <= t.shape[0] <= MAX_QUERIES:
        raise ValueError(f"Q = {t.shape[0]} is outside 1..SS_QUERY_MAX_QUERIES = {MAX_QUERIES}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if method == "topk":
        if k is None:
            raise ValueError("method='topk' needs k")
        if int(k) != k or k < 0:
            raise ValueError(f"k must be a non-negative integer, got {k!r}")
    if max_points is not None and (int(max_points) != max_points or max_points < 0):
        raise ValueError(f"max_points must be a non-negative integer, got {max_points!r}")
    for name, v in (("threshold", threshold), ("kappa", kappa), ("floor", floor)):
        if not np.isfinite(float(v)):
            raise ValueError(f"{name} must be finite, got {v!r}")
    if valid_mask is not None and tuple(valid_mask.shape) != (n,):
        raise ValueError(f"valid_mask must be ({n},), got {tuple(valid_mask.shape)}")


def _features_on_device(features, device):
    if isinstance(features, np.ndarray):
        if features.dtype not in (np.float32, np.float16):
            features = features.astype(np.float32)
        features = torch.from_numpy(np.ascontiguousarray(features))
    if not features.is_cuda:
        features = features.to(device if device is not None else "cuda")
    if features.dtype not in _DTYPES:
        features = features.float()
    return features.contiguous()


def query_scene(features, text_embeddings, method="threshold", threshold=DEFAULT_THRESHOLD, k=None, kappa=2.0, floor=0.0, max_points=None,
                valid_mask=None, return_scores=False, device=None):
    """features (N, D): a device tensor, a CPU tensor or a numpy array (uploaded once); text_embeddings (Q, D) or (D,) -> dict(indices:
    Q ascending int32 device tensors, counts (Q,) int64 numpy, thresholds (Q,) fp32 numpy, best (N,) int32 on the device (the selecting
    query of highest score, -1: none), num_live (int), and scores (Q, N) fp32 on the device when asked).  DESIGN.md 8t.
    ValueError: shapes, D / Q limits, an unknown method, k missing for topk, negative k / max_points."""
    if not isinstance(features, (np.ndarray, torch.Tensor)):
        raise TypeError(f"features: a torch tensor or a numpy array, got {type(features).__name__}")
    t = _as_embeddings(text_embeddings)
    if valid_mask is not None and not isinstance(valid_mask, torch.Tensor):
        valid_mask = torch.from_numpy(np.ascontiguousarray(np.asarray(valid_mask)))
    _validate(features.shape, t, method, threshold, k, kappa, floor, max_points, valid_mask)
    on_device = isinstance(features, torch.Tensor) and features.is_cuda
    if not on_device and device is None and not torch.cuda.is_available():
        raise RuntimeError("query_scene runs on the device: no GPU is available (there is no CPU fallback)")
    from .. import native as nv
    x = _features_on_device(features, device)
    N, Q = x.shape[0], t.shape[0]
    valid = None
    if valid_mask is not None:
        valid = (valid_mask.to(x.device) != 0).to(torch.uint8).contiguous()
    t_hat = torch.from_numpy(unit_rows(t)).to(x.device)
    scores, stats = nv.query_scores(x, t_hat, valid)
    stats_h = stats.cpu().numpy()                                        # host read 1
    if method == "threshold":
        tau = np.full(Q, np.float32(threshold), dtype=np.float32)
    elif method == "adaptive":
        tau = adaptive_threshold(stats_h, kappa, floor)
    else:
        tau = np.full(Q, -np.inf, dtype=np.float32)
    cap = int(k) if method == "topk" else (-1 if max_points is None else int(max_points))
    if method == "topk" and max_points is not None:
        cap = min(cap, int(max_points))
    bitmap, tau_out, counts = nv.query_select(scores, tau, np.full(Q, cap, dtype=np.int64))
    down = torch.cat([counts.to(torch.float64), tau_out.to(torch.float64)]).cpu().numpy()      # host read 2
    counts_h, tau_h = down[:Q].astype(np.int64), down[Q:].astype(np.float32)
    indices = _bitmap_rows(nv, bitmap, N, counts_h)
    out = dict(indices=indices, counts=counts_h, thresholds=tau_h, best=nv.query_best(scores, bitmap), num_live=int(stats_h[0, 0]))
    if return_scores:
        out["scores"] = scores
    return out


def _bitmap_rows(nv, bitmap, N, counts):
    """the Q ascending row lists of a (Q, words) bitmap: ss_pc_compact_scan / ss_pc_compact over as many queries at a time as their
    int32 positions allow; the counts are known already, so nothing is read back here"""
    Q, words = bitmap.shape
    step = max(1, min(Q, (2 ** 31 - 1) // (words * 32)))
    out = []
    for q0 in range(0, Q, step):
        part = bitmap[q0:q0 + step]
        tile_base, _ = nv.pc_compact_scan(part, N)
        rows = nv.pc_compact(part, N, tile_base, int(counts[q0:q0 + step].sum()))
        out.extend(torch.split(rows, [int(c) for c in counts[q0:q0 + step]]))
    return list(out)


# ---- the embeddings file ------------------------------------------------------------------------------------------------------------
def read_class_names(path):
    with open(path, "r") as f:
        return [line.strip() for line in f if line.strip()]


def load_text_queries(embeddings_path, class_names_path, queries):
    """the rows of the reference's *_text_embeddings_*.pt ((C, D) tensor) for the class names `queries` (names file: one per line) ->
    (len(queries), D) fp32 numpy.  KeyError for a name the file does not hold."""
    names = read_class_names(class_names_path)
    emb = torch.load(embeddings_path, map_location="cpu", weights_only=True)
    emb = emb.detach().float().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb, dtype=np.float32)
    if emb.ndim != 2 or emb.shape[0] != len(names):
        raise ValueError(f"{embeddings_path}: expected ({len(names)}, D) embeddings for the {len(names)} names of {class_names_path}, "
                         f"got {tuple(emb.shape)}")
    if isinstance(queries, str):
        queries = [queries]
    row = {name: i for i, name in reversed(list(enumerate(names)))}
    unknown = [q for q in queries if q not in row]
    if unknown:
        raise KeyError(f"unknown class name(s) {unknown}; known: {names}")
    return np.ascontiguousarray(emb[[row[q] for q in queries]])


# ---- the writer ---------------------------------------------------------------------------------------------------------------------
def _load_scene(scene):
    if isinstance(scene, dict):
        return {k: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in scene.items() if k in SCENE_ARRAYS}
    if not os.path.isdir(scene):
        raise FileNotFoundError(f"Scene folder not found: {scene}")
    return {k: np.load(os.path.join(scene, k + ".npy")) for k in SCENE_ARRAYS if os.path.exists(os.path.join(scene, k + ".npy"))}


def _host_indices(result):
    indices = result["indices"] if isinstance(result, dict) else result
    return [np.asarray(i.cpu() if isinstance(i, torch.Tensor) else i).astype(np.int32).reshape(-1) for i in indices]


def _write_folder(folder, arrays, idx, save_ply):
    os.makedirs(folder, exist_ok=True)
    for key, a in arrays.items():
        np.save(os.path.join(folder, key + ".npy"), a[idx])
    if save_ply and "coord" in arrays:
        from .feature_pca import write_ply
        color = arrays["color"][idx].astype(np.float64) if "color" in arrays else np.full((len(idx), 3), 0.5)
        if "color" in arrays and np.issubdtype(arrays["color"].dtype, np.integer):
            color = color / 255.0
        write_ply(os.path.join(folder, "points.ply"), arrays["coord"][idx], color)


def extract_geometry(scene, result, out_dir, names, save_individual=True, save_ply=False):
    """scene: a scene folder or a dict of arrays; result: what query_scene returned, or a list of index arrays (numpy or tensors).
    save_individual: out_dir/<name>/{coord,color,...}.npy per query (the rows of every array the scene has, ascending: a scene folder
    GenericGSDataset reads); else one out_dir/merged/ over the union.  out_dir/<name>_indices.npy always.  -> the folders written."""
    arrays = _load_scene(scene)
    indices = _host_indices(result)
    names = list(names)
    if len(names) != len(indices):
        raise ValueError(f"{len(names)} names for {len(indices)} selections")
    if len(set(names)) != len(names):
        raise ValueError(f"query names repeat: {names}")
    n = {len(a) for a in arrays.values()}
    if len(n) > 1:
        raise ValueError(f"the scene's arrays differ in length: { {k: len(a) for k, a in arrays.items()} }")
    for name, idx in zip(names, indices):
        if n and len(idx) and (idx.min() < 0 or idx.max() >= next(iter(n))):
            raise ValueError(f"{name}: indices outside the scene's {next(iter(n))} rows")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name, idx in zip(names, indices):
        np.save(os.path.join(out_dir, f"{name}_indices.npy"), np.sort(idx))
    if save_individual:
        for name, idx in zip(names, indices):
            folder = os.path.join(out_dir, name)
            _write_folder(folder, arrays, np.sort(idx), save_ply)
            written.append(folder)
    else:
        union = np.unique(np.concatenate(indices)) if indices else np.zeros(0, dtype=np.int32)
        folder = os.path.join(out_dir, "merged")
        _write_folder(folder, arrays, union.astype(np.int32), save_ply)
        written.append(folder)
    return written


def highlight_colors(color, result, palette=None):
    """color (N, 3) (a tensor or an array) with every selected row replaced by its `best` query's palette colour -> a tensor on the
    device of result["best"], in color's dtype (integer colours: the palette times 255)"""
    best = result["best"]
    color = torch.as_tensor(color).to(best.device)
    if color.dim() != 2 or color.shape[0] != best.shape[0] or color.shape[1] != 3:
        raise ValueError(f"color must be ({best.shape[0]}, 3), got {tuple(color.shape)}")
    pal = torch.tensor(PALETTE if palette is None else palette, dtype=torch.float64, device=best.device).reshape(-1, 3)
    if not color.dtype.is_floating_point:
        pal = (pal * 255.0).round()
    pal = pal.to(color.dtype)
    sel = best >= 0
    out = color.clone()
    out[sel] = pal[(best[sel].long() % pal.shape[0])]
    return out


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m scenesplat_amd.pointcept_api.text_query",
                                description="Select the Gaussians of a scene that answer text queries, on the device (no viewer; "
                                            "the queries are class names of an embeddings file: no text encoder here)")
    p.add_argument("scene", help="scene folder (coord.npy, color.npy, ...)")
    p.add_argument("--features", required=True, help="per-Gaussian features: a tester *_feat.pth or a .npy")
    p.add_argument("--embeddings", required=True, help="text embeddings file (*_text_embeddings_*.pt)")
    p.add_argument("--class-names", required=True, help="class names file, one per line, in the order of the embeddings")
    p.add_argument("--queries", nargs="+", required=True, help="class names to query")
    p.add_argument("--method", choices=METHODS, default="threshold")
    p.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD, help="similarity threshold (default: 0.15)")
    p.add_argument("--k", type=int, help="rows per query for --method topk")
    p.add_argument("--kappa", type=float, default=2.0, help="adaptive: mean + kappa * deviation (default: 2.0)")
    p.add_argument("--max-points", type=int, help="keep at most this many rows per query (the best ones)")
    p.add_argument("--save-individual", action="store_true", help="one folder per query (default: one merged folder)")
    p.add_argument("--save-ply", action="store_true", help="also write an x y z red green blue point cloud per folder")
    p.add_argument("--output", required=True, help="output directory")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.method == "topk" and args.k is None:
        parser.error("--k required with --method topk")
    if args.k is not None and args.k < 0:
        parser.error("--k must not be negative")
    if args.max_points is not None and args.max_points < 0:
        parser.error("--max-points must not be negative")
    if len(set(args.queries)) != len(args.queries):
        parser.error("--queries repeat a name")
    if not os.path.isdir(args.scene):
        raise FileNotFoundError(f"Scene folder not found: {args.scene}")
    from .feature_pca import load_features
    emb = load_text_queries(args.embeddings, args.class_names, args.queries)
    features = load_features(args.features)
    print(f"Loaded features {tuple(features.shape)} from {args.features}")
    out = query_scene(features, emb, method=args.method, threshold=args.threshold, k=args.k, kappa=args.kappa, max_points=args.max_points)
    for name, c, tau in zip(args.queries, out["counts"], out["thresholds"]):
        print(f"{name}: {int(c)} of {out['num_live']} Gaussians, threshold {float(tau):.4f}")
    for folder in extract_geometry(args.scene, out, args.output, args.queries, save_individual=args.save_individual, save_ply=args.save_ply):
        print(f"Saved: {folder}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
