"""PCA colours of a feature matrix on the device (the reference's tools/visualize_features_pca.py: sklearn's PCA(n_components <= 3),
each component min-max scaled to [0, 1], the result as RGB on the points).  The definition is DESIGN.md 8r.

    from scenesplat_amd.pointcept_api import pca_colors
    out = pca_colors(features)                 # (N, D) device tensor (fp32 / fp16 / bf16) or a numpy array, D <= 1024
    out["colors"]                              # (N, 3) fp32 on the device

The rows never leave the device: the column sums and the Gram matrix come from csrc/feature_pca.hip (fp32 MFMA products in chains of at
most SS_PCA_GRAM_CHAIN rows, combined in fp64 in a fixed order), the D x D eigen-decomposition runs on the host in fp64
(numpy.linalg.eigh), and the projection, its extremes and the colours are two more passes on the device.  Per call D sums (twice) and
D x D doubles come down, D + k D + k floats go up.

As a tool (the reference's arguments without the Open3D / matplotlib viewers, which are not carried over):

    python -m scenesplat_amd.pointcept_api.feature_pca --features scene_feat.pth --save-colors colors.npy
    python -m scenesplat_amd.pointcept_api.feature_pca --results-dir out --scene-name scene0708_00 --save-ply scene_pca.ply
"""
import argparse
import glob
import os

import numpy as np
import torch

from .. import _lib

MAX_DIM = _lib.CONSTANTS["SS_PCA_MAX_DIM"]
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _check(shape, n_components):
    if n_components not in (1, 2, 3):
        raise ValueError(f"n_components must be 1, 2 or 3, got {n_components!r}")
    if len(shape) != 2:
        raise ValueError(f"features must be (N, D), got {tuple(shape)}")
    n, D = shape
    if n < 2:
        raise ValueError(f"PCA needs at least 2 rows, got {n}")
    if D > MAX_DIM:
        raise ValueError(f"D = {D} is above SS_PCA_MAX_DIM = {MAX_DIM}")
    if n_components > min(n, D):
        raise ValueError(f"n_components = {n_components} is above min(N, D) = {min(n, D)}")


def _on_device(features, n_components, device):
    """validated (N, D) contiguous device tensor in a dtype the kernels read; a numpy array (or CPU tensor) is uploaded once"""
    if isinstance(features, np.ndarray):
        _check(features.shape, n_components)
        if features.dtype not in (np.float32, np.float16):
            features = features.astype(np.float32)
        features = torch.from_numpy(np.ascontiguousarray(features))
    if not isinstance(features, torch.Tensor):
        raise TypeError(f"features: a torch tensor or a numpy array, got {type(features).__name__}")
    _check(features.shape, n_components)
    if not features.is_cuda:
        features = features.to(device if device is not None else "cuda")
    if features.dtype not in _DTYPES:
        features = features.float()
    return features.contiguous()


def sign_fixed(components):
    """svd_flip(u_based_decision=False): in each row the entry of largest magnitude is made positive (equal magnitudes: the lowest index)"""
    components = np.array(components, dtype=np.float64, copy=True)
    for row in components:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1.0
    return components


def components_from_covariance(C, k):
    """steps 2-4 of DESIGN.md 8r: C (D, D) fp64 -> (components (k, D), explained_variance (k,), explained_variance_ratio (k,))"""
    w, v = np.linalg.eigh(np.asarray(C, dtype=np.float64))
    order = np.argsort(-w, kind="stable")[:k]
    components = sign_fixed(v[:, order].T)
    var = w[order]
    return components, var, var / np.trace(C)


def fit_pca(features, n_components=3, device=None):
    """-> dict(components (k, D) f64, mean (D,) f64, explained_variance (k,), explained_variance_ratio (k,), n_components, and what the
    projection needs: features (the device tensor), shift (D,) f32 on the device, offset (k,) f64 = (mean - shift) . components)"""
    from .. import native as nv
    x = _on_device(features, n_components, device)
    n, D = x.shape
    shift64 = nv.pca_col_sums(x).cpu().numpy() / n                       # first-pass mean; its fp32 rounding is the shift
    shift32 = shift64.astype(np.float32)
    shift = torch.from_numpy(shift32).to(x.device)
    down = torch.cat([nv.pca_col_sums(x, shift), nv.pca_gram(x, shift).reshape(-1)]).cpu().numpy()
    d = down[:D] / n                                                      # mean(X - s)
    C = (down[D:].reshape(D, D) - n * np.outer(d, d)) / (n - 1)
    components, var, ratio = components_from_covariance(C, n_components)
    return dict(components=components, mean=shift32.astype(np.float64) + d, explained_variance=var,
                explained_variance_ratio=ratio, n_components=n_components, features=x, shift=shift, offset=components @ d)


def pca_colors(features, n_components=3, device=None):
    """features (N, D): a device tensor or a numpy array -> dict(colors (N, 3) f32 and pca_features (N, k) f32 on the device, components
    (k, D) f64, mean, explained_variance, explained_variance_ratio, n_components).  ValueError: n_components outside {1, 2, 3}, N < 2,
    n_components > min(N, D), D > SS_PCA_MAX_DIM."""
    from .. import native as nv
    fit = fit_pca(features, n_components, device)
    x = fit.pop("features")
    up = torch.from_numpy(np.concatenate([fit["components"].reshape(-1), fit.pop("offset")]).astype(np.float32)).to(x.device)
    k, D = fit["components"].shape
    y, ext = nv.pca_project(x, up[:k * D].view(k, D), fit.pop("shift"), up[k * D:])
    return dict(colors=nv.pca_colors(y, ext), pca_features=y, **fit)


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def load_features(path):
    """.npy, or a tester feat/{name}_feat.pth (a tensor) -> numpy array or CPU tensor"""
    if not os.path.exists(path):
        raise FileNotFoundError(f"Features file not found: {path}")
    if path.endswith((".pth", ".pt")):
        return torch.load(path, map_location="cpu", weights_only=True)
    return np.load(path)


def find_results(results_dir, scene_name):
    """the newest {scene_name}_*_features.npy and {scene_name}_*_coords.npy of a results directory (by modification time)"""
    if not os.path.isdir(results_dir):
        raise FileNotFoundError(f"Results directory not found: {results_dir}")
    found = []
    for kind, what in (("features", "feature"), ("coords", "coordinate")):
        files = glob.glob(os.path.join(glob.escape(results_dir), f"{glob.escape(scene_name)}_*_{kind}.npy"))
        if not files:
            raise FileNotFoundError(f"No {what} files found for scene: {scene_name}")
        found.append(max(files, key=os.path.getmtime))
    return tuple(found)


def write_ply(path, coords, colors):
    """binary little-endian x y z red green blue; colours in [0, 1] -> (c * 255) truncated to uint8"""
    coords = np.asarray(coords, dtype=np.float32).reshape(-1, 3)
    colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if coords.shape[0] != colors.shape[0]:
        raise ValueError(f"{coords.shape[0]} coordinates for {colors.shape[0]} colours")
    rows = np.empty(coords.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, name in enumerate(("x", "y", "z")):
        rows[name] = coords[:, i]
    rgb = np.clip(colors * 255.0, 0.0, 255.0).astype(np.uint8)
    for i, name in enumerate(("red", "green", "blue")):
        rows[name] = rgb[:, i]
    header = ("ply\nformat binary_little_endian 1.0\n" f"element vertex {coords.shape[0]}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rows.tobytes())


def build_parser():
    p = argparse.ArgumentParser(prog="python -m scenesplat_amd.pointcept_api.feature_pca",
                                description="PCA colours of saved features, computed on the device (no viewer)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", help="features .npy, or a tester *_feat.pth")
    src.add_argument("--results-dir", help="results directory to search")
    p.add_argument("--coords", help="coords .npy (needed for --save-ply with --features)")
    p.add_argument("--scene-name", help="scene name to search for (required with --results-dir)")
    p.add_argument("--n-components", type=int, default=3, choices=[1, 2, 3], help="number of PCA components (default: 3)")
    p.add_argument("--random-state", type=int, default=42, help="accepted and ignored: the full eigen-solver has no random step")
    p.add_argument("--save-colors", help="save the (N, 3) colours to this .npy file")
    p.add_argument("--save-ply", help="write an x y z red green blue point cloud (binary little-endian ply)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    coords_path = args.coords
    if args.features:
        features_path = args.features
        if args.save_ply and not coords_path:
            parser.error("--coords required when using --features with --save-ply")
    else:
        if not args.scene_name:
            parser.error("--scene-name required when using --results-dir")
        features_path, coords_path = find_results(args.results_dir, args.scene_name)
    if not (args.save_colors or args.save_ply):
        parser.error("nothing to do: give --save-colors and / or --save-ply (there is no viewer)")
    if coords_path and not os.path.exists(coords_path):
        raise FileNotFoundError(f"Coordinates file not found: {coords_path}")
    features = load_features(features_path)
    print(f"Loaded features {tuple(features.shape)} from {features_path}")
    out = pca_colors(features, n_components=args.n_components)
    ratio = out["explained_variance_ratio"]
    print(f"Explained variance ratio: {ratio}")
    print(f"Total variance explained: {ratio.sum():.2%}")
    colors = out["colors"].cpu().numpy()
    if args.save_colors:
        np.save(args.save_colors, colors)
        print(f"Saved PCA colors to: {args.save_colors}")
    if args.save_ply:
        write_ply(args.save_ply, np.load(coords_path), colors)
        print(f"Saved point cloud to: {args.save_ply}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
