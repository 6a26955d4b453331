"""Headless Gaussian-splat rendering of a scene folder, on the device (the reference's roadmap task "Scene Visualization"; its
tools/visualize_scene.py needs an Open3D window or an interactive matplotlib scatter: the definition here is DESIGN.md 8u).

    from scenesplat_amd.pointcept_api import render_scene, look_at_camera, fit_camera, orbit_cameras, save_image
    cam = fit_camera(coord, width=1280, height=720, fov_y=60.0, view="iso")       # | "top"; frames the 1st..99th percentile box, z up
    out = render_scene("data/scene0011_00", cam, mode="gaussians")                # | "pointcloud" (point_size=2.0 px)
    out["image"]         # (H, W, 3) fp32 on the device; also "alpha" (H, W), "depth" (H, W), "num_pairs", "num_visible"
    out = render_scene(scene, cam, colors=pca["colors"])                          # any (N, 3) fp32 in 0..1 instead of color.npy / 255
    save_image("scene.png", out["image"])

The rows are alpha-composited anisotropic Gaussians (standard EWA splatting, csrc/splat.hip): project, count the (Gaussian, tile) pairs,
sort them by (tile, depth) with the stable radix argsort, composite front to back, one workgroup per 16 x 16 tile.  One small host read
per call: the pair count P after the scan.  Forward only; no window, no viewer.

    python -m scenesplat_amd.pointcept_api.render SCENE_DIR --output scene.png [--width 1280 --height 720 --fov 60 --view iso|top
        --mode gaussians|pointcloud --point-size 2 --views 8 --colors colors.npy --indices chair_indices.npy --background 1 1 1
        --scale-modifier 1.0 --max-pairs N]
"""
import argparse
import dataclasses
import math
import os

import numpy as np
import torch

from .. import _lib

TILE = _lib.CONSTANTS["SS_SPLAT_TILE"]
MAX_DIM = _lib.CONSTANTS["SS_SPLAT_MAX_DIM"]
CAMERA_WORDS = _lib.CONSTANTS["SS_SPLAT_CAMERA_WORDS"]
MODES = ("gaussians", "pointcloud")
VIEWS = ("iso", "top")
MAX_PAIRS = 2 ** 31 - 1                  # the largest count the argsort takes
DEFAULT_WIDTH, DEFAULT_HEIGHT, DEFAULT_FOV = 1280, 720, 60.0        # the reference's window
SCENE_ARRAYS = ("coord", "color", "opacity", "scale", "quat")
FIT_MARGIN = 0.95                        # the fitted box stays inside this share of the half image
ISO_DIRECTION = (1.0, -1.0, 0.8)         # from the target towards the eye


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Camera:
    """world-to-camera R (3, 3), t (3,) in fp64 (p_c = R p + t; the camera looks down +z, x right, y down), pinhole fx, fy, cx, cy in
    pixels (pixel (i, j) has its centre at (i + 0.5, j + 0.5)), the image size and the near plane"""
    R: np.ndarray
    t: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    near: float = 0.01

    def __post_init__(self):
        self.R = np.asarray(self.R, dtype=np.float64).reshape(3, 3)
        self.t = np.asarray(self.t, dtype=np.float64).reshape(3)
        if int(self.width) != self.width or int(self.height) != self.height:
            raise ValueError(f"width and height must be integers, got {self.width!r} x {self.height!r}")
        self.width, self.height = int(self.width), int(self.height)
        if not (1 <= self.width <= MAX_DIM and 1 <= self.height <= MAX_DIM):
            raise ValueError(f"width and height must be in 1..{MAX_DIM}, got {self.width} x {self.height}")
        values = [self.fx, self.fy, self.cx, self.cy, self.near]
        if not (np.isfinite(self.R).all() and np.isfinite(self.t).all() and np.isfinite(values).all()):
            raise ValueError("camera values must be finite")
        if not (self.fx > 0 and self.fy > 0 and self.near > 0):
            raise ValueError(f"fx, fy and near must be positive, got {self.fx}, {self.fy}, {self.near}")

    @property
    def eye(self):
        return -self.R.T @ self.t

    def limits(self):
        """1.3 tan(fov / 2) per axis"""
        return 1.3 * self.width / (2.0 * self.fx), 1.3 * self.height / (2.0 * self.fy)

    def packed(self):
        """the block ss_splat_project reads: fp32 R, t, fx, fy, cx, cy, near, limx, limy (each rounded once), int32 width, height"""
        block = np.zeros(CAMERA_WORDS, dtype=np.float32)
        limx, limy = self.limits()
        block[:19] = np.concatenate([self.R.reshape(-1), self.t, [self.fx, self.fy, self.cx, self.cy, self.near, limx, limy]])
        block.view(np.int32)[19:21] = (self.width, self.height)
        return block

    def project(self, points):
        """fp64 pixel positions and depths of world points (n, 3) -> ((n, 2), (n,))"""
        pc = np.asarray(points, dtype=np.float64).reshape(-1, 3) @ self.R.T + self.t
        z = pc[:, 2]
        return np.stack([self.fx * pc[:, 0] / z + self.cx, self.fy * pc[:, 1] / z + self.cy], axis=1), z


def as_camera(camera):
    if isinstance(camera, Camera):
        return camera
    if isinstance(camera, dict):
        return Camera(**{f.name: camera[f.name] for f in dataclasses.fields(Camera) if f.name in camera})
    raise TypeError(f"camera: a Camera or a dict of its fields, got {type(camera).__name__}")


def _unit(v, what):
    n = float(np.linalg.norm(v))
    if not np.isfinite(n) or n < 1e-12:
        raise ValueError(f"look_at_camera: {what}")
    return v / n


def look_at_camera(eye, target, up=(0.0, 0.0, 1.0), fov_y=DEFAULT_FOV, width=DEFAULT_WIDTH, height=DEFAULT_HEIGHT, near=0.01):
    """the camera at `eye` that looks at `target` (the image centre) with `up` upwards in the image; fov_y in degrees, square pixels"""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    if not 0.0 < float(fov_y) < 180.0:
        raise ValueError(f"fov_y must be inside (0, 180) degrees, got {fov_y!r}")
    forward = _unit(target - eye, "eye and target coincide")
    right = _unit(np.cross(forward, up), "up is parallel to the viewing direction")
    down = np.cross(forward, right)
    R = np.stack([right, down, forward])
    f = 0.5 * height / math.tan(math.radians(float(fov_y)) / 2.0)
    return Camera(R=R, t=-R @ eye, fx=f, fy=f, cx=0.5 * width, cy=0.5 * height, width=width, height=height, near=near)


def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def fitted_box(coord):
    """the 1st..99th percentile box of the finite rows of coord (N, 3) -> (lo (3,), hi (3,)) in fp64"""
    c = _host_array(coord).astype(np.float64).reshape(-1, 3)
    c = c[np.isfinite(c).all(axis=1)]
    if c.shape[0] == 0:
        raise ValueError("coord has no finite row")
    return np.percentile(c, 1.0, axis=0), np.percentile(c, 99.0, axis=0)


def box_corners(lo, hi):
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)


def _view_axes(view):
    if view not in VIEWS:
        raise ValueError(f"view must be one of {VIEWS}, got {view!r}")
    if view == "top":
        return np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])
    d = np.array(ISO_DIRECTION)
    return d / np.linalg.norm(d), np.array([0.0, 0.0, 1.0])


def _fit_distance(corners, target, direction, up, fov_y, width, height, near):
    """the smallest eye distance along `direction` at which every corner lies inside FIT_MARGIN of the half image"""
    probe = look_at_camera(target + direction, target, up, fov_y, width, height, near)
    rel = (corners - target) @ probe.R.T                # camera axes, relative to the target
    tx, ty = FIT_MARGIN * 0.5 * width / probe.fx, FIT_MARGIN * 0.5 * height / probe.fy
    need = np.maximum(np.abs(rel[:, 0]) / tx, np.abs(rel[:, 1]) / ty) - rel[:, 2]
    return float(max(need.max(), (2.0 * near - rel[:, 2]).max(), 1e-6))


def fit_camera(coord, width=DEFAULT_WIDTH, height=DEFAULT_HEIGHT, fov_y=DEFAULT_FOV, view="iso", near=0.01):
    """the camera that frames the 1st..99th percentile box of coord, z up: "iso" from above a corner, "top" straight down (y up in the
    image)"""
    direction, up = _view_axes(view)
    lo, hi = fitted_box(coord)
    target = 0.5 * (lo + hi)
    d = _fit_distance(box_corners(lo, hi), target, direction, up, fov_y, width, height, near)
    return look_at_camera(target + d * direction, target, up, fov_y, width, height, near)


def orbit_cameras(coord, n, width=DEFAULT_WIDTH, height=DEFAULT_HEIGHT, fov_y=DEFAULT_FOV, view="iso", near=0.01):
    """n cameras of a turntable about the z axis through the fitted target, at one distance that frames the box from every one"""
    if int(n) != n or n < 1:
        raise ValueError(f"n must be a positive integer, got {n!r}")
    direction, up = _view_axes(view)
    lo, hi = fitted_box(coord)
    target, corners = 0.5 * (lo + hi), box_corners(lo, hi)
    turned = []
    for k in range(int(n)):
        a = 2.0 * math.pi * k / int(n)
        rot = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        turned.append((rot @ direction, rot @ up))
    d = max(_fit_distance(corners, target, dk, uk, fov_y, width, height, near) for dk, uk in turned)
    return [look_at_camera(target + d * dk, target, uk, fov_y, width, height, near) for dk, uk in turned]


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
def load_scene(scene):
    """a scene folder or a dict of arrays -> dict of the arrays the renderer reads (numpy arrays or tensors, as given)"""
    if isinstance(scene, dict):
        out = {k: scene[k] for k in SCENE_ARRAYS if k in scene}
    elif isinstance(scene, (str, os.PathLike)):
        if not os.path.isdir(scene):
            raise FileNotFoundError(f"Scene folder not found: {scene}")
        out = {k: np.load(os.path.join(scene, k + ".npy")) for k in SCENE_ARRAYS if os.path.exists(os.path.join(scene, k + ".npy"))}
    else:
        raise TypeError(f"scene: a folder or a dict of arrays, got {type(scene).__name__}")
    if "coord" not in out:
        raise ValueError("the scene has no coord")
    return out


def _shape_of(a):
    return tuple(a.shape)


def _check_float(a, name):
    dt = a.dtype
    ok = dt.is_floating_point if isinstance(a, torch.Tensor) else np.issubdtype(dt, np.floating)
    if not ok:
        raise ValueError(f"{name} must be floating point, got {dt}")


def _validate(arrays, colors, mode, point_size, scale_modifier, background, max_pairs):
    """-> N.  ValueError: shapes, dtypes, an unknown mode, colors of the wrong length"""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    coord = arrays["coord"]
    if len(_shape_of(coord)) != 2 or _shape_of(coord)[1] != 3:
        raise ValueError(f"coord must be (N, 3), got {_shape_of(coord)}")
    n = _shape_of(coord)[0]
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"the scene must have 1 <= N < 2^31 rows, got {n}")
    _check_float(coord, "coord")
    need = ("opacity", "scale", "quat") if mode == "gaussians" else ()
    for key in need:
        if key not in arrays:
            raise ValueError(f"mode='gaussians' needs the scene's {key}")
    for key, cols in (("scale", 3), ("quat", 4)):
        if key in arrays:
            if _shape_of(arrays[key]) != (n, cols):
                raise ValueError(f"{key} must be ({n}, {cols}), got {_shape_of(arrays[key])}")
            _check_float(arrays[key], key)
    if "opacity" in arrays:
        if _shape_of(arrays["opacity"]) not in ((n,), (n, 1)):
            raise ValueError(f"opacity must be ({n},) or ({n}, 1), got {_shape_of(arrays['opacity'])}")
        _check_float(arrays["opacity"], "opacity")
    if colors is not None:
        if _shape_of(colors) != (n, 3):
            raise ValueError(f"colors must be ({n}, 3), got {_shape_of(colors)}")
        _check_float(colors, "colors")
    elif "color" not in arrays:
        raise ValueError("the scene has no color and no colors were given")
    elif _shape_of(arrays["color"]) != (n, 3):
        raise ValueError(f"color must be ({n}, 3), got {_shape_of(arrays['color'])}")
    if not (np.isfinite(float(point_size)) and float(point_size) > 0):
        raise ValueError(f"point_size must be positive, got {point_size!r}")
    if not np.isfinite(float(scale_modifier)):
        raise ValueError(f"scale_modifier must be finite, got {scale_modifier!r}")
    bg = np.asarray(background, dtype=np.float64).reshape(-1)
    if bg.shape[0] != 3 or not np.isfinite(bg).all():
        raise ValueError(f"background must be 3 finite values, got {background!r}")
    if max_pairs is not None and (int(max_pairs) != max_pairs or not 0 <= max_pairs <= MAX_PAIRS):
        raise ValueError(f"max_pairs must be an integer in 0..{MAX_PAIRS}, got {max_pairs!r}")
    return n


def scene_colors(color):
    """the folder's color -> (N, 3) fp32 in 0..1: integer colours / 255 in fp32, floating-point colours as they are.  A tensor stays a
    tensor on its device (nothing comes down to the host); an array stays an array."""
    if isinstance(color, torch.Tensor):
        if color.dtype.is_floating_point:
            return color.detach().to(torch.float32)
        # torch divides by a scalar as a product with its reciprocal, which is not the fp32 quotient.  In fp64 either form, rounded to
        # fp32, is: a quotient of integers below 2^24 by 255 lies further from every fp32 rounding boundary than fp64's error.
        return (color.detach().to(torch.float64) / 255.0).to(torch.float32)
    color = np.asarray(color)
    if np.issubdtype(color.dtype, np.integer):
        return color.astype(np.float32) / np.float32(255.0)
    return color.astype(np.float32)


def _f32_on_device(a, device):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    return a.to(device=device, dtype=torch.float32).contiguous()


def render_scene(scene, camera, mode="gaussians", colors=None, point_size=2.0, scale_modifier=1.0, background=(1.0, 1.0, 1.0),
                 max_pairs=None, out=None, device=None):
    """scene: a scene folder or a dict of its arrays (numpy or tensors); camera: a Camera or a dict of its fields -> dict(image (H, W, 3)
    fp32, alpha (H, W), depth (H, W) on the device, num_pairs, num_visible).  colors: any (N, 3) fp32 in 0..1 instead of color / 255.
    out: dict(image, alpha, depth) of device tensors to write.  DESIGN.md 8u.
    ValueError: shapes, dtypes, an unknown mode; RuntimeError: more than max_pairs (Gaussian, tile) pairs (nothing is written)."""
    cam = as_camera(camera)
    arrays = load_scene(scene)
    n = _validate(arrays, colors, mode, point_size, scale_modifier, background, max_pairs)
    cap = MAX_PAIRS if max_pairs is None else int(max_pairs)
    given = [a for a in list(arrays.values()) + [colors] if isinstance(a, torch.Tensor) and a.is_cuda]
    if device is None and not given and not torch.cuda.is_available():
        raise RuntimeError("render_scene runs on the device: no GPU is available (there is no CPU fallback)")
    dev = torch.device(device) if device is not None else (given[0].device if given else torch.device("cuda"))
    from .. import native as nv
    coord = _f32_on_device(arrays["coord"], dev)
    # the point cloud mode reads no shape: a folder without scale / quat / opacity still draws
    scale = _f32_on_device(arrays["scale"], dev) if "scale" in arrays else torch.ones((n, 3), dtype=torch.float32, device=dev)
    if "quat" in arrays:
        quat = _f32_on_device(arrays["quat"], dev)
    else:
        quat = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        quat[:, 0] = 1.0
    opacity = _f32_on_device(arrays["opacity"], dev).reshape(-1) if "opacity" in arrays else torch.ones(n, dtype=torch.float32, device=dev)
    color = _f32_on_device(colors if colors is not None else scene_colors(arrays["color"]), dev)
    W, H = cam.width, cam.height
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    if out is not None:
        for key, shape in (("image", (H, W, 3)), ("alpha", (H, W)), ("depth", (H, W))):
            t = out.get(key)
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out[{key!r}] must be a contiguous fp32 device tensor of shape {shape}")
    block = cam.packed()
    proj = nv.splat_project(coord, scale, quat, opacity, color, block, mode, scale_modifier, point_size)
    offsets, totals = nv.splat_offsets(proj["tiles_touched"])
    P, visible = (int(v) for v in totals.cpu().tolist())                 # the one synchronising read of the call
    if P > cap:
        raise RuntimeError(f"render_scene: the view has {P} (Gaussian, tile) pairs, more than max_pairs = {cap}; nothing was written "
                           f"(a smaller image, a smaller scale_modifier or a camera further inside the scene has fewer)")
    bg = np.asarray(background, dtype=np.float32).reshape(3)
    if out is None:
        out = dict(image=torch.empty((H, W, 3), dtype=torch.float32, device=dev), alpha=torch.empty((H, W), dtype=torch.float32, device=dev),
                   depth=torch.empty((H, W), dtype=torch.float32, device=dev))
    result = dict(image=out["image"], alpha=out["alpha"], depth=out["depth"], num_pairs=P, num_visible=visible)
    if P == 0:                                                           # nothing more is launched: the image is the background
        out["image"].copy_(torch.from_numpy(bg).to(dev).expand(H, W, 3))
        out["alpha"].zero_()
        out["depth"].zero_()
    else:
        keys, rows = nv.splat_keys(proj["depth"], proj["rect"], proj["tiles_touched"], offsets, P, tiles_x, tiles_y)
        key_bits = 32 + max(0, (tiles_x * tiles_y - 1).bit_length())
        order, _, sorted_keys = nv.argsort_i64(keys.view(1, P), key_bits, want_inverse=False, want_sorted=True)
        ranges, sorted_rows = nv.splat_ranges(sorted_keys.view(P), order.view(P), rows, tiles_x * tiles_y)
        nv.splat_composite(proj["mean2d"], proj["conic_opacity"], color, proj["depth"], ranges, sorted_rows, W, H, bg,
                           out=(out["image"], out["alpha"], out["depth"]))
    return result


def image_to_uint8(image):
    """(H, W, 3) fp32 (a tensor or an array) -> uint8(clip(c, 0, 1) * 255 + 0.5) on the host"""
    img = _host_array(image).astype(np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image must be (H, W, 3), got {img.shape}")
    return (np.clip(img, np.float32(0.0), np.float32(1.0)) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def save_image(path, image):
    """writes the image with PIL (the format follows the file name); -> the uint8 array written"""
    from PIL import Image
    u8 = image_to_uint8(image)
    Image.fromarray(u8).save(path)
    return u8


def highlight_rows(color, indices):
    """the colours of `--indices`: the rows `indices` in highlight_colors' palette colour 0, every other row grey (its luminance): a
    single-query highlight_colors -> (N, 3) fp32 on the host"""
    from .text_query import highlight_colors
    base = scene_colors(_host_array(color))
    n = base.shape[0]
    idx = np.asarray(_host_array(indices)).reshape(-1).astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"indices outside the scene's {n} rows")
    lum = base @ np.array([0.299, 0.587, 0.114], dtype=np.float32)
    grey = np.repeat(lum[:, None], 3, axis=1).astype(np.float32)
    best = np.full(n, -1, dtype=np.int32)
    best[idx] = 0
    return highlight_colors(grey, dict(best=torch.from_numpy(best))).numpy()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m scenesplat_amd.pointcept_api.render",
                                description="Render a scene folder to an image on the device: alpha-composited Gaussian splats, "
                                            "no window and no viewer")
    p.add_argument("scene", help="scene folder (coord.npy, color.npy, opacity.npy, scale.npy, quat.npy)")
    p.add_argument("--output", required=True, help="image file to write (with --views n: NAME_000.png ... beside it)")
    p.add_argument("--width", type=int, default=DEFAULT_WIDTH)
    p.add_argument("--height", type=int, default=DEFAULT_HEIGHT)
    p.add_argument("--fov", type=float, default=DEFAULT_FOV, help="vertical field of view in degrees (default: 60)")
    p.add_argument("--view", choices=VIEWS, default="iso")
    p.add_argument("--mode", choices=MODES, default="gaussians")
    p.add_argument("--point-size", type=float, default=2.0, help="pointcloud mode: the splat's size in pixels (default: 2)")
    p.add_argument("--views", type=int, default=1, help="write this many views of a turntable about the z axis")
    p.add_argument("--colors", help="an (N, 3) .npy of colours in 0..1 (pca_colors / highlight_colors) instead of color.npy")
    p.add_argument("--indices", help="a .npy of rows to highlight (a query's *_indices.npy); the rest is drawn grey")
    p.add_argument("--background", type=float, nargs=3, default=[1.0, 1.0, 1.0], metavar=("R", "G", "B"))
    p.add_argument("--scale-modifier", type=float, default=1.0)
    p.add_argument("--max-pairs", type=int, help="refuse a view with more (Gaussian, tile) pairs than this")
    return p


def view_paths(output, n):
    if n == 1:
        return [output]
    stem, ext = os.path.splitext(output)
    return [f"{stem}_{k:03d}{ext or '.png'}" for k in range(n)]


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not (1 <= args.width <= MAX_DIM and 1 <= args.height <= MAX_DIM):
        parser.error(f"--width and --height must be in 1..{MAX_DIM}")
    if args.views < 1:
        parser.error("--views must be at least 1")
    if not 0.0 < args.fov < 180.0:
        parser.error("--fov must be inside (0, 180)")
    if args.point_size <= 0:
        parser.error("--point-size must be positive")
    if args.max_pairs is not None and args.max_pairs < 0:
        parser.error("--max-pairs must not be negative")
    if args.colors and args.indices:
        parser.error("--colors and --indices exclude each other")
    scene = load_scene(args.scene)
    colors = None
    if args.colors:
        colors = np.load(args.colors).astype(np.float32)
    elif args.indices:
        if "color" not in scene:
            raise ValueError("--indices needs the scene's color")
        colors = highlight_rows(scene["color"], np.load(args.indices))
    if args.views == 1:
        cameras = [fit_camera(scene["coord"], args.width, args.height, args.fov, args.view)]
    else:
        cameras = orbit_cameras(scene["coord"], args.views, args.width, args.height, args.fov, args.view)
    for path, cam in zip(view_paths(args.output, args.views), cameras):
        out = render_scene(scene, cam, mode=args.mode, colors=colors, point_size=args.point_size, scale_modifier=args.scale_modifier,
                           background=args.background, max_pairs=args.max_pairs)
        save_image(path, out["image"])
        print(f"Saved: {path} ({cam.width} x {cam.height}, {out['num_visible']} of {len(scene['coord'])} Gaussians, "
              f"{out['num_pairs']} pairs)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
