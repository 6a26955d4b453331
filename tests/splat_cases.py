"""The splat renderer's definition in numpy, twice -- `project` and `composite` take the float type: np.float64 is the
statement, np.float32 the same operations in the stated order, every one rounded to fp32 -- and the builders of the test cases.

The distance between the two forms on a case, times four, is what the kernels are held to: the factor covers the device's expf, sqrt and
division differing from numpy's.  Rows and pixels whose discrete decisions sit on a boundary in fp64 are left out (at most 1 % of a
case, asserted in test_splat_host.py): `project` flags rows whose 3 sqrt(lambda) is within 1e-4 relative of an integer, whose rectangle
edge is within 1e-4 (relative to the larger of |mean|, radius and 16) of a multiple of 16 or whose z is within 1e-4 relative of near;
`composite` flags pixels where some alpha is within 1e-5 relative of 1/255 or some T' within 1e-5 relative of 1e-4."""
import numpy as np

TILE = 16
BATCH = 256
CAMERA_WORDS = 24
ROW_EPS = 1e-4
PIXEL_EPS = 1e-5
FACTOR = 4.0


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
def camera_block(R, t, fx, fy, cx, cy, width, height, near=0.01):
    """the packed block of ss_splat_project: fp32 R, t, fx, fy, cx, cy, near, limx, limy, then int32 width, height"""
    block = np.zeros(CAMERA_WORDS, dtype=np.float32)
    limx, limy = 1.3 * width / (2.0 * fx), 1.3 * height / (2.0 * fy)
    block[:19] = np.concatenate([np.asarray(R, dtype=np.float64).reshape(-1), np.asarray(t, dtype=np.float64).reshape(-1),
                                 [fx, fy, cx, cy, near, limx, limy]])
    block.view(np.int32)[19:21] = (width, height)
    return block


def identity_camera(width, height, f=64.0, near=0.01):
    return camera_block(np.eye(3), np.zeros(3), f, f, width / 2.0, height / 2.0, width, height, near)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    R = np.stack([r, np.cross(f, r), f])
    return R, -R @ eye


def block_size(block):
    w, h = block.view(np.int32)[19:21]
    return int(w), int(h)


def tile_grid(width, height):
    return -(-width // TILE), -(-height // TILE)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def project(coord, scale, quat, opacity, color, block, mode="gaussians", scale_modifier=1.0, point_size=2.0, ft=np.float64):
    """steps 1-5 from fp32 inputs -> dict(keep (N,) bool, mean (N, 2), conic (N, 3), opacity (N,), depth (N,), radius (N,) int64,
    rect (N, 4) int64, touched (N,) int64, boundary (N,) bool); the values of culled rows are 0"""
    f32 = [np.asarray(a, dtype=np.float32) for a in (coord, scale, quat, np.reshape(opacity, -1), color)]
    n = f32[0].shape[0]
    finite = np.ones(n, dtype=bool)
    for a in f32:
        finite &= np.isfinite(a.reshape(n, -1)).all(axis=1)
    p, s, q, o, _ = [np.where(np.isfinite(a), a, np.float32(1.0)).astype(ft) for a in f32]
    cam = block[:19].astype(ft)
    R, t = cam[:9], cam[9:12]
    fx, fy, cx, cy, near, limx, limy = cam[12:19]
    width, height = block_size(block)
    tiles_x, tiles_y = tile_grid(width, height)
    c = ft
    with np.errstate(all="ignore"):
        qn = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        keep = finite & (qn > 0)
        x = ((R[0] * p[:, 0] + R[1] * p[:, 1]) + R[2] * p[:, 2]) + t[0]
        y = ((R[3] * p[:, 0] + R[4] * p[:, 1]) + R[5] * p[:, 2]) + t[1]
        z = ((R[6] * p[:, 0] + R[7] * p[:, 1]) + R[8] * p[:, 2]) + t[2]
        keep &= z > near
        boundary = np.abs(z.astype(np.float64) - float(near)) <= ROW_EPS * float(near)
        xz, yz = x / z, y / z
        if mode == "pointcloud":
            k = c(np.float32(point_size)) / c(3.0)
            a = np.full(n, k * k, dtype=ft)
            b = np.zeros(n, dtype=ft)
            cc_ = a.copy()
            o = np.ones(n, dtype=ft)
        else:
            w_, x_, y_, z_ = (q[:, i] / qn for i in range(4))
            one, two = c(1.0), c(2.0)
            rot = [[one - two * (y_ * y_ + z_ * z_), two * (x_ * y_ - w_ * z_), two * (x_ * z_ + w_ * y_)],
                   [two * (x_ * y_ + w_ * z_), one - two * (x_ * x_ + z_ * z_), two * (y_ * z_ - w_ * x_)],
                   [two * (x_ * z_ - w_ * y_), two * (y_ * z_ + w_ * x_), one - two * (x_ * x_ + y_ * y_)]]
            sm = c(np.float32(scale_modifier))
            e = [s[:, j] * sm for j in range(3)]
            B = [[((R[3 * i] * rot[0][j] + R[3 * i + 1] * rot[1][j]) + R[3 * i + 2] * rot[2][j]) * e[j] for j in range(3)] for i in range(3)]
            tx = np.minimum(limx, np.maximum(-limx, xz))
            ty = np.minimum(limy, np.maximum(-limy, yz))
            j00 = fx / z
            j02 = -(j00 * tx)
            j11 = fy / z
            j12 = -(j11 * ty)
            a0, a1, a2 = (j00 * B[0][j] + j02 * B[2][j] for j in range(3))
            b0, b1, b2 = (j11 * B[1][j] + j12 * B[2][j] for j in range(3))
            a = ((a0 * a0 + a1 * a1) + a2 * a2) + c(0.3)
            b = (a0 * b0 + a1 * b1) + a2 * b2
            cc_ = ((b0 * b0 + b1 * b1) + b2 * b2) + c(0.3)
        det = a * cc_ - b * b
        keep &= det > 0
        inv = c(1.0) / det
        conic = np.stack([cc_ * inv, -(b * inv), a * inv], axis=1)
        mid = c(0.5) * (a + cc_)
        lam = mid + np.sqrt(np.maximum(c(0.1), mid * mid - det))
        r3 = c(3.0) * np.sqrt(lam)
        r = np.ceil(r3)
        mx, my = fx * xz + cx, fy * yz + cy
        keep &= np.isfinite(mx) & np.isfinite(my) & np.isfinite(r) & np.isfinite(conic).all(axis=1)
        boundary |= np.abs(r3 - np.round(r3)) <= ROW_EPS * np.abs(r3)
        edges = [(mx - r), (my - r), ((mx + r) + c(15.0)), ((my + r) + c(15.0))]
        lims = [tiles_x, tiles_y, tiles_x, tiles_y]
        mags = [np.maximum(np.maximum(np.abs(m), r), 16.0) for m in (mx, my, mx, my)]
        rect = np.zeros((n, 4), dtype=np.int64)
        for k_, (edge, lim, mag) in enumerate(zip(edges, lims, mags)):
            tile = np.floor(edge / c(16.0))
            boundary |= np.abs(edge.astype(np.float64) - 16.0 * np.round(edge.astype(np.float64) / 16.0)) <= ROW_EPS * mag
            rect[:, k_] = np.where(np.isfinite(tile), np.minimum(np.maximum(tile, 0), lim), 0).astype(np.int64)
        keep &= (rect[:, 2] > rect[:, 0]) & (rect[:, 3] > rect[:, 1])
    keep_f = keep[:, None]
    out = dict(keep=keep, mean=np.where(keep_f, np.stack([mx, my], axis=1), 0).astype(ft), conic=np.where(keep_f, conic, 0).astype(ft),
               opacity=np.where(keep, o, 0).astype(ft), depth=np.where(keep, z, 0).astype(ft),
               radius=np.where(keep, np.minimum(np.where(np.isfinite(r), r, 0), 2.0 ** 30), 0).astype(np.int64),
               rect=np.where(keep_f, rect, 0), boundary=boundary & finite & (qn > 0))
    out["touched"] = (out["rect"][:, 2] - out["rect"][:, 0]) * (out["rect"][:, 3] - out["rect"][:, 1])
    return out


def depth_order(depth, keep):
    """the kept rows front to back by the fp32 depth, the lower row first among equals"""
    rows = np.nonzero(keep)[0]
    return rows[np.argsort(np.asarray(depth, dtype=np.float32)[rows], kind="stable")]


def composite(mean, conic_opacity, color, depth, rect, keep, width, height, background, ft=np.float64, mark=None):
    """steps 6-8 by brute force: every kept Gaussian in (depth, row) order against every pixel of the tiles of its rectangle ->
    dict(image (H, W, 3), alpha, depth, undecided (H, W) bool, stop_rank (H, W): the rank in its tile's list of the Gaussian that
    stopped the pixel (-1: none), reached (H, W) bool: some Gaussian of `mark` was added to the pixel)"""
    mean, co, col, dep = (np.asarray(a, dtype=np.float32).astype(ft) for a in (mean, conic_opacity, color, depth))
    bg = np.asarray(background, dtype=np.float32).astype(ft)
    c = ft
    tiles_x, tiles_y = tile_grid(width, height)
    T = np.ones((height, width), dtype=ft)
    C = np.zeros((height, width, 3), dtype=ft)
    Z = np.zeros((height, width), dtype=ft)
    done = np.zeros((height, width), dtype=bool)
    undecided = np.zeros((height, width), dtype=bool)
    reached = np.zeros((height, width), dtype=bool)
    stop_rank = np.full((height, width), -1, dtype=np.int64)
    tile_count = np.zeros((tiles_y, tiles_x), dtype=np.int64)
    px = (np.arange(width).astype(ft) + c(0.5))[None, :]
    py = (np.arange(height).astype(ft) + c(0.5))[:, None]
    tile_of_x, tile_of_y = np.arange(width) // TILE, np.arange(height) // TILE
    a_min, a_max, t_min = c(1.0) / c(255.0), c(0.99), c(1e-4)
    for g in depth_order(depth, keep):
        x0, y0, x1, y1 = (int(v) for v in rect[g])
        sx, sy = slice(x0 * TILE, min(x1 * TILE, width)), slice(y0 * TILE, min(y1 * TILE, height))
        rank = tile_count[np.ix_(tile_of_y[sy], tile_of_x[sx])]
        tile_count[y0:y1, x0:x1] += 1
        dx, dy = mean[g, 0] - px[:, sx], mean[g, 1] - py[sy]
        with np.errstate(all="ignore"):
            power = c(-0.5) * ((co[g, 0] * dx) * dx + (co[g, 2] * dy) * dy) - (co[g, 1] * dx) * dy
            alpha = np.minimum(a_max, co[g, 3] * np.exp(power))
        live = ~done[sy, sx] & (power <= 0)                                # (a NaN skips too)
        undecided[sy, sx] |= live & (np.abs(alpha.astype(np.float64) - 1.0 / 255.0) <= PIXEL_EPS / 255.0)
        live &= ~(alpha < a_min)
        Tn = T[sy, sx] * (c(1.0) - alpha)
        undecided[sy, sx] |= live & (np.abs(Tn.astype(np.float64) - 1e-4) <= PIXEL_EPS * 1e-4)
        stop = live & (Tn < t_min)
        stop_rank[sy, sx] = np.where(stop, rank, stop_rank[sy, sx])
        done[sy, sx] |= stop
        add = live & ~stop
        w = np.where(add, alpha * T[sy, sx], c(0.0))
        C[sy, sx] = C[sy, sx] + col[g][None, None, :] * w[:, :, None]
        Z[sy, sx] = Z[sy, sx] + dep[g] * w
        T[sy, sx] = np.where(add, Tn, T[sy, sx])
        if mark is not None and mark[g]:
            reached[sy, sx] |= add
    return dict(image=C + T[:, :, None] * bg[None, None, :], alpha=c(1.0) - T, depth=Z, undecided=undecided, stop_rank=stop_rank,
                reached=reached, tile_count=tile_count)


def tile_lists(depth, rect, keep, width, height):
    """per tile (row major) the kept rows whose rectangle contains it, in (depth, row) order"""
    tiles_x, tiles_y = tile_grid(width, height)
    lists = [[] for _ in range(tiles_x * tiles_y)]
    for g in depth_order(depth, keep):
        x0, y0, x1, y1 = (int(v) for v in rect[g])
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                lists[ty * tiles_x + tx].append(int(g))
    return lists


def distance(a, b, where=None):
    """the largest |a - b| over the entries (rows / pixels) that `where` keeps"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    if where is not None:
        d = d[where]
    return float(d.max()) if d.size else 0.0


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _random_quats(rng, n):
    q = rng.standard_normal((n, 4))
    q *= np.where(q[:, :1] < 0, -1.0, 1.0)
    return (q * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)         # (not unit: the kernel normalises)


def room_case(n, seed, width=200, height=120):
    """n Gaussians of a room seen from inside it, about half of them behind the camera; the image is 13 x 8 tiles, the last ones partial"""
    rng = np.random.default_rng(seed)
    coord = (rng.uniform([-3.0, -3.0, 0.0], [3.0, 3.0, 2.5], (n, 3))).astype(np.float32)
    coord[0] = (2.0, 1.8, 0.8)                                            # (row 0 is in view whatever n is)
    scale = np.exp(rng.uniform(np.log(0.004), np.log(0.25), (n, 3))).astype(np.float32)
    quat = _random_quats(rng, n)
    opacity = rng.uniform(0.05, 1.0, n).astype(np.float32)
    color = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    R, t = look_at((0.4, -0.6, 1.3), (3.0, 2.5, 0.6))
    f = 0.5 * height / np.tan(np.radians(60.0) / 2.0)
    return dict(coord=coord, scale=scale, quat=quat, opacity=opacity, color=color), camera_block(R, t, f, f, width / 2.0, height / 2.0, width, height)


def pixel_gaussians(block, u, v, z, sigma, rng, opacity, isotropic=False):
    """Gaussians under the identity camera `block` whose means land on the pixels (u, v) at the depths z, about sigma pixels wide"""
    f, cx, cy = float(block[12]), float(block[14]), float(block[15])
    u, v, z, sigma = (np.asarray(a, dtype=np.float64) for a in (u, v, z, sigma))
    n = u.shape[0]
    coord = np.stack([(u - cx) * z / f, (v - cy) * z / f, z], axis=1).astype(np.float32)
    shape = np.ones((n, 3)) if isotropic else np.concatenate([np.ones((n, 1)), rng.uniform(0.4, 1.0, (n, 2))], axis=1)
    scale = ((sigma * z / f)[:, None] * shape).astype(np.float32)
    quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32), (n, 1)) if isotropic else _random_quats(rng, n)
    return dict(coord=coord, scale=scale, quat=quat, opacity=np.asarray(opacity, dtype=np.float32).reshape(n),
                color=rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32))


def concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def population_case(width, height, populations, seed, stacks=(), spread=(5.5, 10.5)):
    """a scene whose tile (tx, ty) holds exactly populations[(tx, ty)] Gaussians (every other tile none): small Gaussians (0.3 to 0.8
    pixels wide before the dilation) whose means keep `spread` inside their tile, so that no rectangle reaches a second tile.
    stacks: (tile, (u, v) inside the tile, count, "front" | "back"): that many of the tile's Gaussians are opaque, about one pixel wide,
    on one spot, in front of or behind all the others of the case."""
    rng = np.random.default_rng(seed)
    block = identity_camera(width, height)
    parts = []
    stacked = {}
    for tile, _, count, _ in stacks:
        stacked[tile] = stacked.get(tile, 0) + count
    for (tx, ty), count in sorted(populations.items()):
        m = count - stacked.get((tx, ty), 0)
        assert m >= 0
        if m:
            u, v = tx * TILE + rng.uniform(*spread, m), ty * TILE + rng.uniform(*spread, m)
            parts.append(pixel_gaussians(block, u, v, rng.uniform(2.0, 6.0, m), rng.uniform(0.3, 0.8, m), rng, rng.uniform(0.03, 0.6, m)))
    for (tx, ty), (du, dv), count, where in stacks:
        z = (1.0 + 0.01 * np.arange(count)) if where == "front" else (7.0 + 0.01 * np.arange(count))
        parts.append(pixel_gaussians(block, np.full(count, tx * TILE + du), np.full(count, ty * TILE + dv), z, np.full(count, 1.0), rng,
                                     np.full(count, 0.8), isotropic=True))
    scene = concat(parts)
    perm = rng.permutation(scene["coord"].shape[0])                       # rows in no particular order
    return {k: a[perm] for k, a in scene.items()}, block


def coincident_case(count=300, width=16, height=16):
    """`count` Gaussians of distinct colours on one spot at one depth: the row decides the order"""
    rng = np.random.default_rng(3)
    block = identity_camera(width, height)
    scene = pixel_gaussians(block, np.full(count, 8.3), np.full(count, 7.6), np.full(count, 3.0), np.full(count, 1.5), rng,
                            np.full(count, 0.3), isotropic=True)
    scene["color"] = np.stack([np.linspace(0, 1, count), np.linspace(1, 0, count), (np.arange(count) % 7) / 6.0], axis=1).astype(np.float32)
    return scene, block


COMPOSITE_CASES = {
    # name: (width, height, populations, stacks)
    "1x1": (1, 1, {(0, 0): 257}, ()),
    "16x16": (16, 16, {(0, 0): 256}, ()),
    "17x33": (17, 33, {(0, 0): 513, (1, 0): 1, (0, 1): 257, (1, 2): 256}, ()),
    "37x21": (37, 21, {(0, 0): 1, (1, 0): 257, (2, 0): 300, (0, 1): 513, (2, 1): 40}, ()),
    "64x48": (64, 48, {(0, 0): 256, (1, 0): 257, (3, 0): 1, (1, 1): 600, (2, 1): 700, (0, 2): 100, (3, 2): 513},
              (((1, 1), (6.5, 6.5), 8, "front"), ((1, 1), (10.5, 10.5), 10, "back"))),
}


def composite_case(name):
    width, height, populations, stacks = COMPOSITE_CASES[name]
    spread = (-2.0, 3.0) if name == "1x1" else (5.5, 10.5)                # (one pixel: the Gaussians sit around it)
    scene, block = population_case(width, height, populations, seed=sum(map(ord, name)), stacks=stacks, spread=spread)
    return scene, block, populations


def planted_rows():
    """rows under the identity camera (64 x 48, f = 64, near = 0.5) whose fate is exact -> (scene, block, expectations): per row
    (name, kept, rect or None)"""
    block = identity_camera(64, 48, near=0.5)
    rows = []

    def add(name, kept, rect=None, p=(0.0, 0.0, 2.0), s=(0.01, 0.01, 0.01), q=(1.0, 0.0, 0.0, 0.0), o=0.5, c=(0.2, 0.4, 0.6)):
        rows.append((name, kept, rect, p, s, q, o, c))

    add("plain", True, (1, 1, 3, 2))                                     # mean (32, 24), radius 3: x 29..35 -> tiles 1..2, y 21..27 -> tile 1
    add("z == near", False, p=(0.0, 0.0, 0.5))
    add("z just past near", True, (1, 1, 3, 2), p=(0.0, 0.0, 0.75))
    add("z < 0", False, p=(0.0, 0.0, -2.0))
    add("nan coord", False, p=(np.nan, 0.0, 2.0))
    add("inf coord", False, p=(0.0, np.inf, 2.0))
    add("nan scale", False, s=(0.01, np.nan, 0.01))
    add("inf scale", False, s=(np.inf, 0.01, 0.01))
    add("nan quat", False, q=(1.0, 0.0, np.nan, 0.0))
    add("inf quat", False, q=(np.inf, 0.0, 0.0, 0.0))
    add("nan opacity", False, o=np.nan)
    add("inf opacity", False, o=np.inf)
    add("nan color", False, c=(0.2, np.nan, 0.6))
    add("inf color", False, c=(-np.inf, 0.4, 0.6))
    add("|q| == 0", False, q=(0.0, 0.0, 0.0, 0.0))
    # mean (-608, 24): 20 units left of the axis at z = 2; scale 10 -> sigma 320 pixels and more: the radius reaches back into the image
    add("far off-screen, reaching in", True, (0, 0, 4, 3), p=(-20.0, 0.0, 2.0), s=(10.0, 10.0, 10.0))
    add("far off-screen, not reaching", False, p=(-20.0, 0.0, 2.0))
    add("larger than the image", True, (0, 0, 4, 3), s=(5.0, 5.0, 5.0))
    add("scale == 0", True, (1, 1, 3, 2), s=(0.0, 0.0, 0.0))
    # mean exactly on the corner (16, 16) of four tiles: x = (16 - 32) * 2 / 64, y = (16 - 24) * 2 / 64; radius 3 -> 13..19: tiles 0..1
    add("mean on a tile corner", True, (0, 0, 2, 2), p=(-0.5, -0.25, 2.0), s=(0.0, 0.0, 0.0))
    scene = dict(coord=np.array([r[3] for r in rows], dtype=np.float32), scale=np.array([r[4] for r in rows], dtype=np.float32),
                 quat=np.array([r[5] for r in rows], dtype=np.float32), opacity=np.array([r[6] for r in rows], dtype=np.float32),
                 color=np.array([r[7] for r in rows], dtype=np.float32))
    return scene, block, [(r[0], r[1], r[2]) for r in rows]


def synthetic_folder(path, n=3000, seed=11):
    """a scene folder as the converters write it: coord, color (uint8), opacity (n, 1), scale, quat (w >= 0)"""
    import os
    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    coord = rng.uniform([-2.0, -1.5, 0.0], [2.0, 1.5, 2.0], (n, 3)).astype(np.float32)
    quat = rng.standard_normal((n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat *= np.where(quat[:, :1] < 0, -1.0, 1.0)
    arrays = dict(coord=coord, color=rng.integers(0, 256, (n, 3)).astype(np.uint8), opacity=rng.uniform(0.1, 1.0, (n, 1)).astype(np.float32),
                  scale=np.exp(rng.uniform(np.log(0.01), np.log(0.12), (n, 3))).astype(np.float32), quat=quat.astype(np.float32))
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)
    return arrays
