"""Inputs and fp64 numpy restatements for the self-supervised view transforms (colour chain, sparse voxel blur), shared by
tests/golden/make_golden_ssl_views.py (which stores their results beside the reference's outputs) and the tests.  numpy only."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAY = 1, 2, 3, 4, 5
NAMES = ("brightness", "contrast", "saturation", "hue")

# rows every colour input starts with: exact grays, black, white, pure red, r == g max ties, g == b max ties, values that clip at both
# ends under brightness 1.4 (>= 182.2 clips high; contrast / saturation push dark saturated rows below 0)
SPECIAL_COLORS = np.array([[128, 128, 128], [37.5, 37.5, 37.5], [0, 0, 0], [255, 255, 255], [255, 0, 0], [200, 200, 10], [91, 91, 17.25],
                           [12, 230, 230], [250, 240, 230], [183, 3, 1], [0, 0, 255], [1, 254, 2], [0.5, 0.25, 0.125], [254.5, 255, 0]],
                          dtype=np.float32)


def colors(n, seed):
    """(n, 3) float32 on 0..255: the special rows first (as many as fit), seeded uniform rows behind them"""
    c = (np.random.RandomState(seed).rand(n, 3) * 255).astype(np.float32)
    k = min(n, len(SPECIAL_COLORS))
    c[:k] = SPECIAL_COLORS[:k]
    return c


def fixture(n, seed):
    """the sample the augmentation goldens use (tests/golden/make_golden_augment.fixture): a slab of Gaussians, colours on 0..255"""
    g = np.random.RandomState(seed)
    coord = (g.rand(n, 3) * np.array([4.0, 3.0, 1.5])).astype(np.float32)
    d = dict(coord=coord, color=(g.rand(n, 3) * 2 - 1).astype(np.float32), opacity=g.rand(n, 1).astype(np.float32),
             quat=g.randn(n, 4).astype(np.float32), scale=g.rand(n, 3).astype(np.float32),
             segment=g.randint(-1, 20, n).astype(np.int64), lang_feat=g.randn(n, 16).astype(np.float32),
             valid_feat_mask=(g.rand(n) < 0.9).astype(np.int64), name="scene%d" % seed)
    g = np.random.RandomState(seed + 1000)
    d["color"] = (g.rand(n, 3) * 255).astype(np.float32)
    nrm = g.randn(n, 3)
    d["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return d


def crop_fixture(n, seed):
    """fixture + the two keys only SphereCropRandomMaxPoints crops, and a grid_coord"""
    d = fixture(n, seed)
    g = np.random.RandomState(seed + 2000)
    d["sh"], d["lang_feat_64"] = g.randn(n, 9).astype(np.float32), g.randn(n, 64).astype(np.float32)
    d["grid_coord"] = np.floor(d["coord"] / 0.02).astype(np.int32)
    return d


def gray64(c):
    return 0.2989 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2]


def hue64(c, f):
    """adjust_hue (pointcept/datasets/transform.py:905-979) in fp64, tie rules included"""
    rgb = c / 255.0
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    maxc, minc = rgb.max(1), rgb.min(1)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, 1.0, maxc)
    div = np.where(eqc, 1.0, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = (h / 6.0 + 1.0) % 1.0
    h = (h + f) % 1.0
    i = np.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.astype(np.int64) % 6
    v = maxc
    p = np.clip(v * (1.0 - s), 0.0, 1.0)
    q = np.clip(v * (1.0 - s * fr), 0.0, 1.0)
    t = np.clip(v * (1.0 - s * (1.0 - fr)), 0.0, 1.0)
    rows = np.arange(len(c))
    out = np.stack([np.stack((v, q, p, p, t, v), 1)[rows, i], np.stack((t, v, v, q, p, p), 1)[rows, i],
                    np.stack((p, p, t, v, v, q), 1)[rows, i]], 1)
    return out * 255.0


def chain64(color, steps):
    """the colour chain in fp64: steps = [(code, factor), ...] in order; the contrast mean is taken over the running colours"""
    c = np.asarray(color, dtype=np.float64).copy()
    for code, f in steps:
        f = float(f)
        if code == BRIGHTNESS:
            c = np.clip(f * c, 0, 255)
        elif code == CONTRAST:
            c = np.clip(f * c + (1 - f) * gray64(c).mean(), 0, 255)
        elif code == SATURATION:
            c = np.clip(f * c + (1 - f) * gray64(c)[:, None], 0, 255)
        elif code == HUE:
            c = hue64(c, f)
        elif code == GRAY:
            c = np.repeat(gray64(c)[:, None], 3, 1)
        else:
            raise ValueError(code)
    return c


def steps_of(params, gray=False):
    """RandomColorJitter params (order + four factors) [+ a fired grayscale] -> the (code, factor) list the kernel gets"""
    steps = [(int(i) + 1, params[NAMES[int(i)]]) for i in params["order"] if params[NAMES[int(i)]] is not None]
    return steps + ([(GRAY, 0.0)] if gray else [])


# ---- blur -----------------------------------------------------------------------------------------------------------------------
# tag -> (grid size, sigma, occupancy, origin, opacity rule, extra_keys)
BLUR_CASES = {
    "a": ((7, 5, 3), 1.9, 0.6, (0, 0, 0), "mixed", ("scale", "quat", "opacity")),
    "b": ((12, 9, 4), 0.74, 0.5, (0, 0, 0), "mixed", ("opacity", "scale", "quat", "normal")),
    "flat": ((6, 1, 5), 1.0, 0.7, (3, 9, 1), "mixed", ("scale", "quat", "opacity")),
    "r0": ((5, 5, 5), 0.24, 0.5, (0, 0, 0), "mixed", ("scale", "quat", "opacity")),
    "neg": ((7, 5, 3), 0.9, 0.6, (-7, -3, -11), "mixed", ("scale", "quat", "opacity")),
    "all": ((6, 6, 4), 1.2, 0.5, (0, 0, 0), "all", ("scale", "quat", "opacity")),
    "none": ((6, 6, 4), 1.2, 0.5, (0, 0, 0), "none", ("scale", "quat", "opacity")),
    "one": ((1, 1, 1), 1.0, 1.0, (5, -2, 7), "all", ("scale", "quat", "opacity")),
    "color": ((9, 8, 5), 1.4, 0.4, (0, 0, 0), "mixed", ()),
}


def blur_input(tag, seed=300):
    """the sample of a blur case: unique grid_coord in a shuffled order, colour on 0..255, opacity, scale, quat (not normalised), normal"""
    size, sigma, occ, origin, rule, extra = BLUR_CASES[tag]
    g = np.random.RandomState(seed + sorted(BLUR_CASES).index(tag))
    pts = np.argwhere(g.rand(*size) < occ)
    if len(pts) == 0:
        pts = np.zeros((1, 3), dtype=np.int64)
    pts = pts[g.permutation(len(pts))]
    n = len(pts)
    op = g.rand(n, 1).astype(np.float32)
    if rule == "all":
        op = (0.5 + 0.5 * op + 1e-3).astype(np.float32)
    elif rule == "none":
        op = (0.5 * op).astype(np.float32)
    return dict(grid_coord=(pts + np.array(origin)).astype(np.int32), color=(g.rand(n, 3) * 255).astype(np.float32), opacity=op,
                scale=g.rand(n, 3).astype(np.float32), quat=g.randn(n, 4).astype(np.float32),
                normal=g.randn(n, 3).astype(np.float32), coord=g.rand(n, 3).astype(np.float32))


def wide_input(seed=320, per=100, gap=2000):
    """two clusters of about `per` voxels each, `gap` cells apart on every axis: a dense grid over the box would need hundreds of GB"""
    g = np.random.RandomState(seed)
    a = np.argwhere(g.rand(6, 6, 6) < per / 216.0)
    b = np.argwhere(g.rand(6, 6, 6) < per / 216.0) + gap
    pts = np.concatenate([a, b])
    pts = pts[g.permutation(len(pts))]
    n = len(pts)
    return dict(grid_coord=pts.astype(np.int32), color=(g.rand(n, 3) * 255).astype(np.float32), opacity=g.rand(n, 1).astype(np.float32),
                scale=g.rand(n, 3).astype(np.float32), quat=g.randn(n, 4).astype(np.float32), normal=g.randn(n, 3).astype(np.float32))


def reflect(i, size):
    """scipy.ndimage's `reflect` border (d c b a | a b c d | d c b a), any distance outside"""
    p = 2 * size
    i = np.mod(i, p)
    return np.where(i >= size, p - 1 - i, i)


def blur64(d, sigma, extra_keys):
    """GSGaussianBlurVoxelOpc in its direct sparse form, fp64: per masked voxel the weighted sum over the (2r+1)^3 neighbourhood of
    the masked voxels / (weight sum + 1e-7); then every quat row normalised when quat is blurred.  -> dict of fp64 arrays"""
    gc = d["grid_coord"].astype(np.int64)
    mask = (d["opacity"] > 0.5).ravel()
    keys_ = ["color"] + [k for k in ("opacity", "scale", "quat", "normal") if k in extra_keys]
    out = {k: d[k].astype(np.float64).copy() for k in keys_}
    lo = gc.min(0)
    size = gc.max(0) - lo + 1
    pm = gc[mask] - lo
    if len(pm):
        def cell(x, y, z):
            return (x * int(size[1]) + y) * int(size[2]) + z
        keys = cell(pm[:, 0], pm[:, 1], pm[:, 2])
        order = np.argsort(keys)
        skeys = keys[order]
        vals = np.concatenate([d[k][mask].astype(np.float64) for k in keys_] + [np.ones((len(pm), 1))], 1)
        r = int(2.0 * sigma + 0.5)
        x = np.arange(-r, r + 1)
        w = np.exp(-0.5 * x * x / float(sigma) ** 2)
        w /= w.sum()
        acc = np.zeros_like(vals)
        for dx in x:
            qx = reflect(pm[:, 0] + dx, size[0])
            for dy in x:
                qy = reflect(pm[:, 1] + dy, size[1])
                for dz in x:
                    q = cell(qx, qy, reflect(pm[:, 2] + dz, size[2]))
                    pos = np.minimum(np.searchsorted(skeys, q), len(skeys) - 1)
                    hit = skeys[pos] == q
                    acc[hit] += w[dx + r] * w[dy + r] * w[dz + r] * vals[order[pos[hit]]]
        res = acc[:, :-1] / (acc[:, -1:] + 1e-7)
        c0 = 0
        for k in keys_:
            c1 = c0 + out[k].shape[1]
            out[k][mask] = res[:, c0:c1]
            c0 = c1
    if "quat" in out:
        out["quat"] = out["quat"] / np.linalg.norm(out["quat"], axis=1, keepdims=True)
    return out
