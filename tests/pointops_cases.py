"""Inputs and exact references shared by tests/test_hip_pointops_edges.py (GPU) and tests/test_pointops_host.py (CPU) for the
neighbour-search kernels of csrc/pointops.hip and csrc/knn_grid.hip.  Everything is built on the CPU from seeded generators;
nothing here touches the library under test or oracle/pointops.py.

Exactness: every coordinate is j / 4 with integer |j| < 1024.  A coordinate difference is then i / 4 with |i| < 2048, its square
i^2 / 16 with i^2 < 2^22 and the three-term sum s / 16 with s < 3 * 2^22 < 2^24: each intermediate is a float32 value, whatever the
compiler contracts into an fma.  The references therefore work in int64 on 4 * xyz ("quarters"; a squared distance in quarters is
16 * d2) and the tests compare indices with array_equal and squared distances bit for bit.  Radii have exactly representable
squares (0.5, 1.0, 1.5, 2.0, 2.5), and the smallest non-zero squared distance is 1 / 16, so `d2 <= 1e-5` means d2 == 0."""
import functools
import types

import numpy as np

Q = 4                      # coordinates are j / Q
COORD_LIMIT = 1024         # |j| < COORD_LIMIT
BALL_CAP = 2048            # candidates a ball query keeps (the first in index order)
PG_CAP = 1000              # neighbours ballquery_batch_p keeps per point (the first in index order)
KG_RING_MAX = 6            # rings the grid kNN probes before it scans the batch element wave-wide
RADII = (0.5, 1.0, 1.5, 2.0, 2.5)
KNN_K_BOTH = (1, 5, 7, 8, 9, 25, 32, 33, 64)     # k_knn<8 / 32 / 128> template edges, one list entry per lane of the grid search
KNN_K_BRUTE_ONLY = (65, 128)
KNN_K_MAX = 128


# ---- coordinates ----------------------------------------------------------------------------------------------------------------
def coords(j):
    """(n, 3) float32 = j / 4 for integer j"""
    j = np.asarray(j, np.int64).reshape(-1, 3)
    assert np.abs(j).max(initial=0) < COORD_LIMIT
    return (j / Q).astype(np.float32)


def quarters(xyz):
    """(n, 3) int64 = 4 * xyz; asserts that xyz is float32, a multiple of 1 / 4 and inside the exactness range"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32
    j = np.rint(xyz.astype(np.float64) * Q).astype(np.int64)
    assert np.array_equal((j / Q).astype(np.float32), xyz) and np.abs(j).max(initial=0) < COORD_LIMIT
    return j.reshape(-1, 3)


def d2q(qj, pj):
    """(m, n) int64: squared distances in quarters (16 * d2)"""
    d = qj[:, None, :] - pj[None, :, :]
    return (d * d).sum(-1)


def r2q(radius):
    """16 * radius^2 as an integer"""
    v = (Q * float(radius)) ** 2
    assert v == int(v)
    return int(v)


def segments(offset):
    offset = np.asarray(offset, np.int64)
    return np.concatenate([[0], offset[:-1]]), offset


def batch_of_rows(offset, m):
    """(m) batch element of every row under the cumulative `offset` (empty elements own no row)"""
    return np.searchsorted(np.asarray(offset, np.int64), np.arange(m), side="right")


def _resolve(xyz, offset, new_xyz, new_offset):
    if new_xyz is None:
        new_xyz, new_offset = xyz, offset
    return quarters(xyz), np.asarray(offset, np.int64), quarters(new_xyz), np.asarray(new_offset, np.int64)


# ---- references -----------------------------------------------------------------------------------------------------------------
def knn_ref(k, xyz, offset, new_xyz=None, new_offset=None):
    """The k smallest (d2, index) of the query's batch element, ascending -> idx (m, k) int32 (-1 pad), d2 (m, k) float32
    (1e10 pad).  The top k of a query is the first k columns of its top k' for every k' >= k."""
    pj, off, qj, noff = _resolve(xyz, offset, new_xyz, new_offset)
    m = len(qj)
    idx = np.full((m, k), -1, np.int32)
    d2 = np.full((m, k), 1e10, np.float32)
    (st, en), (qst, qen) = segments(off), segments(noff)
    for b in range(len(off)):
        n_b = int(en[b] - st[b])
        if qen[b] <= qst[b] or n_b == 0:
            continue
        assert n_b <= 8192
        kk = min(k, n_b)
        for r0 in range(int(qst[b]), int(qen[b]), 512):
            r1 = min(r0 + 512, int(qen[b]))
            key = d2q(qj[r0:r1], pj[st[b]:en[b]]) * 8192 + np.arange(n_b)          # unique: (d2, index) in one integer
            top = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
            idx[r0:r1, :kk] = st[b] + (top & 8191)
            d2[r0:r1, :kk] = ((top >> 13) / 16.0).astype(np.float32)
    return idx, d2


def ball_ref(nsample, max_radius, min_radius, xyz, offset, new_xyz=None, new_offset=None):
    """keep d2 <= 1e-5 or min2 <= d2 < max2; the first 2048 in index order; sorted by (d2, index); all of them (-1 / 1e10 pad) or
    the strided sorted[int(float32(num) / float32(nsample) * i)] -> idx (m, nsample) int32, d2 float32, count (m) candidates
    BEFORE the cap."""
    pj, off, qj, noff = _resolve(xyz, offset, new_xyz, new_offset)
    mn, mx = r2q(min_radius), r2q(max_radius)
    m = len(qj)
    idx = np.full((m, nsample), -1, np.int32)
    d2 = np.full((m, nsample), 1e10, np.float32)
    count = np.zeros(m, np.int64)
    st, en = segments(off)
    bq = batch_of_rows(noff, m)
    for q in range(m):
        s, e = int(st[bq[q]]), int(en[bq[q]])
        D = d2q(qj[q:q + 1], pj[s:e])[0]
        cand = np.nonzero((D == 0) | ((D >= mn) & (D < mx)))[0]
        count[q] = len(cand)
        cand = cand[:BALL_CAP]
        cand = cand[np.lexsort((cand, D[cand]))]
        num = len(cand)
        if num > nsample:
            sep = np.float32(num) / np.float32(nsample)
            cand = cand[(sep * np.arange(nsample, dtype=np.float32)).astype(np.int64)]
        idx[q, :len(cand)] = s + cand
        d2[q, :len(cand)] = (D[cand] / 16.0).astype(np.float32)
    return idx, d2, count


def random_ball_ref(nsample, max_radius, min_radius, order, xyz, offset, new_xyz=None, new_offset=None):
    """the first nsample hits along order[start : end] of the query's batch element -> idx, d2, hits (m) before the cut"""
    pj, off, qj, noff = _resolve(xyz, offset, new_xyz, new_offset)
    mn, mx = r2q(min_radius), r2q(max_radius)
    order = np.asarray(order, np.int64)
    m = len(qj)
    idx = np.full((m, nsample), -1, np.int32)
    d2 = np.full((m, nsample), 1e10, np.float32)
    hits = np.zeros(m, np.int64)
    st, en = segments(off)
    bq = batch_of_rows(noff, m)
    for q in range(m):
        o = order[int(st[bq[q]]):int(en[bq[q]])]
        D = d2q(qj[q:q + 1], pj[o])[0]
        hit = np.nonzero((D == 0) | ((D >= mn) & (D < mx)))[0]
        hits[q] = len(hit)
        hit = hit[:nsample]
        idx[q, :len(hit)] = o[hit]
        d2[q, :len(hit)] = (D[hit] / 16.0).astype(np.float32)
    return idx, d2, hits


def fps_ref(xyz, offset, new_offset):
    """per batch element: its first point, then the arg-max of the running minimum distance to the chosen ones, the lowest index
    on ties -> idx (new_offset[-1]) int32"""
    pj = quarters(xyz)
    (st, en), (ost, oen) = segments(offset), segments(new_offset)
    out = np.zeros(int(np.asarray(new_offset)[-1]), np.int32)
    for b in range(len(st)):
        if oen[b] <= ost[b] or en[b] <= st[b]:
            continue
        p = pj[st[b]:en[b]]
        running = np.full(len(p), np.iinfo(np.int64).max)
        cur = 0
        out[ost[b]] = st[b]
        for j in range(int(ost[b]) + 1, int(oen[b])):
            running = np.minimum(running, ((p - p[cur]) ** 2).sum(1))
            cur = int(np.argmax(running))              # first maximum = lowest index
            out[j] = st[b] + cur
    return out


def ballquery_ref(xyz, batch_idxs, batch_offsets, radius):
    """strict d2 < r2, at most 1000 per point in index order -> idx (nActive) int32, start_len (n, 2) int32 (CSR start, length),
    full (n) neighbour counts before the cap"""
    pj = quarters(xyz)
    r2 = r2q(radius)
    n = len(pj)
    parts, start_len, full = [], np.zeros((n, 2), np.int32), np.zeros(n, np.int64)
    pos = 0
    for i in range(n):
        s, e = int(batch_offsets[batch_idxs[i]]), int(batch_offsets[batch_idxs[i] + 1])
        hit = s + np.nonzero(d2q(pj[i:i + 1], pj[s:e])[0] < r2)[0]
        full[i] = len(hit)
        hit = hit[:PG_CAP]
        start_len[i] = (pos, len(hit))
        pos += len(hit)
        parts.append(hit)
    return np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32), start_len, full


def clusters_ref(labels, ball_idx, start_len, threshold):
    """union-find over the ball-query pairs that join equal labels -> list of sorted int64 arrays, the components with at least
    `threshold` points, ordered by their smallest point (the order a sweep over the points discovers them in).  Valid for
    symmetric neighbour lists, i.e. where the 1000-neighbour cap did not cut any."""
    n = len(labels)
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        s, ln = int(start_len[i, 0]), int(start_len[i, 1])
        for j in ball_idx[s:s + ln]:
            if labels[j] == labels[i]:
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(n)])
    return [np.nonzero(root == r)[0] for r in np.unique(root) if int((root == r).sum()) >= threshold]


def clusters_of(cluster_idxs, cluster_offsets):
    """bfs_cluster's (sum, 2) / (nCluster + 1) output as the list clusters_ref returns; asserts that the rows of a cluster are
    contiguous and carry its number, and that every cluster starts with its smallest point"""
    cluster_idxs, cluster_offsets = np.asarray(cluster_idxs, np.int64), np.asarray(cluster_offsets, np.int64)
    out = []
    for c in range(len(cluster_offsets) - 1):
        rows = cluster_idxs[cluster_offsets[c]:cluster_offsets[c + 1]]
        assert (rows[:, 0] == c).all() and rows[0, 1] == rows[:, 1].min()
        out.append(np.sort(rows[:, 1]))
    assert cluster_offsets[0] == 0 and cluster_offsets[-1] == len(cluster_idxs)
    return out


def vote_ref(nn_idx, labels, ignore_label, num_classes):
    """per row: the valid label with the largest count, the smallest label on ties; a neighbour is invalid when its index is < 0
    or its label is the ignore label, < 0 or >= num_classes; ignore_label when no neighbour is valid -> (m) int32"""
    nn_idx, labels = np.asarray(nn_idx, np.int64), np.asarray(labels, np.int64)
    out = np.full(len(nn_idx), ignore_label, np.int32)
    for i, row in enumerate(nn_idx):
        lab = labels[row[row >= 0]]
        lab = lab[(lab != ignore_label) & (lab >= 0) & (lab < num_classes)]
        if len(lab):
            values, counts = np.unique(lab, return_counts=True)         # ascending values: argmax takes the smallest label
            out[i] = values[np.argmax(counts)]
    return out


def grid_strict_emulation(k, xyz, offset, cell):
    """What a ring search returns that admits a candidate only when its distance is STRICTLY below the current k-th distance, with
    candidates arriving in ring, cell and then index order (self query): the admission rule of kg_offer before it carried the k-th
    entry's index.  -> idx (n, k) int32, for comparison with knn_ref on the tie cases."""
    import bisect
    pj, off = quarters(xyz), np.asarray(offset, np.int64)
    n = len(pj)
    cq = int(round(cell * Q))
    cells = (pj - pj.min(0)) // cq
    side = int(cells.max()) + 1
    flat = (cells[:, 0] * side + cells[:, 1]) * side + cells[:, 2]
    out = np.full((n, k), -1, np.int32)
    st, en = segments(off)
    bq = batch_of_rows(off, n)
    for q in range(n):
        s, e = int(st[bq[q]]), int(en[bq[q]])
        ring = np.abs(cells[s:e] - cells[q]).max(1)
        # within a ring the kernel walks the cells of the (2r + 1)^3 cube x-major: the cell-offset order is the flat-index order
        arrival = s + np.lexsort((np.arange(e - s), flat[s:e], ring))
        D = d2q(pj[q:q + 1], pj[arrival])[0]
        best = []
        for d, i in zip(D.tolist(), arrival.tolist()):
            if len(best) == k:
                if not d < best[-1][0]:
                    continue
                best.pop()
            bisect.insort(best, (d, i))
        out[q, :len(best)] = [i for _, i in best]
    return out


# ---- point sets -----------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(90000 + seed)


def lattice(nx, ny, nz, step=Q, origin=(0, 0, 0)):
    """(nx * ny * nz, 3) int64 quarters of a lattice with `step` quarters between neighbours (step = 4: integer coordinates)"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g * step + np.asarray(origin, np.int64)


def _shuffled(j, seed):
    return j[_rng(seed).permutation(len(j))]


def _case(name, parts, queries=None, **extra):
    """parts: list of (n_b, 3) quarter arrays, one per batch element (possibly empty); queries: the same per element, or None for a
    self query"""
    xyz = coords(np.concatenate(parts)) if sum(len(p) for p in parts) else np.zeros((0, 3), np.float32)
    offset = np.cumsum([len(p) for p in parts]).astype(np.int32)
    new_xyz = new_offset = None
    if queries is not None:
        new_xyz = coords(np.concatenate(queries))
        new_offset = np.cumsum([len(p) for p in queries]).astype(np.int32)
    return types.SimpleNamespace(name=name, xyz=xyz, offset=offset, new_xyz=new_xyz, new_offset=new_offset, **extra)


EMPTY = np.zeros((0, 3), np.int64)


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """The kNN cases.  `cells`: the grid cell sizes to run besides the automatic one; `ks`: the neighbour counts."""
    if name == "lat8":                         # 8^3 integer lattice, one element
        return _case(name, [_shuffled(lattice(8, 8, 8), 1)], cells=(1.0, 2.0), ks=KNN_K_BOTH + KNN_K_BRUTE_ONLY)
    if name == "lat8_one":                     # two elements, the second a single point: k > segment pads everywhere
        return _case(name, [_shuffled(lattice(8, 8, 8), 2), np.array([[12, 8, 4]])], cells=(1.0, 2.0), ks=(1, 5, 25))
    if name == "lat8_empty_mid":               # three elements, the middle one empty (offset = [a, a, b]); the last holds 64 points
        return _case(name, [_shuffled(lattice(8, 8, 8), 3), EMPTY, _shuffled(lattice(4, 4, 4, origin=(40, 0, 0)), 4)],
                     cells=(1.0, 2.0), ks=(5, 25, 64, 65, 128))
    if name == "lat16":                        # 4096 points: the size at which impl="auto" takes the grid
        return _case(name, [_shuffled(lattice(16, 16, 16), 5)], cells=(2.0,), ks=(1, 7, 25, 64, 128))
    if name == "lat16_4095":
        return _case(name, [_shuffled(lattice(16, 16, 16), 5)[:4095]], cells=(), ks=(25,))
    if name == "sheet64":                      # a surface, as in rooms
        return _case(name, [_shuffled(lattice(64, 64, 1), 6)], cells=(1.0, 2.0), ks=(5, 9, 32, 33))
    if name == "dup3":                         # every point three times: d2 = 0 ties, k below, at and above the multiplicity
        return _case(name, [_shuffled(np.repeat(lattice(6, 6, 6), 3, 0), 7)], cells=(1.0, 2.0), ks=(1, 2, 3, 4, 5, 25))
    if name == "outside":                      # queries outside the box on all six sides at lattice multiples: ties in rings r0 > 0
        data = _shuffled(lattice(8, 8, 8), 8)
        q = []
        for axis in range(3):
            for pos in (-1, -3, -12, 8, 11, 20):
                for a, b in ((3, 4), (0, 7), (-2, 9), (3.5, 3.5)):     # the last: four nearest points at one distance
                    p = [a, b, b]; p[axis] = pos
                    q.append(p)
        q += [[-3, -3, -3], [10, 10, 10], [-5, 12, 3], [3, -8, 15]]
        return _case(name, [data], [(np.array(q) * Q).astype(np.int64)], cells=(1.0, 2.0), ks=(1, 5, 7, 25, 64))
    if name == "sparse":                       # more than KG_RING_MAX rings between the queries and the lattice cluster
        far = np.array([60, 60, 60]) * Q
        near = far + np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [-2, 0, 0], [0, -2, 0],
                               [0, 0, -2], [5, 5, 0], [5, 0, 5], [0, 5, 5]]) * Q
        data = _shuffled(np.concatenate([lattice(4, 4, 4), near, np.array([[30, 30, 30], [30, 30, 0]]) * Q]), 9)
        return _case(name, [data], cells=(1.0, 2.0), ks=(1, 5, 9, 25, 64))
    if name == "crowded_cells":                # cells of size 2 holding 63, 64, 65 and 129 points of the quarter lattice
        parts = []
        for c, (cnt, org) in enumerate(((63, (0, 0, 0)), (64, (32, 0, 0)), (65, (0, 32, 0)), (129, (32, 32, 0)))):
            inner = lattice(8, 8, 8, step=1)                                  # the 512 quarter positions inside [0, 2)^3
            pick = np.concatenate([[0], 1 + _rng(20 + c).permutation(511)[:cnt - 1]])     # the cell's corner is always present
            parts.append(inner[pick] + np.asarray(org))
        return _case(name, [_shuffled(np.concatenate(parts), 10)], cells=(2.0,), ks=(5, 7, 25, 64))
    raise KeyError(name)


KNN_CASES = ("lat8", "lat8_one", "lat8_empty_mid", "lat16", "lat16_4095", "sheet64", "dup3", "outside", "sparse", "crowded_cells")


@functools.lru_cache(maxsize=None)
def knn_expected(name):
    """(idx, d2) at k = KNN_K_MAX; the first k columns are the reference at k"""
    c = knn_case(name)
    return knn_ref(KNN_K_MAX, c.xyz, c.offset, c.new_xyz, c.new_offset)


def tie_straddles(name, k):
    """number of queries whose k-th and (k + 1)-th candidate are equally far (both exist): where the order among equals decides
    WHICH neighbours are returned"""
    idx, d2 = knn_expected(name)
    assert k < KNN_K_MAX
    return int(((idx[:, k] >= 0) & (d2[:, k - 1] == d2[:, k])).sum())


# ---- ball queries ---------------------------------------------------------------------------------------------------------------
BALL_SHELLS = ((1.0, 0.0), (1.5, 0.5), (2.0, 1.0), (2.5, 2.0), (2.5, 0.0))     # (max_radius, min_radius)
BALL_NSAMPLE = (1, 16, 64, 65)
BALL_COUNTS = (63, 64, 65, 1025, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def ball_case(name):
    if name == "half8":          # 8^3 lattice with spacing 1/2: every radius of RADII is a shell of it (d2 = r^2 occurs)
        return _case(name, [_shuffled(lattice(8, 8, 8, step=2), 11)])
    if name == "half8_b3":       # three elements with an empty one in the middle; separate queries, some coinciding with points
        data = [_shuffled(lattice(8, 8, 8, step=2), 12), EMPTY, _shuffled(lattice(5, 5, 5, step=2, origin=(80, 0, 0)), 13)]
        return _case(name, data, [data[0][:40] + np.array([0, 0, 0]), EMPTY, np.concatenate([data[2][:20], data[2][:5] + np.array([1, 0, 0])])])
    if name.startswith("count"):
        # a query at the origin whose ball of radius 2.5 holds exactly N candidates: N points of the quarter lattice with d2 < 6.25
        # (the last 5 of them duplicates of the first 5), all six axis points ON the shell d2 == 6.25 and points beyond it; shuffled, so
        # the first 2048 in index order are not the nearest 2048
        N = int(name[5:])
        g = _rng(100 + N)
        cube = lattice(21, 21, 21, step=1, origin=(-10, -10, -10))
        dd = (cube * cube).sum(1)
        inside, beyond = cube[dd < 100], cube[dd > 100]
        inside = inside[g.permutation(len(inside))[:N - 5]]
        shell = np.array([[10, 0, 0], [-10, 0, 0], [0, 10, 0], [0, -10, 0], [0, 0, 10], [0, 0, -10]])
        data = np.concatenate([inside, inside[:5], shell, beyond[g.permutation(len(beyond))[:120]]])
        data = data[g.permutation(len(data))]
        queries = np.concatenate([[[0, 0, 0]], data[:31]])
        return _case(name, [data], [queries], target=N)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ball_expected(name, nsample, max_radius, min_radius):
    c = ball_case(name)
    return ball_ref(nsample, max_radius, min_radius, c.xyz, c.offset, c.new_xyz, c.new_offset)


def ball_order(case, seed=0):
    """a permutation of every batch element's rows, as random_ball_query takes it"""
    st, en = segments(case.offset)
    return np.concatenate([s + _rng(300 + seed + b).permutation(int(e - s)) for b, (s, e) in enumerate(zip(st, en))]).astype(np.int32)


# ---- farthest point sampling ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fps_case(name):
    """segment sizes around the 1024-thread stride loop, lattice ties, an all-duplicate segment, a segment sampled completely and
    an empty OUTPUT segment between two non-empty ones"""
    lat = _shuffled(lattice(16, 16, 16), 14)
    if name == "strides":
        parts = [lat[:1], lat[1:1024], lat[1024:2048], lat[2048:3073], np.repeat(np.array([[7, 9, 11]]) * Q, 50, 0),
                 _shuffled(lattice(4, 4, 4, origin=(100, 0, 0)), 15)]
        counts = [1, 40, 40, 40, 10, 64]
    elif name == "long":
        parts = [lat[:2049], lat[2049:2056], lat[2056:2156]]
        counts = [30, 0, 100]
    else:
        raise KeyError(name)
    c = _case(name, parts)
    c.new_offset = np.cumsum(counts).astype(np.int32)
    return c


FPS_CASES = ("strides", "long")


# ---- pointgroup ball query ------------------------------------------------------------------------------------------------------
BQ_SIZES = (1, 1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def bq_case(name):
    """-> xyz, batch_idxs (n), batch_offsets (nb + 1), radius, labels (n)"""
    if name == "capped":     # 1100 points on 27 positions within 1/2 of each other: every ball of radius 1 holds all 1100 (> 1000)
        g = _rng(40)
        crowd = lattice(3, 3, 3, step=1)[g.integers(0, 27, 1100)]
        parts = [crowd, _shuffled(lattice(4, 4, 3, step=2, origin=(200, 0, 0)), 41)]
    else:                    # n points of a lattice with spacing 1/2 (radius 1 is a shell of it), two elements from 1023 points on
        n = int(name[1:])
        pts = _shuffled(lattice(16, 16, 16, step=2), 42)[:n]
        parts = [pts] if n < 1023 else [pts[:n // 3], pts[n // 3:]]
    c = _case(name, parts)
    c.batch_offsets = np.concatenate([[0], c.offset]).astype(np.int32)
    c.batch_idxs = np.repeat(np.arange(len(parts)), [len(p) for p in parts]).astype(np.int32)
    c.radius = 1.0
    c.labels = (quarters(c.xyz)[:, 0] >= 16).astype(np.int32)
    return c


BQ_CASES = tuple("n%d" % n for n in BQ_SIZES) + ("capped",)


@functools.lru_cache(maxsize=None)
def bq_expected(name):
    c = bq_case(name)
    return ballquery_ref(c.xyz, c.batch_idxs, c.batch_offsets, c.radius)


# ---- majority vote --------------------------------------------------------------------------------------------------------------
VOTE_K = (1, 2, 25, 31, 32, 33, 63, 64)            # a group of 32 lanes up to k = 32, of 64 beyond
VOTE_M = (1, 3, 4, 5, 7, 8, 9, 1000)               # 8 or 4 points per 256-thread workgroup


@functools.lru_cache(maxsize=None)
def vote_case(k, m, ignore_label, num_classes=None):
    """-> nn_idx (m, k) int32, labels (n) int32, ignore_label, num_classes.  Labels hold valid classes, the ignore label, negative
    and too-large values; the rows cycle through: random, no valid neighbour (all -1), no valid neighbour (ignored / out-of-range
    labels only), an exact count tie between class 0 and the highest class, a single valid neighbour in the last column."""
    g = _rng(500 + 64 * k + m + (7 if ignore_label == 255 else 0))
    C = num_classes if num_classes is not None else (260 if ignore_label == 255 else 20)
    valid = np.arange(C)
    valid = valid[valid != ignore_label]
    bad = np.array([ignore_label, -1, -2, C, C + 5, 255 if ignore_label != 255 else -7])
    bad = bad[(bad == ignore_label) | (bad < 0) | (bad >= C)]
    labels = np.concatenate([valid, bad, g.choice(valid, 200), g.choice(bad, 40)]).astype(np.int32)
    n_valid, n = len(valid), len(labels)
    bad_rows = np.arange(n_valid, n_valid + len(bad))
    nn = g.integers(-1, n, (m, k))
    for i in range(m):
        kind = i % 5
        if kind == 1:
            nn[i] = -1
        elif kind == 2:
            nn[i] = g.choice(bad_rows, k)
        elif kind == 3:
            nn[i, :] = -1
            half = k // 2
            nn[i, :half] = n_valid - 1                   # the highest valid class first ...
            nn[i, half:2 * half] = 0                     # ... and as many of class valid[0]: the smaller label wins
        elif kind == 4:
            nn[i] = g.choice(bad_rows, k)
            nn[i, k - 1] = n_valid - 1
    return nn.astype(np.int32), labels, int(ignore_label), int(C)


# ---- neighbour voting on the lattice ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def voting_case(n_valid):
    """16^3 shuffled integer lattice, n_valid of its 4096 points valid (4095: brute force under impl="auto", 4096: the grid) ->
    xyz, labels, valid, k, ignore, C and the expected labels from knn_ref + vote_ref"""
    xyz = coords(_shuffled(lattice(16, 16, 16), 16))
    g = _rng(600)
    C, k = 20, 25
    labels = g.integers(0, C, len(xyz)).astype(np.int32)
    labels[g.random(len(xyz)) < 0.1] = -1
    valid = np.ones(len(xyz), bool)
    valid[g.permutation(len(xyz))[:len(xyz) - n_valid]] = False
    vx = xyz[valid]
    idx, _ = knn_ref(k, vx, np.array([len(vx)]), xyz, np.array([len(xyz)]))
    return types.SimpleNamespace(xyz=xyz, labels=labels, valid=valid, k=k, ignore=-1, C=C,
                                 expected=vote_ref(idx, labels[valid], -1, C), nn=idx)
