"""GPU: the neighbour-search kernels of csrc/pointops.hip and csrc/knn_grid.hip against the exact references of
tests/pointops_cases.py, on lattices, coincident points, batch-element edges and the caps of each kernel.  Coordinates are
multiples of 1 / 4, so every squared distance is exact in float32: indices are compared with array_equal and squared distances
bit for bit; no assertion here has a tolerance.  The brute-force and the grid implementation are each held to the reference on
their own (grid-equals-brute on continuous clouds stays in tests/test_hip_pointops.py).  tests/test_pointops_host.py pins the
cases and the references on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointops_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def cu(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t.to(dt) if dt is not None else t


def dev(c):
    """-> xyz, offset, new_xyz, new_offset on the device, and whether the case is a self query"""
    xyz, off = cu(c.xyz), cu(c.offset, torch.int32)
    if c.new_xyz is None:
        return xyz, off, xyz, off, True
    return xyz, off, cu(c.new_xyz), cu(c.new_offset, torch.int32), False


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(idx, d2, ridx, rd2, what):
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    bad = int(((idx != ridx) | (bits(d2) != bits(rd2))).any(1).sum())
    print("%s: %d of %d queries differ from the reference" % (what, bad, len(ridx)))
    assert np.array_equal(idx, ridx), "%s: %d of %d queries differ" % (what, bad, len(ridx))
    assert np.array_equal(bits(d2), bits(rd2)), what


# the kernels behind the Python surface, without its sqrt: squared distances as the kernels write them
def brute_knn(k, xyz, off, nx, noff):
    from scenesplat_amd import pointops as po
    idx = torch.empty((nx.shape[0], k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((nx.shape[0], k), dtype=torch.float32, device="cuda")
    po.check(po.nv.lib().ss_knn_query(nx.shape[0], k, po._p(xyz), po._p(nx), po._p(off), po._p(noff), off.numel(), po._p(idx), po._p(d2),
                                      po._s()), "ss_knn_query")
    return idx, d2


def brute_ball(ns, max_r, min_r, xyz, off, nx, noff):
    from scenesplat_amd import pointops as po
    m = nx.shape[0]
    idx = torch.empty((m, ns), dtype=torch.int32, device="cuda")
    d2 = torch.empty((m, ns), dtype=torch.float32, device="cuda")
    ws = po.nv._ws(po.nv.lib().ss_ball_query_workspace_bytes(m), xyz.device)
    po.check(po.nv.lib().ss_ball_query(m, ns, float(min_r), float(max_r), po._p(xyz), po._p(nx), po._p(off), po._p(noff), off.numel(),
                                       po._p(idx), po._p(d2), po._p(ws), ws.numel(), po._s()), "ss_ball_query")
    return idx, d2


def random_ball(ns, max_r, min_r, order, xyz, off, nx, noff):
    from scenesplat_amd import pointops as po
    m = nx.shape[0]
    idx = torch.empty((m, ns), dtype=torch.int32, device="cuda")
    d2 = torch.empty((m, ns), dtype=torch.float32, device="cuda")
    po.check(po.nv.lib().ss_random_ball_query(m, ns, float(min_r), float(max_r), po._p(order), po._p(xyz), po._p(nx), po._p(off),
                                              po._p(noff), off.numel(), po._p(idx), po._p(d2), po._s()), "ss_random_ball_query")
    return idx, d2


# ---- kNN --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.KNN_CASES)
def test_knn_brute_force_equals_the_reference(name):
    """k_knn<1 / 8 / 32 / 128> at every k of the case, padding included"""
    c = pc.knn_case(name)
    ridx, rd2 = pc.knn_expected(name)
    xyz, off, nx, noff, _ = dev(c)
    for k in c.ks:
        idx, d2 = brute_knn(k, xyz, off, nx, noff)
        same(idx, d2, ridx[:, :k], rd2[:, :k], "knn brute %s k=%d" % (name, k))


GRID_PARAMS = [(name, cell) for name in pc.KNN_CASES for cell in (None,) + tuple(pc.knn_case(name).cells)]


@pytest.mark.parametrize("name,cell", GRID_PARAMS, ids=["%s-cell%s" % (n, "auto" if c is None else c) for n, c in GRID_PARAMS])
def test_knn_grid_equals_the_reference(name, cell):
    """k_kg_query with the automatic cell size and with cells of 1 and 2 (lattice points on cell faces): ties across the k-th place go
    to the smaller index, in the ring search, in rings r0 > 0 and in the wave-wide fallback scan alike"""
    from scenesplat_amd import pointops as po
    c = pc.knn_case(name)
    ridx, rd2 = pc.knn_expected(name)
    xyz, off, nx, noff, self_query = dev(c)
    failed = []
    for k in c.ks:
        if k > 64:
            continue
        idx, d2 = po._knn_grid(k, xyz, off, nx, noff, self_query, cell=cell)
        try:
            same(idx, d2, ridx[:, :k], rd2[:, :k], "knn grid %s cell=%s k=%d" % (name, cell, k))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed


@pytest.mark.parametrize("name", ["lat16_4095", "lat16"])
def test_knn_auto_dispatch_equals_the_reference_on_both_sides_of_the_threshold(name):
    from scenesplat_amd import pointops as po
    c = pc.knn_case(name)
    assert (len(c.xyz) >= po.KNN_GRID_MIN_POINTS) == (name == "lat16") and po.KNN_GRID_MIN_POINTS == 4096
    ridx, rd2 = pc.knn_expected(name)
    idx, dist = po.knn_query(25, cu(c.xyz), cu(c.offset, torch.int32))
    assert np.array_equal(idx.cpu().numpy(), ridx[:, :25])
    assert torch.equal(dist, torch.sqrt(cu(rd2[:, :25])))


@pytest.mark.parametrize("n_valid", [4095, 4096])
def test_neighbor_voting_on_the_lattice_equals_reference_knn_plus_reference_vote(n_valid):
    from scenesplat_amd import pointops as po
    v = pc.voting_case(n_valid)
    out = po.neighbor_voting(cu(v.xyz), cu(v.labels), cu(v.valid), v.k, v.ignore, v.C).cpu().numpy()
    bad = int((out != v.expected).sum())
    print("neighbor_voting, %d valid: %d of %d labels differ from the reference" % (n_valid, bad, len(out)))
    assert np.array_equal(out, v.expected), bad


# ---- ball queries -------------------------------------------------------------------------------------------------------------------
def _ball(impl, ns, mx, mn, xyz, off, nx, noff, self_query):
    from scenesplat_amd import pointops as po
    if impl == "brute":
        return brute_ball(ns, mx, mn, xyz, off, nx, noff)
    return po._knn_grid(ns, xyz, off, nx, noff, self_query, cell=float(mx), ball=(float(mn), float(mx)))


@pytest.mark.parametrize("impl", ["brute", "grid"])
@pytest.mark.parametrize("shell", pc.BALL_SHELLS, ids=["r%s-%s" % s for s in pc.BALL_SHELLS])
@pytest.mark.parametrize("name", ["half8", "half8_b3"])
def test_ball_query_on_lattice_shells_equals_the_reference(name, shell, impl):
    """d2 == max2 excluded, d2 == min2 included, the query's own point kept under min_radius > 0; nsample below and above the count"""
    c = pc.ball_case(name)
    xyz, off, nx, noff, self_query = dev(c)
    for ns in pc.BALL_NSAMPLE:
        ridx, rd2, _ = pc.ball_expected(name, ns, *shell)
        idx, d2 = _ball(impl, ns, shell[0], shell[1], xyz, off, nx, noff, self_query)
        same(idx, d2, ridx, rd2, "ball %s %s %s nsample=%d" % (impl, name, shell, ns))


@pytest.mark.parametrize("impl", ["brute", "grid"])
@pytest.mark.parametrize("count", pc.BALL_COUNTS)
def test_ball_query_at_exact_candidate_counts_equals_the_reference(count, impl):
    """63 / 64 / 65 / 1025 candidates (power-of-two padding of the LDS sort), 2047 / 2048 / 2049 (in cap, at cap, overflow re-scan
    in index order)"""
    name = "count%d" % count
    c = pc.ball_case(name)
    xyz, off, nx, noff, self_query = dev(c)
    for ns, shell in ((16, (2.5, 0.0)), (65, (2.5, 0.0)), (64, (2.5, 0.5))):
        ridx, rd2, cnt = pc.ball_expected(name, ns, *shell)
        assert shell[1] > 0 or cnt[0] == count
        idx, d2 = _ball(impl, ns, shell[0], shell[1], xyz, off, nx, noff, self_query)
        same(idx, d2, ridx, rd2, "ball %s %s %s nsample=%d" % (impl, name, shell, ns))


@pytest.mark.parametrize("name", ["half8", "half8_b3"])
def test_random_ball_query_equals_the_reference(name):
    c = pc.ball_case(name)
    xyz, off, nx, noff, _ = dev(c)
    order = pc.ball_order(c)
    for ns, (mx, mn) in ((16, (2.5, 0.5)), (64, (1.0, 0.0)), (1, (2.0, 1.0)), (65, (1.5, 0.5))):
        ridx, rd2, _ = pc.random_ball_ref(ns, mx, mn, order, c.xyz, c.offset, c.new_xyz, c.new_offset)
        idx, d2 = random_ball(ns, mx, mn, cu(order, torch.int32), xyz, off, nx, noff)
        same(idx, d2, ridx, rd2, "random ball %s (%s, %s) nsample=%d" % (name, mx, mn, ns))


# ---- sampling, pointgroup, vote -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.FPS_CASES)
def test_farthest_point_sampling_equals_the_reference(name):
    from scenesplat_amd import pointops as po
    c = pc.fps_case(name)
    out = po.farthest_point_sampling(cu(c.xyz), cu(c.offset, torch.int32), cu(c.new_offset, torch.int32)).cpu().numpy()
    ref = pc.fps_ref(c.xyz, c.offset, c.new_offset)
    assert np.array_equal(out, ref), int((out != ref).sum())


@pytest.mark.parametrize("name", pc.BQ_CASES)
def test_ballquery_batch_p_and_bfs_cluster_equal_the_references(name):
    """meanActive = 1: the pair buffer regrows.  The union-find reference needs symmetric neighbour lists, so the clusters are
    compared wherever the 1000-neighbour cap cut nothing (every case but `capped`)."""
    from scenesplat_amd import pointops as po
    c = pc.bq_case(name)
    ridx, rsl, _ = pc.bq_expected(name)
    idx, start_len = po.ballquery_batch_p(cu(c.xyz), cu(c.batch_idxs, torch.int32), cu(c.batch_offsets, torch.int32), c.radius, 1)
    assert np.array_equal(start_len.cpu().numpy(), rsl) and np.array_equal(idx.cpu().numpy(), ridx)
    if name != "capped":
        ci, co = po.bfs_cluster(torch.as_tensor(c.labels), idx.cpu(), start_len.cpu(), 3)
        got, ref = pc.clusters_of(ci.numpy(), co.numpy()), pc.clusters_ref(c.labels, ridx, rsl, 3)
        assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("ignore_label", [-1, 255])
@pytest.mark.parametrize("k", pc.VOTE_K)
def test_majority_vote_equals_the_reference(k, ignore_label):
    from scenesplat_amd import pointops as po
    for m in pc.VOTE_M:
        nn, labels, ig, C = pc.vote_case(k, m, ignore_label)
        out = po.majority_vote(cu(nn), cu(labels), ig, C).cpu().numpy()
        assert np.array_equal(out, pc.vote_ref(nn, labels, ig, C)), (k, m)


def test_majority_vote_with_one_class():
    from scenesplat_amd import pointops as po
    for k, m in ((1, 5), (25, 9), (64, 1000)):
        nn, labels, ig, C = pc.vote_case(k, m, -1, num_classes=1)
        out = po.majority_vote(cu(nn), cu(labels), ig, C).cpu().numpy()
        assert np.array_equal(out, pc.vote_ref(nn, labels, ig, C)), (k, m)
