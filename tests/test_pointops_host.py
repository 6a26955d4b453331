"""CPU side of tests/test_hip_pointops_edges.py: pins tests/pointops_cases.py itself.  The new references equal oracle/pointops.py
wherever its loops are affordable, the coordinates are exact in float32, every case reaches the structure it is named for, and a
numpy restatement of the grid search's former admission rule (strictly below the k-th distance, candidates in cell order) disagrees
with the reference on the tie cases -- so those cases tell the two rules apart without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointops_cases as pc  # noqa: E402

from oracle import pointops as opo  # noqa: E402


def _all_cases():
    for name in pc.KNN_CASES:
        yield pc.knn_case(name)
    for name in ("half8", "half8_b3") + tuple("count%d" % n for n in pc.BALL_COUNTS):
        yield pc.ball_case(name)
    for name in pc.FPS_CASES:
        yield pc.fps_case(name)
    for name in pc.BQ_CASES:
        yield pc.bq_case(name)


def _f32_d2(q, p):
    """the kernels' expression in float32, term by term"""
    d = q[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def test_coordinates_are_exact_in_float32():
    for c in _all_cases():
        pj = pc.quarters(c.xyz)                                   # asserts float32, multiples of 1 / 4, |j| < 1024
        qx = c.xyz if c.new_xyz is None else c.new_xyz
        qj = pc.quarters(qx)
        q, p, qq, pp = qx[:64], c.xyz[:1500], qj[:64], pj[:1500]
        f32 = _f32_d2(q, p)
        f64 = _f32_d2(q.astype(np.float64), p.astype(np.float64))
        assert f32.dtype == np.float32
        assert np.array_equal(f32, f64.astype(np.float32)) and np.array_equal(f32.astype(np.float64), f64), c.name
        assert np.array_equal(f64, pc.d2q(qq, pp) / 16.0), c.name
    for r in pc.RADII:
        assert np.float32(r) * np.float32(r) == np.float32(pc.r2q(r) / 16.0) and np.float64(np.float32(r)) ** 2 == pc.r2q(r) / 16.0
    assert 1.0 / 16.0 > 1e-5                                      # `d2 <= 1e-5` is `d2 == 0` on these coordinates


# ---- the references against oracle/pointops.py ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.KNN_CASES)
def test_knn_reference_equals_the_oracle(name):
    c = pc.knn_case(name)
    idx, d2 = pc.knn_expected(name)
    for k in (1, 25, 128) if len(c.xyz) < 1000 else (25,):        # the oracle sorts every segment once per query and k
        oi, od = opo.knn_query(k, c.xyz, c.offset, c.new_xyz, c.new_offset)
        assert np.array_equal(idx[:, :k], oi) and np.array_equal(d2[:, :k], od), (name, k)


@pytest.mark.parametrize("name,shell,ns", [("half8", (1.5, 0.5), 16), ("half8", (2.5, 2.0), 65), ("half8_b3", (2.0, 1.0), 1),
                                           ("half8_b3", (2.5, 0.0), 64), ("count65", (2.5, 0.0), 64), ("count2049", (2.5, 0.5), 64)] +
                         [("count%d" % n, (2.5, 0.0), 65) for n in pc.BALL_COUNTS])
def test_ball_references_equal_the_oracle(name, shell, ns):
    c = pc.ball_case(name)
    idx, d2, _ = pc.ball_expected(name, ns, *shell)
    oi, od = opo.ball_query(ns, shell[0], shell[1], c.xyz, c.offset, c.new_xyz, c.new_offset)
    assert np.array_equal(idx, oi) and np.array_equal(d2, od)
    order = pc.ball_order(c)
    idx, d2, _ = pc.random_ball_ref(ns, shell[0], shell[1], order, c.xyz, c.offset, c.new_xyz, c.new_offset)
    oi, od = opo.random_ball_query(ns, shell[0], shell[1], order, c.xyz, c.offset, c.new_xyz, c.new_offset)
    assert np.array_equal(idx, oi) and np.array_equal(d2, od)


@pytest.mark.parametrize("name", pc.FPS_CASES)
def test_fps_reference_equals_the_oracle(name):
    c = pc.fps_case(name)
    assert np.array_equal(pc.fps_ref(c.xyz, c.offset, c.new_offset), opo.farthest_point_sampling(c.xyz, c.offset, c.new_offset))


@pytest.mark.parametrize("name", pc.BQ_CASES)
def test_pointgroup_references_equal_the_oracle(name):
    c = pc.bq_case(name)
    idx, start_len, _ = pc.bq_expected(name)
    oi, osl = opo.ballquery_batch_p(c.xyz, c.batch_idxs, c.batch_offsets, c.radius)
    assert np.array_equal(idx, oi) and np.array_equal(start_len, osl)
    if name != "capped":         # symmetric neighbour lists: components = what the oracle's sweep finds
        ci, co = opo.bfs_cluster(c.labels, idx, start_len, 3)
        ref = pc.clusters_ref(c.labels, idx, start_len, 3)
        got = pc.clusters_of(ci, co)
        assert len(ref) == len(got) and all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_vote_reference_equals_a_bincount_restatement():
    for k, m, ig in ((25, 1000, -1), (64, 9, 255), (1, 7, -1)):
        nn, labels, ig, C = pc.vote_case(k, m, ig)
        ref = pc.vote_ref(nn, labels, ig, C)
        for i in range(m):
            lab = [int(labels[j]) for j in nn[i] if j >= 0]
            lab = [v for v in lab if v != ig and 0 <= v < C]
            want = int(np.argmax(np.bincount(lab, minlength=C))) if lab else ig
            assert ref[i] == want


# ---- every case reaches what it is named for --------------------------------------------------------------------------------------
def test_knn_cases_have_ties_across_the_kth_place():
    for name, ks in (("lat8", (5, 7, 8, 9, 25, 32, 33, 64)), ("lat16", (7, 25, 64)), ("sheet64", (5, 9, 32, 33)), ("dup3", (1, 2, 4, 5, 25)),
                     ("outside", (1, 5, 7, 25, 64)), ("sparse", (1, 5, 9, 25)), ("crowded_cells", (5, 7, 25, 64)),
                     ("lat8_empty_mid", (5, 25)), ("lat16_4095", (25,))):
        for k in ks:
            assert pc.tie_straddles(name, k) > 0, (name, k)
    assert pc.tie_straddles("dup3", 3) == 0                        # k at the multiplicity: the three coincident points, no choice
    idx, _ = pc.knn_expected("dup3")
    c = pc.knn_case("dup3")
    assert (pc.quarters(c.xyz)[idx[:, :3]] == pc.quarters(c.xyz)[:, None, :]).all()


def test_knn_cases_batches_and_padding():
    c = pc.knn_case("lat8_empty_mid")
    assert c.offset.tolist() == [512, 512, 576]
    idx, d2 = pc.knn_expected("lat8_empty_mid")
    assert (idx[512:, 64:] == -1).all() and (idx[512:, :64] >= 512).all() and (d2[512:, 64:] == np.float32(1e10)).all()
    assert (idx[:512] < 512).all() and (idx[:512] >= 0).all()
    c = pc.knn_case("lat8_one")
    assert c.offset.tolist() == [512, 513]
    idx, _ = pc.knn_expected("lat8_one")
    assert idx[512].tolist() == [512] + [-1] * 127
    assert len(pc.knn_case("lat16").xyz) == 4096 and len(pc.knn_case("lat16_4095").xyz) == 4095
    for name in pc.KNN_CASES:                                       # shuffled: index order is not cell order
        pj = pc.quarters(pc.knn_case(name).xyz)
        key = (pj[:, 0] * 4096 + pj[:, 1]) * 4096 + pj[:, 2]
        assert (np.diff(key) < 0).any(), name


def _cells(c, cell, what=None):
    pj = pc.quarters(c.xyz)
    w = pj if what is None else what
    return (w - pj.min(0)) // int(cell * pc.Q)


def test_knn_grid_geometry_is_reached():
    for name in ("lat8", "sheet64", "lat16"):       # integer lattice: every point on a cell face at cell 1, 7 in 8 of them at cell 2
        pj = pc.quarters(pc.knn_case(name).xyz)
        on_face = lambda cell: (((pj - pj.min(0)) % int(cell * pc.Q)) == 0).any(1)      # noqa: E731
        assert on_face(1.0).all() and on_face(2.0).mean() >= 0.875
    c = pc.knn_case("outside")
    pj, qj = pc.quarters(c.xyz), pc.quarters(c.new_xyz)
    for axis in range(3):
        assert (qj[:, axis] < pj[:, axis].min()).any() and (qj[:, axis] > pj[:, axis].max()).any()
    assert ((qj % (pc.Q // 2)) == 0).all() and ((qj[:, 0] % pc.Q) == 0).sum() > 60      # lattice (or half-lattice) multiples
    for cell in (1.0, 2.0):                                         # first ring that touches the data's box is beyond ring 0
        qc, top = _cells(c, cell, qj), _cells(c, cell).max(0)
        r0 = np.maximum(np.maximum(-qc, qc - top), 0).max(1)
        assert (r0 > 0).sum() >= 50 and r0.max() >= 6
    c = pc.knn_case("sparse")
    for cell in (1.0, 2.0):
        cc = _cells(c, cell)
        ring = np.abs(cc[:, None, :] - cc[None, :, :]).max(-1)
        within = (ring <= pc.KG_RING_MAX).sum(1)
        for k in (5, 9, 25, 64):                                    # fewer than k points within the probed rings: the wave-wide scan
            scanned = np.nonzero(within < k)[0]
            assert len(scanned) >= 2, (cell, k)
            if k <= 25:                                             # ... and it meets tied candidates across the k-th place
                idx, d2 = pc.knn_expected("sparse")
                assert (d2[scanned, k - 1] == d2[scanned, k]).any()
    c = pc.knn_case("crowded_cells")
    cc = _cells(c, 2.0)
    _, counts = np.unique((cc[:, 0] * 100 + cc[:, 1]) * 100 + cc[:, 2], return_counts=True)
    assert sorted(counts.tolist()) == [63, 64, 65, 129]


def test_ball_cases_reach_shells_caps_and_counts():
    c = pc.ball_case("half8")
    D = pc.d2q(pc.quarters(c.xyz), pc.quarters(c.xyz))
    for mx, mn in pc.BALL_SHELLS:
        assert (D == pc.r2q(mx)).any()                              # points exactly ON the outer shell (excluded) ...
        _, _, count = pc.ball_expected("half8", 16, mx, mn)
        inside = ((D == 0) | ((D >= pc.r2q(mn)) & (D < pc.r2q(mx)))).sum(1)
        assert np.array_equal(count, inside)
        if mn > 0:
            assert (D == pc.r2q(mn)).any()                          # ... and on the inner one (included); the query itself passes
            assert (count >= 2).all()                               # by d2 <= 1e-5 although min_radius > 0
    _, _, count = pc.ball_expected("half8", 16, 2.5, 0.0)
    assert (count > 65).any()
    _, _, count = pc.ball_expected("half8", 16, 1.0, 0.0)
    assert (count <= 16).any() and (count > 1).all()
    for n in pc.BALL_COUNTS:
        name = "count%d" % n
        c = pc.ball_case(name)
        idx, d2, count = pc.ball_expected(name, 65, 2.5, 0.0)
        assert count[0] == n and len(c.xyz) <= 4096
        Dq = pc.d2q(pc.quarters(c.new_xyz)[:1], pc.quarters(c.xyz))[0]
        assert (Dq == 100).sum() == 6 and (Dq > 100).sum() == 120 and (Dq == 0).sum() <= 1
        if n == 2049:                                               # overflow: the first 2048 in index order, not the nearest 2048
            kept = np.nonzero(Dq < 100)[0][:pc.BALL_CAP]
            dropped = np.nonzero(Dq < 100)[0][pc.BALL_CAP:]
            assert len(dropped) == 1 and Dq[dropped[0]] < Dq[kept].max()
    c = pc.ball_case("half8_b3")
    assert c.offset.tolist() == [512, 512, 637] and c.new_offset.tolist() == [40, 40, 65]


def test_random_ball_cases_cut_and_pad():
    c = pc.ball_case("half8")
    order = pc.ball_order(c)
    assert sorted(order.tolist()) == list(range(512)) and (np.diff(order) < 0).any()
    _, _, hits = pc.random_ball_ref(16, 2.5, 0.5, order, c.xyz, c.offset)
    assert (hits > 16).all()
    _, _, hits = pc.random_ball_ref(64, 1.0, 0.0, order, c.xyz, c.offset)
    assert (hits < 64).all()


def test_fps_and_pointgroup_cases_reach_their_sizes():
    c = pc.fps_case("strides")
    assert np.diff(np.concatenate([[0], c.offset])).tolist() == [1, 1023, 1024, 1025, 50, 64]
    assert len(np.unique(pc.quarters(c.xyz)[3073:3123], axis=0)) == 1                  # the all-duplicate segment
    assert np.diff(np.concatenate([[0], c.new_offset])).tolist() == [1, 40, 40, 40, 10, 64]     # the last segment is taken whole
    out = pc.fps_ref(c.xyz, c.offset, c.new_offset)
    assert (out[121:131] == 3073).all() and sorted(out[131:].tolist()) == list(range(3123, 3187))
    c = pc.fps_case("long")
    assert np.diff(np.concatenate([[0], c.offset])).tolist() == [2049, 7, 100]
    assert np.diff(np.concatenate([[0], c.new_offset])).tolist() == [30, 0, 100]
    # lattice ties: some arg-max is attained more than once, so "lowest index" decides
    pj = pc.quarters(c.xyz)[:2049]
    ties = 0
    chosen = pc.fps_ref(c.xyz, c.offset, c.new_offset)[:30]
    running = np.full(2049, np.iinfo(np.int64).max)
    for j in chosen[:-1]:
        running = np.minimum(running, ((pj - pj[j]) ** 2).sum(1))
        ties += int((running == running.max()).sum() > 1)
    assert ties > 0
    for n in pc.BQ_SIZES:
        c = pc.bq_case("n%d" % n)
        assert len(c.xyz) == n
        idx, start_len, full = pc.bq_expected("n%d" % n)
        assert full.max(initial=0) <= pc.PG_CAP and (n == 1 or len(idx) > n)           # meanActive = 1 makes the buffer regrow
        if n > 1:
            D = pc.d2q(pc.quarters(c.xyz)[:200], pc.quarters(c.xyz))
            assert (D == pc.r2q(c.radius)).any()                                     # pairs exactly on the shell: strict <
    idx, start_len, full = pc.bq_expected("capped")
    assert (full[:1100] == 1100).all() and (start_len[:1100, 1] == pc.PG_CAP).all() and len(idx) > len(full)


def test_vote_cases_hold_every_row_kind():
    for ig in (-1, 255):
        nn, labels, ig, C = pc.vote_case(32, 1000, ig)
        ref = pc.vote_ref(nn, labels, ig, C)
        assert (ref[1::5] == ig).all() and (ref[2::5] == ig).all()          # rows with no valid neighbour
        assert (ref[3::5] == 0).all()                                       # exact tie between class 0 and the highest class
        assert (ref[4::5] == labels[(nn[4::5, -1])]).all() and (ref[4::5] == C - 1).all()
        assert (labels == ig).any() and (labels < 0).any() and (labels >= C).any() and (nn == -1).any()
    nn, labels, ig, C = pc.vote_case(25, 9, -1, num_classes=1)
    assert C == 1 and set(pc.vote_ref(nn, labels, ig, C).tolist()) <= {0, -1}


def test_voting_cases_sit_on_the_dispatch_threshold():
    for n_valid in (4095, 4096):
        v = pc.voting_case(n_valid)
        assert int(v.valid.sum()) == n_valid and len(v.xyz) == 4096
        assert (v.expected == -1).sum() < 50 and len(np.unique(v.expected)) > 10


# ---- the former admission rule would not pass -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1.0, 2.0])
def test_strict_admission_in_cell_order_disagrees_on_the_tie_cases(cell):
    c = pc.knn_case("lat8")
    idx, _ = pc.knn_expected("lat8")
    wrong = {k: int((pc.grid_strict_emulation(k, c.xyz, c.offset, cell) != idx[:, :k]).any(1).sum()) for k in (1, 5, 25)}
    print("queries differing from the reference under strict admission, cell %.1f: %s" % (cell, wrong))
    assert wrong[1] == 0                      # the nearest point of a self query is the query itself: no tie
    assert wrong[5] > 0 and wrong[25] > 0
