"""GPU: `pc_coord` / `pc_segment` (the point cloud some lists carry beside the Gaussians) through the device transforms, against
OUTPUTS OF THE REFERENCE'S OWN transforms on a sample that carries a cloud (tests/golden/augment_pc.npz, written by
tests/golden/make_golden_pc.py with the seeds -- so the draws -- of augment.npz / augment_b.npz).

  rigid ops       the cloud within 2^-20 max(|x| |A_pc|^T + |b_pc|) of the recorded one (the bound tests/test_hip_augment.py applies
                  to `coord`; its helpers are imported, so the Gaussians are held to exactly the checks made there)
  GridSample      the rows kept of the cloud are the reference's, as a set (rows come out in ascending cell order here, in the
                  order of the FNV hashes there); the pick kernel against a numpy loop, exactly
  sampled_index   idx_unique / sampled_index / grid_coord equal the recorded ones exactly, with the per-voxel pick replayed
  end to end      a shipped `val` list and a shipped `test` list with its post-transform list, into ZeroShotSemSegTester
"""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_augment as A  # noqa: E402

pytestmark = pytest.mark.gpu

_np, _cuda, _affine_bound = A._np, A._cuda, A._affine_bound
KEYS = ("coord", "color", "opacity", "quat", "scale", "segment", "lang_feat", "valid_feat_mask")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return {**np.load(os.path.join(golden_dir, "augment.npz")), **np.load(os.path.join(golden_dir, "augment_b.npz")),
            **np.load(os.path.join(golden_dir, "augment_pc.npz"))}


@pytest.fixture(scope="module")
def base(fx):
    d = A._fixture(int(fx["n"]), int(fx["seed"]))
    d.update(pc_coord=fx["pc_coord"], pc_segment=fx["pc_segment"])
    return d


@pytest.fixture(scope="module")
def lists(golden_dir):
    with open(os.path.join(golden_dir, "pc_configs.txt")) as f:
        return ast.literal_eval(f.read())


def _box(pts):
    return lambda A_, b: np.concatenate([(pts[0] @ A_.T + b).min(0), (pts[0] @ A_.T + b).max(0)])


def _host_state(op, params, coord):
    """what the op folds for a dict with a cloud: the fp64 host composition with a numpy bounding box of the Gaussians"""
    from scenesplat_amd.pointcept_api import transform as tf
    st = tf.RigidState(bbox_fn=_box([coord.astype(np.float64)]))
    op.fold(st, dict(coord=None, pc_coord=None), params)
    return st


# ---- the rigid family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.RIGID_CASES))
def test_each_rigid_op_with_a_cloud_matches_the_reference(fx, base, tag):
    from scenesplat_amd.pointcept_api import TRANSFORMS
    cfg, mk = A.RIGID_CASES[tag]
    op, params = TRANSFORMS.build(cfg), mk(fx)
    st = _host_state(op, params, base["coord"])
    Ag, bg, L = A._host_affine(op, params, base["coord"])
    assert np.array_equal(st.A, Ag) and np.array_equal(st.b, bg)                  # the cloud changes nothing for the Gaussians' affine
    data = _cuda(base)
    out = op.apply(data, params)
    assert out is data
    pc = _np(out["pc_coord"])
    if tag in ("sh", "jit"):                                                      # RandomShift / RandomJitter: the cloud stays behind
        assert not st.pc_pending() and np.array_equal(pc, base["pc_coord"])
    else:
        assert st.pc_pending()
        err = np.abs(pc.astype(np.float64) - fx[tag + "_pc"]).max()
        assert err <= _affine_bound(st.A_pc, st.b_pc, base["pc_coord"]), (tag, err)
        assert np.abs(fx[tag + "_pc"] - base["pc_coord"]).max() > 1e-3
    assert np.array_equal(_np(out["pc_segment"]), base["pc_segment"])
    # the Gaussians: exactly the checks of test_hip_augment.test_each_rigid_op_matches_the_reference
    touched = set()
    for key, bound in (("coord", _affine_bound(Ag, bg, base["coord"])), ("normal", _affine_bound(L, np.zeros(3), base["normal"]))):
        if tag + "_" + key in fx:
            touched.add(key)
            assert np.abs(_np(out[key]).astype(np.float64) - fx[tag + "_" + key]).max() <= bound, (tag, key)
    if tag + "_quat" in fx:
        touched.add("quat")
        A._assert_quat(_np(out["quat"]), fx[tag + "_quat"].astype(np.float64), flipped=tag.startswith("f"))
    if tag + "_scale" in fx:
        touched.add("scale")
        assert A._ulps(_np(out["scale"]), fx[tag + "_scale"]) <= 1
    for key in ("coord", "quat", "scale", "normal", "color", "opacity"):
        if key in touched:
            continue
        want = base[key]
        if tag in ("fx", "fy") and key in ("coord", "normal"):
            want = want * np.array([-1 if tag == "fx" else 1, -1 if tag == "fy" else 1, 1], dtype=np.float32)
        assert np.array_equal(_np(out[key]), want), (tag, key)


@pytest.mark.parametrize("fuse", [True, False])
def test_head_of_the_shipped_list_carries_the_cloud(fx, fuse):
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import Compose, transform as tf
    cfg, params, sample = A._seq(fx)
    cfg, params = cfg[:8], params[:8]                                             # ... RandomJitter: the recorded checkpoint
    sample.update(pc_coord=fx["pc_coord"], pc_segment=fx["pc_segment"])
    comp = Compose(cfg, fuse=fuse)
    calls = []
    orig = nv.aug_gaussians_
    nv.aug_gaussians_ = lambda *a, **k: (calls.append(k.get("coord")), orig(*a, **k))[1]
    try:
        out = comp(_cuda(sample), params=params)
    finally:
        nv.aug_gaussians_ = orig
    # fused: CenterShift | dropout | three rotations + scale + flip + jitter, each flush with a pass over the cloud.  Op by op: the
    # seven of the Gaussians plus CenterShift, three rotations, scale and flip on the cloud (RandomJitter does not touch it).
    assert len(calls) == (4 if fuse else 13)
    on_cloud = sum(c is not None and c.data_ptr() == out["pc_coord"].data_ptr() for c in calls)
    assert on_cloud == (2 if fuse else 6)
    # the composed affines: the rotations about the box centre see the Gaussians RandomDropout kept
    x = sample["coord"].astype(np.float64)
    pts = [x]
    st = tf.RigidState(bbox_fn=_box(pts))
    for i, (op, p) in enumerate(zip(comp.transforms, params)):
        if op.family == "rigid" and "noise" not in p:
            op.fold(st, dict(coord=None, pc_coord=None), p)
        if i == 1:
            pts[0] = x[fx["seq_idx"]]
    assert st.flip == 3 and st.q is not None and st.pc_pending()
    err = np.abs(_np(out["pc_coord"]).astype(np.float64) - fx["seq_pc"]).max()
    assert err <= _affine_bound(st.A_pc, st.b_pc, sample["pc_coord"]), err
    assert np.array_equal(_np(out["pc_segment"]), sample["pc_segment"]) and out["pc_coord"].shape == (len(fx["pc_coord"]), 3)
    # the Gaussians as in test_hip_augment.test_head_of_the_shipped_list_matches_the_reference
    idx = fx["seq_idx"]
    assert np.abs(_np(out["coord"]) - fx["seq_coord"]).max() <= _affine_bound(st.A, st.b, sample["coord"])
    assert np.abs(_np(out["normal"]) - fx["seq_normal"]).max() <= _affine_bound(st.L, np.zeros(3), sample["normal"])
    A._assert_quat(_np(out["quat"]), fx["seq_quat"])
    assert A._ulps(_np(out["scale"]), fx["seq_scale_out"]) <= 1
    for k in ("segment", "lang_feat", "opacity", "valid_feat_mask", "color"):
        assert np.array_equal(_np(out[k]), sample[k][idx]), k


# ---- grid_sample_pc and the pick kernel -------------------------------------------------------------------------------------------
def _pick_loop(order, idx_ptr, label, ignore):
    """the reference's loop (transform.py:1245-1253) over a CSR"""
    out = np.empty(len(idx_ptr) - 1, np.int64)
    for c in range(len(out)):
        cell = order[idx_ptr[c]:idx_ptr[c + 1]]
        valid = cell[label[cell] != ignore] if label is not None else cell[:0]
        out[c] = valid[0] if len(valid) else cell[0]
    return out


def _cells(pc, grid):
    """fp64 cell of every point; the tests use grids that are powers of two, for which the fp32 quotient is exact"""
    return np.floor(pc.astype(np.float64) / grid).astype(np.int64)


def _chosen_ref(pc, grid, seg):
    """one row per occupied cell, in ascending cell order: lowest labelled row, else lowest row"""
    cells = _cells(pc, grid)
    cells -= cells.min(0)
    key = (cells[:, 0] << 42) | (cells[:, 1] << 21) | cells[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.nonzero(np.concatenate(([True], ks[1:] != ks[:-1])))[0]
    return _pick_loop(order, np.concatenate([start, [len(order)]]), seg, -1)


@pytest.mark.parametrize("with_seg", [True, False])
def test_grid_sample_pc_keeps_the_rows_the_reference_keeps(fx, with_seg):
    from scenesplat_amd import gpu_transforms as gt
    pc, seg, grid = fx["pc_coord"], fx["pc_segment"], float(fx["gp_grid"])
    chosen = gt.grid_sample_pc(torch.from_numpy(pc).cuda(), grid, torch.from_numpy(seg).cuda() if with_seg else None)
    assert chosen.dtype == torch.int64 and chosen.is_cuda
    got = _np(chosen)
    want = fx["gp_chosen" if with_seg else "gp_chosen_noseg"]
    assert np.array_equal(np.sort(got), np.sort(want))
    assert np.array_equal(got, _chosen_ref(pc, grid, seg if with_seg else None))             # ... in ascending cell order
    again = gt.grid_sample_pc(torch.from_numpy(pc).cuda(), grid, torch.from_numpy(seg).cuda() if with_seg else None)
    assert torch.equal(chosen, again)
    # the planted cells
    cells = _cells(pc, grid)
    rows = lambda cell: np.nonzero((cells == np.asarray(cell)).all(1))[0]
    by_cell = {tuple(cells[r]): r for r in got}
    all_ignored, late, lng = (rows(c) for c in fx["gp_plant_cells"])
    assert len(all_ignored) >= 3 and (seg[all_ignored] == -1).all()
    assert len(late) >= 3 and seg[late[0]] == -1 and seg[late[-1]] != -1 and (seg[late[:-1]] == -1).all()
    assert len(lng) >= 100 and (seg[lng[:70]] == -1).all() and seg[lng[70]] != -1            # a walk longer than a wave
    assert by_cell[tuple(fx["gp_plant_cells"][0])] == all_ignored[0]                          # no labelled member: the lowest row
    assert by_cell[tuple(fx["gp_plant_cells"][1])] == (late[-1] if with_seg else late[0])
    assert by_cell[tuple(fx["gp_plant_cells"][2])] == (lng[70] if with_seg else lng[0])
    _, inv, cnt = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    single = np.nonzero(cnt[inv.reshape(-1)] == 1)[0]
    assert len(single) >= 50 and np.isin(single, got).all()                                   # single-member cells keep their member


@pytest.mark.parametrize("m", [1, 64, 65])
def test_grid_sample_pc_small_clouds(m):
    from scenesplat_amd import gpu_transforms as gt
    g = np.random.default_rng(m)
    pc = (g.random((m, 3)) * [1.0, 0.75, 0.5] - 0.25).astype(np.float32)           # negative cells too; about two points per cell
    seg = g.integers(-1, 2, m).astype(np.int64)
    for s in (seg, None):
        got = _np(gt.grid_sample_pc(torch.from_numpy(pc).cuda(), 0.25, None if s is None else torch.from_numpy(s).cuda()))
        assert np.array_equal(got, _chosen_ref(pc, 0.25, s)), (m, s is None)


def test_grid_sample_pc_one_long_cell_empty_cloud_and_refusals():
    from scenesplat_amd import gpu_transforms as gt, native as nv
    g = np.random.default_rng(0)
    pc = (0.5 + 0.2 * g.random((3000, 3))).astype(np.float32)                      # one cell of 3000 members
    seg = np.full(3000, -1, np.int64)
    seg[-1] = 3                                                                    # only the last one labelled: the whole walk
    t = torch.from_numpy(pc).cuda()
    assert _np(gt.grid_sample_pc(t, 1.0, torch.from_numpy(seg).cuda())).tolist() == [2999]
    assert _np(gt.grid_sample_pc(t, 1.0, torch.from_numpy(np.full(3000, -1, np.int64)).cuda())).tolist() == [0]
    assert _np(gt.grid_sample_pc(t, 1.0)).tolist() == [0]
    assert _np(gt.grid_sample_pc(t, 1.0, torch.from_numpy(seg).cuda(), ignore_index=3)).tolist() == [0]
    assert _np(gt.grid_sample_pc(t, 1.0, torch.from_numpy(seg).int().cuda())).tolist() == [2999]           # int32 labels are widened
    # an empty cloud: an empty index, and nothing is launched
    launched = []
    saved = nv.argsort_i64, nv.pool_partition, nv.voxel_pick_labelled
    nv.argsort_i64 = nv.pool_partition = nv.voxel_pick_labelled = lambda *a, **k: launched.append(1)
    try:
        out = gt.grid_sample_pc(torch.empty((0, 3), device="cuda"), 0.25, torch.empty(0, dtype=torch.int64, device="cuda"))
    finally:
        nv.argsort_i64, nv.pool_partition, nv.voxel_pick_labelled = saved
    assert out.shape == (0,) and out.dtype == torch.int64 and out.is_cuda and not launched
    assert nv.voxel_pick_labelled(torch.empty(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), 0).shape == (0,)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gt.grid_sample_pc(torch.from_numpy(pc), 1.0)
    with pytest.raises(ValueError, match="rows"):
        gt.grid_sample_pc(t, 1.0, torch.from_numpy(seg[:-1]).cuda())
    with pytest.raises(ValueError, match="21 bits"):
        gt.grid_sample_pc(t, 1e-8)


@pytest.mark.parametrize("ignore", [-1, 255])
def test_voxel_pick_kernel_equals_the_loop(ignore):
    from scenesplat_amd import native as nv
    g = np.random.default_rng(7 + ignore)
    runs = [1, 63, 64, 65, 1000, 1, 64, 65, 2]
    m = sum(runs)
    order = g.permutation(m).astype(np.int32)                                      # any CSR: members need not ascend
    idx_ptr = np.concatenate([[0], np.cumsum(runs)]).astype(np.int32)
    label = np.where(g.random(m) < 0.97, ignore, g.integers(0, 6, m)).astype(np.int64)       # mostly ignored: long walks
    label[order[idx_ptr[5]:idx_ptr[8]]] = ignore                                   # runs of 1, 64, 65 without a labelled member
    label[order[idx_ptr[4 + 1] - 1]] = 2
    label[order[idx_ptr[4]:idx_ptr[4 + 1] - 1]] = ignore                           # the run of 1000: only its last member labelled
    label[order[idx_ptr[1]]] = 1                                                   # the run of 63: its first
    o, p, lab = (torch.from_numpy(v).cuda() for v in (order, idx_ptr, label))
    pad = torch.cat([p, torch.full((7,), -12345, dtype=torch.int32, device="cuda")])          # capacity beyond n_cells + 1 is not read
    for lb, lbn in ((lab, label), (None, None)):
        got = nv.voxel_pick_labelled(o, pad, len(runs), lb, ignore)
        assert got.dtype == torch.int32 and got.shape == (len(runs),)
        assert np.array_equal(_np(got), _pick_loop(order, idx_ptr, lbn, ignore))
    first = nv.voxel_pick_labelled(o, p, 3, lab, ignore)                           # fewer cells than the CSR holds
    assert np.array_equal(_np(first), _pick_loop(order, idx_ptr[:4], label, ignore))
    want = _pick_loop(order, idx_ptr, label, ignore)
    assert want[4] == order[idx_ptr[5] - 1] and want[1] == order[idx_ptr[1]] and want[6] == order[idx_ptr[6]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.voxel_pick_labelled(torch.from_numpy(order), p, len(runs))
    with pytest.raises(RuntimeError, match="idx_ptr"):
        nv.voxel_pick_labelled(o, p, len(runs) + 1)
    with pytest.raises(RuntimeError, match="label"):
        nv.voxel_pick_labelled(o, p, len(runs), lab[:-1])


# ---- GridSample -------------------------------------------------------------------------------------------------------------------
def test_grid_sample_subsets_the_cloud(fx, base):
    from scenesplat_amd import gpu_transforms as gt
    from scenesplat_amd.pointcept_api import TRANSFORMS
    grid = float(fx["gp_grid"])
    op = TRANSFORMS.build(dict(type="GridSample", grid_size=grid, hash_type="fnv", mode="train", keys=KEYS, return_grid_coord=True))
    assert op.apply_to_pc is True
    data = _cuda(base)
    chosen = _np(gt.grid_sample_pc(data["pc_coord"], grid, data["pc_segment"]))
    out = op.apply(data, dict(seed=5))
    assert np.array_equal(_np(out["pc_coord"]), base["pc_coord"][chosen])
    assert np.array_equal(_np(out["pc_segment"]), base["pc_segment"][chosen])
    assert np.array_equal(np.sort(chosen), np.sort(fx["gp_chosen"]))
    plain = op.apply(_cuda({k: v for k, v in base.items() if not k.startswith("pc_")}), dict(seed=5))
    for k in KEYS + ("grid_coord",):                                               # the cloud changes nothing for the Gaussians
        assert torch.equal(out[k], plain[k]), k
    # without pc_segment: the lowest row of every cell
    d = _cuda(base)
    del d["pc_segment"]
    out = op.apply(d, dict(seed=5))
    assert "pc_segment" not in out and np.array_equal(np.sort(_np(gt.grid_sample_pc(_cuda(base)["pc_coord"], grid))), np.sort(fx["gp_chosen_noseg"]))
    assert out["pc_coord"].shape[0] == len(fx["gp_chosen_noseg"])
    # apply_to_pc=False: both keys pass through untouched
    off = TRANSFORMS.build(dict(type="GridSample", grid_size=grid, keys=KEYS, apply_to_pc=False))
    d = _cuda(base)
    pc_t, seg_t = d["pc_coord"], d["pc_segment"]
    out = off.apply(d, dict(seed=5))
    assert out["pc_coord"] is pc_t and out["pc_segment"] is seg_t
    assert np.array_equal(_np(pc_t), base["pc_coord"]) and np.array_equal(_np(seg_t), base["pc_segment"])
    assert out["coord"].shape[0] < len(base["coord"])
    # refusals
    d = _cuda(base)
    d["pc_segment"] = d["pc_segment"][:-1]
    with pytest.raises(ValueError, match="rows"):
        op.apply(d, dict(seed=5))
    d = _cuda(base)
    d["pc_coord"] = d["pc_coord"].cpu()
    with pytest.raises(RuntimeError, match="pc_coord.*no CPU fallback"):
        op.apply(d, dict(seed=5))
    d = _cuda(base)
    d["pc_coord"] = d["pc_coord"].double()
    with pytest.raises(RuntimeError, match="pc_coord"):
        op.apply(d, dict(seed=5))


def test_grid_sample_keeps_the_sampled_index_rows(fx, base):
    from scenesplat_amd import gpu_transforms as gt
    from scenesplat_amd.pointcept_api import TRANSFORMS
    grid = float(fx["gsi_grid"])
    op = TRANSFORMS.build(dict(type="GridSample", grid_size=grid, hash_type="fnv", mode="train", keys=KEYS, return_grid_coord=True))
    sample = {k: v for k, v in base.items() if not k.startswith("pc_")}
    si, merged = fx["gsi_sampled_in"], fx["gsi_idx_unique"]
    d = _cuda(sample)
    d["sampled_index"] = torch.from_numpy(si).cuda()
    out = op.apply(d, dict(seed=1, idx=fx["gsi_pick"]))                            # the pick the reference drew, replayed
    assert np.array_equal(_np(out["sampled_index"]), fx["gsi_sampled_out"])
    assert np.array_equal(_np(out["grid_coord"]), fx["gsi_grid_coord"]) and out["grid_coord"].dtype == torch.int32
    for k in KEYS:
        assert np.array_equal(_np(out[k]), sample[k][merged]), k
    r = gt.grid_sample_train(torch.from_numpy(sample["coord"]).cuda(), grid, sampled_index=torch.from_numpy(si).cuda(),
                             idx_unique=torch.from_numpy(fx["gsi_pick"]).cuda())
    assert np.array_equal(_np(r["idx_unique"]), merged) and len(merged) > len(fx["gsi_pick"])
    # with its own draw: every always-kept row survives and sampled_index points at it; one row per voxel otherwise
    d = _cuda(sample)
    d["sampled_index"] = torch.from_numpy(si).cuda()
    out = op.apply(d, dict(seed=9))
    assert np.array_equal(_np(out["coord"])[_np(out["sampled_index"])], sample["coord"][si])
    gc = _np(out["grid_coord"])
    n_vox = len(np.unique(gc, axis=0))
    assert n_vox == len(fx["gsi_pick"]) and n_vox <= len(gc) <= n_vox + len(si)
    # without sampled_index nothing changes: the replayed pick is the result
    out = op.apply(_cuda(sample), dict(seed=1, idx=fx["gsi_pick"]))
    assert "sampled_index" not in out and np.array_equal(_np(out["coord"]), sample["coord"][fx["gsi_pick"]])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
class PadModel:
    """the StubModel of tests/test_hip_tester.py: point_feat.feat = the input feat, zero-padded to the text dimension"""

    def __init__(self, dim):
        self.calls, self.dim = 0, dim

    def eval(self):
        return self

    def __call__(self, input_dict, chunk_size=None):
        assert chunk_size == 600000 and not torch.is_grad_enabled()
        self.calls += 1
        f = input_dict["feat"]
        return dict(point_feat=dict(feat=torch.nn.functional.pad(f, (0, self.dim - f.shape[1]))))


class Loader(list):
    batch_size = 1


def test_shipped_val_list_carries_the_cloud(lists, base):
    from scenesplat_amd.pointcept_api import Compose
    cfg = lists["configs/matterport3d/lang-pretrain-matt-mcmc-wo-normal-contrastive.py::val::transform"]
    assert [c["type"] for c in cfg] == ["CenterShift", "GridSample", "CenterShift", "NormalizeColor", "ToTensor", "Collect"]
    for fuse in (True, False):
        out = Compose(cfg, seed=3, fuse=fuse)(_cuda(base))
        assert set(out) == {"coord", "grid_coord", "segment", "lang_feat", "valid_feat_mask", "pc_coord", "pc_segment", "offset", "feat"}
        m = out["pc_coord"].shape[0]
        assert out["pc_coord"].is_cuda and out["pc_coord"].dtype == torch.float32 and tuple(out["pc_coord"].shape) == (m, 3)
        assert out["pc_segment"].shape == (m,) and out["pc_segment"].dtype == torch.int64
        # 2 cm cells: the 900 scattered points keep a cell each but for a few, the 100 planted in one 25 cm cell share some
        assert 900 <= m <= len(base["pc_coord"])
        # both CenterShifts moved the cloud by the Gaussians' shift: x and y of the Gaussians end up centred, and the cloud, which
        # fills the same box, is centred with them to within its own margin to the box
        pc, c = _np(out["pc_coord"]), _np(out["coord"])
        assert abs(c[:, 0].min() + c[:, 0].max()) < 1e-5 and abs(pc[:, 0].min() + pc[:, 0].max()) < 0.05
        assert abs(pc[:, 1].min() + pc[:, 1].max()) < 0.05 and abs(pc[:, 2].min()) < 0.05
        rows = {r.tobytes() for r in base["pc_segment"].reshape(-1, 1)}
        assert all(r.tobytes() in rows for r in _np(out["pc_segment"]).reshape(-1, 1))


def test_shipped_test_lists_feed_the_tester_with_the_cloud(lists, base, tmp_path):
    from scenesplat_amd import gpu_transforms as gt
    from scenesplat_amd.pointcept_api import TESTERS, Compose, tester as tester_mod
    name = "configs/matterport3d/lang-pretrain-matt-mcmc-wo-normal-contrastive.py::test[0]::"
    cfg, post = lists[name + "transform"], lists[name + "post_transform"]
    gs = next(c for c in cfg if c["type"] == "GridSample")
    assert gs["apply_to_pc"] is False and gs["return_inverse"] is True
    scene = Compose(cfg, seed=4)(_cuda(base))
    # the cloud went through CenterShift with the Gaussians (origin_coord is the copy taken right after it) and was not subsampled
    shift = (_np(scene["origin_coord"]).astype(np.float64) - base["coord"]).mean(0)
    assert np.abs(_np(scene["pc_coord"]) - (base["pc_coord"] + shift)).max() < 1e-5
    assert np.array_equal(_np(scene["pc_segment"]), base["pc_segment"]) and scene["inverse"].shape[0] == len(base["coord"])
    n_sub = scene["coord"].shape[0]
    assert 0 < n_sub <= len(base["coord"]) and scene["origin_coord"].shape[0] == len(base["coord"])      # (1 cm voxels: few are shared)
    # the fragments: GridSample(mode="test") at the config's voxel size, each through the shipped post-transform list
    frag = gt.grid_sample_test(scene["coord"], 0.02)
    post_comp = Compose(post)
    fragment_list = []
    for p in range(frag["index"].shape[0]):
        idx = frag["index"][p]
        part = {k: scene[k][idx] for k in ("coord", "color", "opacity", "quat", "scale", "lang_feat", "valid_feat_mask")}
        part.update(grid_coord=frag["grid_coord"], index=idx, pc_coord=scene["pc_coord"].clone(), pc_segment=scene["pc_segment"])
        out = post_comp(part)
        assert {"coord", "grid_coord", "index", "feat", "offset", "pc_coord", "pc_segment"} <= set(out)
        assert out["pc_coord"].shape == scene["pc_coord"].shape and out["feat"].shape[1] == 11
        fragment_list.append(out)
    classes, dim = 6, 16
    (tmp_path / "labels.txt").write_text("\n".join(f"c{i}" for i in range(classes)) + "\n")
    torch.save(torch.eye(classes, dim) + 0.1, tmp_path / "text.pt")
    d = dict(fragment_list=fragment_list, name="cloud", segment=scene["segment"], coord=scene["coord"], origin_segment=scene["origin_segment"],
             inverse=scene["inverse"], origin_coord=scene["origin_coord"], origin_feat_mask=scene["origin_feat_mask"],
             pc_coord=scene["pc_coord"], pc_segment=scene["pc_segment"])
    tcfg = dict(save_path=str(tmp_path / "out"), data=dict(test=dict(type="Matterport3DGSDataset", split="test")),
                test=dict(type="ZeroShotSemSegTester", class_names=str(tmp_path / "labels.txt"), text_embeddings=str(tmp_path / "text.pt"),
                          enable_voting=True, vote_k=5, confidence_threshold=0.1))
    model = PadModel(dim)
    records = {}
    orig = tester_mod.final_metrics
    tester_mod.final_metrics = lambda rec, keep=None: (records.update(rec), orig(rec, keep))[1]
    try:
        metrics = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=tcfg, model=model, test_loader=Loader([[d]]))).test()
    finally:
        tester_mod.final_metrics = orig
    assert model.calls == len(fragment_list) >= 1
    # the has_pc branch: voted onto the cloud, scored against pc_segment
    saved = np.load(os.path.join(tcfg["save_path"], "result_Matterport3DGSDataset", "cloud_pred.npy"))
    assert saved.shape == (len(base["pc_coord"]),)
    labelled = int((base["pc_segment"] != -1).sum())
    assert 0 < labelled < len(base["pc_segment"])
    assert int(np.sum(records["cloud"]["target"])) == labelled
    assert 0.0 <= metrics["allAcc"] <= 1.0 and np.isfinite(metrics["mIoU"])
