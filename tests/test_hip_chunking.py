"""GPU: scene chunking (scenesplat_amd/pointcept_api/preprocessing.py over csrc/chunking.hip).

1. chunk_scene against the files the reference's chunking_scene wrote (tests/golden/chunking.npz): directories, file lists, and
   dtype, shape and bytes of every asset, on every deterministic case.
2. row-count edges (1, 255, 256, 257 rows and 6,000: past one 1,024-row workgroup of the membership kernel) against the numpy
   restatement of tests/chunking_cases.py; the running sum of the counts past its 256-wide tile; the membership kernel past the
   2,048 chunks its LDS histogram holds.
3. the grouped gather: every row width of the scene assets in one launch, an unaligned base, a zero-row problem, the pick composition.
4. lang_feat normalisation against fp64 rounded once.
5. the random pick: invariants and uniformity.  6. determinism.  7. round trip into a shipped dataset dict."""
import ast
import functools
import os

import numpy as np
import pytest
import torch

import chunking_cases as cc
from test_datasets_host import pointed

pytestmark = pytest.mark.gpu
LANG_CFG = "configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py"
GOLD = cc.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_scene(tmp_path, arrays, tag="a", **kw):
    from scenesplat_amd.pointcept_api import chunk_scene
    root, out = str(tmp_path / f"in_{tag}"), str(tmp_path / f"out_{tag}")
    cc.write_scene(root, arrays)
    dirs = chunk_scene(cc.SCENE, root, out, cc.SPLIT, kw.pop("grid_size", None), **kw)
    return dirs, out


# ---- 1. the recorded reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(cc.CASES))
def test_bit_equal_with_the_reference(case, tmp_path):
    kw, gold = cc.case_kwargs(case), GOLD[case]
    dirs, out = run_scene(tmp_path, gold["inputs"], **kw)
    if gold["split_dir"] is None:
        assert dirs == [] and not os.path.exists(out)
        return
    assert os.listdir(out) == [gold["split_dir"]]
    assert dirs == [os.path.join(out, gold["split_dir"], d) for d in gold["chunks"]]
    cc.assert_same_chunks(cc.read_chunks(os.path.join(out, gold["split_dir"])), gold["chunks"])


def test_output_dir_none_writes_beside_the_split(tmp_path):
    from scenesplat_amd.pointcept_api import chunk_scene
    kw, gold = cc.case_kwargs("max_chunk_num"), GOLD["max_chunk_num"]
    root = str(tmp_path)
    cc.write_scene(root, gold["inputs"])
    dirs = chunk_scene(cc.SCENE, root, None, cc.SPLIT, **kw)
    assert dirs == [os.path.join(root, gold["split_dir"], d) for d in gold["chunks"]]
    cc.assert_same_chunks(cc.read_chunks(os.path.join(root, gold["split_dir"])), gold["chunks"])


# ---- 2. row-count edges ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_scene(n):
    arrays = cc.scene(n, 100 + n, mask_grid=None)
    arrays["valid_feat_mask"] = (np.random.default_rng(n).random(n) < 0.6).astype(np.uint8)
    return arrays


@pytest.mark.parametrize("grid_size", [None, 0.05])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 6000])
def test_row_count_edges(n, grid_size, tmp_path):
    # one row has no extent: a stride above the range gives it its single chunk
    kw = dict(chunk_range=(1, 1), chunk_stride=(2, 2)) if n == 1 else dict(chunk_range=(2, 2), chunk_stride=(1, 1))
    kw.update(grid_size=grid_size, chunk_minimum_size=0 if n < 6000 else 300, max_chunk_num=None)
    ref = cc.chunk_reference(edge_scene(n), seed=5, **kw)
    assert ref["chunks"] and sum(len(c["coord"]) for c in ref["chunks"].values()) >= n - (0 if grid_size is None else n // 2)
    dirs, out = run_scene(tmp_path, edge_scene(n), seed=5, **kw)
    assert [os.path.basename(d) for d in dirs] == list(ref["chunks"])
    cc.assert_same_chunks(cc.read_chunks(os.path.join(out, cc.split_dir(cc.SPLIT, grid_size, kw["chunk_range"], kw["chunk_stride"]))), ref["chunks"])


@pytest.mark.parametrize("k", [1, 255, 256, 257, 700])
def test_offsets_past_one_tile(k):
    from scenesplat_amd import native as nv
    counts = np.random.default_rng(k).integers(0, 2 ** 31 - 1, k).astype(np.int32)          # (the sums need int64)
    got = nv.chunk_offsets(dev(counts)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, np.concatenate([[0], np.cumsum(counts.astype(np.int64))]))


@pytest.mark.parametrize("nx,ny", [(64, 32), (64, 40)])       # 2,048 chunks: the LDS histogram; 2,560: global atomics
def test_membership_on_both_counting_paths(nx, ny):
    from scenesplat_amd import native as nv
    rng = np.random.default_rng(nx * ny)
    m, rx, ry, slots = 3000, 2, 3, 6                                                        # stride 1: ceil(2 / 1) * ceil(3 / 1) slots
    rec = (rng.integers(0, [nx * 8, ny * 8, 8], (m, 3)) / 8).astype(np.float32)            # many rows exactly on the integer edges
    xs, ys = np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    keys, counts = nv.chunk_membership(dev(rec), None, dev(np.concatenate([xs, xs + rx, ys, ys + ry])), nx, ny, slots, status)
    order = nv.argsort_i64(keys.view(1, -1), 13, want_inverse=False, want_sorted=False)[0][0]
    offsets = nv.chunk_offsets(counts).cpu().numpy()
    rows = nv.chunk_slot_rows(order, int(offsets[-1]), slots).cpu().numpy()
    assert int(status) == 0
    x, y = rec[:, 0].astype(np.float64), rec[:, 1].astype(np.float64)
    for c in rng.permutation(nx * ny)[:300].tolist() + [0, nx * ny - 1]:
        ox, oy = xs[c // ny], ys[c % ny]
        want = np.nonzero((x >= ox) & (x < ox + rx) & (y >= oy) & (y < oy + ry))[0]
        assert np.array_equal(rows[offsets[c]:offsets[c + 1]], want), c
    in_x = np.minimum(np.floor(x), nx - 1) - np.maximum(np.floor(x) - rx + 1, 0) + 1
    in_y = np.minimum(np.floor(y), ny - 1) - np.maximum(np.floor(y) - ry + 1, 0) + 1
    assert offsets[-1] == int((in_x * in_y).sum())


# ---- 3. the grouped gather ---------------------------------------------------------------------------------------------------------------
def test_gather_row_widths_in_one_launch():
    from scenesplat_amd import native as nv
    rng = np.random.default_rng(3)
    n, m = 777, 1301
    srcs = [rng.integers(0, 2, n).astype(np.uint8), rng.integers(-9, 9, n).astype(np.int16), rng.integers(0, 256, (n, 3)).astype(np.uint8),
            rng.standard_normal((n, 3)).astype(np.float16), rng.standard_normal((n, 3)).astype(np.float32),
            rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((n, 768)).astype(np.float16),
            rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64), rng.random((n, 1), dtype=np.float32),
            rng.standard_normal((n, 768)).astype(np.float16), rng.integers(0, 256, (n, 5)).astype(np.uint8),
            rng.integers(0, 9, (n, 2)).astype(np.int16)]
    row_bytes = [a.nbytes // n for a in srcs]
    assert row_bytes == [1, 2, 3, 6, 12, 16, 1536, 8, 4, 1536, 5, 4]
    idx = rng.integers(0, n, m).astype(np.int32)
    idx[:3] = [0, n - 1, 0]
    counts = [m, m, m, m, m, m, m, 257, m, m, 1, 0]                       # a zero-row problem among them, and another behind it
    arena = torch.zeros(sum(a.nbytes + 512 for a in srcs), dtype=torch.uint8, device="cuda")
    stage = torch.full((sum(c * rb + 512 for c, rb in zip(counts, row_bytes)),), 0xAB, dtype=torch.uint8, device="cuda")
    idx_d = dev(idx)
    desc, where, so, do = [], [], 0, 0
    for j, (a, rb, c) in enumerate(zip(srcs, row_bytes, counts)):
        so = -(-so // 256) * 256 + (1 if j == 9 else 0)                   # problem 9: the 1,536-byte rows from a base that is 1 mod 16
        do = -(-do // 64) * 64
        arena[so:so + a.nbytes] = dev(a.reshape(-1).view(np.uint8))
        desc.append((arena.data_ptr() + so, stage.data_ptr() + do, idx_d.data_ptr(), c, rb, 0, n, n))
        where.append(do)
        so, do = so + a.nbytes, do + c * rb + 64
    desc[10], desc[11] = desc[11], desc[10]                               # (the zero-row problem sits INSIDE the launch)
    assert desc[6][0] % 16 == 0 and desc[9][0] % 16 == 1
    nv.chunk_gather_group(np.asarray(desc, dtype=np.int64), torch.device("cuda", torch.cuda.current_device()))
    got = stage.cpu().numpy()
    for a, rb, c, off in zip(srcs, row_bytes, counts, where):
        want = np.ascontiguousarray(a[idx[:c]]).reshape(-1).view(np.uint8)
        assert np.array_equal(got[off:off + c * rb], want), (a.dtype, a.shape)
        assert (got[off + c * rb:off + c * rb + 16] == 0xAB).all()        # nothing written past a block
    # the composition with a subsample: dst[i] = src[pick[idx[i]]], both word sizes
    pick = rng.permutation(n)[:300].astype(np.int32)
    idx2 = rng.integers(0, 300, m).astype(np.int32)
    pick_d, idx2_d = dev(pick), dev(idx2)
    stage.fill_(0xAB)
    desc2 = [(desc[j][0], stage.data_ptr() + where[j], idx2_d.data_ptr(), m, row_bytes[j], pick_d.data_ptr(), n, 300) for j in (2, 6, 9)]
    nv.chunk_gather_group(np.asarray(desc2, dtype=np.int64), torch.device("cuda", torch.cuda.current_device()))
    got = stage.cpu().numpy()
    for j in (2, 6, 9):
        want = np.ascontiguousarray(srcs[j][pick[idx2]]).reshape(-1).view(np.uint8)
        assert np.array_equal(got[where[j]:where[j] + m * row_bytes[j]], want), j


# ---- 4. lang_feat normalisation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [16, 768, 100])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_lang_normalize(width, dtype):
    from scenesplat_amd import native as nv
    rng = np.random.default_rng(width)
    n = 500 if width == 768 else 1201
    x = (rng.standard_normal((n, width)) * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(dtype)
    valid = (rng.random(n) < 0.7).astype(np.uint8)
    valid[:4] = [1, 0, 1, 0]
    x[2] = 0                                                                # a valid all-zero row: 0 / 0, as numpy
    want = cc.normalize_rows(x, valid)
    got = nv.chunk_lang_normalize_(dev(x), dev(valid)).cpu().numpy()
    assert got.dtype == x.dtype and got[valid == 0].tobytes() == x[valid == 0].tobytes()
    assert np.isnan(got[2]).all() and np.isnan(want[2]).all()
    sel = valid == 1
    sel[2] = False
    g, w = got[sel], want[sel]
    assert np.isfinite(g).all()
    if dtype == np.float16:
        gi, wi = g.view(np.int16).astype(np.int64), w.view(np.int16).astype(np.int64)
        gi, wi = np.where(gi < 0, -(gi & 0x7FFF), gi), np.where(wi < 0, -(wi & 0x7FFF), wi)       # sign-magnitude -> ordered integers
        ulp = np.abs(gi - wi)
        print(f"fp16 width {width}: max {ulp.max()} ulp, {100 * (ulp > 0).mean():.2f} % differ")
        assert ulp.max() <= 1
    else:
        x64 = x[sel].astype(np.float64)
        exact = x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))
        rel = np.abs(g.astype(np.float64) - exact) / np.abs(exact)
        print(f"fp32 width {width}: max relative error {rel.max():.3e}")
        assert rel.max() <= 1e-6


# ---- 5. the random pick ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pick_scene():
    """4,096 cells of a 64 x 64 grid of unit cells with exactly 4 valid rows each, and 0..3 invalid rows; 64 more cells without a
    valid row.  Rows shuffled."""
    rng = np.random.default_rng(9)
    cx, cy = np.meshgrid(np.arange(64), np.arange(65), indexing="ij")
    cells = np.stack([cx.reshape(-1), cy.reshape(-1)], 1)
    reps_valid = np.where(cells[:, 1] < 64, 4, 0)
    reps_invalid = np.where(cells[:, 1] < 64, rng.integers(0, 4, len(cells)), rng.integers(1, 4, len(cells)))
    cell_of = np.concatenate([np.repeat(np.arange(len(cells)), reps_valid), np.repeat(np.arange(len(cells)), reps_invalid)])
    valid = np.concatenate([np.ones(reps_valid.sum(), np.uint8), np.zeros(reps_invalid.sum(), np.uint8)])
    perm = rng.permutation(len(cell_of))
    cell_of, valid = cell_of[perm], valid[perm]
    rec = np.concatenate([cells[cell_of] + rng.random((len(cell_of), 2)) * 0.99, rng.random((len(cell_of), 1)) * 0.99], 1).astype(np.float32)
    return rec, valid, cell_of


def device_pick(seed):
    from scenesplat_amd.pointcept_api.preprocessing import subsample_rows
    rec, valid, _ = pick_scene()
    return subsample_rows(dev(rec), 1.0, rec.max(axis=0), dev(valid), seed).cpu().numpy()


def test_pick_invariants_and_uniformity():
    rec, valid, cell_of = pick_scene()
    pick = device_pick(seed=1)
    n_cells = len(np.unique(cell_of))
    assert n_cells == 64 * 65 and len(pick) == n_cells and len(np.unique(cell_of[pick])) == n_cells       # one row per occupied cell
    first = np.full(cell_of.max() + 1, len(cell_of))
    np.minimum.at(first, cell_of, np.arange(len(cell_of)))
    has_valid = np.zeros(cell_of.max() + 1, bool)
    has_valid[cell_of[valid == 1]] = True
    pc = cell_of[pick]
    assert (valid[pick][has_valid[pc]] == 1).all() and np.array_equal(pick[~has_valid[pc]], first[pc][~has_valid[pc]])
    assert (np.diff(first[pc]) > 0).all()                                                               # ordered by the smallest row
    assert np.array_equal(pick, cc.subsample(rec, 1.0, valid, seed=1))                                  # the documented rule, exactly
    assert np.array_equal(pick, device_pick(seed=1)) and not np.array_equal(pick, device_pick(seed=2))
    # position of the pick among the cell's valid rows (ascending): each of the four in 20-30 % of the 4,096 cells (sigma 0.68 %)
    rows = np.nonzero(valid == 1)[0]
    rank = np.zeros(len(cell_of), np.int64)
    order = rows[np.argsort(cell_of[rows], kind="stable")]
    rank[order] = np.arange(len(order)) % 4
    share = np.bincount(rank[pick[has_valid[pc]]], minlength=4) / 4096
    print("share of the four positions:", share)
    assert has_valid[pc].sum() == 4096 and (share >= 0.20).all() and (share <= 0.30).all()


# ---- 6. determinism, 7. round trip ---------------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bytes(tmp_path):
    arrays = cc.scene(6000, 77, lang=16)
    kw = dict(grid_size=0.05, chunk_range=(2, 2), chunk_stride=(1, 1), chunk_minimum_size=300, max_chunk_num=5, seed=3, staging_bytes=1 << 16)
    dirs_a, out_a = run_scene(tmp_path, arrays, "a", **dict(kw))
    dirs_b, out_b = run_scene(tmp_path, arrays, "b", **dict(kw))
    a, b = cc.read_chunks(os.path.join(out_a, os.listdir(out_a)[0])), cc.read_chunks(os.path.join(out_b, os.listdir(out_b)[0]))
    assert len(dirs_a) == 5 and [os.path.basename(d) for d in dirs_a] == list(a)
    assert sum(v.nbytes for c in a.values() for v in c.values()) > 3 * (1 << 16)                         # several staging batches
    cc.assert_same_chunks(a, b)
    # and what the files hold: the restatement's chunks, lang_feat within one fp16 ulp of it
    ref = cc.chunk_reference(arrays, **{k: v for k, v in kw.items() if k != "staging_bytes"})["chunks"]
    assert list(ref) == list(a)
    for d in ref:
        for k, w in ref[d].items():
            if k != "lang_feat":
                assert a[d][k].dtype == w.dtype and a[d][k].tobytes() == w.tobytes(), (d, k)
            else:
                assert np.abs(a[d][k].astype(np.float64) - w.astype(np.float64)).max() <= 2.0 ** -10      # |values| <= 1: an ulp is <= 2^-11


def test_round_trip_into_a_shipped_dataset(tmp_path, golden_dir):
    from scenesplat_amd.pointcept_api import build_dataset, chunk_split
    with open(os.path.join(golden_dir, "dataset_configs.txt")) as f:
        shipped = ast.literal_eval(f.read())[LANG_CFG]
    root = str(tmp_path)
    for s in range(2):
        arrays = cc.scene(900, 40 + s, lang=48)
        arrays["segment20"] = arrays.pop("segment").astype(np.int64).reshape(-1, 1)
        arrays["quat"] = np.tile(np.float32([1, 0, 0, 0]), (900, 1))
        arrays["scale"] = np.full((900, 3), 0.01, np.float32)
        cc.write_scene(root, arrays, name="scene%04d_00" % s)
    done = chunk_split(root, cc.SPLIT, grid_size=0.01, chunk_range=(2, 2), chunk_stride=(1, 1), chunk_minimum_size=50)
    dirs = [d for v in done.values() for d in v]
    split = "train_grid1.0cm_chunk2x2_stride1x1"
    assert sorted(done) == ["scene0000_00", "scene0001_00"] and len(dirs) >= 12 and all(os.path.dirname(d) == os.path.join(root, split) for d in dirs)
    ds = build_dataset(pointed(shipped["data"]["train"], root, split=split))
    assert len(ds) == len(dirs)
    i = [ds.get_data_name(j) for j in range(len(ds))].index("scene0001_00_3")
    sample = ds.get_data(i)
    want = np.load(os.path.join(root, split, "scene0001_00_3", "coord.npy"))
    assert sample["coord"].is_cuda and np.array_equal(sample["coord"].cpu().numpy(), want) and len(want) >= 50
    assert sample["lang_feat"].shape == (len(want), 48) and sample["segment"].shape == (len(want),)
    ds.stager.close()
