"""Generator of tests/golden/pc_attach.npz: the labelled point cloud of chunk folders against the reference's OWN SceneCache.

    python tests/golden/make_golden_pc_attach.py <path of the reference tree>

A synthetic original scene is written to a temporary folder (coord.npy: 5,000 fp32 points in a 2 x 2 x 2 m box; segment20.npy int16
with some -1; segment_nyu_160.npy int32; instance.npy int32) together with three chunk coord.npy of 700 Gaussian centres each, the third
of which partly leaves the box.  The reference's pointcept/datasets/preprocessing/adding_pc_label_to_gs_chunk.py (imported by path)
loads the scene into its SceneCache, and the file records the inputs and, per chunk, what `slice` and `semseg_label_slice` return.
Only data is written; no reference source.

Keys: `pc/coord`, `pc/segment20`, `pc/segment_nyu_160`, `pc/instance`, `chunk<i>/coord`, `chunk<i>/pc_coord`, `chunk<i>/pc_<segment>`,
`chunk<i>/label_<segment>`, `meta` (JSON: seed, k, dist_limit, kept rows per chunk, share of neighbour distances over the limit).

Asserted here (tests/test_pc_attach_host.py asserts the same with numpy), so that a selection by fp32 distances with the smaller-index
tie rule agrees with cKDTree's selection in fp64; the seed is re-drawn until all hold:
* for every Gaussian the 16th and 17th neighbour distances differ by more than 1e-5 relative (and the 1st and 2nd, for the labels);
* none of the 16 neighbour distances lies within 1e-5 of the limit;
and, so that the comparisons cannot be empty: every chunk keeps rows, more than 5 % of the neighbour distances exceed the limit, and
some Gaussian's nearest point lies beyond it."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
K, LIMIT, MARGIN = 16, 0.25, 1e-5
N_CLOUD, N_CHUNK = 5000, 700
SEGMENTS = ("segment20", "segment_nyu_160")


def reference_module(ref_root):
    path = os.path.join(ref_root, "pointcept", "datasets", "preprocessing", "adding_pc_label_to_gs_chunk.py")
    spec = importlib.util.spec_from_file_location("ref_adding_pc_label_to_gs_chunk", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(seed):
    g = np.random.default_rng(seed)
    scene = dict(coord=(g.random((N_CLOUD, 3)) * 2.0).astype(np.float32),
                 segment20=np.where(g.random(N_CLOUD) < 0.1, -1, g.integers(0, 20, N_CLOUD)).astype(np.int16),
                 segment_nyu_160=g.integers(0, 160, N_CLOUD).astype(np.int32),
                 instance=g.integers(-1, 40, N_CLOUD).astype(np.int32))
    lo = np.array([[0.0, 0.0, 0.0], [0.8, 0.9, 0.0], [1.5, 0.2, 0.3]])
    size = np.array([[1.0, 1.0, 2.0], [1.0, 1.0, 2.0], [1.1, 1.2, 1.5]])       # the third reaches x = 2.6: outside the box
    chunks = [(lo[i] + g.random((N_CHUNK, 3)) * size[i]).astype(np.float32) for i in range(3)]
    return scene, chunks


def margins(cloud, chunk):
    """fp64 distances of every Gaussian to its K + 1 nearest cloud points -> (ok, sorted distances (m, K + 1))"""
    d = np.sqrt(((chunk.astype(np.float64)[:, None, :] - cloud.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    d = np.sort(d, axis=1)[:, :K + 1]
    ok = ((d[:, K] - d[:, K - 1]) > MARGIN * d[:, K]).all() and ((d[:, 1] - d[:, 0]) > MARGIN * d[:, 1]).all() \
        and (np.abs(d[:, :K] - LIMIT) > MARGIN).all()
    return bool(ok), d


def main(ref_root):
    ref = reference_module(ref_root)
    assert ref.K_NEIGHBORS == K
    seed = 20250
    while True:
        scene, chunks = draw(seed)
        checks = [margins(scene["coord"], c) for c in chunks]
        if all(ok for ok, _ in checks):
            break
        print(f"seed {seed}: a margin fails, drawing again")
        seed += 1
    dists = np.concatenate([d[:, :K] for _, d in checks])
    over = float((dists > LIMIT).mean())
    out = {f"pc/{k}": v for k, v in scene.items()}
    kept = []
    with tempfile.TemporaryDirectory() as tmp:
        scene_dir = os.path.join(tmp, "val", "scene_a_00")
        os.makedirs(scene_dir)
        for k, v in scene.items():
            np.save(os.path.join(scene_dir, k + ".npy"), v)
        from pathlib import Path
        cache = ref.SceneCache()
        with contextlib.redirect_stdout(io.StringIO()):
            cache.load(Path(scene_dir))
        assert sorted(cache.segments) == sorted(s + ".npy" for s in SEGMENTS)
        for i, chunk in enumerate(chunks):
            pc_coord, pc_seg = cache.slice(chunk, LIMIT)
            labels = cache.semseg_label_slice(chunk, LIMIT)
            out[f"chunk{i}/coord"] = chunk
            out[f"chunk{i}/pc_coord"] = np.asarray(pc_coord)
            for s in SEGMENTS:
                out[f"chunk{i}/pc_{s}"] = np.asarray(pc_seg[s + ".npy"])
                out[f"chunk{i}/label_{s}"] = np.asarray(labels[s + ".npy"])
                assert out[f"chunk{i}/pc_{s}"].dtype == scene[s].dtype and out[f"chunk{i}/label_{s}"].dtype == scene[s].dtype
            kept.append(int(pc_coord.shape[0]))
            assert pc_coord.dtype == np.float32 and pc_coord.shape[0] > 0
    assert over > 0.05, over
    assert any((out[f"chunk{i}/label_segment_nyu_160"] == -1).any() for i in range(3))
    out["meta"] = np.array(json.dumps(dict(seed=seed, k=K, dist_limit=LIMIT, kept=kept, over_limit=over)))
    path = os.path.join(HERE, "pc_attach.npz")
    np.savez_compressed(path, **out)
    print(f"seed {seed}: kept rows {kept}, {over:.1%} of the neighbour distances over the limit -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
