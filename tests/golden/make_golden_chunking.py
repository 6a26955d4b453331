"""Generator of tests/golden/chunking.npz: scene chunking against the reference's OWN chunking_scene.

    python tests/golden/make_golden_chunking.py <path of the reference tree>

For every case of tests/chunking_cases.py::CASES the scene is written to a temporary folder, the reference's
pointcept/datasets/preprocessing/sampling_chunking_data_gs.py (imported by path) chunks it, and the file records the input arrays,
the split directory name, the chunk directory names and every saved asset of every chunk.  Beside them it records the origin table
and the x / y maxima the origins were computed from, as tests/chunking_cases.py::chunk_reference restates them; the generator
asserts that this restatement reproduces the reference's files bit for bit, so the recorded table is the reference's.  Only data is
written; no reference source.

Keys: `index` (JSON {case: {assets, split_dir, chunks}}), `<case>/in/<asset>`, `<case>/out/<chunk dir>/<asset>`, `<case>/origins`,
`<case>/bev_max`.

Asserted here, so that the comparisons of the tests cannot be empty: the counts of the chunks are pairwise distinct wherever
max_chunk_num selects; some case skips a chunk for its size; every case that claims chunks keeps at least one; the edge rows
(a row exactly on a chunk's lower and upper edge, on a cell edge, a duplicated coordinate, the maximum corner) are in the inputs.

It also measures how far numpy's own fp16 normalisation of lang_feat (what the reference does) lies from the fp64 quotient rounded
once, and prints it: the figure quoted in profiles/chunking.md."""
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
sys.path.insert(0, os.path.dirname(HERE))
import chunking_cases as cc  # noqa: E402

CLAIMS_CHUNKS = {"plain", "grid_first", "grid_mask_forced", "max_chunk_num", "min0_empty", "grid_half_cm", "grid_one_mm"}


def reference_module(ref_root):
    path = os.path.join(ref_root, "pointcept", "datasets", "preprocessing", "sampling_chunking_data_gs.py")
    spec = importlib.util.spec_from_file_location("ref_sampling_chunking_data_gs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fp16_distance(ref):
    """numpy's fp16 normalisation against the fp64 quotient rounded once: (largest distance in fp16 ulp, share of elements that differ)"""
    worst, differ, total = 0, 0, 0
    for n, width, seed in ((6000, 16, 11), (500, 768, 12)):
        data = cc.scene(n, seed, lang=width)
        x, valid = data["lang_feat"], data["valid_feat_mask"]
        got = x.copy()
        got[valid == 1] /= np.linalg.norm(got[valid == 1], axis=1, keepdims=True)          # the reference's statement
        want = cc.normalize_rows(x, valid)
        ulp = np.abs(got.view(np.int16).astype(np.int64) - want.view(np.int16).astype(np.int64))    # same sign wherever both are non-zero
        same_sign = (got.view(np.uint16) >> 15) == (want.view(np.uint16) >> 15)
        worst = max(worst, int(ulp[same_sign].max()))
        differ += int((got.view(np.uint16) != want.view(np.uint16)).sum())
        total += x.size
    return worst, differ / total


def main():
    ref = reference_module(sys.argv[1])
    arrays, index = {}, {}
    skipped_for_size = False
    for case, spec in cc.CASES.items():
        kw = cc.case_kwargs(case)
        inputs = cc.scene(**spec["scene"])
        with tempfile.TemporaryDirectory() as tmp:
            cc.write_scene(os.path.join(tmp, "in"), inputs)
            with contextlib.redirect_stdout(io.StringIO()):
                ref.chunking_scene(cc.SCENE, os.path.join(tmp, "in"), os.path.join(tmp, "out"), cc.SPLIT, **kw)
            made = sorted(os.listdir(os.path.join(tmp, "out"))) if os.path.isdir(os.path.join(tmp, "out")) else []
            assert len(made) <= 1, made
            split_dir = made[0] if made else None
            chunks = cc.read_chunks(os.path.join(tmp, "out", split_dir)) if split_dir else {}
        mine = cc.chunk_reference(inputs, **kw)
        cc.assert_same_chunks(mine["chunks"], chunks)                      # the restatement IS the reference on this case
        counts = mine["counts"]
        if kw["max_chunk_num"] is not None and len(counts) > kw["max_chunk_num"]:
            assert len(set(counts.tolist())) == len(counts), (case, counts)
        skipped_for_size |= bool((counts < kw["chunk_minimum_size"]).any())
        assert (case in CLAIMS_CHUNKS) == bool(chunks), (case, len(chunks))
        if split_dir is not None:
            assert split_dir == cc.split_dir(cc.SPLIT, kw["grid_size"], kw["chunk_range"], kw["chunk_stride"])
        if case == "min0_empty":
            assert any(len(c["coord"]) == 0 for c in chunks.values()), "no empty chunk was written"
        if case == "grid_mask_forced":
            rec = inputs["coord"] - inputs["coord"].min(axis=0)
            nvalid = [int((inputs["valid_feat_mask"][g] == 1).sum()) for g in cc.cells_of(rec, kw["grid_size"])]
            assert max(nvalid) == 1 and min(nvalid) == 0 and any(len(g) > 1 for g in cc.cells_of(rec, kw["grid_size"]))
        if case == "plain":
            rec = inputs["coord"] - inputs["coord"].min(axis=0)
            assert (rec[:, 0] == 1.0).any() and (rec[:, 0] == 2.0).any() and (rec[:, 1] == 1.0).any() and (rec[:, 1] == 2.0).any()
            assert (rec == rec.max(axis=0)).all(axis=1).any(), "no row at the maximum corner"
            assert len(np.unique(inputs["coord"], axis=0)) < len(inputs["coord"]), "no duplicated coordinate"
            lower = [d for d, c in chunks.items() if (c["coord"][:, 0] - inputs["coord"][:, 0].min() == 1.0).any()]
            assert lower, "no chunk holds a row on an edge"
        for a, v in inputs.items():
            arrays[f"{case}/in/{a}"] = v
        for d, c in chunks.items():
            for a, v in c.items():
                arrays[f"{case}/out/{d}/{a}"] = v
        arrays[f"{case}/origins"] = mine["origins"]
        arrays[f"{case}/bev_max"] = mine["bev_max"]
        index[case] = dict(assets=list(inputs), split_dir=split_dir, chunks=list(chunks))
        print(f"{case}: {split_dir}, {len(mine['origins'])} origins, counts {counts.tolist()}, {len(chunks)} chunks written")
    assert skipped_for_size, "no case skips a chunk for its size"
    arrays["index"] = np.asarray(json.dumps(index))
    np.savez_compressed(cc.GOLDEN, **arrays)
    print(f"{cc.GOLDEN}: {os.path.getsize(cc.GOLDEN)} bytes")
    worst, share = fp16_distance(ref)
    print(f"numpy fp16 normalisation vs fp64 rounded once: up to {worst} ulp, {100 * share:.1f} % of the elements differ")


if __name__ == "__main__":
    main()
