"""CPU: the host side of the text queries: the numpy statement on hand-worked cases, the embeddings loader, query_scene's
argument checks (before any device use), the geometry writer from numpy indices, the command line's parsing, the header constants."""
import os

import numpy as np
import pytest
import torch

import text_query_cases as tc
from scenesplat_amd import _lib
from scenesplat_amd.pointcept_api import text_query as tq

NINF = -np.inf


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------
def test_statement_ties_go_to_the_lower_row():
    s = np.array([0.5, 0.25, 0.5, 0.25, 0.25, NINF, 0.25], dtype=np.float32)
    rows, tau = tc.select(s, NINF, 3)
    assert rows.tolist() == [0, 1, 2] and tau == np.float32(0.25)
    rows, tau = tc.select(s, NINF, 4)
    assert rows.tolist() == [0, 1, 2, 3]
    rows, tau = tc.select(s, NINF, 1)
    assert rows.tolist() == [0] and tau == np.float32(0.5)


def test_statement_negative_zero_equals_zero():
    s = np.array([0.0, -0.0, -0.0, 0.0, -0.5], dtype=np.float32)
    assert tc.select(s, NINF, 2)[0].tolist() == [0, 1]
    assert tc.select(s, np.float32(0.0), -1)[0].tolist() == [0, 1, 2, 3]
    assert tc.select(s, np.float32(-0.0), 3)[0].tolist() == [0, 1, 2]


def test_statement_k_beyond_the_live_rows_and_all_dead():
    s = np.array([NINF, 0.1, NINF, -0.2], dtype=np.float32)
    rows, tau = tc.select(s, NINF, 10)
    assert rows.tolist() == [1, 3] and tau == np.float32(-0.2)
    dead = np.full(5, NINF, dtype=np.float32)
    rows, tau = tc.select(dead, NINF, 3)
    assert rows.size == 0 and tau == np.inf
    assert tc.select(dead, np.float32(0.15), -1)[0].size == 0
    out = tc.query(dead[None], "adaptive")
    assert out["thresholds"][0] == np.inf and out["counts"][0] == 0 and out["num_live"] == 0 and (out["best"] == -1).all()


def test_statement_threshold_is_inclusive_and_caps():
    s = np.array([0.1, 0.15, 0.2, 0.15, 0.3, NINF], dtype=np.float32)
    rows, tau = tc.select(s, np.float32(0.15), -1)
    assert rows.tolist() == [1, 2, 3, 4] and tau == np.float32(0.15)
    rows, tau = tc.select(s, np.float32(0.15), 3)                        # a cap below the count: the best three, the lower 0.15 row
    assert rows.tolist() == [1, 2, 4] and tau == np.float32(0.15)
    rows, tau = tc.select(s, np.float32(0.15), 2)
    assert rows.tolist() == [2, 4] and tau == np.float32(0.2)
    rows, tau = tc.select(s, np.float32(0.15), 9)                        # a cap above the count changes nothing
    assert rows.tolist() == [1, 2, 3, 4] and tau == np.float32(0.15)
    assert tc.select(s, np.float32(0.15), 0)[0].size == 0 and tc.select(s, np.float32(0.15), 0)[1] == np.inf


def test_statement_adaptive_at_zero_deviation():
    s = np.array([[0.25, NINF, 0.25, 0.25]], dtype=np.float32)
    stats = tc.statistics(s)
    assert stats.tolist() == [[3.0, 0.75, 0.1875]]
    assert tc.adaptive_threshold(stats)[0] == np.float32(0.25)           # sigma = 0: tau = mu, and every live row is selected
    out = tc.query(s, "adaptive")
    assert out["indices"][0].tolist() == [0, 2, 3] and out["num_live"] == 3
    assert tc.adaptive_threshold(stats, floor=0.5)[0] == np.float32(0.5)
    assert np.array_equal(tq.adaptive_threshold(stats), tc.adaptive_threshold(stats))


def test_statement_best_query():
    s = np.array([[0.5, 0.2, 0.3, NINF], [0.5, 0.4, 0.1, NINF], [0.1, 0.4, 0.35, NINF]], dtype=np.float32)
    out = tc.query(s, "threshold", threshold=0.3)
    assert [i.tolist() for i in out["indices"]] == [[0, 2], [0, 1], [1, 2]]
    assert out["best"].tolist() == [0, 1, 2, -1]


def test_unit_rows_match_the_module():
    g = np.load(tc.GOLDEN)
    assert np.array_equal(tq.unit_rows(g["embeddings"]), tc.unit_rows(g["embeddings"]))
    assert tq.unit_rows(np.zeros((1, 4)))[0].tolist() == [0, 0, 0, 0]


# ---- the embeddings file ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def emb_files(tmp_path):
    g = np.load(tc.GOLDEN)
    names = [str(n) for n in g["class_names"]]
    e, c = str(tmp_path / "emb.pt"), str(tmp_path / "names.txt")
    torch.save(torch.from_numpy(g["embeddings"]), e)
    with open(c, "w") as f:
        f.write("\n".join(names) + "\n\n")
    return e, c, names, g["embeddings"]


def test_load_text_queries(emb_files):
    e, c, names, emb = emb_files
    assert len(names) == 20 and emb.shape == (20, 768)
    got = tq.load_text_queries(e, c, ["chair", "shower curtain", "wall"])
    assert got.dtype == np.float32 and np.array_equal(got, emb[[names.index("chair"), names.index("shower curtain"), 0]])
    assert np.array_equal(tq.load_text_queries(e, c, "door"), emb[[names.index("door")]])
    with pytest.raises(KeyError) as err:
        tq.load_text_queries(e, c, ["chair", "spaceship"])
    assert "spaceship" in str(err.value) and "bathtub" in str(err.value)


def test_load_text_queries_shape_mismatch(tmp_path, emb_files):
    e, c, names, emb = emb_files
    short = str(tmp_path / "short.txt")
    with open(short, "w") as f:
        f.write("\n".join(names[:5]))
    with pytest.raises(ValueError):
        tq.load_text_queries(e, short, ["wall"])


# ---- query_scene's checks (all raised before the device is looked at) ---------------------------------------------------------------
X = np.zeros((10, 8), dtype=np.float32)
T = np.ones((2, 8), dtype=np.float32)


@pytest.mark.parametrize("kwargs", [
    dict(features=np.zeros(8, dtype=np.float32)),
    dict(features=np.zeros((0, 8), dtype=np.float32)),
    dict(features=np.zeros((3, tq.MAX_DIM + 1), dtype=np.float32), text_embeddings=np.ones((1, tq.MAX_DIM + 1))),
    dict(text_embeddings=np.ones((2, 7))),
    dict(text_embeddings=np.ones((2, 2, 8))),
    dict(text_embeddings=np.ones((tq.MAX_QUERIES + 1, 8))),
    dict(text_embeddings=np.ones((0, 8))),
    dict(method="nearest"),
    dict(method="topk"),
    dict(method="topk", k=-1),
    dict(method="topk", k=2.5),
    dict(max_points=-1),
    dict(threshold=float("nan")),
    dict(valid_mask=np.ones(9, dtype=bool)),
])
def test_query_scene_value_errors(kwargs):
    args = dict(features=X, text_embeddings=T)
    args.update(kwargs)
    with pytest.raises(ValueError):
        tq.query_scene(**args)


def test_query_scene_type_error_and_no_device():
    with pytest.raises(TypeError):
        tq.query_scene([[1.0, 2.0]], T)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            tq.query_scene(X, T)
        with pytest.raises(RuntimeError):
            tq.query_scene(X, T[0])                                      # (D,) is one query


def test_exported_from_the_package():
    from scenesplat_amd import pointcept_api as api
    assert api.query_scene is tq.query_scene and api.load_text_queries is tq.load_text_queries
    assert api.extract_geometry is tq.extract_geometry and api.highlight_colors is tq.highlight_colors and api.text_query is tq


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
def _scene(n=40, seed=3):
    g = np.random.RandomState(seed)
    return dict(coord=g.randn(n, 3).astype(np.float32), color=g.randint(0, 256, (n, 3)).astype(np.uint8),
                opacity=g.rand(n, 1).astype(np.float32), scale=g.rand(n, 3).astype(np.float32), quat=g.randn(n, 4).astype(np.float32))


def test_extract_geometry_individual(tmp_path):
    scene = _scene()                                                     # no normal.npy: skipped
    folder = tmp_path / "scene"
    folder.mkdir()
    for k, v in scene.items():
        np.save(folder / f"{k}.npy", v)
    np.save(folder / "segment.npy", np.zeros(40, dtype=np.int16))       # not a Gaussian array: not carried
    idx = [np.array([1, 5, 7, 30], dtype=np.int32), np.zeros(0, dtype=np.int32)]
    for src, out in ((str(folder), tmp_path / "a"), (scene, tmp_path / "b")):
        written = tq.extract_geometry(src, idx, str(out), ["chair", "table"], save_individual=True)
        assert written == [str(out / "chair"), str(out / "table")]
        for name, rows in zip(("chair", "table"), idx):
            assert sorted(os.listdir(out / name)) == sorted(f"{k}.npy" for k in scene)
            for k, v in scene.items():
                got = np.load(out / name / f"{k}.npy")
                assert got.dtype == v.dtype and got.shape == (len(rows),) + v.shape[1:] and np.array_equal(got, v[rows])
            saved = np.load(out / f"{name}_indices.npy")
            assert saved.dtype == np.int32 and np.array_equal(saved, rows)
        assert not (out / "merged").exists()


def test_extract_geometry_reads_back_as_a_scene_folder(tmp_path):
    from scenesplat_amd.pointcept_api import GenericGSDataset
    scene = _scene()
    tq.extract_geometry(scene, [np.array([2, 3, 11], dtype=np.int32)], str(tmp_path / "out" / "val"), ["chair"])
    ds = GenericGSDataset(split="val", data_root=str(tmp_path / "out"), transform=None, test_mode=False)
    folder = str(tmp_path / "out" / "val" / "chair")
    assert folder in ds.data_list                                        # (the loader itself needs the device: tests/test_hip_text_query.py)
    assert ds.asset_names(folder) == sorted(scene)


def test_extract_geometry_merged_and_ply(tmp_path):
    scene = _scene()
    idx = [np.array([9, 1, 5], dtype=np.int64), torch.tensor([5, 6, 39], dtype=torch.int32)]
    written = tq.extract_geometry(scene, dict(indices=idx), str(tmp_path), ["a", "b"], save_individual=False, save_ply=True)
    assert written == [str(tmp_path / "merged")]
    union = np.array([1, 5, 6, 9, 39])
    for k, v in scene.items():
        assert np.array_equal(np.load(tmp_path / "merged" / f"{k}.npy"), v[union])
    assert np.array_equal(np.load(tmp_path / "a_indices.npy"), [1, 5, 9])
    assert not (tmp_path / "a").exists()
    with open(tmp_path / "merged" / "points.ply", "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\n")


def test_extract_geometry_errors(tmp_path):
    scene = _scene()
    with pytest.raises(ValueError):
        tq.extract_geometry(scene, [np.array([1])], str(tmp_path), ["a", "b"])
    with pytest.raises(ValueError):
        tq.extract_geometry(scene, [np.array([40])], str(tmp_path), ["a"])
    with pytest.raises(ValueError):
        tq.extract_geometry(scene, [np.array([1]), np.array([2])], str(tmp_path), ["a", "a"])
    with pytest.raises(FileNotFoundError):
        tq.extract_geometry(str(tmp_path / "missing"), [np.array([1])], str(tmp_path), ["a"])


def test_highlight_colors_on_the_host():
    color = np.full((5, 3), 0.5, dtype=np.float32)
    out = tq.highlight_colors(color, dict(best=torch.tensor([-1, 0, 1, -1, 9], dtype=torch.int32)))
    pal = np.array(tq.PALETTE, dtype=np.float32)
    assert np.array_equal(out.numpy(), np.stack([color[0], pal[0], pal[1], color[3], pal[9 % len(pal)]]))
    u8 = tq.highlight_colors(np.zeros((2, 3), dtype=np.uint8), dict(best=torch.tensor([0, -1], dtype=torch.int32)), palette=[(1, 0.5, 0)])
    assert u8.dtype == torch.uint8 and u8.tolist() == [[255, 128, 0], [0, 0, 0]]


# ---- the command line -----------------------------------------------------------------------------------------------------------------
BASE = ["scene", "--features", "f.npy", "--embeddings", "e.pt", "--class-names", "c.txt", "--queries", "chair", "table", "--output", "out"]


def test_cli_parsing():
    a = tq.build_parser().parse_args(BASE)
    assert (a.scene, a.method, a.threshold, a.k, a.kappa, a.max_points) == ("scene", "threshold", 0.15, None, 2.0, None)
    assert a.queries == ["chair", "table"] and not a.save_individual and not a.save_ply
    a = tq.build_parser().parse_args(BASE + ["--method", "topk", "--k", "7", "--max-points", "30000", "--save-individual", "--save-ply"])
    assert (a.method, a.k, a.max_points, a.save_individual, a.save_ply) == ("topk", 7, 30000, True, True)


@pytest.mark.parametrize("argv", [
    BASE[:-2],                                              # no --output
    BASE + ["--method", "nearest"],
    BASE + ["--method", "topk"],                            # no --k
    BASE + ["--method", "topk", "--k", "-3"],
    BASE + ["--max-points", "-1"],
    BASE + ["--queries", "chair", "chair"],
])
def test_cli_error_exits(argv, capsys):
    with pytest.raises(SystemExit) as e:
        tq.main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_missing_scene(tmp_path):
    with pytest.raises(FileNotFoundError):
        tq.main([str(tmp_path / "nowhere")] + BASE[1:])


def test_cli_unknown_query(tmp_path, emb_files):
    e, c, _, _ = emb_files
    with pytest.raises(KeyError):
        tq.main([str(tmp_path), "--features", "f.npy", "--embeddings", e, "--class-names", c, "--queries", "spaceship", "--output", "o"])


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_prototypes():
    c = _lib.CONSTANTS
    assert c["SS_QUERY_MAX_DIM"] == 1024 and c["SS_QUERY_MAX_QUERIES"] == 32
    assert c["SS_QUERY_ROWS"] % 32 == 0 and c["SS_QUERY_SELECT_ROWS"] % 64 == 0
    for name in ("ss_query_scores", "ss_query_scores_workspace_bytes", "ss_query_select", "ss_query_select_workspace_bytes",
                 "ss_query_best"):
        assert name in _lib.PROTOTYPES
    assert tq.MAX_DIM == 1024 and tq.MAX_QUERIES == 32
