"""CPU: the host side of the PCA colours (scenesplat_amd/pointcept_api/feature_pca.py).  The numpy restatement of
tests/feature_pca_cases.py against the recorded outputs of the reference's apply_pca_to_features (tests/golden/feature_pca.npz), the
sign rule, the colour layouts, the refused arguments, the command line (with pca_colors stubbed out: no GPU here) and the ply file."""
import os

import numpy as np
import pytest
import torch

import feature_pca_cases as fc


@pytest.fixture(scope="module")
def fx():
    return np.load(fc.GOLDEN)


@pytest.mark.parametrize("case", sorted(fc.CASES))
def test_restatement_matches_the_recorded_reference(fx, case):
    spec = fc.CASES[case]
    x = fc.features(case, fx[f"{case}.sha256"])
    assert np.array_equal(x[:8], fx[f"{case}.head"])
    got = fc.restated(x, spec["k"])
    assert got["colors"].shape == (spec["n"], 3)
    d_col = np.abs(got["colors"] - fx[f"{case}.colors"]).max()
    d_comp = np.abs(got["components"] - fx[f"{case}.components"]).max()
    d_ratio = np.abs(got["explained_variance_ratio"] / fx[f"{case}.ratio"] - 1.0).max()
    print(case, d_col, d_comp, d_ratio)
    rec = fx[f"{case}.restatement_distance"]
    # the maker's own bar (the colours were stored as fp32: 2^-24 more)
    assert d_col <= fc.MAX_RESTATEMENT_DISTANCE and rec[0] <= fc.MAX_RESTATEMENT_DISTANCE
    assert d_col <= rec[0] + 2.0 ** -24 + 1e-12
    assert d_comp <= 1e-4 and d_ratio <= 1e-4
    ev = got["eigenvalues"][:4]
    assert ((ev[:-1] - ev[1:]) / ev[:-1]).min() >= fc.MIN_EIGEN_GAP


def test_the_module_and_the_restatement_share_the_host_steps(fx):
    """components_from_covariance (the module's steps 2-4) on the fp64 covariance = the restatement"""
    from scenesplat_amd.pointcept_api import feature_pca as fp
    x = fc.features("k2", fx["k2.sha256"]).astype(np.float64)
    ref = fc.restated(x, 2)
    xc = x - x.mean(0)
    comp, var, ratio = fp.components_from_covariance(xc.T @ xc / (len(x) - 1), 2)
    assert np.array_equal(comp, ref["components"]) and np.array_equal(var, ref["explained_variance"])
    assert np.array_equal(ratio, ref["explained_variance_ratio"])
    # the shifted form of step 1 is the same covariance
    s = x.mean(0).astype(np.float32).astype(np.float64) + 1e-3
    d = (x - s).mean(0)
    C = ((x - s).T @ (x - s) - len(x) * np.outer(d, d)) / (len(x) - 1)
    assert np.abs(C - xc.T @ xc / (len(x) - 1)).max() <= 1e-12


def test_sign_rule_on_a_tie():
    from scenesplat_amd.pointcept_api import feature_pca as fp
    rows = np.array([[0.5, -0.5, 0.1],       # equal magnitudes: index 0 decides, already positive
                     [-0.5, 0.5, 0.1],       # index 0 decides: flipped
                     [0.1, -0.7, 0.7],       # index 1 decides: flipped
                     [0.0, 0.0, -1.0]])
    exp = np.array([[0.5, -0.5, 0.1], [0.5, -0.5, -0.1], [-0.1, 0.7, -0.7], [0.0, 0.0, 1.0]])
    for f in (fp.sign_fixed, fc.sign_fixed):
        assert np.array_equal(f(rows), exp)
    assert rows[1, 0] == -0.5                # the input is left alone


def test_colour_layouts_and_zero_range():
    Y = np.array([[0.0, 5.0, 2.0], [1.0, 5.0, 4.0], [4.0, 5.0, 3.0]])
    c3 = fc.colours_from_projection(Y)
    assert np.array_equal(c3, [[0.0, 0.0, 0.0], [0.25, 0.0, 1.0], [1.0, 0.0, 0.5]])          # the constant component: colour 0
    c2 = fc.colours_from_projection(Y[:, [0, 2]])
    assert np.array_equal(c2, [[0.0, 0.0, 0.5], [0.25, 1.0, 0.5], [1.0, 0.5, 0.5]])
    c1 = fc.colours_from_projection(Y[:, :1])
    assert np.array_equal(c1, [[0.0] * 3, [0.25] * 3, [1.0] * 3])


def test_refused_arguments_need_no_device():
    from scenesplat_amd.pointcept_api import feature_pca as fp, pca_colors, fit_pca
    assert pca_colors is fp.pca_colors and fit_pca is fp.fit_pca
    x = np.zeros((10, 8), np.float32)
    for k in (0, 4, -1, 2.5, None):
        with pytest.raises(ValueError, match="n_components"):
            pca_colors(x, n_components=k)
    with pytest.raises(ValueError, match="at least 2 rows"):
        pca_colors(x[:1], n_components=1)
    with pytest.raises(ValueError, match="min"):
        pca_colors(x[:, :2], n_components=3)
    with pytest.raises(ValueError, match="min"):
        pca_colors(torch.zeros(2, 8), n_components=3)
    with pytest.raises(ValueError, match="SS_PCA_MAX_DIM"):
        pca_colors(np.zeros((4, fp.MAX_DIM + 1), np.float16))
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        fit_pca(np.zeros(8, np.float32))
    with pytest.raises(TypeError):
        pca_colors([[0.0, 1.0], [1.0, 0.0]], n_components=1)


def test_header_constants():
    from scenesplat_amd import _lib
    c = _lib.CONSTANTS
    assert c["SS_PCA_MAX_DIM"] == 1024 and c["SS_DTYPE_F16"] not in (c["SS_DTYPE_F32"], c["SS_DTYPE_BF16"])
    chain, rows, share, proj = (c[k] for k in ("SS_PCA_GRAM_CHAIN", "SS_PCA_GRAM_ROWS", "SS_PCA_GRAM_SHARE_MIN", "SS_PCA_PROJECT_ROWS"))
    assert rows > 0 and chain % rows == 0 and share % chain == 0 and proj > 0
    for name in ("ss_pca_col_sums", "ss_pca_gram", "ss_pca_gram_workspace_bytes", "ss_pca_project", "ss_pca_colors"):
        assert name in _lib.PROTOTYPES


# ---- the command line -------------------------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self, n):
        self.calls = []
        g = np.random.RandomState(5)
        self.colors = g.rand(n, 3).astype(np.float32)
        self.colors[0] = [0.0, 1.0, 0.999]
        self.colors[1] = [0.5, 254.5 / 255.0, 1.5 / 255.0]

    def __call__(self, features, n_components=3):
        self.calls.append((features, n_components))
        return dict(colors=torch.from_numpy(self.colors), explained_variance_ratio=np.array([0.5, 0.25, 0.125][:n_components]))


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:end].decode("ascii"), raw[end:]


def test_cli_features_and_ply(tmp_path, monkeypatch, capsys):
    from scenesplat_amd.pointcept_api import feature_pca as fp
    n = 37
    g = np.random.RandomState(1)
    feats, coords = g.randn(n, 12).astype(np.float16), g.randn(n, 3)
    np.save(tmp_path / "f.npy", feats)
    np.save(tmp_path / "c.npy", coords)
    stub = _Stub(n)
    monkeypatch.setattr(fp, "pca_colors", stub)
    assert fp.main(["--features", str(tmp_path / "f.npy"), "--coords", str(tmp_path / "c.npy"), "--n-components", "2",
                    "--save-colors", str(tmp_path / "col.npy"), "--save-ply", str(tmp_path / "o.ply")]) == 0
    assert len(stub.calls) == 1 and stub.calls[0][1] == 2 and np.array_equal(stub.calls[0][0], feats)
    assert stub.calls[0][0].dtype == np.float16                                        # handed over as stored: fp16 goes up as fp16
    assert np.array_equal(np.load(tmp_path / "col.npy"), stub.colors)
    assert "Explained variance ratio" in capsys.readouterr().out
    header, body = _read_ply(tmp_path / "o.ply")
    assert header == ("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
                      "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(body) == n * 15
    rows = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert np.array_equal(rows["xyz"], coords.astype(np.float32))
    assert rows["rgb"][0].tolist() == [0, 255, 254] and rows["rgb"][1].tolist() == [127, 254, 1]       # truncated, not rounded
    assert np.array_equal(rows["rgb"], (stub.colors.astype(np.float64) * 255.0).astype(np.uint8))
    # a tester feature file
    torch.save(torch.from_numpy(feats.astype(np.float32)), tmp_path / "scene_feat.pth")
    assert fp.main(["--features", str(tmp_path / "scene_feat.pth"), "--save-colors", str(tmp_path / "col2.npy")]) == 0
    got = stub.calls[1][0]
    assert isinstance(got, torch.Tensor) and torch.equal(got, torch.from_numpy(feats.astype(np.float32))) and stub.calls[1][1] == 3


def test_cli_results_dir_takes_the_newest_files(tmp_path, monkeypatch):
    from scenesplat_amd.pointcept_api import feature_pca as fp
    n = 5
    for stamp, t in (("20240101", 1000), ("20240301", 3000), ("20240201", 2000)):
        for kind, width in (("features", 4), ("coords", 3)):
            p = tmp_path / f"scene7_{stamp}_{kind}.npy"
            np.save(p, np.full((n, width), float(t)))
            os.utime(p, (t, t))
    np.save(tmp_path / "other_20250101_features.npy", np.zeros((n, 4)))
    assert [os.path.basename(p) for p in fp.find_results(str(tmp_path), "scene7")] == ["scene7_20240301_features.npy",
                                                                                       "scene7_20240301_coords.npy"]
    stub = _Stub(n)
    monkeypatch.setattr(fp, "pca_colors", stub)
    assert fp.main(["--results-dir", str(tmp_path), "--scene-name", "scene7", "--save-ply", str(tmp_path / "o.ply")]) == 0
    assert np.array_equal(stub.calls[0][0], np.full((n, 4), 3000.0))
    header, body = _read_ply(tmp_path / "o.ply")
    assert "element vertex 5\n" in header
    assert np.array_equal(np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))["xyz"], np.full((n, 3), 3000.0))
    with pytest.raises(FileNotFoundError, match="No feature files"):
        fp.find_results(str(tmp_path), "scene8")
    with pytest.raises(FileNotFoundError, match="Results directory"):
        fp.find_results(str(tmp_path / "nowhere"), "scene7")


def test_cli_refuses_incomplete_arguments(tmp_path, monkeypatch):
    from scenesplat_amd.pointcept_api import feature_pca as fp
    monkeypatch.setattr(fp, "pca_colors", _Stub(3))
    np.save(tmp_path / "f.npy", np.zeros((3, 4), np.float32))
    f = str(tmp_path / "f.npy")
    for argv in ([], ["--features", f, "--results-dir", str(tmp_path)], ["--results-dir", str(tmp_path), "--save-colors", "x.npy"],
                 ["--features", f, "--save-ply", str(tmp_path / "o.ply")], ["--features", f],
                 ["--features", f, "--n-components", "4", "--save-colors", "x.npy"]):
        with pytest.raises(SystemExit) as e:
            fp.main(argv)
        assert e.value.code == 2
    with pytest.raises(FileNotFoundError, match="Features file"):
        fp.main(["--features", str(tmp_path / "missing.npy"), "--save-colors", str(tmp_path / "x.npy")])
    with pytest.raises(FileNotFoundError, match="Coordinates file"):
        fp.main(["--features", f, "--coords", str(tmp_path / "missing.npy"), "--save-ply", str(tmp_path / "o.ply")])
    with pytest.raises(ValueError, match="coordinates"):
        fp.write_ply(str(tmp_path / "o.ply"), np.zeros((2, 3)), np.zeros((3, 3)))
