"""GPU: the PCA-colour kernels (csrc/feature_pca.hip) and pca_colors end to end.

  * column sums and Gram matrix on integer data: every product and partial sum is exact, so the result is the int64 numpy one bit for
    bit -- at the sizes around every row quantum the kernel partitions by (row image, fp32 chain, share), in the three input dtypes;
  * Gram matrix and projection on uniform data against fp64 under the fmaf-chain bound of their chain lengths;
  * the extremes equal those of the written projection exactly; the colours equal step 6 in fp32 bit for bit;
  * pca_colors on the recorded outputs of the reference's apply_pca_to_features (tests/golden/feature_pca.npz) within half a step of
    the 8-bit colour a viewer shows; the tester's save_pca."""
import os

import numpy as np
import pytest
import torch

import feature_pca_cases as fc

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return np.load(fc.GOLDEN)


def _quanta():
    from scenesplat_amd import native as nv
    return (nv.PCA_GRAM_ROWS, nv.PCA_GRAM_CHAIN, nv.PCA_GRAM_SHARE_MIN)


def _nan_workspace(nbytes):
    return torch.full((max(nbytes, 256) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda").view(torch.uint8)


def _exact_gram_and_sums(n, d, seed, offset_view=False):
    from scenesplat_amd import native as nv
    xi, si = fc.integer_rows(n, d, seed)
    g_ref = (xi - si).T @ (xi - si)                                                  # int64
    s_ref, s0_ref = (xi - si).sum(0), xi.sum(0)
    shift = torch.from_numpy(si.astype(np.float32)).cuda()
    assert nv.pca_gram_workspace_bytes(n, d) >= 128 * 128 * 8
    share = nv.pca_gram_share_rows(n, d)
    assert share % nv.PCA_GRAM_CHAIN == 0 and share >= nv.PCA_GRAM_SHARE_MIN
    for dt in DTYPES:
        x = torch.from_numpy(xi.astype(np.float32)).cuda().to(dt)
        if offset_view:                                                               # rows that start off a 16-byte boundary: scalar loads
            flat = torch.zeros(n * d + 1, dtype=dt, device="cuda")
            flat[1:] = x.reshape(-1)
            x = flat[1:].view(n, d)
            assert x.is_contiguous() and x.data_ptr() % 8 != 0
        runs = []
        for _ in range(2):
            g = nv.pca_gram(x, shift, workspace=_nan_workspace(nv.pca_gram_workspace_bytes(n, d)))
            s = nv.pca_col_sums(x, shift, workspace=_nan_workspace(8 * 1024 * d))
            runs.append((g, s))
        g, s = runs[0]
        assert g.shape == (d, d) and g.dtype == torch.float64 and s.shape == (d,) and s.dtype == torch.float64
        assert torch.equal(g, runs[1][0]) and torch.equal(s, runs[1][1])              # run to run
        g = g.cpu().numpy()
        assert np.array_equal(g, g_ref.astype(np.float64)), (n, d, dt, np.abs(g - g_ref).max())
        assert np.array_equal(s.cpu().numpy(), s_ref.astype(np.float64)), (n, d, dt)
        assert np.array_equal(nv.pca_col_sums(x).cpu().numpy(), s0_ref.astype(np.float64)), (n, d, dt)
    # without a shift
    g0 = nv.pca_gram(torch.from_numpy(xi.astype(np.float32)).cuda())
    assert np.array_equal(g0.cpu().numpy(), (xi.T @ xi).astype(np.float64))


@pytest.mark.parametrize("n,d", [(1, 3), (2, 3), (63, 33), (64, 32), (65, 96), (300, 768)])
def test_gram_and_sums_exact(n, d):
    _exact_gram_and_sums(n, d, 1000 * d + n)


@pytest.mark.parametrize("d", [40, 130])
def test_gram_and_sums_exact_around_the_row_quanta(d):
    """N at c - 1, c, c + 1 and 3 c + 17 for c = the row image, the fp32 chain and the (least) share of rows; D = 130 crosses a
    128-column tile (three tile pairs, one of them above the diagonal)"""
    seen = set()
    for c in _quanta():
        for n in (c - 1, c, c + 1, 3 * c + 17):
            if n not in seen:
                seen.add(n)
                _exact_gram_and_sums(n, d, 7 * n + d)


def test_gram_exact_from_an_unaligned_base():
    _exact_gram_and_sums(70, 40, 99, offset_view=True)


def test_gram_refuses_a_short_workspace_and_bad_operands():
    from scenesplat_amd import native as nv
    x = torch.zeros((300, 130), device="cuda")
    need = nv.pca_gram_workspace_bytes(300, 130)
    assert need == 3 * 128 * 128 * 8                                                   # one share, three tile pairs
    nv.pca_gram(x, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nv._lib.NativeError, match="workspace too small"):
        nv.pca_gram(x, workspace=torch.empty(need - 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nv._lib.NativeError, match="workspace too small"):
        nv.pca_col_sums(x, workspace=torch.empty(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nv._lib.NativeError, match="workspace too small"):
        nv.pca_project(x, torch.zeros((3, 130), device="cuda"), workspace=torch.empty(8, dtype=torch.uint8, device="cuda"))
    for bad in (torch.zeros((4, 1025), device="cuda"), torch.zeros((4, 8)), torch.zeros((4, 8), device="cuda").double(),
                torch.zeros((0, 8), device="cuda"), torch.zeros((4, 16), device="cuda")[:, :8]):
        with pytest.raises(RuntimeError):
            nv.pca_gram(bad)
    with pytest.raises(RuntimeError):
        nv.pca_gram(torch.zeros((4, 8), device="cuda"), torch.zeros(7, device="cuda"))
    with pytest.raises(RuntimeError):
        nv.pca_project(torch.zeros((4, 2), device="cuda"), torch.zeros((3, 2), device="cuda"))     # k > D


def test_gram_rounding_bound():
    """|dG_ij| <= (CHAIN + 4) 2^-24 (|X - s|^T |X - s|)_ij against the fp64 Gram of the exact x - s: the bound of an fp32 fmaf chain of
    CHAIN terms in any order, plus the one rounding of each shifted operand (the fp64 sum of the chains adds nothing at this scale)"""
    from scenesplat_amd import native as nv
    for n, d in ((5000, 96), (2 * nv.PCA_GRAM_CHAIN + 5, 130)):
        x = fc.uniform_rows(n, d, n + d)
        s = x.astype(np.float64).mean(0).astype(np.float32)
        e = x.astype(np.float64) - s.astype(np.float64)
        ref, bound = e.T @ e, (nv.PCA_GRAM_CHAIN + 4) * U * (np.abs(e).T @ np.abs(e))
        got = nv.pca_gram(torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda()).cpu().numpy()
        err = np.abs(got - ref)
        print(f"gram ({n}, {d}): largest error / bound = {(err / bound).max():.3g}")
        assert (err <= bound).all(), (n, d, (err / bound).max())
        assert np.array_equal(got, got.T)


# ---- projection -------------------------------------------------------------------------------------------------------------------
def _projection_inputs(n, d, k, seed, dtype=torch.float32, edge=256):
    """x (in dtype, as fp32 numpy), comp, off, shift and the fp64 reference; the extremes of component 0 sit in the first and the last
    row, those of component 1 on both sides of a workgroup edge (checked here on the reference, by margins far above the bound)"""
    g = np.random.RandomState(seed)
    x = fc.uniform_rows(n, d, seed)
    comp = g.randn(k, d).astype(np.float32)
    off = (1e-3 * g.randn(k)).astype(np.float32)
    x[0] = 4.0 * np.sign(comp[0])
    if n > 1:
        x[n - 1] = -4.0 * np.sign(comp[0])
    planted = n > edge + 1 and k > 1
    if planted:
        x[edge - 1] = 3.0 * np.sign(comp[1])
        x[edge] = -3.0 * np.sign(comp[1])
    xt = torch.from_numpy(x).to(dtype)
    x = xt.float().numpy()
    s = x.astype(np.float64).mean(0).astype(np.float32)
    e = x.astype(np.float64) - s.astype(np.float64)
    ref = e @ comp.astype(np.float64).T - off.astype(np.float64)
    bound = (d + 4) * U * (np.abs(e) @ np.abs(comp.astype(np.float64)).T)
    if n > 1:
        top = np.sort(ref[:, 0])
        assert ref[:, 0].argmax() == 0 and ref[:, 0].argmin() == n - 1 and top[-1] - top[-2] > 0.1 and top[1] - top[0] > 0.1
    if planted:
        top = np.sort(ref[:, 1])
        assert ref[:, 1].argmax() == edge - 1 and ref[:, 1].argmin() == edge and top[-1] - top[-2] > 0.1 and top[1] - top[0] > 0.1
    return xt, comp, off, s, ref, bound, planted


def _projection_case(n, d, k, seed, dtype=torch.float32):
    from scenesplat_amd import native as nv
    edge = nv.PCA_PROJECT_ROWS
    xt, comp, off, s, ref, bound, planted = _projection_inputs(n, d, k, seed, dtype, edge)
    xt = xt.cuda()
    y, ext = nv.pca_project(xt, torch.from_numpy(comp).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(off).cuda())
    assert y.shape == (n, k) and ext.shape == (2, k) and y.dtype == ext.dtype == torch.float32
    err = np.abs(y.cpu().numpy() - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0      # one row: x - s = 0, bound 0
    print(f"project ({n}, {d}) k = {k} {dtype}: largest error / bound = {worst:.3g}")
    assert (err <= bound).all(), (n, d, k, worst)
    assert torch.equal(ext[0], y.amin(0)) and torch.equal(ext[1], y.amax(0))
    if n > 1:
        assert int(y[:, 0].argmax()) == 0 and int(y[:, 0].argmin()) == n - 1
    if planted:
        assert int(y[:, 1].argmax()) == edge - 1 and int(y[:, 1].argmin()) == edge
    y2, ext2 = nv.pca_project(xt, torch.from_numpy(comp).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(off).cuda())
    assert torch.equal(y, y2) and torch.equal(ext, ext2)
    return y, ext


@pytest.mark.parametrize("d", [3, 33, 768])
def test_projection_bound_and_extremes(d):
    """|dy| <= (D + 4) 2^-24 sum_d |x - s| |comp| against fp64: D fmaf terms in any order, the rounding of the shifted operand, and the
    final subtraction of an offset far below the sum (1e-3: in use it is (mean - shift) . comp, a rounding error of the mean)"""
    for n in (1, 255, 256, 257, 5000):
        _projection_case(n, d, min(3, d), 34 * d + n)


def test_projection_other_widths_and_dtypes():
    for k in (1, 2):
        _projection_case(600, 96, k, 50 + k)
    for dt in (torch.float16, torch.bfloat16):
        _projection_case(600, 96, 3, 60, dt)
        _projection_case(300, 33, 3, 61, dt)
    from scenesplat_amd import native as nv
    x = torch.from_numpy(fc.uniform_rows(100, 8, 3)).cuda()
    comp = torch.from_numpy(fc.uniform_rows(2, 8, 4)).cuda()
    y, ext = nv.pca_project(x, comp)                                                   # no shift, no offset
    ref = x.double() @ comp.double().T
    assert (y.double() - ref).abs().max() <= 12 * U * (x.abs().double() @ comp.abs().double().T).max()


# ---- colours ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_colours_are_step_6_in_fp32(k):
    from scenesplat_amd import native as nv
    g = np.random.RandomState(k)
    y = torch.from_numpy((g.randn(1000, k) * 3.0).astype(np.float32))
    if k > 1:
        y[:, 1] = 0.7                                                                  # a constant component: range 0 -> colour 0
    ext = torch.stack([y.amin(0), y.amax(0)])
    got = nv.pca_colors(y.cuda(), ext.cuda())
    mn, r = ext[0], ext[1] - ext[0]
    r = torch.where(r == 0, torch.ones_like(r), r)
    P = ((y - mn) / r).clamp(0.0, 1.0)                                                 # fp32 on the host: IEEE, one rounding per step
    exp = {1: P.repeat(1, 3), 2: torch.cat([P, torch.full((1000, 1), 0.5)], 1), 3: P}[k]
    assert got.shape == (1000, 3) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), exp)
    assert float(got.min()) == 0.0 and float(got[:, 0].max()) == 1.0
    if k > 1:
        assert torch.equal(got[:, 1].cpu(), torch.zeros(1000))
    # extremes narrower than the data: clipped
    narrow = torch.stack([ext[0] * 0.5, ext[1] * 0.5])
    got = nv.pca_colors(y.cuda(), narrow.cuda()).cpu()
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(fc.CASES))
def test_pca_colors_matches_the_recorded_reference(fx, case):
    """colours within 1 / 510 (half a step of an 8-bit colour) of the reference's, explained-variance ratio within 1e-4 relative"""
    from scenesplat_amd.pointcept_api import pca_colors
    spec = fc.CASES[case]
    x = fc.features(case, fx[f"{case}.sha256"])
    out = pca_colors(x, n_components=spec["k"])
    n, d, k = spec["n"], spec["d"], spec["k"]
    assert set(out) == {"colors", "pca_features", "components", "mean", "explained_variance", "explained_variance_ratio", "n_components"}
    assert out["colors"].shape == (n, 3) and out["colors"].dtype == torch.float32 and out["colors"].is_cuda
    assert out["pca_features"].shape == (n, k) and out["pca_features"].is_cuda
    assert out["components"].shape == (k, d) and out["components"].dtype == np.float64 and out["n_components"] == k
    d_col = float(np.abs(out["colors"].cpu().numpy().astype(np.float64) - fx[f"{case}.colors"]).max())
    d_ratio = float(np.abs(out["explained_variance_ratio"] / fx[f"{case}.ratio"] - 1.0).max())
    d_comp = float(np.abs(out["components"] - fx[f"{case}.components"]).max())
    d_mean = float(np.abs(out["mean"] - x.astype(np.float64).mean(0)).max())
    print(f"pca_colors {case}: colours {d_col:.3g}, ratio (relative) {d_ratio:.3g}, components {d_comp:.3g}, mean {d_mean:.3g}")
    assert d_col <= 1.0 / 510.0
    assert d_ratio <= 1e-4
    assert d_mean <= 1e-12
    # a device tensor gives the same bits as the numpy array, and a second call the same as the first
    again = pca_colors(torch.from_numpy(x).cuda(), n_components=k)
    assert torch.equal(again["colors"], out["colors"]) and np.array_equal(again["components"], out["components"])


# ---- the tester -------------------------------------------------------------------------------------------------------------------
class StubModel:
    """point_feat.feat = the input feat"""

    def eval(self):
        return self

    def __call__(self, input_dict, chunk_size=None):
        return dict(point_feat=dict(feat=input_dict["feat"].clone()))


class Loader(list):
    batch_size = 1


def _tiny_scene(tmp_path, **test_opts):
    n, d = 240, 16
    feat = fc.clustered(n, d, 77).astype(np.float32)
    pts = np.random.RandomState(3).rand(n, 3).astype(np.float32)
    frags = [np.arange(0, n, 2), np.arange(1, n, 2), np.arange(0, n, 3)]                # every point seen once or twice
    fragment_list = [dict(coord=pts[i], grid_coord=np.floor(pts[i] / 0.02).astype(np.int64), index=i, feat=feat[i],
                          offset=np.array([len(i)])) for i in frags]
    data = dict(fragment_list=fragment_list, name="tiny", segment=np.zeros(n, np.int64), coord=pts)
    test = dict(type="ZeroShotSemSegTester", skip_eval=True)
    test.update(test_opts)
    cfg = dict(save_path=str(tmp_path / "out"), test=test, data=dict(test=dict(type="ScanNetGSDataset", split="val")))
    return cfg, Loader([[data]]), n


def test_tester_save_pca(tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS, pca_colors
    cfg, loader, n = _tiny_scene(tmp_path, save_feat=True, save_pca=True)
    assert TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=StubModel(), test_loader=loader)).test() is None
    feat_dir = os.path.join(cfg["save_path"], "result_ScanNetGSDataset", "feat")
    colours = np.load(os.path.join(feat_dir, "tiny_pca_colors.npy"))
    assert colours.shape == (n, 3) and colours.dtype == np.float32
    saved = torch.load(os.path.join(feat_dir, "tiny_feat.pth"), weights_only=True)
    assert saved.shape == (n, 16)
    assert np.array_equal(colours, pca_colors(saved)["colors"].cpu().numpy())          # what the tool gives on the saved file
    assert colours.min() == 0.0 and colours.max() == 1.0
    # off by default; as a constructor argument; and nothing without save_feat
    for sub, opts, kwargs, want in (("b", dict(save_feat=True), {}, False), ("c", dict(save_feat=True), dict(save_pca=True), True),
                                    ("d", dict(save_pca=True), {}, False)):
        cfg, loader, n = _tiny_scene(tmp_path / sub, **opts)
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=StubModel(), test_loader=loader, **kwargs)).test()
        path = os.path.join(cfg["save_path"], "result_ScanNetGSDataset", "feat", "tiny_pca_colors.npy")
        assert os.path.exists(path) == want, (sub, opts, kwargs)
        if want:
            assert np.array_equal(np.load(path), colours)
