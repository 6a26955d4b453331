"""GPU: the splat kernels (csrc/splat.hip) and render_scene end to end.

  * projection against the fp64 statement from the same fp32 inputs: means, conics and depths within four times the distance of the
    numpy fp32 form from the fp64 one on that case; cull flags, radii and rectangles equal away from the decision boundaries;
  * planted rows whose fate is exact;
  * pairs: offsets against numpy's cumsum, every tile's range against the rows whose rectangle contains it, in (depth, row) order;
  * the composite against the fp64 composite fed the device's own projection, within four times the fp32 form's distance;
  * equal bits on a second call, the edges of the call, and the folder / command-line path end to end.

Every measured distance is printed before it is asserted (profiles/splat_render.md quotes them)."""
import os

import numpy as np
import pytest
import torch

import splat_cases as sc

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.9)


def _nv():
    from scenesplat_amd import native as nv
    return nv


def _rd():
    from scenesplat_amd.pointcept_api import render as rd
    return rd


def _nan_workspace(nbytes):
    return torch.full((max(nbytes, 256) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda").view(torch.uint8)


def _dev(scene):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in scene.items()}


def _project(scene, block, **kw):
    d = _dev(scene)
    out = _nv().splat_project(d["coord"], d["scale"], d["quat"], d["opacity"].reshape(-1), d["color"], block, **kw)
    return out, {k: v.cpu().numpy() for k, v in out.items()}


def _check_projection(scene, block, label, **kw):
    _, got = _project(scene, block, **kw)
    p64 = sc.project(**scene, block=block, **kw)
    p32 = sc.project(**scene, block=block, ft=np.float32, **kw)
    n = len(scene["coord"])
    keep = got["tiles_touched"] > 0
    ok = ~p64["boundary"]
    left_out = int((p64["boundary"] & (p64["keep"] | keep)).sum())
    assert left_out <= 0.01 * n, (label, left_out)
    assert np.array_equal(keep[ok], p64["keep"][ok]), label
    assert np.array_equal(got["radius"][ok], p64["radius"][ok]) and np.array_equal(got["rect"][ok], p64["rect"][ok]), label
    assert np.array_equal(got["tiles_touched"][ok], p64["touched"][ok]), label
    # a culled row is all zeros
    dead = ~keep
    assert not got["mean2d"][dead].any() and not got["conic_opacity"][dead].any() and not got["depth"][dead].any() and not got["rect"][dead].any()
    both = ok & p64["keep"]
    assert np.array_equal(got["conic_opacity"][both, 3], p32["opacity"][both])
    for name, dev, key in (("mean", got["mean2d"], "mean"), ("conic", got["conic_opacity"][:, :3], "conic"), ("depth", got["depth"], "depth")):
        bound = sc.FACTOR * sc.distance(p32[key], p64[key], both)
        err = sc.distance(dev, p64[key], both)
        print(f"projection {label} {name}: fp32 form {bound / sc.FACTOR:.3e}, device {err:.3e}, bound {bound:.3e}, rows {int(both.sum())}, "
              f"left out {left_out}")
        assert err <= bound, (label, name, err, bound)
    return got


# ---- projection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_projection_against_fp64(n):
    scene, block = sc.room_case(n, seed=100 + n)
    got = _check_projection(scene, block, f"room n={n}")
    assert got["tiles_touched"][0] > 0


def test_projection_pointcloud_mode_and_scale_modifier():
    scene, block = sc.room_case(3000, seed=9)
    got = _check_projection(scene, block, "pointcloud", mode="pointcloud", point_size=3.5)
    keep = got["tiles_touched"] > 0
    assert (got["conic_opacity"][keep, 3] == 1.0).all() and (got["conic_opacity"][keep, 1] == 0.0).all()
    _check_projection(scene, block, "scale_modifier 0.5", scale_modifier=0.5)


def test_planted_rows():
    scene, block, expect = sc.planted_rows()
    _, got = _project(scene, block)
    for i, (name, kept, rect) in enumerate(expect):
        assert (got["tiles_touched"][i] > 0) == kept, name
        if kept:
            assert tuple(got["rect"][i]) == rect, (name, got["rect"][i])
            assert got["tiles_touched"][i] == (rect[2] - rect[0]) * (rect[3] - rect[1])
        else:
            assert not got["rect"][i].any() and got["radius"][i] == 0 and got["depth"][i] == 0, name
    _, pc = _project(scene, block, mode="pointcloud")
    # as points of 2 pixels nothing reaches in from far off-screen, and nothing is larger than the image
    assert [bool(t > 0) for t in pc["tiles_touched"]] == [kept and name != "far off-screen, reaching in" for name, kept, _ in expect]
    assert tuple(pc["rect"][[name for name, _, _ in expect].index("larger than the image")]) == (1, 1, 3, 2)


# ---- pairs --------------------------------------------------------------------------------------------------------------------------
def _pairs(proj, W, H):
    nv = _nv()
    n = proj["depth"].shape[0]
    ws = _nan_workspace(nv.splat_offsets_workspace_bytes(n))
    offsets, totals = nv.splat_offsets(proj["tiles_touched"], workspace=ws)
    P = int(totals[0])
    tx, ty = sc.tile_grid(W, H)
    if P == 0:
        return offsets, totals, None, None
    keys, rows = nv.splat_keys(proj["depth"], proj["rect"], proj["tiles_touched"], offsets, P, tx, ty)
    order, _, skeys = nv.argsort_i64(keys.view(1, P), 32 + max(0, (tx * ty - 1).bit_length()), want_inverse=False, want_sorted=True)
    ranges, sorted_rows = nv.splat_ranges(skeys.view(P), order.view(P), rows, tx * ty)
    return offsets, totals, ranges, sorted_rows


def _check_pairs(scene, block):
    W, H = sc.block_size(block)
    proj, got = _project(scene, block)
    offsets, totals, ranges, sorted_rows = _pairs(proj, W, H)
    touched = got["tiles_touched"].astype(np.int64)
    assert int(totals[0]) == touched.sum() and int(totals[1]) == (touched > 0).sum()
    assert np.array_equal(offsets.cpu().numpy(), np.cumsum(touched) - touched)
    lists = sc.tile_lists(got["depth"], got["rect"], touched > 0, W, H)
    r, s = ranges.cpu().numpy(), sorted_rows.cpu().numpy()
    assert sum(len(l) for l in lists) == int(totals[0])
    for tile, want in enumerate(lists):
        assert s[r[tile, 0]:r[tile, 1]].tolist() == want, tile
        if not want:
            assert r[tile].tolist() == [0, 0]
    return lists


@pytest.mark.parametrize("n", [1, 2049, 5000])
def test_pairs_of_a_room(n):
    scene, block = sc.room_case(n, seed=40 + n)
    lists = _check_pairs(scene, block)
    assert max(len(l) for l in lists) > (0 if n == 1 else 16)


def test_offsets_across_scan_blocks():
    nv = _nv()
    rng = np.random.default_rng(2)
    for n in (1, nv.SPLAT_SCAN_ROWS - 1, nv.SPLAT_SCAN_ROWS, nv.SPLAT_SCAN_ROWS + 1, 300 * nv.SPLAT_SCAN_ROWS + 77):
        t = rng.integers(0, 5, n).astype(np.int32)
        t[rng.integers(0, n, max(1, n // 8))] = 65536                     # a whole 4096 x 4096 image of tiles: the sums pass 2^31
        offsets, totals = nv.splat_offsets(torch.from_numpy(t).cuda(), workspace=_nan_workspace(nv.splat_offsets_workspace_bytes(n)))
        c = np.cumsum(t.astype(np.int64))
        assert np.array_equal(offsets.cpu().numpy(), c - t) and totals.tolist() == [int(c[-1]), int((t > 0).sum())]
    assert c[-1] > 2 ** 31


def test_pairs_of_the_equal_depth_run():
    scene, block = sc.coincident_case()
    lists = _check_pairs(scene, block)
    assert lists == [list(range(300))]


# ---- composite ----------------------------------------------------------------------------------------------------------------------
def _check_composite(scene, block, label, colors=None, **kw):
    """the device's image against the fp64 composite of the device's own projection -> the three device outputs"""
    nv = _nv()
    W, H = sc.block_size(block)
    proj, got = _project(scene, block, **kw)
    _, totals, ranges, sorted_rows = _pairs(proj, W, H)
    color = scene["color"] if colors is None else colors
    dev = nv.splat_composite(proj["mean2d"], proj["conic_opacity"], torch.from_numpy(color).cuda(), proj["depth"], ranges, sorted_rows, W, H, BG)
    keep = got["tiles_touched"] > 0
    args = (got["mean2d"], got["conic_opacity"], color, got["depth"], got["rect"], keep, W, H, BG)
    r64, r32 = sc.composite(*args), sc.composite(*args, ft=np.float32)
    decided = ~r64["undecided"]
    assert (~decided).sum() <= 0.01 * W * H, label
    for name, t in zip(("image", "alpha", "depth"), dev):
        where = decided if name != "image" else np.repeat(decided[:, :, None], 3, axis=2)
        bound = sc.FACTOR * sc.distance(r32[name], r64[name], where)
        err = sc.distance(t.cpu().numpy(), r64[name], where)
        print(f"composite {label} {name}: fp32 form {bound / sc.FACTOR:.3e}, device {err:.3e}, bound {bound:.3e}, undecided {int((~decided).sum())}")
        assert err <= bound, (label, name, err, bound)
    return dev, r64


@pytest.mark.parametrize("name", list(sc.COMPOSITE_CASES))
def test_composite_against_fp64(name):
    scene, block, populations = sc.composite_case(name)
    W, H = sc.block_size(block)
    dev, r64 = _check_composite(scene, block, name)
    tx, ty = sc.tile_grid(W, H)
    want = np.zeros((ty, tx), dtype=np.int64)
    for (x, y), c in populations.items():
        want[y, x] = c
    assert np.array_equal(r64["tile_count"], want)                        # (the device's rectangles give the planned populations)
    assert tuple(dev[0].shape) == (H, W, 3) and tuple(dev[1].shape) == (H, W) and tuple(dev[2].shape) == (H, W)
    empty = np.repeat(np.repeat(want == 0, 16, axis=0), 16, axis=1)[:H, :W]
    if empty.any():                                                       # a tile without Gaussians is the background, exactly
        assert np.array_equal(dev[0].cpu().numpy()[empty], np.broadcast_to(np.array(BG, dtype=np.float32), (int(empty.sum()), 3)))
        assert not dev[1].cpu().numpy()[empty].any() and not dev[2].cpu().numpy()[empty].any()
    if name == "64x48":
        ranks = r64["stop_rank"][16:32, 16:32]
        assert ((ranks >= 0) & (ranks < sc.BATCH)).any() and (ranks >= 2 * sc.BATCH).any()


def test_composite_of_a_room_both_modes_and_a_colour_override():
    scene, block = sc.room_case(1500, seed=77, width=37, height=21)
    _check_composite(scene, block, "room 37x21")
    _check_composite(scene, block, "room 37x21 pointcloud", mode="pointcloud", point_size=2.0)
    override = np.random.default_rng(1).uniform(0, 1, scene["color"].shape).astype(np.float32)
    a, _ = _check_composite(scene, block, "room 37x21 colors", colors=override)
    b, _ = _check_composite(scene, block, "room 37x21 again")
    assert not torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_composite_of_the_equal_depth_run():
    scene, block = sc.coincident_case()
    _check_composite(scene, block, "coincident")


# ---- render_scene -------------------------------------------------------------------------------------------------------------------
def _camera_of(block):
    W, H = sc.block_size(block)
    f = block.astype(np.float64)
    return _rd().Camera(R=f[:9].reshape(3, 3), t=f[9:12], fx=f[12], fy=f[13], cx=f[14], cy=f[15], width=W, height=H, near=f[16])


def test_render_scene_equals_the_kernels_and_repeats_bit_for_bit():
    rd = _rd()
    scene, block, _ = sc.composite_case("64x48")
    cam = _camera_of(block)
    assert np.array_equal(cam.packed(), block)
    dev, _ = _check_composite(scene, block, "64x48 (render_scene)")
    a = rd.render_scene(scene, cam, background=BG)
    b = rd.render_scene(_dev(scene), cam, background=BG)
    for k, t in zip(("image", "alpha", "depth"), dev):
        assert a[k].is_cuda and a[k].dtype == torch.float32
        assert torch.equal(a[k], t) and torch.equal(a[k], b[k]), k
    assert a["num_pairs"] == len(scene["coord"]) == a["num_visible"]
    override = np.random.default_rng(4).uniform(0, 1, scene["color"].shape).astype(np.float32)
    c = rd.render_scene(scene, cam, background=BG, colors=torch.from_numpy(override).cuda())
    want, _ = _check_composite(scene, block, "64x48 colors", colors=override)
    assert torch.equal(c["image"], want[0]) and not torch.equal(c["image"], a["image"])
    pc = rd.render_scene({k: scene[k] for k in ("coord", "color")}, cam, mode="pointcloud", point_size=2.0, background=BG)
    want, _ = _check_composite(scene, block, "64x48 pointcloud", mode="pointcloud", point_size=2.0)
    assert torch.equal(pc["image"], want[0])


def test_everything_culled_is_the_background():
    rd = _rd()
    scene, block, _ = sc.composite_case("17x33")
    scene = dict(scene, coord=scene["coord"] * np.float32(-1.0))          # behind the camera
    out = rd.render_scene(scene, _camera_of(block), background=BG)
    assert out["num_pairs"] == 0 and out["num_visible"] == 0
    assert np.array_equal(out["image"].cpu().numpy(), np.broadcast_to(np.array(BG, dtype=np.float32), (33, 17, 3)))
    assert not out["alpha"].any() and not out["depth"].any()


def test_max_pairs():
    rd = _rd()
    scene, block, _ = sc.composite_case("37x21")
    cam = _camera_of(block)
    P = rd.render_scene(scene, cam)["num_pairs"]
    assert P == len(scene["coord"])
    out = dict(image=torch.full((21, 37, 3), 7.0, device="cuda"), alpha=torch.full((21, 37), 7.0, device="cuda"),
               depth=torch.full((21, 37), 7.0, device="cuda"))
    with pytest.raises(RuntimeError, match=rf"{P} \(Gaussian, tile\) pairs.*max_pairs = {P - 1}\b"):
        rd.render_scene(scene, cam, max_pairs=P - 1, out=out)
    assert all(bool((t == 7.0).all()) for t in out.values())
    res = rd.render_scene(scene, cam, max_pairs=P, out=out)
    assert res["image"] is out["image"] and res["num_pairs"] == P
    assert torch.equal(out["image"], rd.render_scene(scene, cam)["image"]) and not bool((out["alpha"] == 7.0).any())


def test_workspace_and_device_refusals():
    nv = _nv()
    from scenesplat_amd._lib import NativeError
    n = 70001
    t = torch.ones(n, dtype=torch.int32, device="cuda")
    assert nv.splat_offsets_workspace_bytes(n) > 256
    with pytest.raises(NativeError, match="workspace too small"):
        nv.splat_offsets(t, workspace=torch.zeros(256, dtype=torch.uint8, device="cuda"))
    scene, block = sc.room_case(10, seed=1)
    d = {k: torch.from_numpy(v) for k, v in scene.items()}
    with pytest.raises(RuntimeError, match="GPU tensor"):
        nv.splat_project(d["coord"], d["scale"], d["quat"], d["opacity"], d["color"], block)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        nv.splat_offsets(torch.ones(4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        nv.splat_project(*(d[k].cuda() for k in ("coord", "scale", "quat", "opacity", "color")), block[:20])


# ---- end to end: the folder and the command line ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("splat") / "scene0000_00")
    return path, sc.synthetic_folder(path)


def test_folder_equals_the_loaded_dict(folder):
    rd = _rd()
    path, arrays = folder
    cam = rd.fit_camera(arrays["coord"], width=96, height=64)
    a, b = rd.render_scene(path, cam), rd.render_scene(arrays, cam)
    assert a["num_pairs"] == b["num_pairs"] > 0 and a["num_visible"] > 0.9 * len(arrays["coord"])
    for k in ("image", "alpha", "depth"):
        assert torch.equal(a[k], b[k])
    assert float(a["alpha"].max()) > 0.5                                  # (the camera does look at the scene)
    # the same arrays on the device, the uint8 colour among them: the same bits, and the colour does not come down to the host
    on_device = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    seen = []
    real = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *args, **kw: (seen.append(self.numel()), real(self, *args, **kw))[1]
    try:
        c = rd.render_scene(on_device, cam)
    finally:
        torch.Tensor.cpu = real
    assert seen == [2], seen                                              # the pair count and the visible rows, nothing else
    for k in ("image", "alpha", "depth"):
        assert torch.equal(a[k], c[k])
    assert tuple(a["image"].shape) == (64, 96, 3)


def test_cli_writes_the_image(folder, tmp_path, capsys):
    from PIL import Image
    rd = _rd()
    path, arrays = folder
    out = str(tmp_path / "scene.png")
    assert rd.main([path, "--output", out, "--width", "96", "--height", "64", "--background", "0.2", "0.5", "0.9"]) == 0
    want = rd.image_to_uint8(rd.render_scene(arrays, rd.fit_camera(arrays["coord"], 96, 64), background=BG)["image"])
    with Image.open(out) as f:
        assert f.size == (96, 64) and np.array_equal(np.asarray(f), want)
    assert rd.main([path, "--output", out, "--width", "40", "--height", "30", "--views", "3", "--view", "top", "--mode", "pointcloud"]) == 0
    files = sorted(p for p in os.listdir(tmp_path) if p.startswith("scene_"))
    assert files == ["scene_000.png", "scene_001.png", "scene_002.png"]
    images = []
    for p in files:
        with Image.open(tmp_path / p) as f:
            assert f.size == (40, 30)
            images.append(np.asarray(f).copy())
    assert not np.array_equal(images[0], images[1])
    assert "Saved:" in capsys.readouterr().out


def test_indices_change_the_pixels_the_highlighted_gaussians_reach(folder, tmp_path):
    from PIL import Image
    rd = _rd()
    path, arrays = folder
    chosen = np.nonzero(arrays["coord"][:, 0] > 1.2)[0].astype(np.int32)
    assert 0 < len(chosen) < len(arrays["coord"])
    cam = rd.fit_camera(arrays["coord"], 96, 64)
    grey = rd.highlight_rows(arrays["color"], np.zeros(0, dtype=np.int32))
    lit = rd.highlight_rows(arrays["color"], chosen)
    a = rd.render_scene(arrays, cam, colors=grey)
    b = rd.render_scene(arrays, cam, colors=lit)
    _, proj = _project(dict(arrays, color=grey), cam.packed())
    mark = np.zeros(len(arrays["coord"]), dtype=bool)
    mark[chosen] = True
    r64 = sc.composite(proj["mean2d"], proj["conic_opacity"], grey, proj["depth"], proj["rect"], proj["tiles_touched"] > 0, 96, 64,
                       (1.0, 1.0, 1.0), mark=mark)
    changed = (a["image"] != b["image"]).any(dim=2).cpu().numpy()
    decided = ~r64["undecided"]
    assert decided.mean() >= 0.99 and r64["reached"].any() and not r64["reached"].all()
    assert np.array_equal(changed[decided], r64["reached"][decided])
    assert torch.equal(a["alpha"], b["alpha"]) and torch.equal(a["depth"], b["depth"])
    # the command line: --indices draws what highlight_rows gives
    idx, out = str(tmp_path / "chosen_indices.npy"), str(tmp_path / "lit.png")
    np.save(idx, chosen)
    assert rd.main([path, "--output", out, "--width", "96", "--height", "64", "--indices", idx]) == 0
    with Image.open(out) as f:
        assert np.array_equal(np.asarray(f), rd.image_to_uint8(b["image"]))
