"""CPU: the host side of the splat renderer: cameras, the fp64 statement on hand-worked values, the caps of the case
builders (rows and pixels left out of the GPU comparisons), argument refusals, the command line, save_image and the registry pins.
Nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import splat_cases as sc
from scenesplat_amd import _lib
from scenesplat_amd.pointcept_api import render as rd

BG = (0.2, 0.5, 0.9)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eye,target,up", [((4.0, -4.0, 3.0), (0.0, 0.0, 1.0), (0, 0, 1)), ((0.0, 0.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0)),
                                           ((-1.0, 2.0, 0.5), (3.0, 2.5, 0.7), (0.1, 0.0, 1.0))])
def test_look_at_is_orthonormal_and_right_handed(eye, target, up):
    cam = rd.look_at_camera(eye, target, up, fov_y=60.0, width=320, height=200)
    assert np.allclose(cam.R @ cam.R.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(cam.R), 1.0, atol=1e-14)
    assert np.allclose(cam.eye, eye, atol=1e-12)
    pix, z = cam.project([target])
    assert np.allclose(pix[0], (160.0, 100.0), atol=1e-9) and np.isclose(z[0], np.linalg.norm(np.subtract(target, eye)))
    # x right, y down: a point above the target (along up) lands higher in the image (smaller y)
    above, _ = cam.project([np.asarray(target, dtype=np.float64) + 0.1 * np.asarray(up, dtype=np.float64)])
    assert above[0, 1] < 100.0
    assert np.isclose(cam.fy, 100.0 / np.tan(np.radians(30.0))) and cam.fx == cam.fy
    assert np.array_equal(cam.packed(), sc.camera_block(cam.R, cam.t, cam.fx, cam.fy, cam.cx, cam.cy, 320, 200, cam.near))
    assert cam.packed().dtype == np.float32 and cam.packed().size == _lib.CONSTANTS["SS_SPLAT_CAMERA_WORDS"]


def test_look_at_refusals():
    with pytest.raises(ValueError):
        rd.look_at_camera((0, 0, 1), (0, 0, 1))
    with pytest.raises(ValueError):
        rd.look_at_camera((0, 0, 5), (0, 0, 0), up=(0, 0, 1))
    with pytest.raises(ValueError):
        rd.look_at_camera((1, 1, 1), (0, 0, 0), fov_y=180.0)


def _cloud(seed=0, n=4000):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * [2.0, 1.0, 0.5] + [1.0, -2.0, 0.7]).astype(np.float32)


@pytest.mark.parametrize("view", rd.VIEWS)
@pytest.mark.parametrize("size", [(1280, 720), (200, 333)])
def test_fit_camera_frames_the_box(view, size):
    coord = _cloud()
    cam = rd.fit_camera(coord, width=size[0], height=size[1], fov_y=60.0, view=view)
    lo, hi = rd.fitted_box(coord)
    assert np.allclose(lo, np.percentile(coord.astype(np.float64), 1, axis=0)) and np.allclose(hi, np.percentile(coord.astype(np.float64), 99, axis=0))
    pix, z = cam.project(rd.box_corners(lo, hi))
    assert (z > cam.near).all()
    assert (pix[:, 0] >= 0).all() and (pix[:, 0] <= size[0]).all() and (pix[:, 1] >= 0).all() and (pix[:, 1] <= size[1]).all()
    # ... and tightly: some corner comes within the margin of an edge
    half = np.abs(pix - [size[0] / 2.0, size[1] / 2.0]) / [size[0] / 2.0, size[1] / 2.0]
    assert np.isclose(half.max(), rd.FIT_MARGIN, atol=1e-9)
    centre, _ = cam.project([0.5 * (lo + hi)])
    assert np.allclose(centre[0], (size[0] / 2.0, size[1] / 2.0), atol=1e-9)


def test_fit_camera_skips_rows_that_are_not_finite():
    coord = _cloud()
    dirty = coord.copy()
    dirty = np.concatenate([dirty, [[np.nan, 0, 0], [np.inf, 1, 1]]]).astype(np.float32)
    a, b = rd.fit_camera(coord, 64, 48), rd.fit_camera(torch.from_numpy(dirty), 64, 48)
    assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t)
    with pytest.raises(ValueError):
        rd.fit_camera(np.full((3, 3), np.nan), 64, 48)
    with pytest.raises(ValueError):
        rd.fit_camera(coord, 64, 48, view="side")


@pytest.mark.parametrize("n", [1, 3, 8])
def test_orbit_keeps_the_target_at_the_centre(n):
    coord = _cloud(1)
    cams = rd.orbit_cameras(coord, n, width=320, height=240)
    lo, hi = rd.fitted_box(coord)
    target = 0.5 * (lo + hi)
    assert len(cams) == n
    dist = [np.linalg.norm(c.eye - target) for c in cams]
    assert np.allclose(dist, dist[0])
    for k, cam in enumerate(cams):
        pix, _ = cam.project([target])
        assert np.allclose(pix[0], (160.0, 120.0), atol=1e-8)
        assert np.isclose(cam.eye[2], cams[0].eye[2])                     # a turntable about z: the height stays
        corners, z = cam.project(rd.box_corners(lo, hi))
        assert (z > 0).all() and (corners >= 0).all() and (corners[:, 0] <= 320).all() and (corners[:, 1] <= 240).all()
        angle = np.arctan2(*(cam.eye - target)[[1, 0]]) - np.arctan2(*(cams[0].eye - target)[[1, 0]])
        assert np.isclose(np.exp(1j * angle), np.exp(2j * np.pi * k / n))
    with pytest.raises(ValueError):
        rd.orbit_cameras(coord, 0)


# ---- the statement on hand-worked values ---------------------------------------------------------------------------------------------
def test_statement_one_axis_aligned_gaussian():
    """identity camera, fx = fy = 64, 64 x 48: p = (0.25, -0.125, 2), s = (0.125, 0.0625, 1), q = identity.  x/z = 0.125, y/z = -0.0625:
    mean = (64 * 0.125 + 32, 64 * -0.0625 + 24) = (40, 20).  J = [[32, 0, -4], [0, 32, 2]] (no clamp: the limits are 0.65 and 0.4875), so
    A = J diag(s) = [[4, 0, -4], [0, 2, 2]]: Sigma' = [[32.3, -8], [-8, 8.3]], det = 204.09, conic = [[8.3, 8], [8, 32.3]] / 204.09.
    mid = 20.3, lambda = 20.3 + sqrt(412.09 - 204.09) = 20.3 + sqrt(208) = 34.7222, 3 sqrt(lambda) = 17.68: radius 18.
    x: floor(22 / 16) = 1, floor((58 + 15) / 16) = 4; y: floor(2 / 16) = 0, floor((38 + 15) / 16) = 3: the rectangle (1, 0, 4, 3)."""
    block = sc.identity_camera(64, 48)
    scene = dict(coord=[[0.25, -0.125, 2.0]], scale=[[0.125, 0.0625, 1.0]], quat=[[1.0, 0, 0, 0]], opacity=[0.5], color=[[1.0, 0.5, 0.25]])
    p = sc.project(**scene, block=block)
    assert p["keep"][0] and np.allclose(p["mean"][0], (40.0, 20.0), atol=1e-12) and p["depth"][0] == 2.0
    assert np.allclose(p["conic"][0], np.array([8.3, 8.0, 32.3]) / 204.09, rtol=1e-6)       # (0.3 is the fp32 value)
    assert p["radius"][0] == 18 and tuple(p["rect"][0]) == (1, 0, 4, 3) and p["touched"][0] == 9
    # a quaternion of any length is the same rotation; a quarter turn about z swaps the axes of the scale
    turned = dict(scene, quat=[[3.0 * np.sqrt(0.5), 0, 0, 3.0 * np.sqrt(0.5)]], scale=[[0.0625, 0.125, 1.0]])
    assert np.allclose(sc.project(**turned, block=block)["conic"][0], p["conic"][0], rtol=1e-6)
    # the point cloud mode: (6 / 3)^2 I, opacity 1
    pc = sc.project(**scene, block=block, mode="pointcloud", point_size=6.0)
    assert np.allclose(pc["conic"][0], (0.25, 0.0, 0.25)) and pc["opacity"][0] == 1.0 and pc["radius"][0] == 7   # 3 sqrt(4 + sqrt(0.1)) = 6.23
    # scale_modifier 2 doubles A: Sigma' = [[128.3, -32], [-32, 32.3]]
    big = sc.project(**scene, block=block, scale_modifier=2.0)
    assert np.allclose(big["conic"][0], np.array([32.3, 32.0, 128.3]) / (128.3 * 32.3 - 1024.0), rtol=1e-6)


def test_statement_clamps_the_jacobian_off_screen():
    """x/z = 2 is clamped to limx = 1.3 * 64 / 128 = 0.65 in J, not in the mean"""
    block = sc.identity_camera(64, 48)
    p = sc.project(coord=[[4.0, 0.0, 2.0]], scale=[[0.0, 0.0, 1.0]], quat=[[1.0, 0, 0, 0]], opacity=[1.0], color=[[0, 0, 0]], block=block)
    assert not p["keep"][0]                                              # mean x = 160: its radius does not reach the image
    block = sc.identity_camera(512, 48)
    p = sc.project(coord=[[4.0, 0.0, 2.0]], scale=[[0.0, 0.0, 1.0]], quat=[[1.0, 0, 0, 0]], opacity=[1.0], color=[[0, 0, 0]], block=block)
    assert p["keep"][0] and np.isclose(p["mean"][0, 0], 64.0 * 2.0 + 256.0)
    # limx = 1.3 * 512 / 128 = 5.2: no clamp; a = (32 * 2)^2 + 0.3
    assert np.isclose(p["conic"][0, 2] * (p["conic"][0, 0] * p["conic"][0, 2] - p["conic"][0, 1] ** 2) ** -1, 4096.3, rtol=1e-6)


def _flat(scene, block, ft=np.float64, **kw):
    p = sc.project(**scene, block=block, ft=ft, **kw)
    return p, np.concatenate([p["conic"], p["opacity"][:, None]], axis=1)


def test_statement_front_colour_wins():
    """two opaque Gaussians on one spot: the pixel at their centre takes 0.99 of the front colour, 0.0099 of the back one"""
    block = sc.identity_camera(16, 16)
    scene = dict(coord=np.array([[0.0078125 * 3, 0.0078125 * 3, 3.0], [0.0078125 * 2, 0.0078125 * 2, 2.0]], dtype=np.float32) * 1.0,
                 scale=np.full((2, 3), 0.2, dtype=np.float32), quat=np.array([[1.0, 0, 0, 0]] * 2, dtype=np.float32),
                 opacity=np.array([1.0, 1.0], dtype=np.float32), color=np.array([[0, 0, 1.0], [1.0, 0, 0]], dtype=np.float32))
    p, co = _flat(scene, block)
    assert np.allclose(p["mean"], 8.5)                                   # the centre of pixel (8, 8)
    out = sc.composite(p["mean"], co, scene["color"], p["depth"], p["rect"], p["keep"], 16, 16, BG)
    want = 0.99 * np.array([1.0, 0, 0]) + 0.01 * 0.99 * np.array([0, 0, 1.0]) + 1e-4 * np.array(BG)
    assert np.allclose(out["image"][8, 8], want, atol=1e-7)              # (0.99 is the fp32 value)
    assert np.isclose(out["alpha"][8, 8], 1.0 - 1e-4, atol=1e-7) and np.isclose(out["depth"][8, 8], 0.99 * 2.0 + 0.0099 * 3.0, atol=1e-6)
    # a third one behind them would leave T' = 1e-6 < 1e-4: the pixel stops before adding it
    more = {k: np.concatenate([v, v[:1]]) for k, v in scene.items()}
    more["coord"][2] = more["coord"][0] * (4.0 / 3.0)
    p3, co3 = _flat(more, block)
    out3 = sc.composite(p3["mean"], co3, more["color"], p3["depth"], p3["rect"], p3["keep"], 16, 16, BG)
    assert np.array_equal(out3["image"][8, 8], out["image"][8, 8]) and out3["stop_rank"][8, 8] == 2
    # equal depths: the lower row is in front
    same = dict(scene, coord=np.repeat(scene["coord"][1:], 2, axis=0))
    ps, cos = _flat(same, block)
    outs = sc.composite(ps["mean"], cos, same["color"], ps["depth"], ps["rect"], ps["keep"], 16, 16, BG)
    assert outs["image"][8, 8, 2] > 0.98 and outs["image"][8, 8, 0] < 0.02


def test_statement_tile_rule_and_background():
    """a Gaussian contributes to a pixel iff the pixel's tile lies in its rectangle, however large its value there would be"""
    block = sc.identity_camera(48, 16)
    scene, _ = dict(coord=[[0.0, 0.0, 2.0]], scale=[[0.05, 0.05, 0.05]], quat=[[1.0, 0, 0, 0]], opacity=[1.0], color=[[0, 1.0, 0]]), None
    p, co = _flat(scene, block)
    assert tuple(p["rect"][0]) == (1, 0, 2, 1)                            # mean (24, 8), sigma^2 = 2.86: radius 6 stays inside tile 1
    out = sc.composite(p["mean"], co, scene["color"], p["depth"], p["rect"], p["keep"], 48, 16, BG)
    assert np.array_equal(out["image"][:, :16], np.broadcast_to(np.array(BG, dtype=np.float32).astype(np.float64), (16, 16, 3)))
    assert (out["alpha"][:, :16] == 0).all() and (out["alpha"][:, 32:] == 0).all() and out["alpha"][8, 24] > 0.9
    lists = sc.tile_lists(p["depth"], p["rect"], p["keep"], 48, 16)
    assert lists == [[], [0], []]


def test_planted_rows_in_the_statement():
    scene, block, expect = sc.planted_rows()
    for ft in (np.float64, np.float32):
        p = sc.project(**scene, block=block, ft=ft)
        for i, (name, kept, rect) in enumerate(expect):
            assert p["keep"][i] == kept, (name, ft)
            if kept:
                assert tuple(p["rect"][i]) == rect, (name, ft)
            else:
                assert p["touched"][i] == 0


# ---- the builders stay within their caps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_room_case_boundary_rows_are_few(n):
    scene, block = sc.room_case(n, seed=100 + n)
    p64, p32 = sc.project(**scene, block=block), sc.project(**scene, block=block, ft=np.float32)
    flagged = p64["boundary"] & (p64["keep"] | p32["keep"])
    assert flagged.sum() <= 0.01 * n, (n, int(flagged.sum()))
    assert p64["keep"][0] and p64["keep"].sum() >= 0.2 * n
    ok = ~p64["boundary"]
    # away from the boundaries the fp32 form decides as the fp64 one does
    assert np.array_equal(p64["keep"][ok], p32["keep"][ok]) and np.array_equal(p64["rect"][ok], p32["rect"][ok])
    assert np.array_equal(p64["radius"][ok], p32["radius"][ok])
    assert p32["mean"].dtype == np.float32 and p32["conic"].dtype == np.float32 and p32["depth"].dtype == np.float32
    if n == 70001:
        assert n > 16 * _lib.CONSTANTS["SS_SPLAT_SCAN_ROWS"]              # several scan blocks


@pytest.mark.parametrize("name", list(sc.COMPOSITE_CASES))
def test_composite_case_populations_and_undecided_pixels(name):
    scene, block, populations = sc.composite_case(name)
    W, H = sc.block_size(block)
    p, co = _flat(scene, block, ft=np.float32)                            # (what the device's projection should be)
    out = sc.composite(p["mean"], co, scene["color"], p["depth"], p["rect"], p["keep"], W, H, BG)
    tx, ty = sc.tile_grid(W, H)
    want = np.zeros((ty, tx), dtype=np.int64)
    for (x, y), c in populations.items():
        want[y, x] = c
    assert np.array_equal(out["tile_count"], want)
    assert out["undecided"].sum() <= 0.01 * W * H
    f32 = sc.composite(p["mean"], co, scene["color"], p["depth"], p["rect"], p["keep"], W, H, BG, ft=np.float32)
    assert f32["image"].dtype == np.float32
    assert 0 < sc.distance(out["image"], f32["image"]) < 1e-5
    if name == "64x48":
        # the opaque stacks of tile (1, 1): pixels that stop in the first batch, and pixels that stop in the third
        ranks = out["stop_rank"][16:32, 16:32]
        assert ((ranks >= 0) & (ranks < sc.BATCH)).any() and (ranks >= 2 * sc.BATCH).any() and (ranks < 0).any()
        assert set(populations.values()) >= {1, 256, 257, 513} and (want == 0).any()


def test_room_composite_case_undecided_pixels_are_few():
    scene, block = sc.room_case(1500, seed=77, width=37, height=21)
    for kw in ({}, dict(mode="pointcloud", point_size=2.0)):
        p, co = _flat(scene, block, ft=np.float32, **kw)
        out = sc.composite(p["mean"], co, scene["color"], p["depth"], p["rect"], p["keep"], 37, 21, BG)
        assert out["undecided"].sum() <= 0.01 * 37 * 21 and out["alpha"].max() > 0.5


def test_coincident_case_is_one_run_of_equal_depths():
    scene, block = sc.coincident_case()
    p = sc.project(**scene, block=block, ft=np.float32)
    assert p["keep"].all() and len(np.unique(p["depth"])) == 1 and len(scene["coord"]) == 300
    assert len(np.unique(scene["color"], axis=0)) == 300
    assert sc.tile_lists(p["depth"], p["rect"], p["keep"], 16, 16) == [list(range(300))]


# ---- argument refusals (before any launch) ------------------------------------------------------------------------------------------
def _scene(n=5):
    rng = np.random.default_rng(0)
    return dict(coord=rng.standard_normal((n, 3)).astype(np.float32), color=rng.integers(0, 255, (n, 3)).astype(np.uint8),
                opacity=np.ones((n, 1), dtype=np.float32), scale=np.full((n, 3), 0.1, dtype=np.float32),
                quat=np.tile(np.array([1.0, 0, 0, 0], dtype=np.float32), (n, 1)))


def _cam(width=64, height=48):
    return rd.look_at_camera((3, 3, 3), (0, 0, 0), width=width, height=height)


@pytest.mark.parametrize("change,kw", [
    (dict(coord=np.zeros((5, 2), dtype=np.float32)), {}),
    (dict(coord=np.zeros((0, 3), dtype=np.float32)), {}),
    (dict(coord=np.zeros((5, 3), dtype=np.int32)), {}),
    (dict(scale=np.zeros((4, 3), dtype=np.float32)), {}),
    (dict(quat=np.zeros((5, 3), dtype=np.float32)), {}),
    (dict(quat=np.zeros((5, 4), dtype=np.int64)), {}),
    (dict(opacity=np.zeros((5, 2), dtype=np.float32)), {}),
    (dict(color=np.zeros((4, 3), dtype=np.uint8)), {}),
    ({}, dict(colors=np.zeros((4, 3), dtype=np.float32))),
    ({}, dict(colors=np.zeros((5, 3), dtype=np.uint8))),
    ({}, dict(mode="ellipsoids")),
    ({}, dict(point_size=0.0)),
    ({}, dict(scale_modifier=float("nan"))),
    ({}, dict(background=(1.0, 1.0))),
    ({}, dict(max_pairs=-1)),
    ({}, dict(max_pairs=2 ** 31)),
])
def test_render_scene_refusals(change, kw):
    scene = dict(_scene(), **change)
    with pytest.raises(ValueError):
        rd.render_scene(scene, _cam(), **kw)


def test_render_scene_refuses_missing_arrays_and_types(tmp_path):
    scene = _scene()
    with pytest.raises(ValueError):
        rd.render_scene({k: v for k, v in scene.items() if k != "quat"}, _cam())
    with pytest.raises(ValueError):
        rd.render_scene({k: v for k, v in scene.items() if k != "color"}, _cam(), mode="pointcloud")
    with pytest.raises(ValueError):
        rd.render_scene({k: v for k, v in scene.items() if k != "coord"}, _cam())
    with pytest.raises(FileNotFoundError):
        rd.render_scene(str(tmp_path / "nowhere"), _cam())
    with pytest.raises(TypeError):
        rd.render_scene(7, _cam())
    with pytest.raises(TypeError):
        rd.render_scene(scene, "camera")


@pytest.mark.parametrize("width,height", [(0, 48), (4097, 48), (64, 0), (64, 4097), (64.5, 48)])
def test_camera_size_refusals(width, height):
    with pytest.raises(ValueError):
        _cam(width, height)
    with pytest.raises(ValueError):
        rd.as_camera(dict(R=np.eye(3), t=np.zeros(3), fx=50.0, fy=50.0, cx=1.0, cy=1.0, width=width, height=height))


def test_camera_dict_and_limits():
    cam = rd.as_camera(dict(R=np.eye(3), t=[0, 0, 0], fx=64.0, fy=32.0, cx=32.0, cy=24.0, width=4096, height=1))
    assert cam.near == 0.01 and cam.limits() == (1.3 * 4096 / 128.0, 1.3 / 64.0)
    block = cam.packed()
    assert block.view(np.int32)[19:21].tolist() == [4096, 1] and block[16] == np.float32(0.01) and (block[21:] == 0).all()
    for bad in (dict(fx=0.0), dict(near=0.0), dict(cx=float("nan")), dict(R=np.full((3, 3), np.inf))):
        with pytest.raises(ValueError):
            rd.as_camera(dict(dict(R=np.eye(3), t=[0, 0, 0], fx=64.0, fy=32.0, cx=32.0, cy=24.0, width=8, height=8), **bad))


def test_scene_colors_and_highlight_rows():
    u8 = np.array([[0, 255, 51], [255, 255, 255]], dtype=np.uint8)
    assert np.array_equal(rd.scene_colors(u8), u8.astype(np.float32) / np.float32(255))
    f = np.array([[0.25, 0.5, 1.0]], dtype=np.float64)
    assert rd.scene_colors(f).dtype == np.float32 and np.array_equal(rd.scene_colors(f), f.astype(np.float32))
    t = rd.scene_colors(torch.from_numpy(u8))                            # a tensor stays a tensor, with the same values
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), rd.scene_colors(u8))
    assert np.array_equal(rd.scene_colors(torch.from_numpy(f)).numpy(), f.astype(np.float32))
    from scenesplat_amd.pointcept_api.text_query import PALETTE
    out = rd.highlight_rows(u8, np.array([1]))
    lum = np.float32(0.587) * np.float32(1.0) + np.float32(0.114) * np.float32(0.2)
    assert out.dtype == np.float32 and np.allclose(out[0], lum, atol=1e-6) and np.allclose(out[1], PALETTE[0])
    assert np.array_equal(rd.highlight_rows(u8, np.zeros(0, dtype=np.int64))[1], np.ones(3, dtype=np.float32))
    with pytest.raises(ValueError):
        rd.highlight_rows(u8, np.array([2]))


# ---- save_image ---------------------------------------------------------------------------------------------------------------------
def test_save_image_round_trips_through_pil(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.2, 1.2, (37, 21, 3)).astype(np.float32)
    img[0, 0] = (0.0, 1.0, 0.5)
    img[0, 1] = (0.49803922, 0.5 / 255.0 - 1e-4, 254.5 / 255.0 + 1e-4)
    want = (np.clip(img, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    assert want[0, 0].tolist() == [0, 255, 128] and want[0, 1].tolist() == [127, 0, 255]
    for k, image in enumerate((img, torch.from_numpy(img))):
        path = str(tmp_path / f"a{k}.png")
        assert np.array_equal(rd.save_image(path, image), want)
        with Image.open(path) as f:
            assert f.size == (21, 37) and f.mode == "RGB" and np.array_equal(np.asarray(f), want)
    with pytest.raises(ValueError):
        rd.save_image(str(tmp_path / "b.png"), np.zeros((4, 4), dtype=np.float32))


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_parsing():
    a = rd.build_parser().parse_args(["scene", "--output", "o.png"])
    assert (a.scene, a.output, a.width, a.height, a.fov, a.view, a.mode) == ("scene", "o.png", 1280, 720, 60.0, "iso", "gaussians")
    assert (a.point_size, a.views, a.colors, a.indices, a.background, a.scale_modifier, a.max_pairs) == (2.0, 1, None, None, [1.0, 1.0, 1.0], 1.0, None)
    a = rd.build_parser().parse_args(["s", "--output", "o.png", "--width", "64", "--height", "48", "--fov", "45", "--view", "top", "--mode",
                                      "pointcloud", "--point-size", "3", "--views", "8", "--colors", "c.npy", "--background", "0", "0.5", "1",
                                      "--scale-modifier", "0.5", "--max-pairs", "1000"])
    assert (a.width, a.height, a.fov, a.view, a.mode, a.point_size, a.views) == (64, 48, 45.0, "top", "pointcloud", 3.0, 8)
    assert (a.colors, a.background, a.scale_modifier, a.max_pairs) == ("c.npy", [0.0, 0.5, 1.0], 0.5, 1000)
    assert rd.view_paths("out/scene.png", 1) == ["out/scene.png"]
    assert rd.view_paths("out/scene.png", 3) == ["out/scene_000.png", "out/scene_001.png", "out/scene_002.png"]


@pytest.mark.parametrize("argv", [
    ["scene"],                                                            # no --output
    ["scene", "--output", "o.png", "--mode", "ellipsoids"],
    ["scene", "--output", "o.png", "--view", "side"],
    ["scene", "--output", "o.png", "--width", "0"],
    ["scene", "--output", "o.png", "--height", "4097"],
    ["scene", "--output", "o.png", "--views", "0"],
    ["scene", "--output", "o.png", "--fov", "180"],
    ["scene", "--output", "o.png", "--point-size", "0"],
    ["scene", "--output", "o.png", "--max-pairs", "-1"],
    ["scene", "--output", "o.png", "--background", "1", "1"],
    ["scene", "--output", "o.png", "--colors", "c.npy", "--indices", "i.npy"],
])
def test_cli_error_exits(argv, capsys):
    with pytest.raises(SystemExit) as e:
        rd.main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_missing_scene(tmp_path):
    with pytest.raises(FileNotFoundError):
        rd.main([str(tmp_path / "nowhere"), "--output", str(tmp_path / "o.png")])


# ---- the header and the registries ----------------------------------------------------------------------------------------------------
def test_header_constants_and_prototypes():
    import ctypes
    c = _lib.CONSTANTS
    assert (c["SS_SPLAT_TILE"], c["SS_SPLAT_BATCH"], c["SS_SPLAT_MAX_DIM"], c["SS_SPLAT_CAMERA_WORDS"]) == (16, 256, 4096, 24)
    assert c["SS_SPLAT_SCAN_ROWS"] % 256 == 0 and (c["SS_SPLAT_MODE_GAUSSIANS"], c["SS_SPLAT_MODE_POINTCLOUD"]) == (0, 1)
    assert (sc.TILE, sc.BATCH, sc.CAMERA_WORDS) == (c["SS_SPLAT_TILE"], c["SS_SPLAT_BATCH"], c["SS_SPLAT_CAMERA_WORDS"])
    for name in ("ss_splat_project", "ss_splat_offsets", "ss_splat_offsets_workspace_bytes", "ss_splat_keys", "ss_splat_ranges",
                 "ss_splat_composite"):
        assert name in _lib.PROTOTYPES
    # the camera travels as one host pointer; no double by value anywhere
    res, args = _lib.PROTOTYPES["ss_splat_project"]
    assert res is ctypes.c_int and args[6] is ctypes.c_void_p and args[8] is ctypes.c_float and args[9] is ctypes.c_float
    assert (rd.TILE, rd.MAX_DIM, rd.MAX_PAIRS) == (16, 4096, 2 ** 31 - 1)


def test_nothing_new_is_registered():
    import scenesplat_amd.pointcept_api as api
    import inspect
    for name in ("render_scene", "look_at_camera", "fit_camera", "orbit_cameras", "save_image"):
        assert getattr(api, name) is getattr(rd, name)
    assert api.render is rd
    assert "register_module" not in inspect.getsource(rd)
    for name in ("HOOKS", "TESTERS", "DATASETS", "TRANSFORMS", "MODELS", "LOSSES"):
        table = getattr(api, name).module_dict
        assert not [k for k, cls in table.items() if cls.__module__ == rd.__name__ or "splat" in k.lower() or "render" in k.lower()]
