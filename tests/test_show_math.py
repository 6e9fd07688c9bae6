"""CPU checks of neat_amd.show: the orbit cameras and the projection against the reference's recorded numbers
(tests/golden/g21_show_cameras.npz, made by tests/golden/make_show_golden.py), the numpy restatement of the picture (tests/show_f64.py)
against pixels computed by hand, and the ABI block (header and binding name the same neat_show_* set; the version stays 15)."""
import os
import re

import numpy as np
import pytest

from neat_amd import _lib, show
from tests import show_f64 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = os.path.join(ROOT, "tests", "golden", "g21_show_cameras.npz")
POSE_KEYS = {"dtu": "dtu", "scan": "scan", "none": None}


def _front_cam(W, H, f=128.0):
    """A camera at the origin looking down +z with the world's axes: x = f X / Z + cx (f a power of two: _at round-trips exactly)."""
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]])
    return show.pack_cameras(np.eye(4)[None], K)[0]


def _at(cam, x, y, z):
    """The world point that lands on pixel coordinates (x, y) at depth z under _front_cam."""
    fx, fy, cx, cy, _, _ = S.split_cam(cam)
    return [(x - cx) * z / fx, (y - cy) * z / fy, z]


@pytest.mark.parametrize("name", ["dtu", "scan", "none"])
def test_orbit_matches_the_reference_pose(name):
    g = np.load(G21)
    rx, ry, rz, t = g["pose_" + name]
    assert show.POSES[POSE_KEYS[name]] == (rx, ry, rz, t)
    w2c = show.orbit(rx, ry, rz, t, frames=72, step=5.0)
    assert w2c.shape == (72, 4, 4) and w2c.dtype == np.float64
    for off in g["offsets"]:
        c2w = g["c2w_%s_%d" % (name, off)]
        k = int(off) // 5
        # the reference's camera looks down -z with y up: orbit() changes to the project's axes (z forward, rows down), nothing else
        np.testing.assert_allclose(np.linalg.inv(show.CAMERA_AXES @ w2c[k]), c2w, rtol=0, atol=1e-12)
        np.testing.assert_allclose(show.CAMERA_AXES @ w2c[k], np.linalg.inv(c2w), rtol=0, atol=1e-12)
        origin = w2c[k] @ np.array([0.0, 0.0, 0.0, 1.0])
        np.testing.assert_allclose(origin, [0.0, 0.0, t, 1.0], rtol=0, atol=1e-6)          # the scene's centre straight ahead at distance t
        np.testing.assert_allclose(show.camera_to_world(rx, (ry + off) % 360, rz, t), c2w, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["dtu", "scan", "none"])
def test_projection_matches_the_reference_arithmetic(name):
    g = np.load(G21)
    W, H = int(g["width"]), int(g["height"])
    K = show.intrinsics(W, H, float(g["fov"]))
    np.testing.assert_allclose(K, g["K"], rtol=0, atol=1e-12)
    assert K[0, 0] == K[1, 1] and K[0, 2] == (W - 1) / 2 and K[1, 2] == (H - 1) / 2
    np.testing.assert_allclose(K[1, 1], 0.5 * H / np.tan(np.radians(30.0)), rtol=1e-15)
    w2c = show.orbit(*g["pose_" + name], frames=72, step=5.0)
    for off in g["offsets"]:
        cam = show.pack_cameras(w2c[int(off) // 5], K)[0]
        Xc = S.to_cam(cam, g["lines3d"].reshape(-1, 3))
        x, y, ok = S.project(cam, Xc)
        assert ok.all() and (Xc[:, 2] > 1.0).all()
        # show.py:313-317 divides by the reference camera's negative z: its x is this picture's mirrored about the principal point
        # (y / z keeps its value when both change sign)
        got = np.stack([2.0 * K[0, 2] - x, y], -1).reshape(-1, 2, 2)
        np.testing.assert_allclose(got, g["lines2d_%s_%d" % (name, off)], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("width", [1.0, 1.5, 2.0])
def test_horizontal_segment_on_an_integer_row(width):
    W, H = 24, 12
    cam = _front_cam(W, H)
    line = np.array([[_at(cam, 4.0, 5.0, 2.0), _at(cam, 18.0, 5.0, 2.0)]])
    r = S.render(line, cam[None], H, W, width=width)
    cov = r["cov"][0]
    assert np.all(cov[5, 4:19] == 1.0)
    side = np.float32(min(max(width / 2 - 0.5, 0.0), 1.0))          # hw - 1 = w / 2 + 0.5 - 1
    np.testing.assert_allclose(cov[4, 4:19], side, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov[6, 4:19], side, rtol=0, atol=1e-12)
    assert np.all(cov[:3] == 0) and np.all(cov[8:] == 0) and np.all(cov[:, :2] == 0) and np.all(cov[:, 21:] == 0)
    # the caps: distance 1 past the end along the row
    np.testing.assert_allclose(cov[5, [3, 19]], side, rtol=0, atol=1e-12)
    assert (r["rgb"][0, 5, 10] == 0).all() and (r["rgb"][0, 0, 0] == 255).all()
    grey = int(np.floor(255.0 * (1.0 - float(side)) + 0.5))
    assert (r["rgb"][0, 4, 10] == grey).all()


def test_zero_length_segment_is_a_disc():
    W, H = 15, 13
    cam = _front_cam(W, H)
    p = _at(cam, 7.0, 6.0, 2.0)
    r = S.render(np.array([[p, p]]), cam[None], H, W, width=3.0)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    want = np.clip(2.0 - np.hypot(j - 7.0, i - 6.0), 0, 1)
    np.testing.assert_allclose(r["cov"][0], want, rtol=0, atol=1e-6)
    assert r["cov"][0, 6, 7] == 1.0 and r["cov"][0, 6, 9] == 0.0 and r["cov"][0, 6, 8] == 1.0
    # the points pass draws the same disc for radius = width / 2
    rp = S.render(None, cam[None], H, W, points=np.array([p]), radius=1.5)
    assert np.array_equal(rp["covp"][0], r["cov"][0])


def _tri_scene(W, H, cam):
    verts = np.array([_at(cam, 2.0, 1.0, 2.0), _at(cam, 12.0, 2.0, 2.0), _at(cam, 5.0, 9.0, 2.0),          # far, z = 2
                      _at(cam, 4.0, 3.0, 1.5), _at(cam, 9.0, 3.0, 1.5), _at(cam, 6.0, 7.0, 1.5)])          # near, z = 1.5, inside the far one
    return verts


def test_triangle_covers_its_vertices_and_the_nearer_wins():
    W, H = 16, 12
    cam = _front_cam(W, H)
    verts = _tri_scene(W, H, cam)
    r = S.render(None, cam[None], H, W, verts=verts, faces=[[0, 1, 2]])
    idx, depth = r["index"][0], r["depth"][0]
    for (x, y) in ((2, 1), (12, 2), (5, 9)):
        assert idx[y, x] == 0, (x, y)
    assert idx[0, 0] == -1 and np.isinf(depth[0, 0]) and depth[4, 6] == np.float32(2.0)
    # both windings draw the same pixels
    r2 = S.render(None, cam[None], H, W, verts=verts, faces=[[0, 2, 1]])
    assert np.array_equal(r2["index"][0], idx)
    # a nearer triangle wins whatever its place in the list
    for faces, near_k in (([[0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [0, 1, 2]], 0)):
        rr = S.render(None, cam[None], H, W, verts=verts, faces=faces)
        assert rr["index"][0, 4, 6] == near_k and rr["depth"][0, 4, 6] == np.float32(1.5)
        assert rr["index"][0, 1, 2] == 1 - near_k
    # the shade of a triangle facing the camera is 1: mesh_color itself
    assert (r["rgb"][0, 4, 6] == int(np.floor(255 * 0.8 + 0.5))).all()


def test_equal_depth_duplicate_goes_to_the_lower_index():
    W, H = 16, 12
    cam = _front_cam(W, H)
    verts = _tri_scene(W, H, cam)
    r = S.render(None, cam[None], H, W, verts=verts, faces=[[3, 4, 5], [0, 1, 2], [0, 1, 2], [1, 2, 0]])
    idx = r["index"][0]
    assert idx[1, 2] == 1 and set(np.unique(idx)) == {-1, 0, 1}
    assert r["second"][0, 1, 2] == r["depth"][0, 1, 2]          # the duplicate is the runner-up at the same depth


def test_hidden_segment_follows_hidden_alpha():
    W, H = 16, 12
    cam = _front_cam(W, H)
    verts = _tri_scene(W, H, cam)
    line = np.array([[_at(cam, 1.0, 4.0, 3.0), _at(cam, 14.0, 4.0, 3.0)]])          # behind the far triangle at z = 2
    for alpha in (0.0, 0.25, 1.0):
        r = S.render(line, cam[None], H, W, verts=verts, faces=[[0, 1, 2]], hidden_alpha=alpha, width=1.0)
        assert r["cov"][0, 4, 6] == np.float32(alpha) and r["cov"][0, 4, 1] == 1.0          # x = 1 is outside the triangle
    shade = int(np.floor(255 * 0.8 * 0.75 + 0.5))
    r = S.render(line, cam[None], H, W, verts=verts, faces=[[0, 1, 2]], hidden_alpha=0.25, width=1.0)
    assert (r["rgb"][0, 4, 6] == shade).all()


def test_near_plane_rules():
    W, H = 16, 12
    cam = _front_cam(W, H)
    a, b = _at(cam, 3.0, 5.0, 2.0), [0.0, 0.0, -1.0]
    assert S.clip_segment(cam, [b, [0.1, 0.0, 0.01]], 0.05) is None               # both ends behind
    assert S.clip_segment(cam, [a, [np.nan, 0, 1]], 0.05) is None
    seg = S.clip_segment(cam, [a, b], 0.05)
    assert seg[5] == 0.05 and seg[2] == 2.0
    seg = S.clip_segment(cam, [a, [0.0, 0.0, 0.05]], 0.05)                         # exactly at the plane: kept as it is
    assert seg[5] == 0.05 and (seg[3], seg[4]) == ((W - 1) / 2, (H - 1) / 2)
    verts = np.array([_at(cam, 2.0, 1.0, 2.0), _at(cam, 12.0, 2.0, 2.0), [0.0, 0.0, 0.01]])
    assert (S.render(None, cam[None], H, W, verts=verts, faces=[[0, 1, 2]])["index"] == -1).all()      # a vertex behind drops the triangle


def test_header_and_binding_name_the_same_show_entries():
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(neat_show_[a-z0-9_]+)\s*\(", text)))
    bound = sorted(n for n in _lib.exported_symbols() if n.startswith("neat_show_"))
    assert declared == bound
    assert set(bound) == {"neat_show_ws_bytes", "neat_show_ws_layout", "neat_show_clear", "neat_show_mesh", "neat_show_lines", "neat_show_points",
                          "neat_show_resolve"}
    assert _lib.ABI_VERSION == 15


def test_bad_arguments_are_rejected_on_the_host():
    """Every check below returns before a launch, so it runs without a device."""
    import ctypes
    lib = _lib.lib()
    assert lib.neat_abi_version() == 15
    assert lib.neat_show_ws_bytes(0, 4, 4) == 0 and lib.neat_show_ws_bytes(1, 0, 4) == 0 and lib.neat_show_ws_bytes(1, 4, -1) == 0
    assert lib.neat_show_ws_bytes(1, 40000, 4) == 0
    n = 3 * 80 * 96
    offs = (ctypes.c_size_t * 4)()
    assert lib.neat_show_ws_layout(3, 80, 96, offs) == 0
    assert offs[0] == 0 and offs[1] >= 8 * n and offs[2] >= offs[1] + 4 * n and offs[3] >= offs[2] + 4 * n
    assert all(o % 256 == 0 for o in offs) and lib.neat_show_ws_bytes(3, 80, 96) >= offs[3] + 4
    assert lib.neat_show_ws_layout(0, 80, 96, offs) == -1 and lib.neat_show_ws_layout(3, 80, 96, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    colors = (ctypes.c_double * 12)(*([0.5] * 12))
    assert lib.neat_show_clear(None, 1, 4, 4, None) == -1 and lib.neat_show_clear(p, 0, 4, 4, None) == -1
    assert lib.neat_show_mesh(p, 3, p, 1, None, 1, 4, 4, 0.05, p, None) == -1          # no cameras
    assert lib.neat_show_mesh(p, 3, p, 1, p, 1, 4, 4, 0.0, p, None) == -1           # near must be positive
    assert lib.neat_show_mesh(None, 3, p, 1, p, 1, 4, 4, 0.05, p, None) == -1
    assert lib.neat_show_mesh(p, 3, p, -1, p, 1, 4, 4, 0.05, p, None) == -1
    assert lib.neat_show_lines(p, 1, p, 1, 4, 4, 0.05, -1.0, 0.01, 0.0, p, None) == -1       # a negative width
    assert lib.neat_show_lines(p, 1, p, 1, 4, 4, 0.05, 1.5, 0.01, 1.5, p, None) == -1        # hidden_alpha outside [0, 1]
    assert lib.neat_show_lines(None, 1, p, 1, 4, 4, 0.05, 1.5, 0.01, 0.0, p, None) == -1
    assert lib.neat_show_lines(p, 1, p, 1, 4, 4, 0.05, 1.5, 0.01, 0.0, None, None) == -1
    assert lib.neat_show_lines(p, 1, p, 0, 4, 4, 0.05, 1.5, 0.01, 0.0, p, None) == -1
    assert lib.neat_show_points(p, 1, p, 1, 4, 4, 0.05, -0.5, 0.01, 0.0, p, None) == -1      # a negative radius
    assert lib.neat_show_points(p, -1, p, 1, 4, 4, 0.05, 2.5, 0.01, 0.0, p, None) == -1
    assert lib.neat_show_resolve(None, 0, None, 0, p, 1, 4, 4, colors, p, None, None) == -1   # no output
    assert lib.neat_show_resolve(None, 0, None, 0, p, 1, 4, 4, None, p, p, None) == -1
    assert lib.neat_show_resolve(None, 0, None, 0, p, 1, 4, 4, colors, p, ctypes.c_void_p(p.value + 1), None) == -1
    colors[4] = 1.5
    assert lib.neat_show_resolve(None, 0, None, 0, p, 1, 4, 4, colors, p, p, None) == -1
