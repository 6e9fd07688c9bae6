"""neat_amd.show on the device against its numpy float64 restatement (tests/show_f64.py).

Bounds.  Every operation of the picture is one IEEE float64 operation on both sides and in the same order, so only a square root or a
quotient may differ in its last place before the value is rounded to float32: the float32 coverage is compared within 4 ulp, and the set
of covered pixels (coverage > 0) must be the same.  The winning triangle and the float32 depth are compared bit for bit, leaving out
pixels where the restatement's two best keys lie within 2 float32 ulp of depth or where an edge function of the winner is within
1e-9 |A| of zero; the restatement alone must leave out at most 0.5 % of its covered pixels.  Bytes are compared exactly, except where the
restatement's 255 rgb + 0.5 lies within 1e-6 of an integer (one level allowed there; at most 0.1 % of the pixels)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from neat_amd import _lib, run_io, show
from tests import show_f64 as S
from tests import show_scenes as Z

pytestmark = pytest.mark.gpu

W0, H0 = 96, 80          # a multiple of neither 64 nor 16
FRAMES = [(96, 80), (1, 1), (17, 1), (1, 70)]          # (W, H)


def _cams(W, H, F):
    """F frames of the dtu orbit, 40 degrees apart."""
    return show.orbit(*show.POSES["dtu"], frames=F, step=40.0), show.intrinsics(W, H, 60.0)


def _front(W, H):
    K = np.array([[128.0, 0, (W - 1) / 2], [0, 128.0, (H - 1) / 2], [0, 0, 1.0]])
    return np.eye(4)[None], K


def _at(K, x, y, z):
    return [(x - K[0, 2]) * z / K[0, 0], (y - K[1, 2]) * z / K[1, 1], z]


def _ulps(a, b):
    """Distance in float32 places between non-negative float32 arrays."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _run(lines, w2c, K, W, H, mesh=None, points=None, **style):
    out, buf = show.render(lines, w2c, K, W, H, mesh=mesh, points=points, return_buffers=True, **style)
    torch.cuda.synchronize()
    return {"rgb": out.cpu().numpy(), "cov": buf.cov.cpu().numpy(), "covp": buf.covp.cpu().numpy(), "depth": buf.depth.cpu().numpy(),
            "index": buf.index.cpu().numpy()}


def _ref(lines, w2c, K, W, H, mesh=None, points=None, **style):
    names = {"line_width": "width", "point_radius": "radius", "depth_bias": "bias"}
    st = {names.get(k, k): v for k, v in style.items()}
    verts, faces = mesh if mesh is not None else (None, None)
    return S.render(lines, show.pack_cameras(w2c, K), H, W, verts=verts, faces=faces, points=points, **st)


def _check_cov(got, want, what):
    worst = int(_ulps(got, want).max()) if got.size else 0
    print("%s: worst coverage difference %d ulp, %d covered pixels" % (what, worst, int((want > 0).sum())))
    assert np.array_equal(got > 0, want > 0), what
    assert worst <= 4, (what, worst)


def _check_bytes(got, ref, what, most=None):
    """most: the largest share of pixels the restatement may have within 1e-6 of a rounding step (asserted for the composite frames; a
    coverage of exactly one half, as beside an axis-aligned segment, lands on a step by construction and is computed exactly)."""
    near = np.abs(ref["pre"] - np.rint(ref["pre"])) < 1e-6
    frac = float(near.any(-1).mean())
    diff = np.abs(got.astype(np.int64) - ref["rgb"].astype(np.int64))
    print("%s: %.4f %% of the pixels within 1e-6 of a rounding step, %d bytes differ" % (what, 100 * frac, int((diff > 0).sum())))
    assert most is None or frac <= most, (what, frac)
    assert (diff[~near] == 0).all() and (diff[near] <= 1).all(), what


# ------------------------------------------------------------------ lines alone
@pytest.mark.parametrize("n,width,F", [(0, 1.5, 1), (1, 1.0, 1), (63, 1.5, 3), (64, 6.0, 1), (65, 1.0, 3), (257, 1.5, 1)])
def test_random_segments(n, width, F):
    w2c, K = _cams(W0, H0, F)
    lines = Z.random_segments(np.random.default_rng(100 + n), n, w2c[0], K, W0, H0)
    got = _run(lines, w2c, K, W0, H0, line_width=width)
    ref = _ref(lines, w2c, K, W0, H0, line_width=width)
    assert got["cov"].shape == (F, H0, W0)
    _check_cov(got["cov"], ref["cov"], "segments n=%d w=%g F=%d" % (n, width, F))
    assert n == 0 or (ref["cov"] > 0).reshape(F, -1).any(1).all()
    assert np.isinf(got["depth"]).all() and (got["index"] == -1).all() and (got["covp"] == 0).all()
    _check_bytes(got["rgb"], ref, "segments n=%d" % n)


def _fixed_segments(K, W, H):
    nan = float("nan")
    return np.array([
        [_at(K, 10.0, 7.0, 2.0), _at(K, 10.0, 7.0, 2.0)],                          # zero length
        [_at(K, 3.0, 12.0, 2.0), _at(K, 60.0, 12.0, 2.5)],                         # horizontal, integer row
        [_at(K, 20.0, 3.0, 2.0), _at(K, 20.0, 70.0, 1.5)],                         # vertical, integer column
        [_at(K, 5.5, 30.5, 2.0), _at(K, 80.5, 30.5, 2.0)],                         # horizontal, half-integer
        [_at(K, 40.5, 2.5, 3.0), _at(K, 40.5, 75.5, 3.0)],                         # vertical, half-integer
        [_at(K, 0.0, 0.0, 2.0), _at(K, W - 1.0, H - 1.0, 2.0)],                    # the full diagonal
        [_at(K, -0.5, H - 0.5, 2.0), _at(K, W - 0.5, -0.5, 4.0)],                  # the other one, corner to corner of the frame's edge
        [_at(K, -300.0, -40.0, 2.0), _at(K, -30.0, -200.0, 2.0)],                  # wholly off-screen
        [_at(K, 70.0, 60.0, 2.0), [0.3, 0.2, -1.0]],                               # one end behind the near plane
        [[0.1, 0.1, 0.01], [0.2, -0.1, -2.0]],                                     # both ends behind
        [_at(K, 30.0, 50.0, 1.0), _at(K, 50.0, 66.0, 0.05)],                       # an end exactly at z = near
        [_at(K, 30.0, 20.0, 2.0), [nan, 0.0, 2.0]],                                # a NaN endpoint
        [[0.0, 0.0, np.inf], _at(K, 30.0, 20.0, 2.0)],
    ], dtype=np.float64)


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("width", [1.0, 1.5, 6.0])
def test_fixed_segments(W, H, width):
    w2c, K = _front(W0, H0)              # the same camera for every frame size: the small frames are corners of the large one
    lines = _fixed_segments(K, W0, H0)
    if (W, H) != (W0, H0):               # bring something onto the tiny frames
        lines = np.concatenate([lines, [[_at(K, -3.0, -2.0, 2.0), _at(K, 9.0, 40.0, 2.0)], [_at(K, 0.0, 0.0, 2.0), _at(K, 0.0, 0.0, 3.0)]]])
    got = _run(lines, w2c, K, W, H, line_width=width)
    ref = _ref(lines, w2c, K, W, H, line_width=width)
    _check_cov(got["cov"], ref["cov"], "fixed segments %dx%d w=%g" % (W, H, width))
    assert (ref["cov"] > 0).any()
    _check_bytes(got["rgb"], ref, "fixed segments")
    # each dropped segment alone leaves the frame empty; the cut ones draw
    if (W, H) == (W0, H0):
        for k, drawn in ((7, False), (8, True), (9, False), (10, True), (11, False), (12, False)):
            one = _run(lines[k:k + 1], w2c, K, W, H, line_width=width)["cov"]
            assert bool((one > 0).any()) == drawn, k
            assert np.array_equal(one > 0, _ref(lines[k:k + 1], w2c, K, W, H, line_width=width)["cov"] > 0), k


def test_points():
    w2c, K = _cams(W0, H0, 3)
    lines = Z.random_segments(np.random.default_rng(5), 40, w2c[0], K, W0, H0)
    pts = show.endpoints(lines)
    assert pts.shape == (80, 3)
    for radius in (0.0, 2.5):
        got = _run(lines, w2c, K, W0, H0, points=pts, point_radius=radius, show_lines=False)
        ref = _ref(None, w2c, K, W0, H0, points=pts, point_radius=radius)
        _check_cov(got["covp"], ref["covp"], "points r=%g" % radius)
        assert (got["cov"] == 0).all() and (ref["covp"] > 0).any()
        _check_bytes(got["rgb"], ref, "points")


# ------------------------------------------------------------------ mesh alone
def _fixed_triangles(K):
    """-> verts, faces: a degenerate one, the two windings, one larger than the frame (behind everything), sub-pixel ones that hold no pixel
    centre, one across the near plane."""
    v = [_at(K, 10.0, 10.0, 2.0), _at(K, 20.0, 15.0, 2.0), _at(K, 30.0, 20.0, 2.0),                    # collinear: A = 0
         _at(K, 50.0, 5.0, 2.0), _at(K, 70.0, 9.0, 2.2), _at(K, 55.0, 25.0, 1.8),                     # wound one way ...
         _at(K, 50.0, 45.0, 2.0), _at(K, 55.0, 65.0, 1.8), _at(K, 70.0, 49.0, 2.2),                   # ... and the other
         _at(K, -400.0, -300.0, 6.0), _at(K, 700.0, -250.0, 6.5), _at(K, 100.0, 900.0, 7.0),          # larger than the frame
         _at(K, 5.2, 60.2, 2.0), _at(K, 5.7, 60.3, 2.0), _at(K, 5.4, 60.8, 2.0),                      # sub-pixel, no centre inside
         _at(K, 8.1, 70.6, 2.0), _at(K, 8.9, 70.7, 2.0), _at(K, 8.5, 70.9, 2.0),
         _at(K, 30.0, 60.0, 2.0), _at(K, 40.0, 70.0, 2.0), [0.0, 0.1, 0.01]]                           # a vertex behind the near plane
    return np.array(v, dtype=np.float64), np.arange(21, dtype=np.int32).reshape(7, 3)


def _check_mesh(got, ref, what):
    covered = ref["index"] >= 0
    tie = covered & (_ulps(np.where(covered, ref["depth"], 0), np.where(np.isfinite(ref["second"]), ref["second"], 0)) <= 2) \
        & np.isfinite(ref["second"])
    edge = covered & (ref["edge_margin"] < 1e-9)
    out = tie | edge
    frac = float(out.sum()) / max(int(covered.sum()), 1)
    print("%s: %d covered pixels, %d left out (%.3f %%)" % (what, int(covered.sum()), int(out.sum()), 100 * frac))
    assert frac <= 5e-3, (what, frac)
    keep = ~out
    assert np.array_equal(got["index"][keep], ref["index"][keep]), what
    assert np.array_equal(got["depth"][keep].view(np.int32), ref["depth"][keep].view(np.int32)), what


@pytest.mark.parametrize("n,F", [(0, 1), (1, 1), (255, 3), (257, 1)])
def test_random_triangles(n, F):
    w2c, K = _cams(W0, H0, F)
    verts, faces = Z.random_triangles(np.random.default_rng(200 + n), n, w2c[0], K, W0, H0, margin=10.0 if n > 1 else -30.0)      # one: inside
    got = _run(None, w2c, K, W0, H0, mesh=(verts, faces))
    ref = _ref(None, w2c, K, W0, H0, mesh=(verts, faces))
    _check_mesh(got, ref, "triangles n=%d F=%d" % (n, F))
    assert n == 0 or (ref["index"] >= 0).any()
    if n:
        _check_bytes(got["rgb"], ref, "triangles n=%d" % n)


@pytest.mark.parametrize("W,H", FRAMES)
def test_fixed_triangles(W, H):
    w2c, K = _front(W0, H0)
    verts, faces = _fixed_triangles(K)
    got = _run(None, w2c, K, W, H, mesh=(verts, faces))
    ref = _ref(None, w2c, K, W, H, mesh=(verts, faces))
    _check_mesh(got, ref, "fixed triangles %dx%d" % (W, H))
    drawn = set(np.unique(ref["index"]).tolist())
    assert (got["index"] >= 0).all() and drawn <= {1, 2, 3}          # the large triangle lies behind every pixel; 0, 4, 5, 6 draw nothing
    if (W, H) == (W0, H0):
        assert drawn == {1, 2, 3}
        assert int((got["index"] == 1).sum()) == int((got["index"] == 2).sum()) > 100          # the two windings, mirror images


def test_more_large_triangles_than_the_queue_holds():
    """Large boxes (over 32 pixels) are queued for a second launch; the queue holds 2^20 of them and the rest are walked by the first
    launch.  24 large triangles repeated 15 000 times over 3 frames are 1.08 million boxes: both paths run.  A repeated triangle has the
    depth of its first copy bit for bit, so the lowest index wins and the picture is that of the 24 alone."""
    w2c, K = _cams(W0, H0, 3)
    verts, faces = Z.random_triangles(np.random.default_rng(31), 24, w2c[0], K, W0, H0, size=9.0, margin=-10.0)
    ref = _ref(None, w2c, K, W0, H0, mesh=(verts, faces))
    assert int((ref["index"] >= 0).sum()) > 1000
    got = _run(None, w2c, K, W0, H0, mesh=(verts, np.tile(faces, (15000, 1))))
    assert 3 * 15000 * 24 > 2 ** 20 and got["index"].max() < 24
    _check_mesh(got, ref, "repeated large triangles")


def test_coplanar_duplicates_go_to_the_lower_index():
    w2c, K = _front(W0, H0)
    v = np.array([_at(K, 10.0, 10.0, 2.0), _at(K, 80.0, 20.0, 3.0), _at(K, 30.0, 70.0, 2.5)])
    for faces, first in (([[0, 1, 2], [0, 1, 2]], 0), ([[1, 2, 0], [0, 1, 2], [0, 1, 2]], 0)):
        got = _run(None, w2c, K, W0, H0, mesh=(v, np.array(faces, dtype=np.int32)))
        ref = _ref(None, w2c, K, W0, H0, mesh=(v, np.array(faces, dtype=np.int32)))
        same_order = got["index"][(got["index"] >= 0)]
        assert same_order.size > 500
        if len(faces) == 2:
            assert (same_order == first).all()
            assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["depth"].view(np.int32), ref["depth"].view(np.int32))
        else:                   # a rotated vertex order may round a depth differently: only the exact duplicates 1 and 2 are ordered
            assert not (same_order == 2).any()


# ------------------------------------------------------------------ hidden lines
WC, HC = 128, 96


def _cube_view():
    verts, faces, edges = Z.cube()
    w2c, K = show.orbit(*show.POSES["dtu"], frames=1, step=5.0), show.intrinsics(WC, HC, 60.0)
    cam = show.pack_cameras(w2c, K)[0]
    zc = S.to_cam(cam, verts)[:, 2]
    far = verts[np.argmax(zc)]
    is_far = np.array([bool((e == far).all(1).any()) for e in edges])
    mid = edges.mean(1)
    x, y, _ = S.project(cam, S.to_cam(cam, mid))
    return verts, faces, edges, w2c, K, cam, is_far, np.rint(x).astype(int), np.rint(y).astype(int)


def test_hidden_lines_of_a_cube():
    verts, faces, edges, w2c, K, cam, is_far, mx, my = _cube_view()
    assert int(is_far.sum()) == 3
    line_color, mesh_color = (1.0, 0.0, 0.0), (0.8, 0.8, 0.8)
    # width 3: the pixel nearest a midpoint is at most 0.71 from the line, inside the full-coverage core of hw - 1 = 1.  The bias is a
    # fifth of the smallest depth gap between a far edge's midpoint and the face in front of it (> 0.25 for the unit cube at this pose)
    style = dict(line_width=3.0, depth_bias=0.05, line_color=line_color, mesh_color=mesh_color)
    for alpha in (0.0, 1.0, 0.25):
        got = _run(edges, w2c, K, WC, HC, mesh=(verts, faces), hidden_alpha=alpha, **style)
        ref = _ref(edges, w2c, K, WC, HC, mesh=(verts, faces), hidden_alpha=alpha, **style)
        _check_cov(got["cov"], ref["cov"], "cube alpha=%g" % alpha)
        _check_bytes(got["rgb"], ref, "cube alpha=%g" % alpha)
        for e in range(12):
            px = got["rgb"][0, my[e], mx[e]].astype(int)
            k = got["index"][0, my[e], mx[e]]
            line = np.floor(255.0 * np.array(line_color) + 0.5).astype(int)
            if not is_far[e] or alpha == 1.0:
                assert (px == line).all(), (alpha, e, px)
            else:
                assert k >= 0, e
                base = np.array(mesh_color) * S.shade(cam, verts, faces[k])
                want = np.floor(255.0 * (base * (1.0 - np.float32(alpha)) + np.array(line_color) * np.float64(np.float32(alpha))) + 0.5).astype(int)
                assert (px == want).all(), (alpha, e, px, want)
                if alpha == 0.0:
                    assert (px == np.floor(255.0 * base + 0.5).astype(int)).all()


# ------------------------------------------------------------------ everything together
def test_composite_frames():
    w2c, K = _cams(W0, H0, 3)
    rng = np.random.default_rng(7)
    lines = np.concatenate([Z.random_segments(rng, 200, w2c[0], K, W0, H0), Z.cube()[2]])
    verts, faces, _ = Z.cube()
    pts = show.endpoints(lines[-12:])
    style = dict(line_width=1.5, hidden_alpha=0.3, bg=(0.92, 0.95, 1.0), line_color=(0.12, 0.0, 0.22), point_color=(0.0, 0.45, 1.0),
                 mesh_color=(0.7, 0.8, 0.6))
    got = _run(lines, w2c, K, W0, H0, mesh=(verts, faces), points=pts, **style)
    ref = _ref(lines, w2c, K, W0, H0, mesh=(verts, faces), points=pts, **style)
    _check_mesh(got, ref, "composite")
    _check_cov(got["cov"], ref["cov"], "composite lines")
    _check_cov(got["covp"], ref["covp"], "composite points")
    _check_bytes(got["rgb"], ref, "composite", most=1e-3)
    assert len(np.unique(got["rgb"].reshape(-1, 3), axis=0)) > 50


def test_order_independence():
    w2c, K = _cams(W0, H0, 3)
    rng = np.random.default_rng(11)
    lines = Z.random_segments(rng, 129, w2c[0], K, W0, H0)
    verts, faces = Z.random_triangles(rng, 130, w2c[0], K, W0, H0)
    a = _run(lines, w2c, K, W0, H0, mesh=(verts, faces), hidden_alpha=0.5)
    pl, pf = rng.permutation(len(lines)), rng.permutation(len(faces))
    b = _run(lines[pl], w2c, K, W0, H0, mesh=(verts, faces[pf]), hidden_alpha=0.5)
    assert np.array_equal(a["depth"].view(np.int32), b["depth"].view(np.int32))
    assert np.array_equal(a["cov"].view(np.int32), b["cov"].view(np.int32))
    hit = b["index"] >= 0
    assert np.array_equal(hit, a["index"] >= 0) and hit.any()
    # index k of the permuted call is triangle pf[k] of the first.  Where two different triangles round to the same float32 depth the
    # lower index of each call wins, which the permutation changes: those pixels (found by the restatement) are compared by depth alone
    ref = _ref(None, w2c, K, W0, H0, mesh=(verts, faces))
    tied = (ref["index"] >= 0) & (ref["second"].view(np.int32) == ref["depth"].view(np.int32))
    assert tied.mean() < 5e-3
    mapped = np.where(hit, pf[np.where(hit, b["index"], 0)], -1)
    assert np.array_equal(mapped[~tied], a["index"][~tied])
    # and the same call twice is the same bits
    c = _run(lines, w2c, K, W0, H0, mesh=(verts, faces), hidden_alpha=0.5)
    assert all(np.array_equal(a[k], c[k]) for k in ("rgb", "index")) and np.array_equal(a["cov"].view(np.int32), c["cov"].view(np.int32))


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    F, H, W = 1, 8, 8
    buf = show.Buffers(F, H, W, dev)
    w2c, K = _front(W, H)
    cams = torch.tensor(show.pack_cameras(w2c, K), device=dev)
    lines = torch.zeros(2, 6, device=dev, dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.neat_show_clear(p(buf.ws), F, H, W, s) == 0
    torch.cuda.synchronize()
    before = buf.ws.clone()
    assert lib.neat_show_lines(p(lines), 2, p(cams), 0, H, W, 0.05, 1.5, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_lines(p(lines), 2, p(cams), F, 0, W, 0.05, 1.5, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_lines(p(lines), 2, p(cams), F, H, -3, 0.05, 1.5, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_lines(None, 2, p(cams), F, H, W, 0.05, 1.5, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_lines(p(lines), 2, None, F, H, W, 0.05, 1.5, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_lines(p(lines), 2, p(cams), F, H, W, 0.05, -1.0, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_points(p(lines), 2, p(cams), F, H, W, 0.05, -0.1, 0.01, 0.0, p(buf.ws), s) == -1
    assert lib.neat_show_mesh(None, 3, p(lines), 1, p(cams), F, H, W, 0.05, p(buf.ws), s) == -1
    torch.cuda.synchronize()
    assert torch.equal(before, buf.ws)


def test_face_index_out_of_range():
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    w2c, K = _front(W0, H0)
    verts, faces = _fixed_triangles(K)
    bad = faces.copy()
    bad[2, 1] = len(verts)
    with pytest.raises(RuntimeError, match="face index"):
        show.render(None, w2c, K, W0, H0, mesh=(verts, bad))
    bad[2, 1] = -1
    with pytest.raises(RuntimeError, match="face index"):
        show.render(None, w2c, K, W0, H0, mesh=(verts, bad))
    # the output stays as it was
    F, H, W = 1, H0, W0
    buf = show.Buffers(F, H, W, dev)
    cams = torch.tensor(show.pack_cameras(w2c, K), device=dev)
    v, f = torch.tensor(verts, device=dev), torch.tensor(bad, device=dev)
    out = torch.full((F, H, W, 3), 7, device=dev, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    colors = (ctypes.c_double * 12)(*([0.5] * 12))
    assert lib.neat_show_clear(p(buf.ws), F, H, W, s) == 0
    assert lib.neat_show_mesh(p(v), len(verts), p(f), len(bad), p(cams), F, H, W, 0.05, p(buf.ws), s) == 0
    assert lib.neat_show_resolve(p(v), len(verts), p(f), len(bad), p(cams), F, H, W, colors, p(buf.ws), p(out), s) == 0
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 1 and bool((out == 7).all())
    # a clear and a good mesh afterwards draw
    good = torch.tensor(faces, device=dev)
    assert lib.neat_show_clear(p(buf.ws), F, H, W, s) == 0
    assert lib.neat_show_mesh(p(v), len(verts), p(good), len(faces), p(cams), F, H, W, 0.05, p(buf.ws), s) == 0
    assert lib.neat_show_resolve(p(v), len(verts), p(good), len(faces), p(cams), F, H, W, colors, p(buf.ws), p(out), s) == 0
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0 and not bool((out == 7).all())


# ------------------------------------------------------------------ the command line
def test_cli_end_to_end(tmp_path, capsys):
    from PIL import Image
    from neat_amd.ply import write_ply
    verts, faces, edges = Z.cube()
    run = tmp_path / "run" / "wireframes"
    run.mkdir(parents=True)
    data, ply = str(run / "cube-wfi_checked.npz"), str(tmp_path / "surface_2000.ply")
    np.savez(data, lines3d=edges.astype(np.float32))
    write_ply(ply, verts.astype(np.float32), faces)
    argv = ["--data", data, "--mesh", ply, "--pose", "dtu", "--frames", "4", "--step", "90", "--width", "128", "--height", "96", "--show-points"]
    assert show.main(argv) == 0
    text = capsys.readouterr().out
    assert "device rendering" in text and "encoding" in text and "12 segments, 12 triangles, 4 frames" in text
    out = os.path.join(str(run), "..", "video")
    w2c = show.orbit(*show.POSES["dtu"], frames=4, step=90.0)
    lines = run_io.load_lines(data)[0]
    want = show.render(lines, w2c, show.intrinsics(128, 96, 60.0), 128, 96, mesh=(verts.astype(np.float32), faces),
                       points=show.endpoints(lines)).cpu().numpy()
    assert want.shape == (4, 96, 128, 3) and len(np.unique(want.reshape(-1, 3), axis=0)) > 10
    for k in range(4):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%04d.png" % k)).convert("RGB")), want[k]), k
    assert not np.array_equal(want[0], want[1])
    assert Image.open(out + ".gif").n_frames == 4
    with open(os.path.join(out, "cam.json")) as fh:
        assert np.array_equal(np.asarray(json.load(fh)), w2c)
    again = str(tmp_path / "again")
    assert show.main(["--data", data, "--mesh", ply, "--cam-json", os.path.join(out, "cam.json"), "--width", "128", "--height", "96",
                      "--show-points", "--save-path", again, "--name", "fixed", "--no-gif"]) == 0
    for k in range(4):
        assert np.array_equal(np.asarray(Image.open(os.path.join(again, "fixed", "%04d.png" % k)).convert("RGB")), want[k]), k
    assert not os.path.exists(os.path.join(again, "fixed.gif"))
