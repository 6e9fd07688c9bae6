"""The closed loop on the host: the float64 restatements chained (scenegen_f64 -> detect_f64 -> triangulate_f64, oracle.camera_rays,
oracle/attraction_oracle.py) and held to the analytic truth of tests/closed_loop.py, with the bars that tests/test_closed_loop_gpu.py
holds the device to.  No GPU.  It shows that the scenes sit inside every bar before a kernel is involved, that the half-pixel mistakes
fall outside them, and that the truth agrees with itself.

Settings: scenegen.cameras(12, 128), ss = 3, shapes through scenegen.normalise, detector scale 1, defaults elsewhere.  What the float64
side measures (box, L-block; the assertions below re-measure every row):

    quantity                                                      measured                    bar          the half-pixel mistake
    runs: p2 against the written-out projection of p3             2.8e-14 px on both          1e-9 px
    runs: p3 off its edge                                         0 on both                   1e-12
    oracle.camera_rays of a pixel, projected back (float32)       at most 2.1e-5 px           2.4e-4 px    0.5 px
    oracle.project2d of the runs' p3 against p2 (float32)         at most 9.2e-6 px           2.4e-4 px
    pixel-centre rays: depth against the slab form (box)          1.3e-15                     4.8e-7
    pixels with a partial sub-sample count (view 3)               1.3 % and 1.5 %             3 %          (a full pixel misses)
    attraction field: foot points off their runs                  5.3e-6 and 4.7e-6 px        1e-3 px      0.5 px
    the field's segment: its distance over the nearest run's      0 on both                   1e-4 px
    rays with two runs within 1e-4 px of each other               5.9 % and 7.3 %             (none is left out, see check_attraction)
    detected segments: midpoint to nearest projected edge         0.457 and 0.225 px          0.5 px       0.79 and 0.72 px
    detected segments: mean offset, each component                0.0097 and 0.0034 px        0.25 px      0.29 and 0.27 px
    detected segments: solved shift, each component               0.022 and 0.0072 px         0.25 px      0.48 and 0.49 px
    detection: judged regions                                     1 of 79 and 0 of 118        1 % of 197
    triangulation from the runs: lines, edges covered over 80 %   12, 12 of 12 and 17, 17 of 18
    the same: end points off the nearest edge's infinite line     8.1e-7 and 2.7e-7           1e-4         1.1e-2 and 1.2e-2
    triangulation from the detections: lines                      4 and 10                    positive
    the same: end points off the nearest edge's infinite line     6.4e-4 and 1.2e-2           recorded
    closest_f64 against the box's closed form, 257 points         1.11e-16                    1.2e-16 (the device: 4 x)

Every measured value goes through tests/f64_table.record, so NEAT_F64_TABLE lists it."""
import numpy as np
import pytest
import torch

from tests import closed_loop as C
from tests.f64_table import record, write_table  # noqa: F401  (write_table: the NEAT_F64_TABLE writer, autouse)

BUILD = "closed_loop_f64"
DISTANCE = 10.0                      # BlenderDataset's distance_threshold
CAMERA_VIEWS = (0, 5, 11)


def rec(name, P):
    return lambda entry, err: record(BUILD, f"{name}:{entry}", P, err)


def oracle_rays(sc, v, uv):
    """oracle.camera_rays in float32 -> (origin [3], dirs [n,3]) as float64 values."""
    from oracle import neat_oracle as O
    K = torch.from_numpy(sc["K"][v].astype(np.float32))[None]
    pose = torch.from_numpy(sc["poses"][v].astype(np.float32))[None]
    d, o = O.camera_rays(torch.from_numpy(np.asarray(uv, np.float32))[None], pose, K)
    return o[0].numpy().astype(np.float64), d[0].numpy().astype(np.float64)


# ---- the truth against itself -----------------------------------------------------------------------------------------------------
def test_a_pixels_ray_projects_back_to_the_pixel():
    sc = C.scene("box")
    rng = np.random.default_rng(0)
    uv = np.concatenate([C.camera_pixels(sc["K"][0], 256, 0), rng.uniform(-0.5, C.RES - 0.5, (256, 2))])
    for v in range(C.VIEWS):
        o, d = C.pixel_ray(sc["K"][v], sc["poses"][v], uv)
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-14
        for t in (0.5, 2.0, 5.0):
            back, depth = C.project(sc["K"][v], sc["poses"][v], o + t * d)
            assert np.abs(back - uv).max() < 1e-9 and (depth > 0).all()
        # the cameras look at the origin: it is seen at the principal point, from the radius
        centre, depth = C.project(sc["K"][v], sc["poses"][v], np.zeros(3))
        assert np.abs(centre - C.RES / 2.0).max() < 1e-5 and abs(depth - 2.0) < 1e-6


def test_the_box_distance_equals_brute_force_over_its_triangles():
    from tests import closest_f64 as Q
    sc = C.scene("box")
    pts = C.closest_points(sc["h"])
    want = C.box_sdf(pts, sc["h"])
    assert pts.shape == (257, 3) and (want < 0).sum() >= 40 and (want > 0).sum() >= 100 and (want[-17:] == 0).all()
    d2, tri, q, _ = Q.closest_all(sc["verts"], sc["faces"], pts)
    err = record(BUILD, "box:closest", 257, np.abs(np.sqrt(d2) - np.abs(want)).max())
    assert err <= C.CLOSEST_F64, err
    assert np.abs(C.box_sdf(q, sc["h"])).max() <= C.CLOSEST_F64            # the closest point lies on the surface
    # the slab form: a ray towards a point inside ends on the surface before it; the ray away from the box misses; from inside it leaves
    o, inside = np.array([1.5, -1.0, 0.75]), pts[200:240]
    d = (inside - o) / np.linalg.norm(inside - o, axis=1, keepdims=True)
    t = C.box_slab(o, d, sc["h"])
    assert np.abs(C.box_sdf(o + t[:, None] * d, sc["h"])).max() < 1e-15 and (t < np.linalg.norm(inside - o, axis=1)).all() and (t > 0).all()
    assert np.isinf(C.box_slab(o, -d, sc["h"])).all()
    t = C.box_slab(inside, d, sc["h"])
    assert np.abs(C.box_sdf(inside + t[:, None] * d, sc["h"])).max() < 1e-15 and (t > 0).all()
    # distances: a point's foot on a segment and on its line
    a, b = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0])
    assert C.point_segment(np.array([3.0, 4.0, 0.0]), a, b)[0] == np.hypot(1.0, 4.0) and C.point_line(np.array([3.0, 4.0, 0.0]), a, b) == (4.0, 1.5)
    assert C.point_segment(np.array([1.0, 1.0]), a[:2], b[:2])[0] == 1.0 and C.point_segment(np.array([1.0, 1.0]), a[:2], a[:2])[0] == np.sqrt(2.0)


# ---- the legs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SHAPES)
def test_runs_are_the_projection_of_their_edges(name):
    sc = C.scene(name)
    r = sc["runs"]
    C.check_runs(sc, r["idx"], r["p2"], r["p3"], rec(name, r["idx"].shape[0]))
    assert all(s.shape[0] > 0 for s in sc["segs"])
    with pytest.raises(AssertionError):                                       # runs moved by half a pixel
        C.check_runs(sc, r["idx"], r["p2"] + 0.5, r["p3"], lambda k, e: e)


@pytest.mark.parametrize("R", [256, 257])
@pytest.mark.parametrize("name", C.SHAPES)
def test_training_camera(name, R):
    from oracle import neat_oracle as O
    sc = C.scene(name)
    for v in CAMERA_VIEWS:
        uv = C.camera_pixels(sc["K"][v], R, seed=R + v)
        assert uv.shape == (R, 2)
        o, d = oracle_rays(sc, v, uv)
        err = C.check_camera(sc, v, uv, o, d, rec(name, R), f"camera_rays_v{v}")
        assert err <= C.BAR_CAM, err
        o, d = oracle_rays(sc, v, uv + 0.5)                                   # the pixel-centre mix-up
        assert C.check_camera(sc, v, uv, o, d, lambda k, e: e, "") > 0.49
        p2, p3 = C.view_runs(sc, v)
        pose = sc["poses"][v]
        Rm = torch.from_numpy(pose[:3, :3].T.astype(np.float32))
        T = torch.from_numpy((-pose[:3, :3].T @ pose[:3, 3]).astype(np.float32))[:, None]
        got = O.project2d(torch.from_numpy(sc["K"][v].astype(np.float32)), Rm, T, torch.from_numpy(p3.astype(np.float32)))
        err = record(BUILD, f"{name}:project2d_v{v}", p3.shape[0] * 2, np.abs(got.numpy().astype(np.float64).reshape(-1, 4) - p2).max())
        assert err <= C.BAR_CAM, err


@pytest.mark.parametrize("name", C.SHAPES)
def test_pictures_against_the_training_rays(name):
    from tests import scenegen_f64 as G
    sc = C.scene(name)
    v = 3
    o, d = oracle_rays(sc, v, C.pixel_grid())
    t, _ = G.closest(sc["verts"], sc["faces"], o, d)
    C.check_pictures(sc, v, o, d, t, rec(name, C.RES * C.RES), "pictures")
    share = [1.0 - ((sc["hits"][f] == 0) | (sc["hits"][f] == C.SS ** 2)).mean() for f in range(C.VIEWS)]
    assert 0.005 < min(share) and max(share) <= C.PARTIAL_CAP                  # the silhouette's pixels, in every view
    o, d = oracle_rays(sc, v, C.pixel_grid() + 0.5)                           # the pixel-centre mix-up: a full pixel misses
    with pytest.raises(AssertionError):
        C.check_pictures(sc, v, o, d, G.closest(sc["verts"], sc["faces"], o, d)[0], lambda k, e: e, "")


@pytest.mark.parametrize("name", C.SHAPES)
def test_attraction_field(name):
    sc = C.scene(name)
    for v in sc["attraction_views"]:
        uv, uv_proj, lines2d = C.support_rays(sc, v, DISTANCE)
        assert uv.shape[0] > 1000
        run, ties = C.check_attraction(sc["segs"][v], uv, uv_proj, lines2d, DISTANCE, rec(name, uv.shape[0]), f"attraction_v{v}")
        assert 0.02 < ties < 0.10                                             # the corner sectors beyond the shared junctions: exact ties
        assert np.unique(run).size == sc["segs"][v].shape[0]                   # every run has its support
        # the runs are the truth's edges: a foot point lies on a projected edge as well
        a, b = C.edges_2d(sc["K"][v], sc["poses"][v], sc["junctions"], sc["edges"])
        assert C.point_segment(uv_proj[:, None], a[None], b[None])[0].min(axis=1).max() <= C.BAR_FOOT
        with pytest.raises(AssertionError):                                   # a field laid half a pixel off
            C.check_attraction(sc["segs"][v], uv, uv_proj + 0.5, lines2d, DISTANCE, lambda k, e: e, "")


def test_detections_lie_on_the_projected_edges():
    refs = [C.scene(name)["det"] for name in C.SHAPES]
    for name, det in zip(C.SHAPES, refs):
        sc = C.scene(name)
        C.check_detections(sc, det["lines"], det["offsets"], rec(name, det["lines"].shape[0]))
        with pytest.raises(AssertionError):                                   # detections moved by half a pixel
            C.check_detections(sc, det["lines"] + 0.5, det["offsets"], lambda k, e: e)
        shift = C.check_detections(sc, det["lines"], det["offsets"], lambda k, e: e)[1]
        moved = np.concatenate([C.offsets_to_edges(s + 0.5, sc["K"][v], sc["poses"][v], sc["junctions"], sc["edges"])[0]
                                for v, s in enumerate(sc["det_segs"])])
        assert np.abs(moved.mean(axis=0)).max() > C.BAR_DET_MEAN and np.abs(shift).max() < 0.1 * C.BAR_DET_MEAN
    # the judge cap of tests/test_detect_gpu.compare holds over the closed loop's pictures taken together: one call for both shapes
    both = C.merge_detections(refs)
    assert [int(r["cand_judge"].sum()) for r in refs] == [1, 0]
    assert both["cand_judge"].sum() <= 0.01 * len(both["cand"]) and both["offsets"][-1] == both["lines"].shape[0] == len(both["view"])
    assert both["grey"].shape == (2 * C.VIEWS, C.RES, C.RES) and both["view"].max() == 2 * C.VIEWS - 1


@pytest.mark.parametrize("name", C.SHAPES)
def test_triangulated_lines_lie_on_the_edges(name):
    from tests import triangulate_f64 as T
    sc = C.scene(name)
    lines = sc["tri_runs"]["lines3d"]
    C.check_lines3d(sc, lines, rec(name, lines.shape[0]), "triangulate_runs")
    assert lines.shape[0] == {"box": 12, "lblock": 17}[name]
    moved = T.lines([s + 0.5 for s in sc["segs"]], sc["K"], sc["poses"])["lines3d"]          # runs moved by half a pixel
    assert moved.shape[0] > 0 and C.nearest_edge_line(moved, sc["junctions"], sc["edges"])[1].max() > 50 * C.BAR_TRI
    with pytest.raises(AssertionError):
        C.check_lines3d(sc, moved, lambda k, e: e, "")
    det = sc["tri_det"]["lines3d"]
    assert det.shape[0] == {"box": 4, "lblock": 10}[name]
    record(BUILD, f"{name}:triangulate_detections", det.shape[0], C.nearest_edge_line(det, sc["junctions"], sc["edges"])[1].max())
