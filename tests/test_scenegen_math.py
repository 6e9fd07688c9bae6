"""The float64 restatement of scene generation (tests/scenegen_f64.py) against independent facts: which edges of a convex
box a camera sees, where an occluder cuts an edge, the hull of a box's picture, the brightness of a face-on plane, the cuts at the near
plane and at the border of the picture, and the cameras.  No device is touched; tests/test_scenegen_gpu.py holds the device to these
functions byte for byte."""
import math

import numpy as np

from neat_amd import scenegen
from neat_amd.synth import look_at_pose
from tests import raycast_f64 as rc
from tests import scenegen_f64 as sg

D = scenegen.DEFAULTS


def shape(name, sub=0):
    verts, faces, junctions, edges = scenegen.shapes[name]
    verts, faces = scenegen.subdivide(verts, faces, sub)
    verts, junctions = scenegen.normalise(verts, junctions)
    return verts, faces, junctions, edges


def box_edge_seen(verts, a, b, c):
    """An edge of a convex box is seen from c iff one of its two faces looks at c."""
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    return any((c[k] > hi[k]) if a[k] == hi[k] else (c[k] < lo[k]) for k in range(3) if a[k] == b[k])


def check_box_view(verts, faces, J, E, K, pose, res):
    runs = sg.visible_edges(verts, faces, J, E, K[None], pose[None], res, res, D["step"], D["min_len"], D["bias"], D["near"])
    seen = [j for j, (a, b) in enumerate(E) if box_edge_seen(verts, J[a], J[b], pose[:3, 3])]
    assert runs["idx"][:, 1].tolist() == seen                                   # one run per seen edge, none of a hidden one
    assert runs["junc"].all()
    np.testing.assert_array_equal(runs["p3"][:, 0], J[E[seen, 0]])               # the whole edge, end to end
    np.testing.assert_array_equal(runs["p3"][:, 1], J[E[seen, 1]])
    assert (runs["idx"][:, 2] == 0).all()
    return len(seen)


def test_box_from_a_corner_shows_nine_whole_edges_and_hides_three():
    verts, faces, J, E = shape("box")
    K, _ = scenegen.cameras(1, 128)
    c = 2.0 * np.array([1.0, 0.8, 0.6]) / math.sqrt(2.0)
    assert check_box_view(verts, faces, J, E, K[0], look_at_pose(c).astype(np.float64), 128) == 9
    assert E.shape == (12, 2)


def test_box_edges_in_every_view_of_the_default_spiral():
    """The defaults of bias and min_len hold for all 16 views at 128 pixels: 9 edges from a corner, 7 over an edge, 4 face on."""
    verts, faces, J, E = shape("box")
    K, poses = scenegen.cameras(16, 128)
    seen = [check_box_view(verts, faces, J, E, K[v], poses[v], 128) for v in range(16)]
    assert set(seen) <= {4, 7, 9} and 9 in seen


def test_hidden_box_edges_leave_only_runs_shorter_than_min_len():
    """What min_len removes: next to a silhouette junction a hidden edge's first samples lie less than bias behind the face in front."""
    verts, faces, J, E = shape("box")
    K, poses = scenegen.cameras(16, 128)
    runs = sg.visible_edges(verts, faces, J, E, K, poses, 128, 128, D["step"], 0.0, D["bias"], D["near"], all_runs=True)
    partial = ~runs["junc"].all(axis=1)
    assert partial.any() and runs["length"][partial].max() < D["min_len"] <= runs["length"][~partial].min()


def point_line_distance(p, a, b):
    d = (b - a) / np.linalg.norm(b - a)
    return abs(d[0] * (p[1] - a[1]) - d[1] * (p[0] - a[0]))


def test_lblock_arm_in_front_of_an_edge_cuts_it_at_the_silhouette():
    """From in front of and above the arm along x, the upright edge at the far end of the inner wall is hidden below and seen above: its
    run ends where the arm's upper back edge crosses it in the picture."""
    verts, faces, J, E = shape("lblock")
    K, _ = scenegen.cameras(1, 128)
    pose = look_at_pose((0.3, -2.0, 0.8)).astype(np.float64)
    upright = [j for j, (a, b) in enumerate(E) if {tuple(J[a]), tuple(J[b])} == {(0.0, 0.5, -0.25), (0.0, 0.5, 0.25)}][0]
    runs = sg.visible_edges(verts, faces, J, E, K, pose[None], 128, 128, D["step"], D["min_len"], D["bias"], D["near"])
    mine = np.nonzero(runs["idx"][:, 1] == upright)[0]
    assert len(mine) == 1
    r = mine[0]
    junc, ends = runs["junc"][r], runs["p2"][r].reshape(2, 2)
    assert junc.sum() == 1                                                        # one end is the upper junction, the other a T-junction
    top = runs["p3"][r][list(junc).index(1)]
    assert top[2] == 0.25
    cut = ends[list(junc).index(0)]
    a = np.array(sg.project(K[0], sg.to_camera(pose, np.array([0.0, 0.0, 0.25]))))     # the arm's upper back edge: y = 0, z = 0.25
    b = np.array(sg.project(K[0], sg.to_camera(pose, np.array([0.5, 0.0, 0.25]))))
    assert point_line_distance(cut, a, b) <= D["step"]


def hull(points):
    """Andrew's monotone chain -> the hull's corners, counter-clockwise."""
    pts = sorted(map(tuple, points))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1])


def test_mask_of_the_box_counts_the_sub_samples_inside_the_hull():
    verts, faces, J, E = shape("box")
    H, W, ss = 40, 48, 3
    K = np.array([[50.0, 0.0, W / 2.0], [0.0, 50.0, H / 2.0], [0.0, 0.0, 1.0]])
    pose = look_at_pose((1.3, 1.1, 0.9)).astype(np.float64)
    _, mask, hits = sg.pictures(verts, faces, K[None], pose[None], H, W, ss, counts=True)
    corners = hull([sg.project(K, sg.to_camera(pose, v)) for v in J])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    want, unsure = np.zeros((H, W), np.int32), np.zeros((H, W), bool)
    for j in range(ss):
        for i in range(ss):
            u, v = xs + (i + 0.5) / ss - 0.5, ys + (j + 0.5) / ss - 0.5
            inside = np.ones((H, W), bool)
            for k in range(len(corners)):                       # left of every edge of the counter-clockwise hull: no ray is cast
                a, b = corners[k], corners[(k + 1) % len(corners)]
                side = ((b[0] - a[0]) * (v - a[1]) - (b[1] - a[1]) * (u - a[0])) / np.hypot(b[0] - a[0], b[1] - a[1])
                inside &= side > 0
                unsure |= np.abs(side) < 1e-6
            want += inside
    assert unsure.mean() < 0.01
    assert 0 < want.sum() < H * W * ss * ss and (want == ss * ss).any() and ((want > 0) & (want < ss * ss)).any()
    np.testing.assert_array_equal(hits[0][~unsure], want[~unsure])
    np.testing.assert_array_equal(mask[0][~unsure], np.where(want > 0, 255, 0)[~unsure])


def test_face_on_square_has_the_albedo_everywhere():
    verts = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    K = np.array([[1000.0, 0.0, 8.0], [0.0, 1000.0, 8.0], [0.0, 0.0, 1.0]])       # 16 pixels see 0.032 of the square: |cos| > 1 - 1e-4
    pose = np.eye(4)
    pose[:3, :3] = np.diag([1.0, -1.0, -1.0])                                      # looking down -z from z = 2
    pose[2, 3] = 2.0
    for albedo in (0.8, 0.42):                                                     # 204.0 and 107.1: the 1e-4 stays clear of a rounding step
        rgb, mask = sg.pictures(verts, faces, K[None], pose[None], 16, 16, 3, albedo=albedo, ambient=0.25)
        assert (rgb == math.floor(255.0 * albedo + 0.5)).all() and (mask == 255).all()
    rgb, mask = sg.pictures(verts, np.zeros((0, 3), np.int32), K[None], pose[None], 16, 16, 2, background=1.0)
    assert (rgb == 255).all() and (mask == 0).all()


def test_edges_cut_at_the_near_plane_and_at_the_border():
    none = np.zeros((0, 3), np.int32)                                               # nothing occludes
    K = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
    pose = np.eye(4)                                                                # the camera at the origin looking down +z
    H, W, near = 48, 64, 0.05
    J = np.array([[0.1, 0.0, -1.0], [0.1, 0.05, -0.5],                              # 0 - 1 behind the camera
                  [0.0, 0.0, 1.0], [0.01, 0.005, -1.0],                            # 2 - 3 across the near plane, near the axis
                  [0.0, 0.1, 1.0], [1.0, 0.1, 1.0],                                 # 4 - 5 across the right border
                  [-0.1, 0.1, 1.0], [0.1, -0.1, 2.0],                               # 6 - 7 inside
                  [0.0, 0.0, 0.01], [0.001, 0.0, 0.02]])                            # 8 - 9 nearer than near
    E = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [3, 2]], np.int32)
    runs = sg.visible_edges(J[:3], none, J, E, K[None], pose[None], H, W, 1.0, 2.0, 0.002, near)
    assert runs["idx"][:, 1].tolist() == [1, 2, 3, 5]
    by_edge = {int(e): k for k, e in enumerate(runs["idx"][:, 1])}
    r = by_edge[1]                                                                  # ends on z = near, not a junction
    assert runs["junc"][r].tolist() == [1, 0] and abs(runs["p3"][r, 1, 2] - near) < 1e-12
    np.testing.assert_array_equal(runs["p3"][r, 0], J[2])
    r = by_edge[5]                                                                  # the same edge the other way round: the cut end comes first
    assert runs["junc"][r].tolist() == [0, 1] and abs(runs["p3"][r, 0, 2] - near) < 1e-12
    r = by_edge[2]                                                                  # ends on the right border x = W - 0.5
    assert runs["junc"][r].tolist() == [1, 0] and abs(runs["p2"][r, 2] - (W - 0.5)) < 1e-9 and abs(runs["p2"][r, 3] - 34.0) < 1e-9
    assert abs(runs["p3"][r, 1, 0] - 0.315) < 1e-9
    r = by_edge[3]
    assert runs["junc"][r].tolist() == [1, 1]
    np.testing.assert_array_equal(runs["p3"][r], J[[6, 7]])
    n = runs["idx"][r, 3] + 1                                                       # ceil(length / step) + 1 samples
    assert n == math.ceil(np.hypot(*(runs["p2"][r, 2:] - runs["p2"][r, :2]))) + 1


def test_an_edge_seen_end_on_is_one_sample_and_no_run():
    """A degenerate projection: both ends fall on one pixel position, n = 1, the run has length 0 and min_len > 0 drops it."""
    K = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
    J = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]])
    E, none = np.array([[0, 1]], np.int32), np.zeros((0, 3), np.int32)
    e = sg.Edge(K, np.eye(4), J[0], J[1], 48, 64, 1.0, 0.05)
    assert e.n == 1
    assert sg.visible_edges(J, none, J, E, K[None], np.eye(4)[None], 48, 64, 1.0, 2.0, 0.002)["idx"].shape[0] == 0
    runs = sg.visible_edges(J, none, J, E, K[None], np.eye(4)[None], 48, 64, 1.0, 0.0, 0.002)
    assert runs["idx"].tolist() == [[0, 0, 0, 0]] and runs["junc"].tolist() == [[1, 1]]      # sample 0 is also sample n - 1: both flags, by the rule
    np.testing.assert_array_equal(runs["p3"][0], J[[0, 0]])


def test_subdividing_a_flat_faced_shape_changes_no_byte():
    """Triangle g becomes 4 g .. 4 g + 3 with the same plane, so the closest hit keeps its depth and, by the tie rule, its parent; the
    shapes' coordinates are dyadic, so the mid points are exact and the normals are the parent's scaled by a power of two, which no
    rounding sees."""
    K, poses = scenegen.cameras(3, 24)
    for name in ("box", "lblock"):
        verts, faces, _, _ = shape(name)
        v2, f2 = scenegen.subdivide(verts, faces, 2)
        assert f2.shape[0] == 16 * faces.shape[0]
        a = sg.pictures(verts, faces, K, poses, 24, 24, 2)
        b = sg.pictures(v2, f2, K, poses, 24, 24, 2)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert 0 < (a[1] == 255).mean() < 1


def test_cameras_sit_on_the_sphere_and_look_at_the_origin():
    K, poses = scenegen.cameras(100, 512)
    assert K.shape == (100, 3, 3) and poses.shape == (100, 4, 4) and K.dtype == poses.dtype == np.float64
    np.testing.assert_array_equal(K[7], [[560.0, 0.0, 256.0], [0.0, 560.0, 256.0], [0.0, 0.0, 1.0]])
    np.testing.assert_array_equal(poses.astype(np.float32).astype(np.float64), poses)         # a float32 reader loses nothing
    c, R = poses[:, :3, 3], poses[:, :3, :3]
    np.testing.assert_allclose(np.linalg.norm(c, axis=1), 2.0, atol=1e-6)
    np.testing.assert_allclose(np.cross(R[:, :, 2], -c), 0.0, atol=1e-6)                       # the view direction passes through the origin
    assert (np.einsum("va,va->v", R[:, :, 2], -c) > 0).all()
    np.testing.assert_allclose(np.einsum("vab,vac->vbc", R, R), np.broadcast_to(np.eye(3), (100, 3, 3)), atol=1e-6)
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-6)
    np.testing.assert_array_equal(poses[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (100, 4)))
    again = scenegen.cameras(100, 512)
    np.testing.assert_array_equal(again[1], poses)
    K2, p2 = scenegen.cameras(5, 128, focal=400.0, radius=3.0)
    assert K2[0, 0, 0] == 100.0 and K2[0, 0, 2] == 64.0
    np.testing.assert_allclose(np.linalg.norm(p2[:, :3, 3], axis=1), 3.0, atol=1e-6)
    d = np.linalg.norm(c[:, None] - c[None], axis=-1) + 10.0 * np.eye(100)
    assert d.min() > 0.3                                                                        # spread out: no two centres close


def test_shapes_and_normalise():
    verts, faces, J, E = scenegen.shapes["lblock"]
    assert J.shape == (12, 3) and E.shape == (18, 2) and faces.shape == (20, 3)
    assert scenegen.shapes["box"][3].shape == (12, 2) and scenegen.shapes["box"][1].shape == (12, 3)
    for name in ("box", "lblock"):                                   # closed: every edge of the mesh is shared by two triangles
        f = scenegen.shapes[name][1]
        pairs = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        assert (np.unique(pairs, axis=0, return_counts=True)[1] == 2).all()
    v, j = scenegen.normalise(verts * 3.0 + 5.0, J * 3.0 + 5.0, extent=2.0)
    np.testing.assert_allclose(v.min(axis=0) + v.max(axis=0), 0.0, atol=1e-12)
    assert abs((v.max(axis=0) - v.min(axis=0)).max() - 2.0) < 1e-12
    np.testing.assert_allclose(j, J * 2.0, atol=1e-12)


def test_many_ray_rule_is_the_rule_of_raycast_f64():
    verts, faces, _, _ = shape("lblock", 1)
    rng = np.random.default_rng(3)
    o = np.broadcast_to(np.array([1.2, -1.4, 0.9], np.float32), (200, 3))
    d = rng.uniform(-0.7, 0.7, (200, 3)) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    t, tri, _ = rc.cast_all(verts, faces, o, d)
    t2, tri2 = sg.closest(verts, faces, o[0].astype(np.float64), d.astype(np.float64), chunk=64)
    np.testing.assert_array_equal(tri, tri2)
    np.testing.assert_array_equal(t, t2)
    assert 20 < (tri >= 0).sum() < 200
    lim = np.where(np.isfinite(t), t, 1.0).astype(np.float32)
    hit = sg.any_hit(verts, faces, o[0].astype(np.float64), d.astype(np.float64), lim.astype(np.float64) + 1e-3)
    np.testing.assert_array_equal(hit, tri >= 0)
    assert not sg.any_hit(verts, faces, o[0].astype(np.float64), d.astype(np.float64), lim.astype(np.float64) * 0.5).any()
