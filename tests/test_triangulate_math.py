"""CPU tests of the triangulation rule as tests/triangulate_f64.py states it: what it finds on the fixture and on an exact
synthetic scene, what the pair test rejects, the margins of the scenes the device is compared on, and the ABI of the new entry points.
No device is touched."""
import math
import os

import numpy as np
import pytest

from tests import triangulate_f64 as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample_distance(line, seg, n=16):
    """The largest distance of n points along `line` [2,3] to the segment `seg` [2,3]."""
    p = line[0][None, :] + np.linspace(0.0, 1.0, n)[:, None] * (line[1] - line[0])[None, :]
    d = seg[1] - seg[0]
    t = np.clip(((p - seg[0]) @ d) / (d @ d), 0.0, 1.0)
    return float(np.linalg.norm(p - (seg[0] + t[:, None] * d), axis=1).max())


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_with_defaults_recovers_the_ground_truth():
    """25 views of ABC 00075213 with the HAWP detections.  Recorded with this reference: 4056 hypotheses, 162 estimates, 19 lines; 18 of
    the 19 lie within 0.7 % of the scene diagonal of a ground-truth line and 17 of the 18 ground-truth lines are covered likewise.  The
    conditions asserted leave room: 15 of 18 covered within 2 %, 85 % of the lines within 2 % of a ground-truth line."""
    fx = T.fixture_scene()[3]
    res = T.reference("fixture")
    counts = (res["rows"].shape[0], int(res["kept"].sum()), res["lines3d"].shape[0])
    gt = fx["gt_lines"]
    diag = float(np.linalg.norm(gt.reshape(-1, 3).max(0) - gt.reshape(-1, 3).min(0)))
    to_gt = np.array([min(sample_distance(l, g) for g in gt) for l in res["lines3d"]]) / diag
    covered = np.array([min(sample_distance(g, l) for l in res["lines3d"]) for g in gt]) / diag
    print(f"hypotheses, estimates, lines = {counts}; lines within 2 %: {(to_gt <= 0.02).sum()} of {to_gt.size} (0.7 %: {(to_gt <= 0.007).sum()}); "
          f"ground truth covered within 2 %: {(covered <= 0.02).sum()} of {covered.size} (0.7 %: {(covered <= 0.007).sum()})")
    assert counts == (4056, 162, 19)
    assert (covered <= 0.02).sum() >= 15 and gt.shape[0] == 18
    assert (to_gt <= 0.02).mean() >= 0.85
    assert res["views"].min() >= 3 and res["lines3d"].dtype == np.float64 and res["views"].dtype == np.int32
    assert abs(float(fx["gt_scale"]) - 15.0) < 0.1 and np.abs(fx["gt_offset"] - [5.0, 7.5, 3.0]).max() < 0.05


# ---- 2. an exact scene --------------------------------------------------------------------------------------------------------------------------
def test_cube_edges_come_back_once_and_exactly():
    """The 12 edges of a cube and 8 random segments, 12 ring cameras, exact projections: every camera sees every edge whole, the
    arithmetic is exact up to rounding, so every edge comes back with end points within 1e-9 (a conditioning bound of float64 at these
    baselines, not a tuned bar), and no line comes back twice."""
    segments, Ks, poses, world = T.cube_scene()
    res = T.lines(segments, Ks, poses)
    got = res["lines3d"]
    hits = []
    for w in world[:12]:
        err = np.minimum(np.abs(got - w[None]).max(axis=(1, 2)), np.abs(got[:, ::-1] - w[None]).max(axis=(1, 2)))
        assert err.min() <= 1e-9, err.min()
        hits.append(int(err.argmin()))
    assert len(set(hits)) == 12
    for i in range(len(got)):
        for j in range(i + 1, len(got)):
            assert min(np.abs(got[i] - got[j]).max(), np.abs(got[i, ::-1] - got[j]).max()) > 1e-6, (i, j)
    assert res["views"].max() <= 12 and res["views"].min() >= 3


# ---- 3. rejections, each as a two-view case ------------------------------------------------------------------------------------------------------
K0 = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])


def pose_at(C, R=np.eye(3)):
    p = np.eye(4)
    p[:3, :3], p[:3, 3] = R, C
    return p


def two_views(line_a, line_b, Cb=(1.0, 0.0, 0.0), **kw):
    """World lines [n,2,3] seen by camera a at the origin and camera b at Cb (both looking along +z) -> the reference's hypotheses."""
    Ks, poses = np.stack([K0, K0]), np.stack([pose_at(np.zeros(3)), pose_at(np.asarray(Cb, dtype=np.float64))])
    sa = T.project(np.asarray(line_a, dtype=np.float64).reshape(-1, 2, 3), K0, poses[0])[0]
    sb = T.project(np.asarray(line_b, dtype=np.float64).reshape(-1, 2, 3), K0, poses[1])[0]
    return T.hypotheses([sa, sb], Ks, poses, **kw), (sa, sb, Ks, poses)


GENERIC = [[-0.3, -0.4, 4.0], [0.5, 0.6, 5.0]]


def rows_of(h, a):
    return h["rows"][h["rows"][:, 0] == a]


def test_a_generic_pair_is_a_hypothesis_with_the_true_depths():
    h, _ = two_views(GENERIC, GENERIC)
    assert rows_of(h, 0).tolist() == [[0, 0, 0, 0]] and rows_of(h, 1).tolist() == [[1, 0, 0, 0]]
    assert np.allclose(h["depths"][0], [4.0, 5.0], rtol=1e-12)              # K^-1 (p, 1) has z = 1: the depth along it is the camera's z


def test_segment_through_the_epipole_is_rejected():
    """A world line in a plane through both centres (y = 0 contains the baseline): in either view its segment lies on the line through
    the epipole, the partner's plane holds the other centre, and s = 0 / 0 or 0: never a hypothesis.  A generic second segment beside it
    still is one."""
    epi = [[0.2, 0.0, 4.0], [0.7, 0.0, 6.0]]
    h, _ = two_views([epi, GENERIC], [epi, GENERIC])
    assert h["rows"].tolist() == [[0, 1, 0, 1], [1, 1, 0, 1]]


def test_zero_length_segment_is_rejected_on_either_side():
    point = [[0.1, 0.2, 4.0], [0.1, 0.2, 4.0]]
    h, _ = two_views([point, GENERIC], [GENERIC, point])
    assert h["rows"].tolist() == [[0, 1, 0, 0], [1, 0, 0, 1]]


def test_planes_closer_than_angle_min_are_rejected():
    """A line along z through (0.5, y0, .), midway between the centres (0, 0, 0) and (1, 0, 0): the planes through it and a centre have the
    normals (y0, -0.5, 0) and (y0, 0.5, 0), which meet at 2 atan(0.5 / y0).  At 2 degrees the pair is refused with angle_min = 5 and
    accepted with angle_min = 1; at 1.999 and 2.001 degrees it sits to either side of angle_min = 2."""
    def line(deg):
        y0 = 0.5 / math.tan(0.5 * deg * math.pi / 180.0)
        return [[0.5, y0, 40.0], [0.5, y0, 60.0]]
    assert two_views(line(2.0), line(2.0))[0]["rows"].shape[0] == 0
    assert two_views(line(2.0), line(2.0), angle_min=1.0)[0]["rows"].shape[0] == 2
    assert two_views(line(1.999), line(1.999), angle_min=2.0)[0]["rows"].shape[0] == 0
    assert two_views(line(2.001), line(2.001), angle_min=2.0)[0]["rows"].shape[0] == 2


def test_a_hypothesis_behind_either_camera_is_rejected():
    """b ten units ahead of a on the common axis: a line at z = 5 is in front of a and behind b (its mirrored projection in b still lies on
    the partner's image line); with b ten units behind a it is a line at z = -5 that a sees mirrored."""
    line = [[1.0, 0.5, 5.0], [1.0, -0.6, 5.0]]
    h, (sa, sb, _, _) = two_views(line, line, Cb=(0.0, 0.0, 10.0))
    assert np.isfinite(sa).all() and np.isfinite(sb).all() and h["rows"].shape[0] == 0
    back = [[1.0, 0.5, -5.0], [1.0, -0.6, -5.0]]
    assert two_views(back, back, Cb=(0.0, 0.0, -10.0))[0]["rows"].shape[0] == 0
    assert two_views(line, line, Cb=(0.0, 0.0, -10.0))[0]["rows"].shape[0] == 2          # in front of both


def test_overlap_just_below_and_just_above_the_threshold():
    """The partner covers a part of the world line.  The overlap ratio along the partner is worked out here from the projections (the
    ends of a's segment land on the partner's image line at t_1, t_2), and overlap_min is set a millionth to either side of it."""
    A, B = np.array(GENERIC[0]), np.array(GENERIC[1])
    part = [A + 0.6 * (B - A), A + 1.4 * (B - A)]
    _, (sa, sb, Ks, poses) = two_views(GENERIC, part)
    ends = T.project(np.array([GENERIC]), K0, poses[1])[0].reshape(2, 2)      # a's end points as b sees them
    q1, u = sb[0, :2], sb[0, 2:] - sb[0, :2]
    t = sorted(((e - q1) @ u) / (u @ u) for e in ends)
    ratio = (min(t[1], 1.0) - max(t[0], 0.0)) / (max(t[1], 1.0) - min(t[0], 0.0))
    assert 0.2 < ratio < 0.4
    above = T.hypotheses([sa, sb], Ks, poses, overlap_min=ratio * (1.0 + 1e-6))
    below = T.hypotheses([sa, sb], Ks, poses, overlap_min=ratio * (1.0 - 1e-6))
    assert rows_of(above, 0).shape[0] == 0 and rows_of(below, 0).tolist() == [[0, 0, 0, 0]]


def test_more_neighbours_than_other_views_is_clipped():
    seg, Ks, poses = T.random_scene([5, 6, 7], 10, seed=5)
    a, b = T.lines(seg, Ks, poses, neighbours=6), T.lines(seg, Ks, poses, neighbours=2)
    assert a["neighbours"].shape == (3, 2) and np.array_equal(a["neighbours"], b["neighbours"])
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["depths"], b["depths"]) and np.array_equal(a["lines3d"], b["lines3d"])
    near = T.neighbour_table(np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [3.0, 0, 0]]), 3)
    assert near.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [1, 0, 2]]              # ties go to the lower index


def test_a_view_without_segments_and_too_few_views():
    seg, Ks, poses = T.random_scene([6, 0, 6, 6], 6, seed=6)
    res = T.lines(seg, Ks, poses, min_score=0.5)
    assert res["offsets"].tolist() == [0, 6, 6, 12, 18] and not (res["rows"][:, 0] == 1).any() and res["rows"].shape[0] > 0
    slot_of_empty = [int(np.nonzero(res["neighbours"][a] == 1)[0][0]) for a in (0, 2, 3)]
    for a, m in zip((0, 2, 3), slot_of_empty):
        assert not ((res["rows"][:, 0] == a) & (res["rows"][:, 2] == m)).any()
    for V in (0, 1, 2):
        seg, Ks, poses = T.random_scene([8] * V, 8, seed=7)
        res = T.lines(seg, Ks, poses)
        assert res["lines3d"].shape == (0, 2, 3) and res["views"].shape == (0,) and res["members"].shape == (8 * V,) and (res["members"] == -1).all()
        assert res["rows"].shape[0] == (0 if V < 2 else res["rows"].shape[0]) and not res["kept"].any()      # one slot never scores
    assert T.lines(*T.random_scene([8, 8], 8, seed=7), min_score=0.0, min_views=2)["rows"].shape[0] > 0


# ---- 4. the margins of every scene the device is compared on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v2", "v3", "v7", "f32"])
def test_pair_margins_of_the_hypothesis_scenes(name):
    """No accepted or rejected pair lies within 1e-12 of a threshold of the pair test.  The largest neighbourhood holds the pairs of every
    smaller one (slots are ranks)."""
    assert T.reference(name, "hypotheses", neighbours=6)["margin"] > 1e-12


@pytest.mark.parametrize("name", ["v7", "capacity", "fixture", "fixture_slice"])
def test_decision_margins_of_the_line_scenes(name):
    m = T.reference(name)["margins"]
    print(name, m)
    assert m["pair"] > 1e-12 and m["score"] > 1e-9 and m["top2"] > 1e-9 and m["link"] > 1e-9


def test_capacity_scene_crosses_the_wavefront():
    res = T.reference("capacity")
    per_segment = np.bincount(res["offsets"][res["rows"][:, 0]] + res["rows"][:, 1])
    assert per_segment[0] > 64                                                        # a wave strides over the hypotheses of view 0's segment
    assert np.bincount(res["labels"][res["labels"] >= 0]).max() > 64 and res["views"].tolist() == [70]


# ---- 5. the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points():
    import re
    from neat_amd import _lib
    lib = _lib.lib()
    assert lib.neat_abi_version() == 15 == _lib.ABI_VERSION
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neat_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(neat_[a-z0-9_]+)\s*\(", text)))
    assert names == _lib.exported_symbols()
    tri = [n for n in names if n.startswith("neat_tri_")]
    assert tri == ["neat_tri_count", "neat_tri_fill", "neat_tri_lines", "neat_tri_scratch_bytes"] and not any(n.endswith("_ws_bytes") for n in tri)
    q = lib.neat_tri_scratch_bytes
    assert q(64, 32000, 10, 500) > 0 and q(64, 32000, 10, 500) % 256 == 0 and q(0, 0, 0, 0) % 256 == 0 and q(1, 5, 0, 5) > 0
    assert q(64, 32000, 10, 500) > q(64, 32000, 6, 500) > q(64, 16000, 6, 500)
    for bad in [(-1, 0, 0, 0), (2, -1, 1, 0), (2, 4, -1, 4), (2, 4, 1, -1), (2, 4, 2, 4), (2, 4, 1, 5), (65536, 4, 1, 4),
                (2, 2 ** 31 - 1, 1, 10), (20, 2 ** 27, 17, 10), (65535, 2 ** 24, 64, 2 ** 24)]:
        assert q(*bad) == 0, bad
    # the calls refuse before any launch: no device is needed to be told so
    assert lib.neat_tri_count(None, None, 2, -1, 0, None, 1, None, 0.9, 0.25, None, None, None, None, None) == -1
    assert lib.neat_tri_fill(None, 2, 4, 4, None, 1, None, 0.9, 0.25, None, 2 ** 31, None, None, None, None) == -1
    assert lib.neat_tri_lines(None, 2, 4, 4, None, 1, None, None, None, None, -1, None, None, None, 2.5, 1.5, 3, *[None] * 10) == -1
