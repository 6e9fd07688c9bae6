"""CPU tests of the 2-D wireframe rule as tests/junctions2d_f64.py restates it, against answers known without it: rotated
lattices, the closed-loop scenes' projected junctions (tests/closed_loop.py) and small inputs whose graphs are written out here.

The bars.  BAR_EXACT = 1e-9 px: segments that lie on lines through a common point give that point up to float64 rounding (3e-13
measured).  RECOVERED = 0.9: the share of the truth's junctions that come back as exactly their set of ends; the rest are corners whose
visible edges project within the angle of each other and occlusion ends inside a corner's window (76 of 78 on the box, 102 of 108 on the
L block).  BAR_DET_JUNCTION: a junction of detected segments against the projected one.  A detected segment lies within BAR_DET_MID =
0.5 px of its edge; two such lines that cross at an angle no less than 10 degrees could move their crossing by far more, but the
detector's offsets are small and even: the restatement measures 0.3104 px at the worst on the box (run on the CPU, here), and the bar
is that with a margin of 2.  On the L block an occluding edge makes apparent junctions that are none in 3-D: at most BEYOND = 10 % of
the junctions may lie beyond the bar (3 of 62 measured).  Every input's decisions keep 1e-9 from their thresholds, so a float64
implementation that forms the same operations takes the same decisions."""
import numpy as np
import pytest

from tests import closed_loop as C
from tests import junctions2d_f64 as J

BAR_EXACT = 1e-9
RECOVERED = 0.9
BAR_DET_JUNCTION = 2.0 * 0.3104
BEYOND = 0.10
MARGIN = 1e-9


def offsets(segs):
    return np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)


# ---- 1. lattices ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (3, 2), (11, 11)])
def test_rotated_lattice_gives_its_nodes(m, n):
    seg, nodes = J.lattice(m, n)
    res = J.build(seg, [0, seg.shape[0]], np.ones(seg.shape[0]))
    assert res["vertices"].shape == ((m + 1) * (n + 1), 2) and res["edges"].shape == (m * (n + 1) + n * (m + 1), 2)
    hist = np.bincount(res["degree"], minlength=5)
    assert hist.tolist() == [0, 0, 4, 2 * (m - 1) + 2 * (n - 1), (m - 1) * (n - 1)], hist
    d = np.linalg.norm(res["vertices"][:, None] - nodes[None], axis=2)
    worst = d.min(axis=1).max()
    print(f"{m} x {n}: {res['vertices'].shape[0]} vertices, degrees {hist[2:].tolist()}, worst {worst:.1e} px, margin {res['margin']:.3g}")
    assert worst <= BAR_EXACT and sorted(d.argmin(axis=1).tolist()) == list(range(nodes.shape[0]))
    assert (res["kind"] == 1).all() and (res["t_edge"] == -1).all() and np.array_equal(res["esrc"], np.arange(seg.shape[0]))
    assert np.abs(res["spread"] - 1.0).max() < 1e-9 and res["margin"] >= MARGIN


# ---- 2. the closed loop: shrunk runs against the projection ---------------------------------------------------------------------------------
def shrunk_runs(sc):
    """The visible runs, each end pulled in by min(1, 0.2 L) -> (segments per view, truth: per view {junction index: set of endpoints})."""
    runs = sc["runs"]
    segs, truth = [], []
    for v in range(C.VIEWS):
        m = np.nonzero(runs["idx"][:, 0] == v)[0]
        p2 = runs["p2"][m]
        d = p2[:, 2:] - p2[:, :2]
        L = np.linalg.norm(d, axis=1)
        cut = (np.minimum(1.0, 0.2 * L) / L)[:, None] * d
        segs.append(np.concatenate([p2[:, :2] + cut, p2[:, 2:] - cut], axis=1))
        groups = {}
        for i, r in enumerate(m):
            for k in range(2):
                if runs["junc"][r, k]:
                    groups.setdefault(int(sc["edges"][runs["idx"][r, 1], k]), set()).add(2 * i + k)
        truth.append(groups)
    return segs, truth


@pytest.mark.parametrize("name", C.SHAPES)
def test_shrunk_runs_recover_the_projected_junctions(name):
    sc = C.scene(name)
    segs, truth = shrunk_runs(sc)
    off = offsets(segs)
    res = J.build(np.concatenate(segs), off, np.ones(off[-1]), gap=3.0)
    total = found = 0
    worst = 0.0
    for v in range(C.VIEWS):
        proj = C.project(sc["K"][v], sc["poses"][v], sc["junctions"])[0]
        # a flagged end is its edge's own junction: the run ends there
        runs_v = sc["runs"]["p2"][sc["runs"]["idx"][:, 0] == v].reshape(-1, 2)
        for j, ends in truth[v].items():
            assert np.abs(runs_v[sorted(ends)] - proj[j]).max() <= C.BAR_P2
        have = J.members(res, v, off)
        verts = res["vertices"][res["voff"][v]:res["voff"][v + 1]]
        for j, ends in truth[v].items():
            if len(ends) < 2:
                continue
            total += 1
            q = have.get(frozenset(ends))
            if q is not None:
                found += 1
                worst = max(worst, float(np.linalg.norm(verts[q] - proj[j])))
    print(f"{name}: {found} of {total} junctions recovered as their exact sets, the worst {worst:.1e} px off; margin {res['margin']:.3g}")
    assert total > 0 and worst <= BAR_EXACT
    assert found >= RECOVERED * total, (found, total)
    assert res["margin"] >= MARGIN


# ---- 3. the detector's own segments ---------------------------------------------------------------------------------------------------------
def detected(sc):
    off = offsets(sc["det_segs"])
    weight = 1.0 - 10.0 ** -sc["det"]["nfa"]
    return np.concatenate(sc["det_segs"]), off, weight


@pytest.mark.parametrize("name", C.SHAPES)
def test_detected_segments_meet_at_the_projected_junctions(name):
    sc = C.scene(name)
    seg, off, weight = detected(sc)
    res = J.build(seg, off, weight)
    dist = []
    for v in range(C.VIEWS):
        proj = C.project(sc["K"][v], sc["poses"][v], sc["junctions"])[0]
        view = J.view_of(res, v)
        X = view["vertices"][view["kind"] == 1]
        dist += np.linalg.norm(X[:, None] - proj[None], axis=2).min(axis=1).tolist()
    dist = np.array(dist)
    beyond = int((dist > BAR_DET_JUNCTION).sum())
    print(f"{name}: {seg.shape[0]} segments, {res['vertices'].shape[0]} vertices, {dist.shape[0]} junctions, worst {dist.max():.4f} px, "
          f"median {np.median(dist):.4f} px, {beyond} beyond {BAR_DET_JUNCTION:.3f} px; margin {res['margin']:.3g}")
    assert dist.shape[0] >= 2 * C.VIEWS
    if name == "box":
        assert beyond == 0, dist.max()
    else:
        assert beyond <= BEYOND * dist.shape[0], (beyond, dist.shape[0])
    assert res["margin"] >= MARGIN
    assert res["vertices"].shape[0] < 2 * seg.shape[0] and res["edges"].shape[0] <= seg.shape[0]


# ---- 4. the small inputs, their graphs written out ------------------------------------------------------------------------------------------
CASES = J.cases()


def run(name, **kw):
    seg, off, weight = CASES[name]
    return J.build(seg, off, weight, **kw), seg, off


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_decision_of_a_case_is_near_its_threshold(name):
    res, seg, off = run(name)
    assert res["margin"] >= MARGIN, res["margin"]
    assert res["voff"].shape == off.shape == res["eoff"].shape and res["ends"].shape == (seg.shape[0], 2)
    for v in range(off.shape[0] - 1):                                    # every index is its view's own and in range
        view, n = J.view_of(res, v), off[v + 1] - off[v]
        nv = view["vertices"].shape[0]
        ends = res["ends"][off[v]:off[v + 1]]
        assert ends.size == 0 or (ends.min() >= 0 and ends.max() < nv and np.unique(ends).shape[0] == nv)
        assert np.array_equal(view["edges"], ends[view["esrc"]]) and (view["esrc"] < max(n, 1)).all() and (np.diff(view["esrc"]) > 0).all()
        assert np.array_equal(np.bincount(ends.reshape(-1), minlength=nv), view["degree"])
        assert ((view["kind"] == 1) == (view["degree"] >= 2)).all() and ((view["kind"] == 2) == (view["t_edge"] >= 0)).all()


def test_empty_and_tiny_views():
    res, _, _ = run("no_views")
    assert res["voff"].tolist() == [0] and res["eoff"].tolist() == [0] and res["vertices"].shape == (0, 2)
    res, _, _ = run("tiny_views")
    assert res["voff"].tolist() == [0, 0, 2, 5] and res["eoff"].tolist() == [0, 0, 1, 3]
    assert res["kind"].tolist() == [0, 0, 0, 1, 0] and res["degree"].tolist() == [1, 1, 1, 2, 1]
    assert np.abs(res["vertices"][3] - [50.0, 50.0]).max() <= BAR_EXACT and res["ends"].tolist() == [[0, 1], [0, 1], [1, 2]]
    assert res["score"].tolist() == [0.5, 0.5, 0.501, 0.502, 0.502] and abs(res["spread"][3] - 1.0) <= BAR_EXACT


def test_degenerate_segments_take_part_in_nothing():
    res, seg, _ = run("degenerate")
    assert res["vertices"].shape[0] == 11 and res["edges"].shape[0] == 6 and res["kind"].tolist().count(1) == 1
    j = int(np.nonzero(res["kind"] == 1)[0][0])
    assert res["ends"][0, 1] == j == res["ends"][3, 0] and np.abs(res["vertices"][j] - [50.0, 50.0]).max() <= BAR_EXACT
    for i in (1, 2, 4, 5):                                               # free ends, where they were
        for k in range(2):
            q = res["ends"][i, k]
            assert res["kind"][q] == 0 and np.array_equal(res["vertices"][q], seg[i, 2 * k:2 * k + 2], equal_nan=True)


def test_collinear_ends_are_never_joined():
    res, seg, _ = run("parallel")
    assert res["vertices"].shape[0] == 8 and (res["kind"] == 0).all() and res["edges"].shape[0] == 4
    assert np.array_equal(res["vertices"], seg.reshape(-1, 2))


@pytest.mark.parametrize("n", [J.TILE - 1, J.TILE, J.TILE + 1])
def test_a_junction_and_a_tee_across_tiles(n):
    res, seg, _ = run(f"tile_{n}")
    assert seg.shape[0] == n and res["vertices"].shape[0] == 2 * n - 1 and res["edges"].shape[0] == n
    j, t = res["ends"][0, 1], res["ends"][1, 1]
    assert j == res["ends"][n - 1, 0] and res["kind"][j] == 1 and np.abs(res["vertices"][j] - [50.0, 50.0]).max() <= BAR_EXACT
    assert res["kind"][t] == 2 and res["t_edge"][t] == n - 2 and np.abs(res["vertices"][t] - [130.0, 200.0]).max() <= BAR_EXACT
    assert abs(res["spread"][t] - 2.0) <= BAR_EXACT and np.bincount(res["kind"]).tolist() == [2 * n - 3, 1, 1]
    off_t = J.build(seg, [0, n], np.ones(n), t_junctions=False)
    assert off_t["kind"][t] == 0 and np.array_equal(off_t["vertices"][t], seg[1, 2:]) and np.array_equal(off_t["ends"], res["ends"])


def test_a_component_is_transitive_across_three_tiles():
    res, seg, _ = run("chain")
    n = seg.shape[0]
    mid = J.TILE + 11
    assert n > 2 * J.TILE and mid >= J.TILE and n - 1 >= 2 * J.TILE
    j = res["ends"][0, 1]
    assert j == res["ends"][mid, 0] == res["ends"][n - 1, 1] and res["degree"][j] == 3 and np.bincount(res["kind"]).tolist() == [2 * n - 3, 1]
    assert np.abs(res["vertices"][j] - [50.0, 50.0]).max() <= BAR_EXACT
    # the two shallow segments alone do not meet
    two = J.build(seg[[0, n - 1]], [0, 2], np.ones(2))
    assert (two["kind"] == 0).all()


@pytest.mark.parametrize("m", [63, 64, 65])
def test_a_star_is_one_junction(m):
    res, seg, _ = run(f"star_{m}")
    assert res["vertices"].shape[0] == m + 1 and res["degree"][0] == m and res["kind"][0] == 1 and (res["ends"][:, 0] == 0).all()
    assert np.abs(res["vertices"][0] - [200.0, 200.0]).max() <= BAR_EXACT and abs(res["spread"][0] - 1.0) <= BAR_EXACT
    assert res["score"][0] == 0.506 and res["edges"].shape[0] == m


def test_ragged_views_are_their_own_results():
    res, seg, off = run("ragged")
    assert off.tolist() == [0, 7, 11, 11, 28, 30] and res["voff"].tolist() == [0, 6, 10, 10, 22, 25] and res["eoff"].tolist() == [0, 7, 11, 11, 28, 30]
    for v in range(5):
        alone = J.build(seg[off[v]:off[v + 1]], [0, off[v + 1] - off[v]], CASES["ragged"][2][off[v]:off[v + 1]])
        part = J.view_of(res, v)
        for k in part:
            assert part[k].tobytes() == alone[k].tobytes(), (v, k)


def test_duplicate_edges_keep_the_heavier_then_the_lower():
    res, _, _ = run("duplicate_equal")
    assert res["vertices"].shape[0] == 4 and sorted(res["degree"].tolist()) == [2, 2, 3, 3] and res["esrc"].tolist() == [0, 2, 3, 4]
    assert res["ends"][0].tolist() == res["ends"][1].tolist()
    res, _, _ = run("duplicate_heavier")
    assert res["esrc"].tolist() == [1, 2, 3, 4] and res["eweight"].tolist() == [0.8, 0.6, 0.6, 0.6]


def test_a_segment_inside_one_junction_is_dropped():
    res, _, _ = run("collapsed")
    assert res["ends"].tolist() == [[0, 1], [2, 1], [1, 1]] and res["degree"].tolist() == [1, 4, 1] and res["esrc"].tolist() == [0, 1]
    assert np.abs(res["vertices"][1]).max() < 1.0 and res["spread"][1] < 2.0


def test_a_tee_takes_the_nearest_bar_then_the_lower():
    res, _, _ = run("tee_two_bars")
    t = res["ends"][3, 1]
    assert res["vertices"].shape[0] == 8 and res["kind"][t] == 2 and res["t_edge"][t] == 1 and res["degree"][t] == 1
    assert np.abs(res["vertices"][t] - [50.0, 50.0]).max() <= BAR_EXACT and np.bincount(res["kind"]).tolist() == [7, 0, 1]
    assert res["edges"].shape[0] == 4                                    # the bar is not split


def test_bad_options_are_refused():
    seg, off, weight = CASES["tiny_views"]
    for kw in ({"gap": 0.0}, {"frac": 0.5}, {"frac": 0.0}, {"angle": 0.0}, {"angle": 91.0}):
        with pytest.raises(ValueError):
            J.build(seg, off, weight, **kw)
