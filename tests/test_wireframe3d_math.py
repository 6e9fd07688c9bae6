"""CPU tests of the 3-D wireframe rule as tests/wireframe3d_f64.py states it: the closed-loop scenes against their analytic
wireframes, the cases written out, a cubic lattice, the margins of every input the device is compared on, and the size query."""
import json
import os

import numpy as np
import pytest

from tests import closed_loop as C
from tests import wireframe3d_f64 as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = os.path.join(ROOT, "tests", "wireframe3d_sizes.json")
MARGIN = 1e-6
# what the restatement gives on the runs of the two scenes: links, free ends, edges (the box has 24 line ends; one bottom corner is seen
# by one pair of views only, so one end stays free)
COUNTS = {"box": (22, 1, 12), "lblock": (30, 1, 17)}
# Detected segments (detect_f64 -> junctions2d_f64 -> triangulate_f64 -> the rule), measured: the box gives 4 lines and 3 junctions, the
# worst 3.5e-4 from its corner; the L block 10 lines and 3 junctions, the worst 4.42e-4.  The bar gives the worst a factor of 4
DET_WORST = 4.42e-4
BAR_DET = 4.0 * DET_WORST
DET_JUNCTIONS = {"box": 3, "lblock": 3}


def run(a, **kw):
    return W.build(*W.arrays_of(a), **kw)


def graphs(segs):
    g = [W.weld(s) for s in segs]
    return [x[0] for x in g], [x[1] for x in g]


def to_truth(sc, out, bar):
    """Every junction lies within `bar` of a true junction, no two on the same one -> the true junction of every vertex."""
    d = np.linalg.norm(out["junctions3d"][:, None] - sc["junctions"][None], axis=2)
    near = d.argmin(axis=1)
    isj = out["kind"] == 1
    worst = d.min(axis=1)[isj].max()
    print(f"{sc['name']}: {int(isj.sum())} junctions, the worst {worst:.3g} from its own")
    assert worst <= bar, worst
    assert len(set(near[isj].tolist())) == int(isj.sum())
    return near, worst


@pytest.mark.parametrize("name", C.SHAPES)
def test_closed_loop_runs_give_the_analytic_wireframe(name):
    sc = C.scene(name)
    vertices, edges = graphs(sc["segs"])
    for v, e, s in zip(vertices, edges, sc["segs"]):
        assert np.array_equal(v[e].reshape(-1, 4), s)
    endv, view, _ = W.graph_arrays(edges, [v.shape[0] for v in vertices])
    R = sc["tri_runs"]                                                    # triangulate_f64.lines of those very segments
    out = W.build(R["lines3d"], R["support"], R["members"], R["estimate"], endv, view, C.VIEWS)
    near, _ = to_truth(sc, out, C.BAR_TRI)
    assert sorted(near[out["kind"] == 1].tolist()) == list(range(sc["junctions"].shape[0]))          # all 8, all 12
    true_edges = {tuple(sorted(e)) for e in sc["edges"].tolist()}
    got = [tuple(sorted((int(near[a]), int(near[b])))) for a, b in out["edges3d"]]
    assert all(e in true_edges for e in got) and len(set(got)) == len(got)
    print(name, "margins", out["margins"])
    assert all(m > MARGIN for m in out["margins"].values()), out["margins"]
    assert (len(out["links"]), int((out["kind"] == 0).sum()), out["edges3d"].shape[0]) == COUNTS[name]
    assert np.array_equal(out["lines3d_wf"], out["junctions3d"][out["edges3d"]]) and out["degree"].sum() == 2 * R["lines3d"].shape[0]


@pytest.mark.parametrize("name", C.SHAPES)
def test_closed_loop_detected_segments(name):
    """The whole chain on the host from the pictures: what comes out is few (the detector's segments stop short of the corners), and
    each junction is a true one to BAR_DET."""
    from tests import junctions2d_f64 as J2
    sc = C.scene(name)
    seg = np.concatenate(sc["det_segs"])
    off = np.concatenate([[0], np.cumsum([len(s) for s in sc["det_segs"]])])
    g = J2.build(seg, off, 1.0 - 10.0 ** -sc["det"]["nfa"])
    parts = [J2.view_of(g, v) for v in range(C.VIEWS)]
    out = W.wireframe([p["vertices"] for p in parts], [p["edges"] for p in parts], sc["K"], sc["poses"])
    to_truth(sc, out, BAR_DET)
    assert int((out["kind"] == 1).sum()) == DET_JUNCTIONS[name]


def corner_views(shared_views, V=2):
    """CORNER seen by V views; in the first `shared_views` of them the two lines' ends 0 are one 2-D vertex."""
    segs = []
    for v in range(V):
        b = 4 * v
        segs += [(v, 0, (b, b + 1), (0.0, 1.0)), (v, 1, (b if v < shared_views else b + 2, b + 3), (0.0, 1.0))]
    return segs


def test_one_view_is_one_vote():
    a = W.written(W.CORNER, corner_views(1), 2)
    out = run(a)
    assert out["links"] == [] and out["kind"].tolist() == [0, 0, 0, 0] and out["esrc"].tolist() == [0, 1]
    assert out["junctions3d"].tobytes() == a["lines3d"].reshape(4, 3).tobytes()                 # free ends stay, bit for bit
    out = run(a, min_votes=1)
    assert out["links"] == [(0, 2)] and out["kind"].tolist() == [1, 0, 0] and out["degree"].tolist() == [2, 1, 1] and out["votes"].tolist() == [1, 0, 0]
    assert np.abs(out["junctions3d"][0] - [0.0, 0.0, 0.0005]).max() < 1e-12 and out["edges3d"].tolist() == [[0, 1], [0, 2]]
    assert abs(out["spread"][0] - np.hypot(0.05, 0.0005)) < 1e-12


def test_parallel_lines_are_a_continuation():
    lines = [[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[1.1, 0.0, 0.0], [2.0, 0.001, 0.0]]]
    segs = [(v, 0, (4 * v + 1, 4 * v), (0.0, 1.0)) for v in range(2)] + [(v, 1, (4 * v, 4 * v + 2), (0.0, 1.0)) for v in range(2)]
    out = run(W.written(lines, segs, 2))
    assert out["pairs"] == 2 and out["links"] == [] and (out["kind"] == 0).all() and out["edges3d"].shape[0] == 2


def test_a_crossing_beyond_reach():
    lines = [[[0.4, 0.0, 0.0], [1.0, 0.0, 0.0]], W.CORNER[1]]              # line 0 would have to grow by two thirds
    a = W.written(lines, corner_views(2), 2)
    assert run(a)["links"] == [] and run(a, reach=0.7)["links"] == [(0, 2)]


def test_an_inner_end_votes_for_nothing():
    segs = [(v, 0, (4 * v + 1, 4 * v), (0.0, 0.5)) for v in range(2)] + [(v, 1, (4 * v, 4 * v + 2), (0.0, 1.0)) for v in range(2)]
    out = run(W.written([[[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], W.CORNER[1]], segs, 2))
    assert out["pairs"] == 0 and out["links"] == [] and out["margins"]["ends"] > 0.19          # taus 0, 0.5 and 1 against 0.2 and 0.8


def test_a_line_inside_one_junction_is_dropped():
    """A short line between the arms of a corner: its two ends reach the corner's junction through the arms, each pair in its own two views."""
    lines = [[[-1.0, 0.0, 0.0], [-0.05, 0.0, 0.0]], [[0.0, -1.0, 0.0], [0.0, -0.05, 0.0]], [[-0.05, -0.004, 0.0], [-0.004, -0.05, 0.0]]]
    segs = []
    for v, (La, ea, Lb, eb) in enumerate([(0, 1, 2, 0)] * 2 + [(0, 1, 1, 1)] * 2 + [(1, 1, 2, 1)] * 2):
        b = 4 * v
        segs += [(v, La, (b + 1, b) if ea else (b, b + 1), (0.0, 1.0)), (v, Lb, (b + 2, b) if eb else (b, b + 2), (0.0, 1.0))]
    out = run(W.written(lines, segs, 6))
    assert sorted(out["links"]) == [(1, 3), (1, 4), (3, 5)] and out["degree"].tolist() == [1, 4, 1] and out["esrc"].tolist() == [0, 1]
    assert all(m > MARGIN for m in out["margins"].values())


@pytest.mark.parametrize("support,kept", [([1.0, 2.0, 1.0, 1.0], 1), ([2.0, 2.0, 1.0, 1.0], 0), ([3.0, 2.0, 1.0, 1.0], 0)])
def test_of_two_lines_between_two_junctions_the_better_supported_stays(support, kept):
    lines = [[[0.05, 0.0, 0.0], [0.95, 0.0, 0.0]], [[0.05, 0.001, 0.0], [0.95, 0.0005, 0.0]], [[0.0, 0.05, 0.0], [0.0, 1.0, 0.0]],
             [[1.0, 0.05, 0.0], [1.0, 1.0, 0.0]]]
    segs = []
    for v in range(2):
        b = 4 * v
        segs += [(v, 0, (b, b + 1), (0.0, 1.0)), (v, 1, (b, b + 1), (0.0, 1.0)), (v, 2, (b, b + 2), (0.0, 1.0)), (v, 3, (b + 1, b + 3), (0.0, 1.0))]
    out = run(W.written(lines, segs, 2, support))
    assert (0, 2) not in out["links"] and out["degree"].tolist() == [3, 3, 1, 1] and out["esrc"].tolist() == [kept, 2, 3]
    assert out["edges3d"].tolist() == [[0, 1], [0, 2], [1, 3]]


def test_empty_inputs():
    for name in ("nothing", "no_lines"):
        a, kw = W.cases()[name]
        out = run(a, **kw)
        assert out["junctions3d"].shape == (0, 3) and out["edges3d"].shape == (0, 2) and out["lines3d_wf"].shape == (0, 2, 3)
    for name in ("no_members", "no_segments"):
        a, kw = W.cases()[name]
        out = run(a, **kw)
        assert out["junctions3d"].tobytes() == a["lines3d"].tobytes() and (out["kind"] == 0).all() and out["esrc"].tolist() == list(range(20))
    with pytest.raises(ValueError):
        run(W.cases()["nothing"][0], end_frac=0.5)


def test_cubic_lattice():
    a, nodes, ends = W.lattice(54, V=4, n=3)
    out = run(a)
    assert out["junctions3d"].shape == (27, 3) and (out["kind"] == 1).all() and out["edges3d"].shape == (54, 2)
    assert np.bincount(out["degree"]).tolist() == [0, 0, 0, 8, 12, 6, 1]
    d = np.linalg.norm(out["junctions3d"][:, None] - nodes[None], axis=2)
    assert d.min(axis=1).max() <= 1e-9 and sorted(d.argmin(axis=1).tolist()) == list(range(27))
    u = a["lines3d"][:, 1] - a["lines3d"][:, 0]
    for qa, qb in out["links"]:                                           # collinear rods never link; they meet through the others
        assert abs(W.dot3(u[qa >> 1], u[qb >> 1])) < 1e-9
    centre = int(np.nonzero(out["degree"] == 6)[0][0])
    assert np.abs(out["junctions3d"][centre] - nodes[13]).max() <= 1e-9 and (out["votes"] == 4).all()
    assert np.array_equal(np.sort(d.argmin(axis=1)[out["edges3d"]], axis=1), np.sort(ends, axis=1))


@pytest.mark.parametrize("name", sorted(W.cases()))
def test_no_device_input_has_a_decision_at_its_threshold(name):
    a, kw = W.cases()[name]
    out = run(a, **kw)
    print(name, out["junctions3d"].shape[0], "vertices", out["edges3d"].shape[0], "edges", len(out["links"]), "links", out["pairs"], "votes cast", out["margins"])
    assert all(m > MARGIN for m in out["margins"].values()), out["margins"]
    if name.startswith("fan"):
        m = int(name.split("_")[1])
        assert out["degree"].max() == m and out["pairs"] == 3 * m * (m - 1) // 2 and out["junctions3d"].shape[0] == m + 1
    if name.startswith("twice"):
        assert len(out["links"]) == (1 if kw["min_votes"] == 2 else 0) and out["pairs"] == 2


def test_the_size_query():
    """Python allocates the workspace from this query, so its values are part of the ABI: tests/wireframe3d_sizes.json holds them as
    the built library gave them."""
    from neat_amd import _lib
    size = _lib.lib().neat_wf3d_scratch_bytes
    assert size(0, 0, 0, 0, 0) > 0 and size(3, 10, 5, 12, 100) % 256 == 0
    for args in ((-1, 0, 0, 0, 0), (1, -1, 0, 1, 0), (1, 1, -1, 1, 0), (1, 1, 1, -1, 0), (1, 1, 1, 1, -1), (65536, 1, 1, 1, 1), (1, 1, 2 ** 23, 1, 1),
                 (1, 2 ** 31 // 6 + 1, 1, 1, 1), (1, 1, 1, 1, 2 ** 31), (0, 1, 1, 1, 1), (1, 1, 1, 0, 1)):
        assert size(*args) == 0, args
    assert size(65535, 2 ** 31 // 6 - 1, 2 ** 23 - 1, 2 ** 31 - 1, 2 ** 31 - 1) > 0
    table = json.load(open(SIZES))
    assert sorted(tuple(row[:5]) for row in table) == [(1, 1, 1, 2, 1), (3, 771, 257, 774, 100000), (12, 150, 17, 140, 4096), (64, 128000, 40000, 90000, 512000)]
    for *args, want in table:
        assert size(*args) == want, args
