"""GPU tests of neat_wf3d_build (csrc/kernels_wireframe3d.hpp) and triangulate.wireframe against the float64 definition
tests/wireframe3d_f64.py.

Every array must be the reference's: the integer arrays equal, the float64 arrays the same bits.  Both sides form each vertex from the
same IEEE operations in the same order without contraction, so no tolerance is needed and none is given.  The inputs are
wireframe3d_f64.cases(): the arrays go straight to the entry point.  They are the smallest that reach every path: lattices whose rod
counts straddle the wavefront and the workgroup, two views where every link needs both, a view that votes for one pair three times, a
2-D vertex of 65 and of 257 ends whose component is as large (more than a wavefront; more than a workgroup), every empty input.  No
decision of any of them lies within 1e-6 of its threshold: asserted here on the reference's margins."""
import numpy as np
import pytest
import torch

from tests import closed_loop as C
from tests import wireframe3d_f64 as W

CASES = W.cases()
ROOM = 100000                 # pair keys the workspace holds; fan_257 casts 3 x 257 x 256 / 2 = 98688
FLOATS = ("junctions3d", "spread", "lines3d_wf")
INTS = ("degree", "kind", "votes", "edges3d", "esrc")
_refs = {}


def dev():
    return torch.device("cuda:0")


def reference(name):
    if name not in _refs:
        a, kw = CASES[name]
        _refs[name] = W.build(*W.arrays_of(a), **kw)
    return _refs[name]


def device_arrays(a):
    d = lambda x, t: torch.tensor(np.ascontiguousarray(x), dtype=t, device=dev())
    return {"lines3d": d(a["lines3d"], torch.float64), "support": d(a["support"], torch.float64), "members": d(a["members"], torch.int32),
            "estimate": d(a["estimate"], torch.float64), "endv": d(a["endv"], torch.int32), "view": d(a["view"], torch.int32)}


def raw_build(a, room=ROOM, end_frac=0.2, reach=0.25, min_votes=2, angle=10.0, t=None, counts=None, ws="own", **repl):
    """One call of the entry point on the arrays `a` -> (return code, the output tensors, counts int32 [2])."""
    from neat_amd import _lib
    lib, p = _lib.lib(), _lib.ptr
    t = t or device_arrays(a)
    N, S = a["lines3d"].shape[0], a["members"].shape[0]
    V, NV = repl.pop("V", a["V"]), repl.pop("NV", a["NV"])
    N, S = repl.pop("N", N), repl.pop("S", S)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev())
    cap = max(a["lines3d"].shape[0], 1)
    out = dict(junctions3d=f64(2 * cap, 3), degree=i32(2 * cap), kind=i32(2 * cap), votes=i32(2 * cap), spread=f64(2 * cap), edges3d=i32(cap, 2), esrc=i32(cap))
    counts = i32(2) - 7 if counts is None else counts
    if ws == "own":
        ws = torch.empty(max(lib.neat_wf3d_scratch_bytes(a["V"], a["members"].shape[0], a["lines3d"].shape[0], a["NV"], room), 256), dtype=torch.uint8, device=dev())
    ptr = lambda k: None if repl.get(k, 1) is None else p(out[k])
    code = lib.neat_wf3d_build(p(t["lines3d"]), p(t["support"]), N, p(t["members"]), p(t["estimate"]), p(t["endv"]), p(t["view"]), V, S, NV, room,
                               end_frac, reach, W.sin_min(angle) if "smin" not in repl else repl["smin"], min_votes, p(ws) if ws is not None else None,
                               ptr("junctions3d"), ptr("degree"), ptr("kind"), ptr("votes"), ptr("spread"),
                               None if repl.get("n_vertices", 1) is None else p(counts[0:1]), ptr("edges3d"), ptr("esrc"),
                               None if repl.get("n_edges", 1) is None else p(counts[1:2]), _lib.stream())
    torch.cuda.synchronize()
    return code, out, counts


def device_build(a, **kw):
    code, out, counts = raw_build(a, **kw)
    assert code == 0
    J, E = counts.tolist()
    assert 0 <= J <= 2 * a["lines3d"].shape[0] and 0 <= E <= a["lines3d"].shape[0]
    got = {k: v[:E if k in ("edges3d", "esrc") else J].cpu().numpy() for k, v in out.items()}
    got["lines3d_wf"] = got["junctions3d"][got["edges3d"]].reshape(-1, 2, 3)
    return got


def same(got, want):
    assert all(m > 1e-6 for m in want["margins"].values()), want["margins"]       # no decision of the input is near its threshold
    for k in INTS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_reference_twice(name):
    a, kw = CASES[name]
    want = reference(name)
    first, second = device_build(a, **kw), device_build(a, **kw)
    print(f"{name}: {a['lines3d'].shape[0]} lines, {a['members'].shape[0]} segments, {want['junctions3d'].shape[0]} vertices, "
          f"{int((want['kind'] == 1).sum())} junctions of up to {want['degree'].max() if want['degree'].size else 0} ends, {want['edges3d'].shape[0]} edges")
    same(first, want)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


@pytest.mark.gpu
def test_the_room_for_votes():
    """With room for exactly the votes cast the answer is the same; with less, the call says how much it needs."""
    a, _ = CASES["fan_65"]
    cast = 3 * 65 * 64 // 2
    same(device_build(a, room=cast), reference("fan_65"))
    code, _, counts = raw_build(a, room=cast - 1)
    assert code == 0 and counts.tolist() == [-1, cast]
    code, _, counts = raw_build(a, room=0)
    assert code == 0 and counts.tolist() == [-1, cast]


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    a, _ = CASES["lattice_63"]
    t = device_arrays(a)
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev())
    bad = ({"N": -1}, {"S": -1}, {"V": -1}, {"NV": -1}, {"room": -1}, {"V": 65536}, {"N": 2 ** 23}, {"S": 2 ** 31 // 6 + 1}, {"room": 2 ** 31},
           {"min_votes": 0}, {"end_frac": 0.0}, {"end_frac": 0.5}, {"reach": 0.0}, {"reach": 1.5}, {"smin": 0.0}, {"smin": 1.5},
           {"end_frac": float("nan")}, {"ws": None}, {"n_vertices": None}, {"n_edges": None}, {"junctions3d": None}, {"esrc": None})
    for kw in bad:
        code, _, _ = raw_build(a, t=t, counts=counts, **kw)
        assert code == -1, kw
    assert counts.tolist() == [-7, -7]                                     # nothing was launched: the counts were never written
    code, _, _ = raw_build(a, t=t, counts=counts)
    assert code == 0 and counts.tolist() == [reference("lattice_63")["junctions3d"].shape[0], reference("lattice_63")["edges3d"].shape[0]]


@pytest.mark.gpu
def test_wireframe_on_the_box_scene():
    """triangulate.wireframe on the box's views as graphs: the keys of triangulate.lines bit for bit, the new keys the reference's on
    those lines, and the box's wireframe: 8 junctions, 12 edges."""
    from neat_amd import triangulate
    sc = C.scene("box")
    graphs = [W.weld(s) for s in sc["segs"]]
    vertices, edges = [torch.tensor(g[0], device=dev()) for g in graphs], [torch.tensor(g[1], device=dev()) for g in graphs]
    plain = triangulate.lines([torch.tensor(s, device=dev()) for s in sc["segs"]], sc["K"], sc["poses"])
    got = triangulate.wireframe(vertices, edges, sc["K"], sc["poses"])
    assert sorted(got) == sorted(list(plain) + list(triangulate.WIREFRAME_KEYS))
    for k in plain:
        assert got[k].dtype == plain[k].dtype and got[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    host = {k: v.cpu().numpy() for k, v in got.items()}
    endv, view, _ = W.graph_arrays([g[1] for g in graphs], [g[0].shape[0] for g in graphs])
    want = W.build(host["lines3d"], host["support"], host["members"], host["estimate"], endv, view, C.VIEWS)
    same(host, want)
    assert int((host["kind"] == 1).sum()) == 8 and host["edges3d"].shape == (12, 2)
    d = np.linalg.norm(host["junctions3d"][host["kind"] == 1][:, None] - sc["junctions"][None], axis=2)
    assert d.min(axis=1).max() <= C.BAR_TRI and sorted(d.argmin(axis=1).tolist()) == list(range(8))
    small = triangulate.wireframe(vertices, edges, sc["K"], sc["poses"], pairs_max=1)           # asks again with the room the votes need
    for k in got:
        assert small[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    with pytest.raises(RuntimeError, match="no CPU path"):
        triangulate.wireframe([v.cpu() for v in vertices], [e.cpu() for e in edges], sc["K"], sc["poses"])
    for kw in ({"end_frac": 0.5}, {"reach": 0.0}, {"min_votes": 0}, {"angle": 91.0}):
        with pytest.raises(ValueError):
            triangulate.wireframe(vertices, edges, sc["K"], sc["poses"], **kw)
