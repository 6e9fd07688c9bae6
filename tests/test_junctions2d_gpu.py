"""GPU tests of detect.junctions (csrc/kernels_wireframe2d.hpp) against the float64 definition tests/junctions2d_f64.py.

Every array must be the reference's: the integer arrays equal, the float64 arrays the same bits.  Both sides form each vertex from the
same IEEE operations in the same order without contraction (products, sums, one division a coordinate, one square root for the
spread), so no tolerance is needed and none is given.  tests/test_junctions2d_math.py asserts that no decision of these inputs lies
within 1e-9 of its threshold.  The inputs are the smallest that reach every path: views of 0, 1 and 2 segments, segments that take
part in nothing, a view of the pair tile's size and one less and more with a junction and a T across tiles, a component across three
tiles, junctions of 63, 64 and 65 ends (a wavefront walks the members 64 at a time), ragged views, duplicate and collapsed segments."""
import os

import numpy as np
import pytest
import torch

from tests import closed_loop as C
from tests import junctions2d_f64 as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz")
FLOATS = ("vertices", "score", "spread", "eweight")
INTS = ("degree", "kind", "t_edge", "voff", "ends", "edges", "esrc", "eoff")
CASES = J.cases()


def dev():
    return torch.device("cuda:0")


def device_build(seg, off, weight, host_offsets=True, **kw):
    from neat_amd import detect
    offsets = np.asarray(off) if host_offsets else torch.as_tensor(np.asarray(off, dtype=np.int32)).to(dev())
    res = detect.junctions(torch.tensor(np.asarray(seg, np.float64).reshape(-1, 4), device=dev()), torch.tensor(np.asarray(weight, np.float64), device=dev()),
                           offsets, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(got, want):
    assert want["margin"] >= 1e-9                                        # no decision of the input is near its threshold
    for k in INTS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert sorted(got) == sorted(INTS + FLOATS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_reference(name):
    seg, off, weight = CASES[name]
    want = J.build(seg, off, weight)
    got = device_build(seg, off, weight)
    print(f"{name}: {seg.shape[0]} segments, {want['vertices'].shape[0]} vertices, {want['edges'].shape[0]} edges, kinds {np.bincount(want['kind'], minlength=3).tolist()}")
    same(got, want)
    same(device_build(seg, off, weight, host_offsets=False), want)       # offsets on the device: the grid sized for S segments a view
    if name in ("tile_257", "tee_two_bars", "star_65"):
        kw = {"t_junctions": False, "gap": 2.5, "frac": 0.3, "angle": 20.0}
        same(device_build(seg, off, weight, **kw), J.build(seg, off, weight, **kw))


@pytest.mark.gpu
def test_lattice_equals_the_reference_and_its_nodes():
    seg, nodes = J.lattice(11, 11)
    weight = np.linspace(0.1, 0.9, seg.shape[0])
    got = device_build(seg, [0, seg.shape[0]], weight)
    same(got, J.build(seg, [0, seg.shape[0]], weight))
    assert got["vertices"].shape == (144, 2) and np.bincount(got["degree"]).tolist() == [0, 0, 4, 40, 100]
    assert np.linalg.norm(got["vertices"][:, None] - nodes[None], axis=2).min(axis=1).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_closed_loop_scenes_equal_the_reference(name):
    sc = C.scene(name)
    seg = np.concatenate(sc["det_segs"])
    off = np.concatenate([[0], np.cumsum([len(s) for s in sc["det_segs"]])])
    weight = 1.0 - 10.0 ** -sc["det"]["nfa"]
    want = J.build(seg, off, weight)
    assert (want["kind"] == 1).sum() >= 2 * C.VIEWS
    same(device_build(seg, off, weight), want)


@pytest.mark.gpu
def test_fixture_views_batch_and_determinism():
    """The eight fixture views' detected segments: the device equals the reference, two calls give the same bytes, and a batch gives
    each view's own result."""
    from neat_amd import detect
    images = torch.from_numpy(np.load(FIXTURE)["images"]).to(dev())
    lines, _, nfa, _, _, offsets = detect.lines(images)
    weight = detect.nfa_weight(nfa).double().to(dev())
    seg = lines.float().double()
    off = offsets.cpu().numpy()
    want = J.build(seg.cpu().numpy(), off, weight.cpu().numpy())
    a, b = detect.junctions(seg, weight, offsets), detect.junctions(seg, weight, offsets)
    same({k: v.cpu().numpy() for k, v in a.items()}, want)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    print(f"{seg.shape[0]} segments, {2 * seg.shape[0]} soup vertices, {want['vertices'].shape[0]} built vertices, "
          f"{int((want['kind'] == 1).sum())} junctions, {int((want['kind'] == 2).sum())} T ends, {want['edges'].shape[0]} edges")
    assert 0 < want["vertices"].shape[0] < 2 * seg.shape[0] and (want["kind"] == 1).any()
    for v in range(images.shape[0]):
        alone = detect.junctions(seg[off[v]:off[v + 1]], weight[off[v]:off[v + 1]], [0, int(off[v + 1] - off[v])])
        part = J.view_of(want, v)
        for k in part:
            assert alone[k].cpu().numpy().tobytes() == part[k].tobytes(), (v, k)
    wfs = detect.wireframes(lines, nfa, offsets, images.shape[1], images.shape[2])
    assert len(wfs) == 8 and [wf.vertices.shape[0] for wf in wfs] == np.diff(want["voff"]).tolist()
    assert wfs[0].vertices.dtype == torch.float32 and wfs[0].edges.dtype == torch.long and wfs[0].kind == J.view_of(want, 0)["kind"].tolist()


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    from neat_amd import _lib, detect
    seg, off, weight = CASES["tiny_views"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        detect.junctions(torch.tensor(seg), torch.tensor(weight), off)
    d = lambda x: torch.tensor(x, device=dev())
    for kw in ({"gap": 0.0}, {"frac": 0.5}, {"angle": 0.0}, {"angle": 91.0}, {"gap": float("nan")}):
        with pytest.raises(ValueError):
            detect.junctions(d(seg), d(weight), off, **kw)
    for bad in ([0, 1, 2], [1, 2, 3], [0, 2, 1, 3]):
        with pytest.raises(ValueError):
            detect.junctions(d(seg), d(weight), bad)
    with pytest.raises(RuntimeError):
        detect.junctions(d(seg)[:, :3], d(weight), off)
    lib = _lib.lib()
    assert lib.neat_wf2d_scratch_bytes(3, 3, 2) > 0 and lib.neat_wf2d_scratch_bytes(0, 0, 0) == 0
    for args in ((-1, 0, 0), (1, -1, 0), (1, 3, 4), (0, 3, 3), (1, 3, 0), (65536, 3, 3), (1, 2 ** 31 // 10 + 1, 1)):
        assert lib.neat_wf2d_scratch_bytes(*args) == 0, args
    ws = torch.empty(lib.neat_wf2d_scratch_bytes(3, 3, 2), dtype=torch.uint8, device=dev())
    out = detect.junctions(d(seg), d(weight), off)
    p = _lib.ptr
    segoff, dseg, dweight = d(np.asarray(off, np.int32)), d(seg), d(weight)          # held: the calls take addresses
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev())
    bufs = dict(vertices=f64(6, 2), degree=i32(6), kind=i32(6), score=f64(6), spread=f64(6), t_edge=i32(6), voff=i32(4), ends=i32(3, 2),
                edges=i32(3, 2), eweight=f64(3), esrc=i32(3), eoff=i32(4))
    call = lambda V=3, S=3, nmax=2, gap=4.0, frac=0.4, smin=0.17, w=ws, **repl: lib.neat_wf2d_build(
        p(dseg), p(segoff), p(dweight), V, S, nmax, gap, frac, smin, 1, p(w) if w is not None else None,
        *(None if repl.get(k, 1) is None else p(bufs[k]) for k in detect.JUNCTION_KEYS), _lib.stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert bufs["voff"].tolist() == out["voff"].tolist() and torch.equal(bufs["vertices"][:5], out["vertices"])
    for kw in ({"V": -1}, {"S": -1}, {"nmax": 4}, {"nmax": 0}, {"gap": 0.0}, {"frac": 0.5}, {"smin": 0.0}, {"smin": 1.5}, {"w": None}, {"voff": None},
               {"eoff": None}, {"vertices": None}, {"ends": None}, {"esrc": None}):
        assert call(**kw) == -1, kw
