"""neat_amd.creases on the device against tests/creases_f64.py, the rule of DESIGN 3n in plain float64: every array equal, bit for bit."""
import numpy as np
import pytest
import torch

from tests import creases_f64 as F
from neat_amd import creases, scenegen

pytestmark = pytest.mark.gpu


def _solid(name, level, variant):
    verts, faces, _, _ = scenegen.shapes[name]
    verts, faces = scenegen.subdivide(verts, faces, level)
    if variant == "rotated":
        verts, _ = F.rotated(verts)
    elif variant == "soup":
        verts, faces = F.soup(verts, faces)
    elif variant == "reversed":
        faces = F.reverse_third(faces)
    return verts, faces


def _same(verts, faces, **kw):
    """The device's answer equals the restatement's, array for array; -> the device's."""
    want = F.lines(verts, faces, **kw)
    got = creases.lines(verts, faces, device="cuda", **kw)
    assert got.stats == want["stats"]
    for name, dtype in (("junctions", torch.float64), ("lines", torch.int32), ("kind", torch.uint8), ("curved", torch.bool), ("vertex", torch.int32)):
        g = getattr(got, name)
        assert g.is_cuda and g.dtype == dtype and tuple(g.shape) == want[name].shape, name
        g = g.cpu().numpy()
        if name == "junctions":
            assert np.array_equal(g.view(np.uint64), np.ascontiguousarray(want[name]).view(np.uint64)), name
        else:
            assert np.array_equal(g, want[name]), name
    return got


@pytest.mark.parametrize("variant", ["as_is", "rotated", "soup", "reversed"])
@pytest.mark.parametrize("name", ["box", "lblock"])
def test_solids_equal_the_restatement(name, variant):
    edges = len(scenegen.shapes[name][3])
    for level in range(4):
        got = _same(*_solid(name, level, variant))
        assert got.lines.shape[0] == edges and not bool(got.curved.any())


def test_open_box_fin_and_small_meshes():
    verts, faces = scenegen.subdivide(*F.open_box(), 2)
    assert _same(verts, faces).lines.shape[0] == 12
    assert _same(verts, faces, boundary=False).lines.shape[0] == 8
    assert sorted(_same(*F.fin()).kind.tolist()) == [0] * 11 + [1, 1, 2]
    box_v, box_f = scenegen.shapes["box"][:2]
    for nf in (0, 1, 2, 12):
        _same(box_v, box_f[:nf])
    _same(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert _same([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]]).lines.shape[0] == 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_roof_chain_lengths(n):
    """One chain of n edges along the ridge: around the wavefront, around the workgroup, and deeper than one pass of the union-find."""
    got = _same(*F.roof(n))
    assert got.lines.shape[0] == 7 and got.junctions.shape[0] == 6 and got.stats["edges"] == 3 * n + 4


def test_bent_roof_comes_out_curved():
    got = _same(*F.roof(65, bend=1e-4))
    assert int(got.curved.sum()) == 65


@pytest.mark.parametrize("half", [False, True])
def test_prisms_at_both_turns(half):
    verts, faces = F.ngon_prism(96, half)
    _same(verts, faces, turn=1.0)
    got = _same(verts, faces, turn=5.0, deviation=1e-3)
    assert int(got.curved.sum()) == (96 if half else 192)
    got = _same(verts, faces, turn=5.0, deviation=1e-3, drop_curved=True)
    assert got.vertex.tolist() == ([0, 48, 49, 97] if half else [])
    _same(verts, faces, turn=5.0, deviation=1e-3, min_len=0.1)


@pytest.mark.parametrize("angle", [30.0, 90.0, 120.0])
def test_both_branches_of_the_crease_test(angle):
    """cos(angle) >= 0 and < 0; the L block holds a reflex edge, the prism dihedral angles near 180 degrees."""
    for level in (0, 2):
        _same(*_solid("lblock", level, "reversed"), angle=angle)
    _same(*F.ngon_prism(7, False), angle=angle)
    _same(*F.ngon_prism(5, False), angle=angle)


def test_negative_zero_twins_weld():
    verts, faces = F.soup(*_solid("box", 1, "as_is"))
    verts = verts - verts.min(axis=0)                       # zeros on three sides
    verts[::2] = np.where(verts[::2] == 0.0, -0.0, verts[::2])
    assert np.signbit(verts).any()
    got = _same(verts, faces)
    assert got.lines.shape[0] == 12 and got.stats["welded"] == 26


def test_two_runs_give_the_same_bytes():
    verts, faces = F.roof(257, bend=1e-4)
    a = creases.lines(verts, faces, device="cuda")
    b = creases.lines(verts, faces, device="cuda")
    for x, y in zip(a[:5], b[:5]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a.stats == b.stats


def test_refusals_give_a_status_and_no_output():
    verts, faces = scenegen.shapes["box"][:2]
    bad = faces.copy()
    bad[5, 1] = len(verts)
    got = _same(verts, bad)
    assert got.stats["status"] == 1 and got.lines.shape[0] == 0 and got.junctions.shape[0] == 0
    bad[5, 1] = -1
    assert _same(verts, bad).stats["status"] == 1
    nan = verts.copy()
    nan[3, 2] = np.nan
    got = _same(nan, faces)
    assert got.stats["status"] == 2 and got.lines.shape[0] == 0
    nan[3, 2] = np.inf
    assert _same(nan, faces).stats["status"] == 2


def test_a_cpu_tensor_raises():
    verts, faces = scenegen.shapes["box"][:2]
    with pytest.raises(RuntimeError):
        creases.lines(torch.as_tensor(verts), torch.as_tensor(faces))
    with pytest.raises(RuntimeError):
        creases.lines(verts, faces, device="cpu")
