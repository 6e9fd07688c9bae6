"""CPU checks of the crease rule: tests/creases_f64.py, the float64 restatement the device is held to, against answers written
out by hand; the lines.json writer; the workspace query.  No device work."""
import json
import os

import numpy as np
import pytest
import torch

from neat_amd import _lib, creases, scenegen
from tests import creases_f64 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = os.path.join(ROOT, "tests", "crease_sizes.json")
VARIANTS = ["as_is", "rotated", "soup", "reversed"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["box", "lblock"])
def test_solids_give_their_own_wireframe(name, level, variant):
    verts, faces, junctions, edges = scenegen.shapes[name]
    verts, faces = scenegen.subdivide(verts, faces, level)
    if variant == "rotated":
        verts, move = F.rotated(verts)
        junctions = move(junctions)
    elif variant == "soup":
        verts, faces = F.soup(verts, faces)
    elif variant == "reversed":
        faces = F.reverse_third(faces)
    r = F.lines(verts, faces)
    assert r["status"] == 0 and len(r["lines"]) == len(edges) == {"box": 12, "lblock": 18}[name] and not r["curved"].any()
    assert len(r["junctions"]) == len(junctions) == {"box": 8, "lblock": 12}[name] and (r["kind"] == 0).all()
    if variant != "rotated":
        assert F.coordinate_pairs(r["junctions"], r["lines"]) == F.coordinate_pairs(junctions, edges)
    else:
        # coordinates below 1, a few roundings of 2^-53 between the moved junction and the moved mesh vertex: each end within 1e-14
        near = [int(np.argmin(np.abs(junctions - p).max(axis=1))) for p in r["junctions"]]
        assert np.abs(junctions[near] - r["junctions"]).max() <= 1e-14 and len(set(near)) == len(near)
        got = {frozenset((near[a], near[b])) for a, b in r["lines"]}
        assert got == {frozenset((int(a), int(b))) for a, b in edges}


def test_open_box_and_fin():
    verts, faces = scenegen.subdivide(*F.open_box(), 2)
    r = F.lines(verts, faces)
    assert len(r["lines"]) == 12 and int((r["kind"] == 1).sum()) == 4 and int((r["kind"] == 0).sum()) == 8 and not r["curved"].any()
    assert len(F.lines(verts, faces, boundary=False)["lines"]) == 8
    r = F.lines(*F.fin())
    assert len(r["lines"]) == 14 and np.bincount(r["kind"], minlength=3).tolist() == [11, 2, 1]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_roof(n):
    r = F.lines(*F.roof(n))
    assert len(r["lines"]) == 7 and len(r["junctions"]) == 6 and np.bincount(r["kind"], minlength=3).tolist() == [1, 6, 0] and not r["curved"].any()
    assert r["vertex"].tolist() == [0, 1, 2, 3 * n, 3 * n + 1, 3 * n + 2]
    ridge = r["lines"][r["kind"] == 0][0]
    assert r["vertex"][ridge].tolist() == [1, 3 * n + 1]


def test_bent_roof_is_curved():
    r = F.lines(*F.roof(64, bend=1e-4))
    ridge = r["kind"] == 0
    assert int(ridge.sum()) == 64 and r["curved"][ridge].all() and not r["curved"][~ridge].any() and int((~ridge).sum()) == 6


def test_prisms():
    verts, faces = F.ngon_prism(96, half=False)
    r = F.lines(verts, faces, turn=1.0)
    assert len(r["lines"]) == 192 and not r["curved"].any()                    # 96 uprights, 2 x 96 rim edges that turn by 3.75 degrees; the
    r = F.lines(verts, faces, turn=5.0, deviation=1e-3)                        # side quads meet at 3.75 degrees: no creases
    assert len(r["lines"]) == 192 and r["curved"].all() and r["stats"]["chains"] == 2
    assert len(F.lines(verts, faces, turn=5.0, deviation=1e-3, drop_curved=True)["lines"]) == 0
    verts, faces = F.ngon_prism(96, half=True)
    r = F.lines(verts, faces, turn=5.0, deviation=1e-3)
    assert len(r["lines"]) == 100 and int(r["curved"].sum()) == 96
    r = F.lines(verts, faces, turn=5.0, deviation=1e-3, drop_curved=True)
    assert r["vertex"].tolist() == [0, 48, 49, 97] and r["lines"].tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]] and not r["curved"].any()


def test_smallest_meshes():
    r = F.lines([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    assert len(r["lines"]) == 3 and (r["kind"] == 1).all()
    r = F.lines(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    for name, shape, dtype in (("junctions", (0, 3), np.float64), ("lines", (0, 2), np.int32), ("kind", (0,), np.uint8), ("curved", (0,), bool),
                               ("vertex", (0,), np.int32)):
        assert r[name].shape == shape and r[name].dtype == dtype
    r = F.lines([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]])
    assert len(r["lines"]) == 4 and (r["kind"] == 1).all()
    assert F.coordinate_pairs(r["junctions"], r["lines"]) == F.coordinate_pairs(r["junctions"], [(0, 1), (1, 2), (2, 3), (3, 0)])
    # a sliver of zero area and a face that names a vertex twice are dropped
    r = F.lines([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], [[0, 1, 2], [0, 1, 1], [0, 1, 3]])
    assert r["stats"]["dropped_faces"] == 2 and len(r["lines"]) == 3
    assert F.lines([[0, 0, 0]], [[0, 1, 0]])["status"] == 1 and F.lines([[0, 0, np.inf]], np.zeros((0, 3)))["status"] == 2


def test_write_lines_reads_back_the_same_values(tmp_path):
    verts, _ = F.rotated(scenegen.shapes["lblock"][0], seed=5, scale=1.0 / 3.0)
    r = F.lines(verts, scenegen.shapes["lblock"][1])
    res = creases.Creases(torch.as_tensor(r["junctions"]), torch.as_tensor(r["lines"]), torch.as_tensor(r["kind"]), torch.as_tensor(r["curved"]),
                          torch.as_tensor(r["vertex"]), r["stats"])
    path = str(tmp_path / "deep" / "lines.json")
    creases.write_lines(path, res)
    junctions, edges = scenegen.read_lines(path)
    assert junctions.tobytes() == np.ascontiguousarray(r["junctions"]).tobytes() and np.array_equal(edges, r["lines"]) and edges.dtype == np.int32
    doc = json.load(open(path))
    assert doc["kind"] == r["kind"].tolist() and doc["curved"] == r["curved"].tolist() and sorted(doc) == ["curved", "junctions", "kind", "lines"]
    assert os.listdir(os.path.dirname(path)) == ["lines.json"]


def test_scratch_query():
    """Python allocates the workspace from this query, so its values are part of the ABI: tests/crease_sizes.json holds them as the
    built library gave them."""
    size = _lib.lib().neat_crease_scratch_bytes
    assert size(0, 0) > 0 and size(-1, 4) == 0 and size(4, -1) == 0 and size((1 << 26) + 1, 1) == 0 and size(1, (1 << 24) + 1) == 0
    grid = [0, 1, 255, 256, 257, 4096, 4097, 100000]
    for nv in grid:
        for a, b in zip(grid, grid[1:]):
            assert size(nv, a) <= size(nv, b) and size(a, nv) <= size(b, nv) and size(nv, a) % 256 == 0
    table = json.load(open(SIZES))
    assert sorted(tuple(row[:2]) for row in table) == [(1, 1), (255, 256), (256, 257), (4097, 4096)]
    for nv, nf, want in table:
        assert size(nv, nf) == want, (nv, nf)
