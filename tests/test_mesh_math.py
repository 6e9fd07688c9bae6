"""CPU: the marching-tetrahedra definitions of DESIGN 3b through their float64 restatement (tests/mesh_f64.py) on analytic grids --
closedness, orientation, Euler characteristic, components, second-order vertex error --, the 16-case table, the literal tables of
csrc/kernels_mesh.hpp against the restatement's rules, the linspace rule of the grid nodes, the PLY writer and the argument checks of
the C entry points (no device work)."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import mesh_f64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B0, B1 = -1.5, 1.5
C0 = np.array([0.013, -0.007, 0.021])       # offsets that put no node on the level


def sphere(c, r):
    return lambda p: np.linalg.norm(p - np.asarray(c, dtype=np.float64), axis=-1) - r


def torus(c, R, r):
    def f(p):
        q = p - np.asarray(c, dtype=np.float64)
        return np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - R) ** 2 + q[..., 2] ** 2) - r
    return f


def union(f, g):
    return lambda p: np.minimum(f(p), g(p))


def sample(fn, shape, b0=B0, b1=B1):
    axes = [M.linspace_f32(b0, b1, n).astype(np.float64) for n in shape]
    return fn(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1))


def gradient(fn, p, h=1e-6):
    e = np.eye(3) * h
    return np.stack([(fn(p + e[a]) - fn(p - e[a])) / (2 * h) for a in range(3)], axis=-1)


def check_orientation(fn, verts, faces):
    """Every non-degenerate face normal has a positive dot product with the analytic gradient at the centroid -> share of degenerate faces."""
    n = M.face_normals(verts, faces)
    length = np.linalg.norm(n, axis=1)
    good = length > 1e-14
    g = gradient(fn, verts[faces].mean(axis=1))
    assert (np.einsum("ij,ij->i", n, g)[good] > 0).all()
    return 1.0 - good.mean()


CLOSED = {
    "sphere33": (sphere(C0, 0.5), (33, 33, 33), 2, 1),
    "sphere100": (sphere(C0, 0.5), (100, 100, 100), 2, 1),
    "torus": (torus(C0, 0.7, 0.25), (49, 49, 33), 0, 1),
    "two_spheres": (union(sphere(C0 + [0.6, 0, 0], 0.3), sphere(C0 - [0.6, 0.1, 0], 0.35)), (41, 37, 33), 4, 2),
}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_surfaces_are_oriented_manifolds(name):
    fn, shape, chi, ncomp = CLOSED[name]
    g = sample(fn, shape)
    assert not (g == 0).any()
    verts, faces = M.extract(g, B0, B1)
    assert len(verts) > 100 and faces.min() == 0 and faces.max() == len(verts) - 1
    ne, ok, _ = M.edge_report(faces)
    assert ok.all()                                             # every edge in exactly two faces, once in each direction
    assert len(verts) - ne + len(faces) == chi
    assert len(np.unique(M.components(len(verts), faces))) == ncomp
    degenerate = check_orientation(fn, verts, faces)
    print(name, "vertices", len(verts), "faces", len(faces), "degenerate share", degenerate)
    assert degenerate < 0.01


def test_surface_cut_by_the_grid_boundary_is_open_only_there():
    fn = sphere([1.3, 0.02, -0.01], 0.5)
    g = sample(fn, (41, 41, 41))
    verts, faces = M.extract(g, B0, B1)
    _, ok, edges = M.edge_report(faces)
    assert (~ok).any()
    ends = verts[edges[~ok]]                                    # [boundary edges, 2, 3]
    on_face = (np.abs(ends[..., 0] - np.float32(B1)) == 0).all(axis=1)
    assert on_face.all()                                        # boundary edges lie in the grid face x = b1 and nowhere else
    assert check_orientation(fn, verts, faces) < 0.01


def test_vertices_converge_to_the_level_set_at_second_order():
    fn = sphere(C0, 0.5)
    err = {}
    for n in (33, 65):
        verts, _ = M.extract(sample(fn, (n, n, n)), B0, B1)
        err[n] = np.abs(fn(verts)).max()
    h = 3.0 / 32
    print("max |sdf(vertex)|: n=33 %.3e, n=65 %.3e, ratio %.3f; h^2 / (8 r) at n=33 = %.3e" % (err[33], err[65], err[33] / err[65], h * h / 4))
    assert 3.0 <= err[33] / err[65] <= 5.0                     # second order; the device is held to the restatement, not to the sphere


def _tet_triangles(points, values, level=0.0):
    """The case table applied to one positively oriented tetrahedron -> list of triangles [3, 3]."""
    mask = sum(1 << l for l in range(4) if values[l] < level)
    out = []
    for tri in M.case_table()[mask]:
        vs = []
        for a, b in tri:
            s, e = (a, b) if values[a] < level else (b, a)
            t = (level - values[s]) / (values[e] - values[s])
            vs.append(points[s] + t * (points[e] - points[s]))
        out.append(np.stack(vs))
    return out


def test_case_table_complement_and_orientation_preserving_permutations():
    table = M.case_table()
    assert [len(t) for t in table] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    rot = lambda tri: min(tuple(tri[i:] + tri[:i]) for i in range(3))
    for mask in range(16):                                       # a case and its complement: the same triangles, reversed
        a = sorted(rot(list(t)) for t in table[mask])
        b = sorted(rot(list(t)[::-1]) for t in table[15 - mask])
        assert a == b, mask
    rng = np.random.default_rng(5)
    even = [p for p in itertools.permutations(range(4)) if M._even(p)]
    assert len(even) == 12
    for mask in range(1, 15):
        pts = rng.normal(size=(4, 3))
        if np.linalg.det(pts[1:] - pts[0]) < 0:
            pts[[1, 2]] = pts[[2, 1]]
        vals = np.where([(mask >> l) & 1 for l in range(4)], -1.0, 1.0) * rng.uniform(0.2, 1.0, 4)
        grad = np.linalg.solve(np.c_[pts, np.ones(4)], vals)[:3]          # the linear interpolant's gradient
        ref = _tet_triangles(pts, vals)
        area = sum(np.cross(t[1] - t[0], t[2] - t[0]) for t in ref) / 2
        assert np.dot(area, grad) > 0 and np.allclose(np.cross(area, grad), 0, atol=1e-12)      # outwards, in the level plane
        key = lambda tris: sorted(tuple(np.round(v, 9)) for t in tris for v in t)
        for p in even:
            got = _tet_triangles(pts[list(p)], vals[list(p)])
            assert len(got) == len(ref)
            assert np.allclose(sum(np.cross(t[1] - t[0], t[2] - t[0]) for t in got) / 2, area, atol=1e-12), (mask, p)
            assert set(key(got)) == set(key(ref)), (mask, p)


def test_kernel_tables_equal_the_restatement():
    text = open(os.path.join(ROOT, "neat_amd", "csrc", "kernels_mesh.hpp")).read()

    def table(name):
        body = re.search(name + r"(?:\[\d+\])+\s*=\s*(\{.*?\});", text, flags=re.S).group(1)
        return json.loads(body.replace("{", "[").replace("}", "]"))
    assert [tuple(t) for t in table("MESH_TET")] == M.tetrahedra()
    cases = M.case_table()
    assert table("MESH_NTRI") == [len(c) for c in cases]
    for mask, row in enumerate(table("MESH_TRI")):
        want = [(a << 2) | b for tri in cases[mask] for a, b in tri]
        assert row == want + [0] * (6 - len(want)), mask
    assert int(re.search(r"MESH_TILE\s*=\s*(\d+)", text).group(1)) == 2048      # tests/test_mesh_gpu.py sizes its tile-edge cases by it


def test_tetrahedra_tile_the_cell_and_share_face_diagonals():
    tets = M.tetrahedra()
    vol = 0.0
    for t in tets:
        m = np.stack([M._corner_vec(t[l]) - M._corner_vec(t[0]) for l in (1, 2, 3)])
        assert np.linalg.det(m) > 0
        vol += np.linalg.det(m) / 6
        assert all((min(a, b) & max(a, b)) == min(a, b) for a, b in itertools.combinations(t, 2))      # every edge goes up: one owner, one class
    assert abs(vol - 1.0) < 1e-12
    # the diagonal of the face x = 0 (corners 0..3) is 0-3, that of x = 1 (4..7) is 4-7: the same offset, so neighbours agree; same for y, z
    diag = {frozenset((a, b)) for t in tets for a, b in itertools.combinations(t, 2) if bin(a ^ b).count("1") == 2}
    assert diag == {frozenset(p) for p in ((0, 3), (4, 7), (0, 5), (2, 7), (0, 6), (1, 7))}


def test_linspace_rule_is_numpy_linspace():
    from neat_amd import mesh
    confs = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_confs.json")))
    blocks = [c["plot"] for c in confs.values() if "plot" in c]
    assert len(blocks) == 8
    cases = {(float(b["grid_boundary"][0]), float(b["grid_boundary"][1]), int(b["resolution"])) for b in blocks}
    cases |= {(lo, hi, n) for n in (2, 3, 100, 512) for lo, hi in ((-1.5, 1.5), (-1.0, 1.0), (-0.7, 2.3), (0.1, 0.30000001))}
    for lo, hi, n in sorted(cases):
        want = np.linspace(lo, hi, n).astype(np.float32)
        assert np.array_equal(mesh.linspace_f32(lo, hi, n), want), (lo, hi, n)
        assert np.array_equal(M.linspace_f32(lo, hi, n), want), (lo, hi, n)
    with pytest.raises(ValueError):
        mesh.linspace_f32(0, 1, 1)


def test_ply_round_trip(tmp_path):
    from neat_amd import ply
    rng = np.random.default_rng(0)
    v = rng.normal(size=(11, 3)).astype(np.float32)
    n = rng.normal(size=(11, 3)).astype(np.float32)
    f = rng.integers(0, 11, size=(7, 3)).astype(np.int32)
    for normals in (n, None):
        path = str(tmp_path / "m.ply")
        ply.write_ply(path, v, f, normals)
        v2, n2, f2 = M.read_ply(path)
        assert np.array_equal(v2, v) and np.array_equal(f2, f)
        assert (n2 is None) if normals is None else np.array_equal(n2, n)
        assert not os.path.exists(path + ".tmp")
    with pytest.raises(ValueError):
        ply.write_ply(str(tmp_path / "bad.ply"), v, f, n[:3])


def test_entry_points_check_their_arguments_before_any_launch():
    import ctypes
    from neat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.lib()
    names = ("neat_grid_points", "neat_mesh_ws_bytes", "neat_mesh_count", "neat_mesh_emit", "neat_unit_rows3")
    for name in names:
        assert name in _lib.exported_symbols()
        assert not hasattr(lib, "f16_" + name)                 # compiled once: no 16-bit twin
    assert lib.neat_abi_version() == _lib.ABI_VERSION
    ws = lib.neat_mesh_ws_bytes
    assert ws(1, 2, 2) == 0 and ws(2, 2, 1) == 0 and ws(-5, 2, 2) == 0
    assert ws(2048, 2048, 512) == 0 and ws(65536, 65536, 2) == 0          # 2^31 nodes and more are not indexed
    for n in ((2, 2, 2), (100, 100, 100), (512, 512, 512), (1024, 1024, 1024)):
        nodes = n[0] * n[1] * n[2]
        assert 5 * nodes <= ws(*n) <= 32 * nodes + 4096, n
    assert ws(512, 512, 512) <= 32 * 512 ** 3
    i3, d3 = ctypes.c_int * 3, ctypes.c_double * 3
    lo, hi = d3(-1.5, -1.5, -1.5), d3(1.5, 1.5, 1.5)
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert lib.neat_grid_points(None, 64, 0, 8, i3(2, 2, 2), lo, hi, None) == -1          # null destination
    assert lib.neat_grid_points(p, 64, 0, 8, i3(2, 1, 2), lo, hi, None) == -1             # an axis under 2 nodes
    assert lib.neat_grid_points(p, 4, 0, 8, i3(2, 2, 2), lo, hi, None) == -1              # stride below the count
    assert lib.neat_grid_points(p, 64, 1, 8, i3(2, 2, 2), lo, hi, None) == -1             # past the last node
    assert lib.neat_grid_points(p, 64, 0, 8, None, lo, hi, None) == -1
    assert lib.neat_grid_points(p, 64, 0, 8, i3(2, 2, 2), d3(float("nan"), 0, 0), hi, None) == -1
    assert lib.neat_mesh_count(None, 2, 2, 2, 0.0, p, p, None) == -1
    assert lib.neat_mesh_count(p, 2, 2, 2, 0.0, None, p, None) == -1
    assert lib.neat_mesh_count(p, 2, 2, 2, 0.0, p, None, None) == -1
    assert lib.neat_mesh_count(p, 2, 1, 2, 0.0, p, p, None) == -1
    assert lib.neat_mesh_count(p, 2048, 2048, 512, 0.0, p, p, None) == -1
    assert lib.neat_mesh_count(p, 2, 2, 2, float("nan"), p, p, None) == -1
    assert lib.neat_mesh_emit(None, 2, 2, 2, lo, hi, 0.0, p, p, 1, p, 1, None) == -1
    assert lib.neat_mesh_emit(p, 2, 2, 2, lo, hi, 0.0, p, None, 1, p, 1, None) == -1      # vertices expected, no room given
    assert lib.neat_mesh_emit(p, 2, 2, 2, lo, hi, 0.0, p, p, -1, p, 1, None) == -1
    assert lib.neat_mesh_emit(p, 2, 2, 2, None, hi, 0.0, p, p, 1, p, 1, None) == -1
    assert lib.neat_mesh_emit(p, 2, 2, 2, lo, hi, 0.0, p, None, 0, None, 0, None) == 0    # an empty mesh: nothing to launch
    assert lib.neat_unit_rows3(None, 0, None) == 0 and lib.neat_unit_rows3(None, 5, None) == -1 and lib.neat_unit_rows3(p, -1, None) == -1


def test_cpu_grids_are_refused():
    import torch
    from neat_amd import mesh
    with pytest.raises(RuntimeError):
        mesh.extract(torch.zeros(3, 3, 3), -1.5, 1.5)            # no host fallback
