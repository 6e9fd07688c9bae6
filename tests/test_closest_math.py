"""CPU: the closest-point rule of tests/closest_f64.py against a formula that shares nothing with it, on hand-made triangles
where the answer is known exactly, and the argument checks of neat_raycast_closest, which touch no device.

Rule against candidate_distance, the largest |sqrt(d2) - candidate| over the queries of each scene, as observed here: icosphere 3
3.3e-16, icosphere 4 2.2e-16, box 2.2e-16, strips(64) 0.  The bar is 1e-12: the scenes are of unit scale, and the candidate
formula cancels differently on thin triangles."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import closest_f64 as CP

INF = float("inf")
SCENES = {"ico3": lambda: CP.icosphere(3), "ico4": lambda: CP.icosphere(4), "box": lambda: CP.box(), "strips": lambda: CP.strips(64)}


def _queries(verts, faces, seed):
    rng = np.random.default_rng(seed)
    edges = CP.mesh_edges(faces)
    e = edges[rng.choice(len(edges), min(64, len(edges)), replace=False)]
    v = verts[rng.choice(len(verts), min(64, len(verts)), replace=False)]
    return np.concatenate([rng.uniform(-1.5, 1.5, (256, 3)), v, (verts[e[:, 0]] + verts[e[:, 1]]) / 2, np.zeros((1, 3))])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_rule_agrees_with_the_candidate_formula(name):
    verts, faces = SCENES[name]()
    tv = verts[faces]
    pts = _queries(verts, faces, 5)
    d2, tri, q, uv = CP.closest_all(verts, faces, pts)
    assert (tri >= 0).all() and np.isfinite(d2).all()
    worst = 0.0
    for i, p in enumerate(pts):
        cand = CP.candidate_distance(tv, p)
        worst = max(worst, abs(math.sqrt(d2[i]) - cand.min()))
        assert abs(cand[tri[i]] - cand.min()) <= 1e-12                 # the triangle it names is a closest one
    print("  %s: %d queries, max |sqrt(d2) - candidate| %.3g" % (name, len(pts), worst))
    assert worst <= 1e-12
    # q is the point the barycentrics name, and it is as far from p as d2 says
    t = tv[tri]
    recon = (1.0 - uv[:, :1] - uv[:, 1:]) * t[:, 0] + uv[:, :1] * t[:, 1] + uv[:, 1:] * t[:, 2]
    assert np.abs(recon - q).max() <= 1e-15 and (uv >= 0).all() and (uv.sum(1) <= 1 + 1e-15).all()
    assert np.abs(np.linalg.norm(pts - q, axis=1) - np.sqrt(d2)).max() <= 1e-15


def test_every_region_is_reached_with_its_point_and_barycentrics():
    tv = np.array([[[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]])
    cases = [("A", (-1.0, -1.0, 2.0), (0.0, 0.0, 0.0), (0.0, 0.0)), ("B", (6.0, -1.0, 1.0), (4.0, 0.0, 0.0), (1.0, 0.0)),
             ("AB", (1.0, -2.0, 1.0), (1.0, 0.0, 0.0), (0.25, 0.0)), ("C", (-1.0, 6.0, 1.0), (0.0, 4.0, 0.0), (0.0, 1.0)),
             ("AC", (-2.0, 3.0, 1.0), (0.0, 3.0, 0.0), (0.0, 0.75)), ("BC", (4.0, 2.0, 1.0), (3.0, 1.0, 0.0), (0.75, 0.25)),
             ("in", (1.0, 2.0, -3.0), (1.0, 2.0, 0.0), (0.25, 0.5))]
    seen = []
    for name, p, q_want, uv_want in cases:
        d2, q, uv, region = CP.rule(tv, np.array(p))
        seen.append(CP.REGIONS[int(region[0])])
        assert seen[-1] == name, (name, seen[-1])
        assert np.array_equal(q[0], q_want) and np.array_equal(uv[0], uv_want), (name, q, uv)
        assert d2[0] == sum((x - y) ** 2 for x, y in zip(p, q_want)), name
        one = CP.closest_one(tv, np.array([True]), p)
        assert one[0] == d2[0] and one[1] == 0 and np.array_equal(one[2], q_want) and np.array_equal(one[3], uv_want)
    assert seen == list(CP.REGIONS)
    # the inclusive comparisons, in the book's order: on the line through A perpendicular to AB the vertex region wins over the edge's
    assert CP.REGIONS[int(CP.rule(tv, np.array([0.0, -1.0, 0.0]))[3][0])] == "A"
    assert CP.REGIONS[int(CP.rule(tv, np.array([4.0, -1.0, 0.0]))[3][0])] == "B"
    assert CP.REGIONS[int(CP.rule(tv, np.array([2.0, 0.0, 0.0]))[3][0])] == "AB"             # on the edge itself: vc = 0


def test_exact_zeros():
    tv = np.array([[[0.5, 0.25, -1.0], [2.5, 0.25, -1.0], [0.5, 1.25, 3.0]]])                # dyadic coordinates
    a, b, c = tv[0]
    for p in (a, b, c, (a + b) / 2, (b + c) / 2, (a + c) / 2, a + 0.25 * (b - a) + 0.5 * (c - a), a + 0.125 * (b - a) + 0.125 * (c - a)):
        d2, q, _, _ = CP.rule(tv, p)
        assert d2[0] == 0.0 and np.array_equal(q[0], p), p
    verts, faces = CP.icosphere(2)
    d2, tri, q, _ = CP.closest_all(verts, faces, verts)
    assert (d2 == 0.0).all() and np.array_equal(q, verts)
    assert np.array_equal(tri, [min(g for g in range(len(faces)) if i in faces[g]) for i in range(len(verts))])


def test_ties_go_to_the_lowest_face_index():
    verts, faces = CP.box()
    p = np.array([[0.7, 0.1, 0.05], [0.0, 0.0, 0.0], [0.9, 0.9, 0.9]])
    ref = CP.closest_all(verts, faces, p)
    twice = CP.closest_all(verts, np.concatenate([faces, faces]), p)                         # every face a second time: the first wins
    assert all(np.array_equal(x, y) for x, y in zip(ref, twice))
    back = CP.closest_all(verts, np.concatenate([faces[::-1], faces]), p)
    assert np.array_equal(back[0], ref[0]) and (back[1] < len(faces)).all()                 # never the later copy
    # a shared edge: the two triangles of a quad, queried above the diagonal, and both orders of the two
    quad = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    on_diagonal = np.array([[0.5, 0.5, 0.25], [0.25, 0.25, 1.0], [1.0, 1.0, 2.0], [2.0, 2.0, 0.0]])
    for order in (f, f[::-1]):
        d2, tri, q, _ = CP.closest_all(quad, order, on_diagonal)
        both = CP.rule(quad[order][None], on_diagonal[:, None, :])[0]
        assert (both[:, 0] == both[:, 1]).all()                                              # a tie in d2, to the last bit
        assert (tri == 0).all()
        assert np.array_equal(q, [[0.5, 0.5, 0.0], [0.25, 0.25, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0]])


def test_the_bound_is_inclusive():
    verts, faces = CP.box()
    p = np.array([[0.75, 0.1, 0.05]])                                                        # 0.25 from the face x = 0.5
    d2, tri, _, _ = CP.closest_all(verts, faces, p)
    assert d2[0] == 0.0625 and tri[0] >= 0
    at = CP.closest_all(verts, faces, p, max_d2=0.0625)
    assert at[0][0] == 0.0625 and at[1][0] == tri[0]
    below = CP.closest_all(verts, faces, p, max_d2=np.nextafter(0.0625, 0.0))
    assert below[0][0] == INF and below[1][0] == -1 and not below[2].any() and not below[3].any()
    zero = CP.closest_all(verts, faces, np.stack([verts[7], p[0]]), max_d2=0.0)              # only a point of the mesh itself is within 0
    assert zero[0].tolist() == [0.0, INF] and zero[1][0] >= 0 and zero[1][1] == -1


def test_never_closest_inputs():
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [0.0, 1.0, 5.0],
                      [np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0]])
    faces = np.array([[0, 1, 3], [0, 0, 1], [7, 1, 2], [8, 1, 2], [4, 5, 6], [1, 1, 1]], np.int32)      # collinear, repeated, NaN, inf, good, point
    p = np.array([[0.25, 0.0, 0.0], [0.0, 0.0, 0.1], [0.3, 0.3, 4.0]])
    d2, tri, q, _ = CP.closest_all(verts, faces, p)
    assert (tri == 4).all() and np.array_equal(q[:, 2], [5.0, 5.0, 5.0]) and np.isfinite(d2).all()
    none = CP.closest_all(verts, faces[[0, 1, 2, 3, 5]], p)
    assert (none[1] == -1).all() and np.isinf(none[0]).all()
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [0.3, 0.3, 4.0]])
    d2, tri, q, uv = CP.closest_all(verts, faces, bad)
    assert tri.tolist() == [-1, -1, -1, 4] and np.isinf(d2[:3]).all() and not q[:3].any() and not uv[:3].any()
    assert CP.closest_one(verts[faces], CP.valid_triangles(verts, faces), bad[0])[1] == -1
    # the empty mesh and the refused one
    assert (CP.closest_all(verts, faces[:0], p)[1] == -1).all()
    assert (CP.closest_all(verts, np.array([[0, 1, 9]], np.int32), p)[1] == -1).all()


def test_line_points_are_the_formula_bit_for_bit():
    from neat_amd import raycast
    rng = np.random.default_rng(3)
    lines = rng.standard_normal((17, 2, 3)) * np.array([1.0, 1e3, 1e-3])
    for samples in (2, 3, 16, 32, 33):
        t = np.linspace(0, 1, samples).reshape(1, -1, 1)
        want = (lines[:, :1] * t) + (lines[:, 1:] * (1 - t))
        got = raycast.line_points(torch.from_numpy(lines), samples).numpy()
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), samples
        assert CP.line_samples(lines, samples).tobytes() == want.tobytes()
    assert np.array_equal(got[:, 0], lines[:, 1]) and np.array_equal(got[:, -1], lines[:, 0])          # t = 0 is the second end point
    with pytest.raises(ValueError):
        raycast.line_distance(None, torch.from_numpy(lines), samples=1)


def test_closest_rejects_bad_arguments_before_any_launch():
    """neat_raycast_closest validates on the host and returns -1 without touching a device (so this runs without a GPU)."""
    from neat_amd import _lib
    lib = _lib.lib()
    assert "neat_raycast_closest" in _lib.exported_symbols()
    size = lib.neat_raycast_bvh_bytes(12)
    buf = (ctypes.c_ubyte * (size + 4096))()
    base = (ctypes.addressof(buf) + 255) & ~255
    out = (ctypes.c_double * 64)()
    o = ctypes.addressof(out)

    def call(bvh=base, nf=12, points=o, N=4, max_d2=INF, d2=o, tri=o, point=o, uv=o, counts=None):
        return lib.neat_raycast_closest(bvh, nf, points, N, max_d2, d2, tri, point, uv, counts, None)
    assert call(N=0) == 0 and call(N=0, points=None, d2=None, tri=None, point=None, uv=None) == 0        # nothing to do: no launch
    assert call(N=-1) == -1
    assert call(nf=-1) == -1 and call(nf=(1 << 24) + 1) == -1
    assert call(max_d2=-1.0) == -1 and call(max_d2=float("nan")) == -1 and call(max_d2=-0.5, N=0) == -1
    assert call(bvh=None) == -1 and call(bvh=base + 8) == -1
    for name in ("points", "d2", "tri", "point", "uv"):
        assert call(**{name: None}) == -1, name


def test_python_layer_refuses_what_the_library_would():
    from neat_amd import ops, raycast
    with pytest.raises(RuntimeError):
        ops.raycast_closest(torch.zeros(8, dtype=torch.uint8), 0, torch.zeros(4, 3, dtype=torch.float64))      # no CPU path
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            raycast.closest(None, torch.zeros(4, 3), max_dist=bad)
