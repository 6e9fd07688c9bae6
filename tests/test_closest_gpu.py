"""neat_raycast_closest on the device against the float64 restatement of tests/closest_f64.py: d2, tri, point and uv equal the brute
force over all triangles bit for bit (not a tolerance), at sizes where the padding of the tree and the workgroup boundaries bite."""
import numpy as np
import pytest
import torch

from tests import closest_f64 as CP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = float("inf")
SCENES = {"ico0": lambda: CP.icosphere(0), "ico2": lambda: CP.icosphere(2), "strips": lambda: CP.strips(), "box": lambda: CP.box()}
CENTRE = {"ico0": (0.0, 0.0, 0.0), "ico2": (0.0, 0.0, 0.0), "strips": (0.5, 0.5, 0.5), "box": (0.0, 0.0, 0.0)}
_cache = {}


def _queries(verts, faces, centre, seed, n=2048):
    """n queries: half uniform in +-1.5 about the centre, an eighth each on vertices and on edge midpoints, the centre itself (on the
    icosphere every triangle is near-equidistant from it: nothing can be pruned), the rest far outside (+-1e3)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    edges = CP.mesh_edges(faces)
    e = edges[rng.integers(0, len(edges), n // 8)]
    parts = [c + rng.uniform(-1.5, 1.5, (n // 2, 3)), verts[rng.integers(0, len(verts), n // 8)], (verts[e[:, 0]] + verts[e[:, 1]]) / 2, c[None]]
    parts.append(c + rng.uniform(-1e3, 1e3, (n - sum(len(p) for p in parts), 3)))
    return np.concatenate(parts)[rng.permutation(n)]


def _reference(name):
    """Scene `name`, its 2048 queries and the brute-force answer, computed once and left unchanged."""
    if name not in _cache:
        verts, faces = SCENES[name]()
        pts = _queries(verts, faces, CENTRE[name], 21)
        _cache[name] = dict(verts=verts, faces=faces, pts=pts, ref=CP.closest_all(verts, faces, pts))
    return _cache[name]


def _ico4():
    if "ico4" not in _cache:
        _cache["ico4"] = CP.icosphere(4)
    return _cache["ico4"]


def _closest(scene, pts, max_d2=INF, counts=None):
    """The library call itself (ops.raycast_closest: d2, no square root) -> numpy (d2, tri, point, uv)."""
    from neat_amd import ops
    out = ops.raycast_closest(scene.bvh, scene.nf, torch.from_numpy(np.ascontiguousarray(pts, np.float64)).to(DEV).reshape(-1, 3), max_d2, counts)
    return tuple(x.cpu().numpy() for x in out)


def _same_bytes(got, ref, what):
    d2, tri, q, uv = got
    n = ref[0].shape[0]
    assert d2.dtype == np.float64 and tri.dtype == np.int32 and q.dtype == np.float64 and uv.dtype == np.float64, what
    assert d2.shape == (n,) and tri.shape == (n,) and q.shape == (n, 3) and uv.shape == (n, 2), what
    for name, g, r in zip(("d2", "tri", "point", "uv"), got, ref):
        r = np.ascontiguousarray(r, g.dtype)
        if g.tobytes() != r.tobytes():
            bad = np.nonzero((g != r).reshape(n, -1).any(1) | (np.signbit(g) != np.signbit(r)).reshape(n, -1).any(1))[0]
            raise AssertionError("%s: %s differs on %d of %d queries, first %d: %r != %r" % (what, name, len(bad), n, bad[0], g[bad[0]], r[bad[0]]))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_point_equals_brute_force(name):
    from neat_amd import raycast
    s = _reference(name)
    scene = raycast.build(s["verts"], s["faces"], DEV)
    assert scene.status == 0 and scene.nf == s["faces"].shape[0]
    d2, tri = s["ref"][:2]
    assert (tri >= 0).all() and np.isfinite(d2).all() and (d2 == 0).sum() >= 256 and d2.max() > 1e5
    tied = (CP.rule(s["verts"][s["faces"]][None], s["pts"][:, None, :])[0] == d2[:, None]).sum(1) > 1
    print("  %s: %d queries, %d with a tie in d2" % (name, len(d2), int(tied.sum())))
    assert tied.sum() >= 256                                   # the tie rule is exercised, not an edge case
    _same_bytes(_closest(scene, s["pts"]), s["ref"], name)


@pytest.mark.parametrize("nf", [0, 1, 2, 3, 63, 64, 65, 320, 1025, 5120])
def test_sizes_where_padding_and_workgroup_boundaries_bite(nf):
    """The first nf faces of the level-4 icosphere (1025 and 5120 make the refit cross workgroups and reach its second launch), query
    counts around the wavefront and the workgroup; the queries: uniform ones, and ones near the patch."""
    from neat_amd import raycast
    verts, faces = _ico4()
    faces = faces[:nf]
    rng = np.random.default_rng(nf)
    near = verts[faces[rng.integers(0, nf, 128)]].mean(1) * rng.uniform(0.9, 1.1, (128, 1)) if nf else rng.uniform(-1, 1, (128, 3))
    pts = np.concatenate([near, rng.uniform(-1.5, 1.5, (129, 3))])[rng.permutation(257)]
    ref = CP.closest_all(verts, faces, pts)
    assert (ref[1] >= 0).all() if nf else (ref[1] == -1).all()
    scene = raycast.build(verts, faces, DEV)
    assert scene.status == 0
    for N in (0, 1, 255, 256, 257):
        _same_bytes(_closest(scene, pts[:N]), tuple(x[:N] for x in ref), "nf %d N %d" % (nf, N))


def test_max_dist_cuts_the_queries_in_half():
    from neat_amd import raycast
    s = _reference("ico2")
    scene = raycast.build(s["verts"], s["faces"], DEV)
    free = _closest(scene, s["pts"])
    bound = float(np.sort(free[0])[1024])                                              # the d2 of a query: that query sits on the bound
    ref = CP.closest_all(s["verts"], s["faces"], s["pts"], max_d2=bound)
    got = _closest(scene, s["pts"], max_d2=bound)
    _same_bytes(got, ref, "bounded")
    miss = got[1] < 0
    assert 900 < miss.sum() < 1148
    assert np.array_equal(miss, free[0] > bound)                                       # inclusive: the query at the bound itself is a hit
    assert (got[0] == bound).any() and np.isposinf(got[0][miss]).all() and not got[2][miss].any() and not got[3][miss].any()
    for g, f in zip(got, free):                                                        # a hit under the bound is the unbounded hit
        assert g[~miss].tobytes() == f[~miss].tobytes()
    # through raycast.closest: max_dist is squared once on the host in float64
    md = float(np.sqrt(bound))
    dist, tri, _, _ = raycast.closest(scene, torch.from_numpy(s["pts"]).to(DEV), max_dist=md)
    want = CP.closest_all(s["verts"], s["faces"], s["pts"], max_d2=md * md)
    assert np.array_equal(tri.cpu().numpy(), want[1]) and dist.cpu().numpy().tobytes() == np.sqrt(want[0]).tobytes()


def test_order_and_determinism():
    from neat_amd import raycast
    s = _reference("ico2")
    verts, faces, pts, ref = s["verts"], s["faces"], s["pts"], s["ref"]
    scene = raycast.build(verts, faces, DEV)
    first = _closest(scene, pts)
    for a, b in zip(first, _closest(scene, pts)):                                      # two runs: the same bytes
        assert a.tobytes() == b.tobytes()
    rng = np.random.default_rng(4)
    perm = rng.permutation(len(pts))                                                   # permuting the queries permutes the outputs
    for a, b in zip(first, _closest(scene, pts[perm])):
        assert a[perm].tobytes() == b.tobytes()
    parts = [_closest(scene, pts[i:j]) for i, j in ((0, 1), (1, 300), (300, 300), (300, 2048))]      # chunked calls equal one call
    for k in range(4):
        assert np.concatenate([p[k] for p in parts]).tobytes() == first[k].tobytes()
    # permuting the faces: d2 keeps its bytes; where no second triangle ties, tri changes through the permutation and nothing else does
    fperm = rng.permutation(len(faces))
    shuffled = faces[fperm]
    got = _closest(raycast.build(verts, shuffled, DEV), pts)
    _same_bytes(got, CP.closest_all(verts, shuffled, pts), "shuffled faces")
    assert got[0].tobytes() == first[0].tobytes()
    single = (CP.rule(verts[faces][None], pts[:, None, :])[0] == ref[0][:, None]).sum(1) == 1
    assert single.sum() >= 512
    assert np.array_equal(fperm[got[1][single]], first[1][single])
    assert got[2][single].tobytes() == first[2][single].tobytes() and got[3][single].tobytes() == first[3][single].tobytes()
    assert (first[1][~single] <= fperm[got[1][~single]]).all()                        # a tie went to the lowest index in the first order


def test_bad_face_index_refuses_the_tree():
    from neat_amd import raycast
    s = _reference("ico2")
    faces = s["faces"].copy()
    faces[17, 1] = len(s["verts"])
    scene = raycast.build(s["verts"], faces, DEV)
    assert scene.status == 1
    d2, tri, q, uv = _closest(scene, s["pts"][:300])
    assert np.isposinf(d2).all() and (tri == -1).all() and not q.any() and not uv.any()
    _same_bytes((d2, tri, q, uv), CP.closest_all(s["verts"], faces, s["pts"][:300]), "refused")


def test_never_closest_triangles_and_queries():
    from neat_amd import raycast
    verts, faces = CP.box()
    verts = np.concatenate([verts, [[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]]])
    faces = np.concatenate([[[8, 0, 1], [9, 10, 11], [9, 9, 10]], faces]).astype(np.int32)          # NaN, collinear through the box, repeated
    pts = np.concatenate([np.random.default_rng(6).uniform(-1, 1, (253, 3)), [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.0, 0.0, 0.0]]])
    ref = CP.closest_all(verts, faces, pts)
    assert (ref[1][:253] >= 3).all() and ref[1][253:256].tolist() == [-1, -1, -1] and ref[1][256] >= 3
    _same_bytes(_closest(raycast.build(verts, faces, DEV), pts), ref, "never closest")


def test_the_tree_prunes():
    """Queries within 0.1 of the level-4 icosphere (5120 triangles): the cap nf / 4 only shows that pruning happens.
    Measured on an MI355X: 196.1 node boxes and 13.48 triangles tested per query, at most 45 triangles."""
    from neat_amd import raycast
    verts, faces = _ico4()
    rng = np.random.default_rng(8)
    u = rng.standard_normal((1024, 3))
    pts = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (1024, 1))
    scene = raycast.build(verts, faces, DEV)
    counts = torch.zeros(1024, 2, device=DEV, dtype=torch.int32)
    got = _closest(scene, pts, counts=counts)
    c = counts.cpu().numpy()
    print("  per query: %.1f node boxes and %.2f triangles tested (of %d), at most %d" % (c[:, 0].mean(), c[:, 1].mean(), len(faces), c[:, 1].max()))
    assert (c[:, 1] >= 1).all() and c[:, 1].mean() < len(faces) / 4
    _same_bytes(got, CP.closest_all(verts, faces, pts), "pruned")
    assert np.abs(np.sqrt(got[0]) - np.abs(np.linalg.norm(pts, axis=1) - 1.0)).max() < 0.01          # the sphere's own answer, coarsely


def test_application_layer():
    from neat_amd import raycast
    s = _reference("ico2")
    verts, faces, pts, ref = s["verts"], s["faces"], s["pts"], s["ref"]
    scene = raycast.build(verts, faces, DEV)
    counts = torch.zeros(len(pts), 2, device=DEV, dtype=torch.int32)
    dist, tri, point, uv = raycast.closest(scene, torch.from_numpy(pts).to(DEV), counts=counts)
    assert dist.dtype == torch.float64 and dist.device == DEV and tri.dtype == torch.int32
    assert dist.cpu().numpy().tobytes() == np.sqrt(ref[0]).tobytes()                   # dist == sqrt(d2), correctly rounded
    _same_bytes((ref[0], tri.cpu().numpy(), point.cpu().numpy(), uv.cpu().numpy()), ref, "closest")
    c = counts.cpu().numpy()
    assert (c[:, 0] >= 1).all() and (c[:, 1] >= 1).all() and c[:, 1].max() <= 320
    # float32 queries are widened exactly; a host array goes to the scene's device
    p32 = pts[:300].astype(np.float32)
    d32 = raycast.closest(scene, p32)[0].cpu().numpy()
    assert d32.tobytes() == np.sqrt(CP.closest_all(verts, faces, p32.astype(np.float64))[0]).tobytes()
    # a miss is +inf
    far = raycast.closest(scene, torch.tensor([[5.0, 0.0, 0.0], [float("nan"), 0.0, 0.0]]), max_dist=1.0)
    assert torch.isinf(far[0]).all() and (far[1] == -1).all()
    # line_distance: the samples of the formula, each against the mesh
    rng = np.random.default_rng(9)
    lines = rng.uniform(-1.2, 1.2, (37, 2, 3))
    for samples in (2, 32):
        got, gtri = raycast.line_distance(scene, lines, samples=samples, with_tri=True)
        want = CP.closest_all(verts, faces, CP.line_samples(lines, samples).reshape(-1, 3))
        assert got.shape == (37, samples) and got.cpu().numpy().tobytes() == np.sqrt(want[0]).tobytes()
        assert np.array_equal(gtri.cpu().numpy().reshape(-1), want[1])
        assert torch.equal(raycast.line_distance(scene, torch.from_numpy(lines), samples=samples), got)
    assert raycast.line_distance(scene, np.zeros((0, 2, 3)), samples=4).shape == (0, 4)
