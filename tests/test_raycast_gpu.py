"""neat_raycast_* on the device against the float64 restatement of tests/raycast_f64.py: equality with the brute-force rule over all
triangles (not a tolerance), at sizes where the padding of the tree and the workgroup boundaries of its refit bite."""
import numpy as np
import pytest
import torch

from tests import raycast_f64 as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCENES = {"ico0": lambda: RC.icosphere(0), "ico2": lambda: RC.icosphere(2), "strips": lambda: RC.strips(), "box": lambda: RC.box()}
CENTRE = {"ico0": (0.0, 0.0, 0.0), "ico2": (0.0, 0.0, 0.0), "strips": (0.5, 0.5, 0.5), "box": (0.0, 0.0, 0.0)}
_cache = {}


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def _cast(scene, o, d, t_min=None, t_max=None, any_hit=False, counts=None):
    from neat_amd import raycast
    t, tri, uv = raycast.cast(scene, _dev(o), _dev(d), None if t_min is None else _dev(t_min), None if t_max is None else _dev(t_max),
                              any_hit=any_hit, counts=counts)
    return t.cpu().numpy(), tri.cpu().numpy(), uv.cpu().numpy()


def _reference(name):
    """Scene `name`, its fan of 1025 rays and the brute-force answer, computed once."""
    if name not in _cache:
        verts, faces = SCENES[name]()
        o, d = RC.fan(11, 1025, centre=CENTRE[name])
        _cache[name] = dict(verts=verts, faces=faces, o=o, d=d, ref=RC.cast_all(verts, faces, o, d), excluded=RC.judge(verts, faces, o, d))
    return _cache[name]


def _within_one_ulp(t32, ref64):
    r = ref64.astype(np.float32)
    return (t32 >= np.nextafter(r, np.float32(-np.inf))) & (t32 <= np.nextafter(r, np.float32(np.inf)))


def _compare(got, ref, excluded, what):
    t, tri, uv = got
    rt, rtri, ruv = ref
    assert t.dtype == np.float32 and tri.dtype == np.int32 and uv.dtype == np.float32 and uv.shape == (t.shape[0], 2)
    n = t.shape[0]
    assert excluded.sum() <= 0.01 * max(n, 1), what
    ok = ~excluded
    miss = rtri < 0
    print("  %s: %d rays, %d hits, %d excluded; tri differs on %d, max |uv - ref| %.3g" % (
        what, n, int((~miss).sum()), int(excluded.sum()), int((tri != rtri)[ok].sum()), float(np.abs(uv - ruv)[ok].max()) if ok.any() else 0.0))
    assert np.array_equal(tri[ok], rtri[ok]), what
    assert (np.isposinf(t[ok & miss])).all() and (tri[ok & miss] == -1).all(), what
    hit = ok & ~miss
    assert _within_one_ulp(t[hit], rt[hit]).all(), what
    assert (np.abs(uv[hit] - ruv[hit]) <= 1e-6).all(), what


def _aimed(verts, faces, n, seed):
    """n rays from outside, each aimed at a random point of a random triangle of the mesh."""
    rng = np.random.default_rng(seed)
    tv = verts[faces[rng.integers(0, faces.shape[0], n)]]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    p = (w[:, :, None] * tv).sum(1)
    u = p / np.linalg.norm(p, axis=1, keepdims=True) + 0.3 * rng.standard_normal((n, 3))
    o = 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_hit_equals_brute_force(name):
    from neat_amd import raycast
    s = _reference(name)
    scene = raycast.build(s["verts"], s["faces"], DEV)
    assert scene.status == 0 and scene.nf == s["faces"].shape[0]
    hits = int((s["ref"][1] >= 0).sum())
    assert 100 < hits < 925                                      # hits and misses mixed
    _compare(_cast(scene, s["o"], s["d"]), s["ref"], s["excluded"], name)


@pytest.mark.parametrize("nf", [0, 1, 2, 3, 63, 64, 65, 320, 1025, 5120])
def test_sizes_where_padding_and_workgroup_boundaries_bite(nf):
    """The first nf faces of the level-4 icosphere (nf = 1025 and 5120 make the refit cross workgroups and reach its second launch),
    ray counts around the wavefront and the workgroup; half the rays aimed at the patch, half a fan."""
    from neat_amd import raycast
    if "ico4" not in _cache:
        _cache["ico4"] = RC.icosphere(4)
    verts, faces = _cache["ico4"]
    faces = faces[:nf]
    assert faces.shape[0] == nf
    fo, fd = RC.fan(7, 513)
    ao, ad = _aimed(verts, faces, 512, 9) if nf else RC.fan(8, 512)
    o, d = np.concatenate([ao, fo]), np.concatenate([ad, fd])
    perm = np.random.default_rng(1).permutation(1025)
    o, d = o[perm], d[perm]
    ref, excluded = RC.cast_all(verts, faces, o, d), RC.judge(verts, faces, o, d)
    if nf:
        assert (ref[1] >= 0).sum() >= 256 and (ref[1] < 0).sum() >= 100
    scene = raycast.build(verts, faces, DEV)
    assert scene.status == 0
    for R in (0, 1, 63, 64, 65, 1025):
        got = _cast(scene, o[:R], d[:R])
        assert got[0].shape == (R,)
        _compare(got, tuple(x[:R] for x in ref), excluded[:R], "nf %d R %d" % (nf, R))


@pytest.mark.parametrize("level", [0, 2])
def test_watertight_from_the_centre(level):
    """One ray through every vertex and every edge midpoint of the closed icosphere and 1025 random ones: every ray hits."""
    from neat_amd import raycast
    verts, faces = RC.icosphere(level)
    edges = sorted({(min(a, b), max(a, b)) for f in faces for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))})
    mids = np.stack([(verts[a] + verts[b]) / 2 for a, b in edges])
    rng = np.random.default_rng(2)
    rnd = rng.standard_normal((1025, 3))
    targets = np.concatenate([verts, mids, rnd / np.linalg.norm(rnd, axis=1, keepdims=True)])
    d = targets.astype(np.float32)
    o = np.zeros_like(d)
    nv, ne = verts.shape[0], len(edges)
    scene = raycast.build(verts, faces, DEV)
    t, tri, uv = _cast(scene, o, d)
    assert (tri >= 0).all() and np.isfinite(t).all()                          # every ray hits
    rt, rtri, _ = RC.cast_all(verts, faces, o, d)
    assert np.array_equal(tri, rtri) and _within_one_ulp(t, rt).all()
    tv, valid = verts[faces], RC.valid_triangles(verts, faces)
    for r in range(nv + ne):
        share = [g for g in range(faces.shape[0]) if (r in faces[g] if r < nv else (edges[r - nv][0] in faces[g] and edges[r - nv][1] in faces[g]))]
        assert len(share) == (2 if r >= nv else (5 if r < 12 else 6))
        acc, tt, _, _, _, _ = RC.rule_one_ray(tv, valid, o[r].astype(np.float64), d[r].astype(np.float64), 0.0, np.inf)
        best = [g for g in share if acc[g] and tt[g] == tt[acc].min()]
        assert tri[r] in share and acc[tri[r]] and tri[r] == min(best), r
    # the distance: along the ray to the plane of the triangle that was hit, in units of |d|
    n = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])[tri]
    analytic = (n * tv[tri, 0]).sum(1) / (n * d.astype(np.float64)).sum(1)
    assert np.abs(t - analytic).max() < 1e-6
    assert np.abs(t[:nv] * np.linalg.norm(d[:nv].astype(np.float64), axis=1) - 1.0).max() < 1e-6          # a vertex lies on the unit sphere
    assert np.abs(t[nv:nv + ne] - 1.0).max() < 1e-6                                                        # d is the midpoint itself: t = 1


def test_rule_edges():
    from neat_amd import raycast
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [np.nan, 0, 0], [2, 0, 0], [2, 1, 0], [3, 0, 0]], np.float64)
    # 0, 1: identical coplanar triangles; 2: opposite winding of another; 3: zero area (collinear); 4: a NaN vertex; 5: a good neighbour
    faces = np.array([[0, 1, 2], [0, 1, 2], [1, 2, 3][::-1], [0, 4, 3], [0, 5, 2], [6, 8, 7]], np.int32)
    assert RC.valid_triangles(verts, faces).tolist() == [True, True, True, False, False, True]
    scene = raycast.build(verts, faces, DEV)
    down = np.array([0, 0, -1.0], np.float32)
    o = np.array([[0.25, 0.25, 1.0], [0.75, 0.75, 1.0], [2.25, 0.25, 1.0], [0.25, 0.25, -1.0], [0.75, 0.75, -1.0], [-1.0, 0.25, 0.0], [5.0, 5.0, 1.0]],
                 np.float32)
    d = np.stack([down, down, down, -down, -down, np.array([1.0, 0, 0], np.float32), down])
    ref = RC.cast_all(verts, faces, o, d)
    assert ref[1].tolist() == [0, 2, 5, 0, 2, -1, -1]              # the lower of two identical triangles; both windings from both sides; in-plane: a miss
    t, tri, uv = _cast(scene, o, d)
    assert tri.tolist() == ref[1].tolist() and np.array_equal(t, ref[0].astype(np.float32)) and np.abs(uv - ref[2]).max() <= 1e-6
    assert t[:5].tolist() == [1.0] * 5 and np.isposinf(t[5:]).all() and (uv[5:] == 0).all()
    # the half-open interval at the float32 neighbours of the hit distance
    one = np.float32(1.0)
    below, above = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))
    for t_min, t_max, hit in ((None, one, False), (None, above, True), (one, None, True), (above, None, False), (below, above, True),
                              (below, one, False)):
        lo = None if t_min is None else np.full(1, t_min, np.float32)
        hi = None if t_max is None else np.full(1, t_max, np.float32)
        for any_hit in (False, True):
            got = _cast(scene, o[:1], d[:1], lo, hi, any_hit=any_hit)
            assert (got[1][0] >= 0) == hit and np.isfinite(got[0][0]) == hit, (t_min, t_max, any_hit)


def test_order_independence_determinism_and_chunks():
    from neat_amd import raycast
    s = _reference("ico2")
    verts, faces, o, d = s["verts"], s["faces"], s["o"], s["d"]
    scene = raycast.build(verts, faces, DEV)
    a = _cast(scene, o, d)
    perm = np.random.default_rng(4).permutation(faces.shape[0])
    b = _cast(raycast.build(verts, faces[perm], DEV), o, d)
    ok = ~s["excluded"]
    assert a[0].tobytes() == b[0].tobytes()                                    # no t changes
    hit = ok & (a[1] >= 0)
    assert np.array_equal(perm[b[1][hit]], a[1][hit]) and np.array_equal(b[1][~hit & ok], a[1][~hit & ok])
    # two runs, build included: the same bytes
    c = _cast(raycast.build(verts, faces, DEV), o, d)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    # chunks
    parts = [_cast(scene, o[i:j], d[i:j]) for i, j in ((0, 1), (1, 64), (64, 129), (129, 1025))]
    for k in range(3):
        assert np.concatenate([p[k] for p in parts]).tobytes() == a[k].tobytes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_any_hit_equals_closest_hit(name):
    from neat_amd import raycast
    s = _reference(name)
    scene = raycast.build(s["verts"], s["faces"], DEV)
    t_max = np.random.default_rng(6).uniform(1.5, 4.5, 1025).astype(np.float32)
    t_closest = _cast(scene, s["o"], s["d"])[0]
    t_any, tri_any, _ = _cast(scene, s["o"], s["d"], t_max=t_max, any_hit=True)
    blocked = np.isfinite(t_any)
    assert np.array_equal(blocked, t_closest < t_max) and np.array_equal(blocked, tri_any >= 0)
    assert 50 < blocked.sum() < (t_closest < np.inf).sum()                   # the clip takes some hits away
    assert (t_any[blocked] < t_max[blocked]).all() and (t_any[blocked] >= t_closest[blocked]).all()


def test_the_tree_culls():
    from neat_amd import raycast
    if "ico4" not in _cache:
        _cache["ico4"] = RC.icosphere(4)
    verts, faces = _cache["ico4"]
    o, d = RC.fan(11, 1025)
    scene = raycast.build(verts, faces, DEV)
    counts = torch.zeros(1025, 2, device=DEV, dtype=torch.int32)
    t, tri, _ = _cast(scene, o, d, counts=counts)
    counts = counts.cpu().numpy()
    model = RC.Tree(verts, faces).cast(o[:129], d[:129])
    print("  triangles tested per ray: device %.2f (nodes %.1f), model on the first 129 rays %.2f (nodes %.1f); nf / 8 = %d" % (
        counts[:, 1].mean(), counts[:, 0].mean(), model[3][:, 1].mean(), model[3][:, 0].mean(), faces.shape[0] // 8))
    assert counts[:, 1].mean() < faces.shape[0] / 8
    assert counts[:, 0].min() >= 1 and (counts[tri >= 0, 1] >= 1).all()
    assert np.array_equal(tri[:129], model[1]) and _within_one_ulp(t[:129], model[0]).all()


def test_a_face_index_out_of_range_sets_the_status_and_every_cast_misses():
    from neat_amd import raycast
    verts, faces = RC.icosphere(2)
    bad = faces.copy()
    bad[200, 1] = verts.shape[0]                      # == nv: checked before any vertex is read
    scene = raycast.build(verts, bad, DEV)
    assert scene.status == 1
    o, d = RC.fan(11, 257)
    for any_hit in (False, True):
        t, tri, uv = _cast(scene, o, d, any_hit=any_hit)
        assert np.isposinf(t).all() and (tri == -1).all() and (uv == 0).all()
    bad[200, 1] = -1
    assert raycast.build(verts, bad, DEV).status == 1
    assert raycast.build(verts, faces, DEV).status == 0


def _look_at_pose():
    a = 0.7
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    b = -0.4
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Ry @ Rx
    pose = np.eye(4)
    pose[:3, :3] = R
    pose[:3, 3] = -3.0 * R[:, 2]                      # the camera looks along its +z, at the origin
    return pose


def test_view_and_visibility():
    from neat_amd import raycast
    verts, faces = RC.icosphere(2)
    scene = raycast.build(verts, faces, DEV)
    H, W = 48, 64
    pose = _look_at_pose()
    K = np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]])
    depth, normal, tri = raycast.view(scene, torch.from_numpy(pose), torch.from_numpy(K), H, W)
    assert depth.shape == (H, W) and normal.shape == (H, W, 3) and tri.shape == (H, W) and depth.dtype == torch.float32 and tri.dtype == torch.int32
    depth, normal, tri = depth.reshape(-1), normal.reshape(-1, 3), tri.reshape(-1)
    hit = tri >= 0
    assert hit.sum() > 200 and (~hit).sum() > 200
    assert torch.isnan(depth[~hit]).all() and torch.isfinite(depth[hit]).all() and (normal[~hit] == 0).all()
    assert (normal[hit].norm(dim=1) - 1).abs().max() < 1e-5
    # the rays of the view, as the library makes them
    from neat_amd import ops
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    uv = torch.stack([xs, ys], -1).reshape(1, -1, 2).float()
    dirs, _, origins = ops.camera_rays(uv, _dev(pose)[None], _dev(K)[None], with_origins=True)
    dirs = dirs.reshape(-1, 3)
    assert ((normal[hit] * dirs[hit]).sum(-1) < 0).all()                       # turned towards the camera
    # the same pixels from the float64 rule
    rt, rtri, _ = RC.cast_all(verts, faces, origins.cpu().numpy(), dirs.cpu().numpy())
    assert np.array_equal(tri.cpu().numpy(), rtri) and _within_one_ulp(depth[hit].cpu().numpy(), rt[rtri >= 0]).all()
    n64 = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)                          # outward on this mesh: towards the camera where it is hit from outside
    assert np.abs(normal[hit].cpu().numpy() - n64[rtri[rtri >= 0]]).max() < 1e-6
    # visibility on both sides of the surface
    bias = 0.01
    idx = torch.nonzero(hit).flatten()
    front = origins[idx] + (depth[idx] - 2 * bias)[:, None] * dirs[idx]
    back = origins[idx] + (depth[idx] + 2 * bias)[:, None] * dirs[idx]
    cam = np.linalg.inv(pose)[None]
    seen_front = raycast.visible_points(scene, front, cam, bias=bias)
    seen_back = raycast.visible_points(scene, back, cam, bias=bias)
    frac = raycast.visible_lines(scene, torch.stack([front, back], 1), cam, bias=bias)
    assert seen_front.shape == (1, idx.numel()) and seen_front.dtype == torch.bool and frac.shape == (1, idx.numel()) and frac.dtype == torch.float32
    print("  %d hits: front not seen %d, back seen %d, fraction not strictly between 0 and 1: %d" % (
        idx.numel(), int((~seen_front).sum()), int(seen_back.sum()), int(((frac <= 0) | (frac >= 1)).sum())))
    assert seen_front.all() and not seen_back.any() and ((frac > 0) & (frac < 1)).all()
    # targets outside any sphere about the origin are not refused: a point far behind the camera is seen, one behind the mesh is not
    far = torch.tensor([[0.0, 0.0, 0.0]], device=DEV) + _dev(pose[:3, 3])[None] * 50.0
    behind = -_dev(pose[:3, 3])[None] * 50.0
    assert raycast.visible_points(scene, torch.cat([far, behind]), cam).cpu().tolist() == [[True, False]]
    empty = raycast.visible_points(scene, torch.zeros(0, 3, device=DEV), np.stack([cam[0], cam[0]]))
    assert empty.shape == (2, 0) and empty.dtype == torch.bool
    assert raycast.visible_lines(scene, torch.zeros(0, 2, 3, device=DEV), cam).shape == (1, 0)
