"""neat_amd.evaluate on the device against tests/eval_f64.py and against g20_evaluation.npz (made by the reference's own scripts):
sampling bit for bit, thinning and mask flags identical, nearest distances within 2 ulp (only the square root may differ), every printed
number within n 2^-53 relative, n the number of distances its mean averages (the bar of tests/test_eval_math.py), the edge cases, and one large case against scipy's cKDTree."""
import warnings

import numpy as np
import pytest
import torch

from tests import eval_f64 as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bar(n):
    return n * 2.0 ** -53


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_evaluation")


@pytest.fixture(scope="module")
def E():
    from neat_amd import evaluate
    return evaluate


def t64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(DEV)


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_inf = np.isinf(a) & np.isinf(b)
    d = np.abs(a.view(np.int64) - b.view(np.int64))
    return np.where(both_inf, 0, d)


def kw(g, **extra):
    return dict(obs_mask=g["obs"], bb=g["bb"], res=float(g["res"]), plane=g["plane"], patch=float(g["patch"]), **extra)


def test_sampled_points_equal_numpy_bit_for_bit(E, g20):
    ref = F.sample_mesh(g20["verts"], g20["faces"], 0.2)
    got = E.sample_mesh(t64(g20["verts"]), torch.as_tensor(g20["faces"]).to(DEV), 0.2).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got.view(np.int64), ref.view(np.int64))
    rng = np.random.default_rng(1)
    # sizes around the four triangles of a workgroup and the 64 rows of a wavefront's pass; long, thin and tiny triangles
    for nf, scale in ((1, 30.0), (3, 2.0), (4, 1.0), (5, 0.3), (257, 0.7), (64, 13.0)):
        v = rng.normal(size=(nf + 2, 3)) * scale
        f = np.stack([np.arange(nf), np.arange(nf) + 1, np.arange(nf) + 2], 1).astype(np.int32)
        f[0] = [0, 0, 1]                      # zero area
        ref = F.sample_mesh(v, f, 0.2)
        got = E.sample_mesh(t64(v), torch.as_tensor(f).to(DEV), 0.2).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.view(np.int64), ref.view(np.int64)), (nf, scale)
    with pytest.raises(RuntimeError):
        E.sample_mesh(t64(np.eye(3)), torch.tensor([[0, 1, 3]]).to(DEV), 0.2)


def test_grid_offsets_past_1024_buckets(E):
    """11^3 = 1331 dense buckets: the one workgroup of 1024 that scans the histogram (eval_exscan_kernel) takes a second round with a
    carry.  start must be numpy's exclusive cumulative sum of the histogram; the slot of a point within its bucket is handed out by an
    atomic countdown, so the slots are compared bucket by bucket."""
    rng = np.random.default_rng(9)
    p = rng.uniform(0, 1, (1025, 3))
    p[0], p[1] = 0.0, 1.0                                                 # the box is the unit cube: 10 cells of 0.1 and the far face
    grid = E.Grid(t64(p), 0.1)
    assert grid.dense and grid.dim == [11, 11, 11] and grid.buckets == 1331
    c = np.clip(np.floor((p - 0.0) / grid.cell).astype(np.int64), 0, 10)
    bucket = (c[:, 0] * 11 + c[:, 1]) * 11 + c[:, 2]
    hist = np.bincount(bucket, minlength=1331)
    assert (hist[1024:] > 0).any() and (hist[:1024] > 0).any()
    start = grid.start.cpu().numpy()
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(hist)]))
    sidx = grid.sidx.cpu().numpy()
    assert np.array_equal(np.sort(sidx), np.arange(1025)) and np.array_equal(bucket[sidx], np.repeat(np.arange(1331), hist))
    assert np.array_equal(grid.spts.cpu().numpy(), p[sidx])


def test_thinning_equals_the_reference_s_data_down(E, g20):
    cloud = E.sample_mesh(t64(g20["verts"]), torch.as_tensor(g20["faces"]).to(DEV), 0.2)
    kept = E.thin(cloud, 0.2, order=g20["mesh_perm"])
    assert np.array_equal(cloud[kept].cpu().numpy(), g20["mesh_data_down"])
    pcd = t64(g20["pcd_cloud"])
    assert np.array_equal(pcd[E.thin(pcd, 0.2, order=g20["pcd_perm"])].cpu().numpy(), g20["pcd_data_down"])
    with pytest.raises(ValueError):
        E.thin(pcd, 0.2, order=np.zeros(len(g20["pcd_cloud"]), dtype=np.int64))


@pytest.mark.parametrize("case", ["lattice", "duplicates", "identical", "one_cell", "one", "empty", "sparse", "tile"])
def test_thinning_edge_cases(E, case):
    rng = np.random.default_rng(5)
    a = np.arange(12) * 0.2
    pts = {"lattice": np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3),          # order=None on an unshuffled lattice
           "duplicates": np.repeat(rng.uniform(0, 2, (400, 3)), 3, axis=0)[rng.permutation(1200)],
           "identical": np.tile([[0.3, -1.0, 7.0]], (777, 1)),
           "one_cell": rng.uniform(0, 0.19, (500, 3)),
           "one": np.array([[1.0, 2.0, 3.0]]),
           "empty": np.zeros((0, 3)),
           "sparse": rng.uniform(-500, 500, (3000, 3)),                                          # far more cells than a dense box holds
           "tile": rng.uniform(0, 4, (1025, 3))}[case]
    for n in ((255, 256, 257, 1023, 1025) if case == "tile" else (len(pts),)):
        p = pts[:n]
        kept, rounds = E.thin(t64(p), 0.2, return_rounds=True)
        assert np.array_equal(kept.cpu().numpy(), np.nonzero(F.thin_sequential(p, 0.2))[0]), (case, n)
        assert rounds <= max(n, 1)


@pytest.mark.parametrize("f32_quotient", [False, True])
def test_mask_flags_are_identical(E, g20, f32_quotient):
    g = g20
    rng = np.random.default_rng(2)
    bb32 = g["bb"].astype(np.float32)
    res, patch = float(g["res"]), float(g["patch"])
    faces = np.concatenate([bb32[:1] - np.float32(patch), bb32[1:] + np.float32(patch * 2), bb32[:1], bb32[1:]]).astype(np.float64)
    edge = np.concatenate([faces, np.nextafter(faces, -np.inf), np.nextafter(faces, np.inf)])
    half = bb32[0].astype(np.float64) + (rng.integers(-2, 32, (500, 3)) + 0.5) * res               # quotients that end in .5: ties of the rounding
    pts = np.concatenate([g["mesh_data_down"], edge, half, np.nextafter(half, np.inf), rng.uniform(-7, 7, (4000, 3))])
    ref = F.obs_flags(pts, g["obs"], g["bb"], res, patch, f32_quotient)
    got = E.obs_flags(t64(pts), g["obs"], g["bb"], res, patch, f32_quotient).cpu().numpy()
    assert np.array_equal(got, ref)


def test_nearest_distances_within_two_ulp_of_brute_force(E, g20):
    stl = g20["stl"].astype(np.float64)
    q = g20["mesh_data_down"]
    ref_d, ref_i = F.nearest_brute(stl, q)
    d, i = E.nearest(t64(stl), t64(q), 20.0)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert ulps(d, ref_d).max() <= 2
    d2 = F.d2_rows(q[:, None, :], stl[None])
    unique = (d2 == d2.min(1, keepdims=True)).sum(1) == 1
    assert unique.sum() > 0.9 * len(q) and np.array_equal(i[unique], ref_i[unique])
    # a cap that bites: beyond it inf and -1, below it the same numbers
    d_cap, i_cap = E.nearest(t64(stl), t64(q), 0.3)
    d_cap, i_cap = d_cap.cpu().numpy(), i_cap.cpu().numpy()
    far = ref_d > 0.3 * (1 + 1e-9)
    assert far.any() and np.isinf(d_cap[far]).all() and (i_cap[far] == -1).all()
    near = ref_d < 0.3
    assert near.any() and np.array_equal(d_cap[near], d[near])


def test_nearest_over_hashed_buckets(E):
    """A cloud whose cell count exceeds a dense box: 3000 points over +-800 at a cell of 25 are 65^3 cells, so the cells are hashed into
    2^13 buckets, several cells share a bucket and a ring can meet the same bucket twice.  Capped and uncapped."""
    rng = np.random.default_rng(9)
    cloud = rng.uniform(-800, 800, (3000, 3))
    cloud[100:200] = cloud[:100] + rng.uniform(-1, 1, (100, 3))             # close pairs, so that a cap of 40 keeps some
    q = np.concatenate([cloud[:300] + rng.normal(0, 8, (300, 3)), rng.uniform(-900, 900, (700, 3)), cloud[:30]])
    ref_d, ref_i = F.nearest_brute(cloud, q)
    grid = E.Grid(t64(cloud), 25.0)
    assert not grid.dense and grid.buckets < grid.dim[0] * grid.dim[1] * grid.dim[2]
    for cap in (float("inf"), 40.0):
        d, i = E.nearest(t64(cloud), t64(q), cap, grid=grid)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        near = ref_d < cap
        assert near.sum() > 300 and (np.isinf(cap) or (~near).sum() > 300)
        assert ulps(d[near], ref_d[near]).max() <= 2 and np.array_equal(i[near], ref_i[near]), cap
        far = ref_d > cap * (1 + 1e-9)
        assert np.isinf(d[far]).all() and (i[far] == -1).all(), cap


@pytest.mark.parametrize("case", ["one", "identical", "one_cell", "sparse", "planar", "boundaries", "tile"])
def test_nearest_edge_cases(E, case):
    rng = np.random.default_rng(8)
    cloud = {"one": np.array([[0.5, 0.5, 0.5]]),
             "identical": np.tile([[1.0, 1.0, 1.0]], (300, 1)),
             "one_cell": rng.uniform(0, 1e-3, (400, 3)),
             "sparse": rng.uniform(-800, 800, (2000, 3)),
             "planar": np.concatenate([rng.uniform(-3, 3, (1500, 2)), np.zeros((1500, 1))], 1),
             "boundaries": np.stack(np.meshgrid(*[np.arange(6) * 0.5] * 3, indexing="ij"), -1).reshape(-1, 3),
             "tile": rng.uniform(0, 3, (513, 3))}[case]
    span = np.ptp(cloud, axis=0).max() + 1.0
    q = np.concatenate([cloud[:50], cloud.mean(0) + rng.normal(0, span, (600, 3)), cloud[:20] + 0.25])
    for m in ((255, 256, 257) if case == "tile" else (len(q),)):
        ref_d, ref_i = F.nearest_brute(cloud, q[:m])
        d, i = E.nearest(t64(cloud), t64(q[:m]))
        assert ulps(d.cpu().numpy(), ref_d).max() <= 2, case
        assert np.array_equal(i.cpu().numpy(), ref_i), case            # ties included: the lowest index


def test_empty_inputs_and_queries_beyond_the_cap(E, g20):
    g = g20
    d, i = E.nearest(t64(np.zeros((0, 3))), t64(np.ones((5, 3))), 20.0)
    assert np.isinf(d.cpu().numpy()).all() and (i.cpu().numpy() == -1).all()
    d, i = E.nearest(t64(np.ones((5, 3))), t64(np.zeros((0, 3))), 20.0)
    assert d.shape == (0,) and i.shape == (0,)
    assert E.sample_mesh(t64(np.zeros((0, 3))), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 0.2).shape == (0, 3)
    # everything farther than max_dist: numpy's mean of an empty slice, NaN with a RuntimeWarning
    pts = g["pcd_cloud"] + [0.0, 0.0, 0.0]
    with pytest.warns(RuntimeWarning):
        acc, comp = E.dtu_scores(t64(pts), g["stl"].astype(np.float64) + 100.0, max_dist=1.0, order=g["pcd_perm"], **kw(g))
    assert np.isnan(acc) and np.isnan(comp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = F.dtu_scores(pts, g["stl"].astype(np.float64) + 100.0, max_dist=1.0, order=g["pcd_perm"], **kw(g))
    assert np.isnan(ref[0]) and np.isnan(ref[1])


def test_every_printed_number_of_the_four_scripts(E, g20):
    g = g20
    stl = t64(g["stl"])
    cloud = E.sample_mesh(t64(g["verts"]), torch.as_tensor(g["faces"]).to(DEV), 0.2)

    def close(got, ref, n, what):
        print(what, got, ref, "rel %.3g" % (abs(got - ref) / ref), "bar %.3g" % bar(n))
        assert abs(got - ref) <= bar(n) * ref, what

    def counts(det, max_dist=20.0):          # the number of averaged distances of each of the two means
        return int((det["dist_d2s"] < max_dist).sum().item()), int((det["dist_s2d"] < max_dist).sum().item())

    for name, pts, perm in (("mesh", cloud, g["mesh_perm"]), ("pcd", t64(g["pcd_cloud"]), g["pcd_perm"])):
        det = {}
        acc, comp = E.dtu_scores(pts, stl, order=perm, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        close((acc + comp) / 2, ref[2], max(na, nc) + 1, name + " overall")
        if name == "mesh":          # the error colours the reference handed to write_point_cloud, at 8 bits
            d2s, s2d = E.vis_colors(det, len(g["stl"]), 10.0, 20.0)
            assert np.array_equal((d2s * 255).round().astype(np.uint8), g["mesh_colors_d2s"])
            assert np.array_equal((s2d * 255).round().astype(np.uint8), g["mesh_colors_s2d"])
    for name, lines in (("lines", g["lines"]), ("lines_score", g["lines"][g["scores"] < 0.6])):
        det = {}
        pts, mean_length = E.line_cloud(lines, g["scale_mat"])
        acc, comp = E.dtu_scores(pts, stl, order=g[name + "_perm"], f32_quotient=True, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        close(mean_length, ref[2], lines.shape[0], name + " length")
        assert lines.shape[0] == ref[3]
    for name in ("junc_pth", "junc_npz"):
        det = {}
        pts, count = E.junction_cloud(torch.tensor(g["lines"]), g["scale_mat"])
        acc, comp = E.dtu_scores(pts, stl, order=g[name + "_perm"], f32_quotient=True, thinning=False, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        assert count == ref[2]


def test_abc_counts_and_printed_lines(E, g20):
    g = g20
    res = E.abc_scores(g["abc_junctions_pred"], g["lines"], g["abc_junctions_gt"], g["abc_edges_gt"], g["abc_offset_scale"])
    ref = F.abc_scores(g["abc_junctions_pred"], g["lines"], g["abc_junctions_gt"], g["abc_edges_gt"], g["abc_offset_scale"])
    assert res["junctions_correct"] == ref["junctions_correct"] and res["lines_correct"] == ref["lines_correct"]
    assert list(E.abc_lines(res)) == [str(s) for s in g["abc_lines"]]
    cj, cl, _ = F.abc_costs(g["abc_junctions_pred"], g["lines"], g["abc_junctions_gt"], g["abc_edges_gt"], g["abc_offset_scale"])
    off = g["abc_offset_scale"]
    s = 1.0 / off[-1]
    jp = (g["abc_junctions_pred"] @ (np.eye(3) * s).T) + (-off[:3])
    lp = (g["lines"].reshape(-1, 3) @ (np.eye(3) * s).T) + (-off[:3])
    lg = g["abc_junctions_gt"][g["abc_edges_gt"]]
    assert ulps(E.line_cost(jp, g["abc_junctions_gt"], 1).cpu().numpy(), cj).max() <= 2
    assert ulps(E.line_cost(lp, lg.reshape(-1, 3), 2).cpu().numpy(), cl).max() <= 4          # two square roots and their mean


def test_large_case_against_ckdtree(E):
    """2 M cloud points against 2 M queries, and a 2 M-point thinning: distances of a 100 000-query sample against cKDTree (none skipped),
    and the two defining properties of the thinned set over all points."""
    from scipy.spatial import cKDTree
    n = 2_000_000
    gen = torch.Generator(device="cpu").manual_seed(0)
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    cloud = (d / d.norm(dim=1, keepdim=True) * 100.0 + 0.05 * torch.randn(n, 3, generator=gen, dtype=torch.float64)).numpy()
    q = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    q = (q / q.norm(dim=1, keepdim=True) * 100.0 + 0.3 * torch.randn(n, 3, generator=gen, dtype=torch.float64)).numpy()
    q[:1000] *= 1.5                                           # beyond max_dist
    dist, idx = E.nearest(t64(cloud), t64(q), 20.0)
    dist = dist.cpu().numpy()
    sample = np.random.default_rng(0).choice(n, 100_000, replace=False)
    sample[:500] = np.arange(500)
    tree = cKDTree(cloud)
    ref, _ = tree.query(q[sample], k=1, workers=16)
    got = dist[sample]
    beyond = ref >= 20.0 * (1 + 1e-9)
    assert beyond.sum() >= 500 and np.isinf(got[beyond]).all()
    ok = ~beyond                                              # every query of the sample is asserted on one side or the other: none is skipped
    assert ulps(got[ok], ref[ok]).max() <= 4                  # cKDTree sums the squares in its own order: 1 ulp of d2 more than brute force
    # thinning at the reference's radius
    order = np.random.default_rng(1).permutation(n)
    kept = E.thin(t64(cloud), 0.2, order=order).cpu().numpy()
    state = np.zeros(n, dtype=bool)
    state[kept] = True
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    assert (np.diff(rank[kept]) > 0).all()                    # in visiting order
    pairs = cKDTree(cloud[kept]).query_pairs(0.2 * (1 - 1e-12), output_type="ndarray")
    assert len(pairs) == 0                                    # no two kept points within the radius
    removed = np.nonzero(~state)[0]
    kept_tree = cKDTree(cloud[kept])
    nb = kept_tree.query_ball_point(cloud[removed], 0.2 * (1 + 1e-12), workers=16)
    kept_rank = rank[kept]
    bad = sum(1 for r, lst in zip(removed, nb) if not len(lst) or kept_rank[lst].min() > rank[r])
    assert bad == 0                                           # every removed point has an earlier kept neighbour
