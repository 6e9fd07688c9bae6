"""The analytic truth of the closed-loop tests (tests/test_closed_loop_math.py, tests/test_closed_loop_gpu.py): the generated scenes of
scenegen.shapes against the camera model and the solids written out in plain numpy float64.  Nothing here is shared with a
tests/*_f64.py restatement; from neat_amd come only the inputs (scenegen.shapes, scenegen.normalise, scenegen.cameras).

The camera: K [3,3], pose [4,4] camera-to-world = [R | C].  A world point X is seen at
    x = K R^T (X - C),   (column, row) = (x[0] / x[2], x[1] / x[2]),
and a pixel's centre IS its integer (column, row); the ray of a pixel is C + t (R^T)^-1 K^-1 (column, row, 1).

`scene(name)` builds the shared case once per process: 12 views of 128 x 128, ss = 3, the shape through scenegen.normalise, the float64
restatements chained on the host (scenegen_f64 -> detect_f64 -> triangulate_f64, oracle.attraction_oracle) and the truth beside them.
The bars of both test modules stand here, each with where it comes from; none is taken from what the device gives.
"""
import numpy as np

VIEWS, RES, SS = 12, 128, 3
SHAPES = ("box", "lblock")
U32 = 2.0 ** -24                      # the rounding unit of float32

# ---- the bars ---------------------------------------------------------------------------------------------------------------------
BAR_P2 = 1e-9                         # px: float64 runs against the written-out projection (the restatement measures 1.4e-14)
BAR_P3 = 1e-12                        # world: a run's end off its edge (the restatement measures 0)
# The float32 camera kernels.  A pixel is f X/Z + c with f = 140 = 1.09 x 128 px.  An error e in each camera-frame coordinate, relative
# to the vector's length, moves it by f e (1 + |X/Z|) / (Z / |X|): |X/Z| <= 64/140 = 0.46 and Z / |X| >= 0.84 inside the picture, and the
# rotation mixes three such errors (sqrt 3): 1.09 x 1.46 / 0.84 x 1.73 = 3.3, taken as 4, in units of 128 px.  e is 8 roundings: the two
# divisions by the focal length, the rotation's three products and two sums, the normalisation (or, projecting, the inverse pose's entry,
# R X + T, K's row with its cancelling c Z term, and the division); that a float32 pose is orthonormal to 2^-24 only, so that the kernels' R
# is not the truth's (R^T)^-1, is one of them.  8 x 2^-24 x 128 x 4 = 2.4e-4 px: fifty times the 5e-6 px that the
# float32 oracle measures, two thousand times below the half pixel.
BAR_CAM = 8 * U32 * 128.0 * 4.0
assert BAR_CAM < 1e-3
BAR_DEPTH = 2.0 ** -23 * 4.0          # a hit depth is a float32 below 4 (the cameras stand at 2, the solid ends at 0.7): one unit in the last place
PARTIAL_CAP = 0.03                    # share of pixels with some but not all sub-samples hit: the silhouette's pixels, 1 to 2 % at this size
BAR_FOOT = 1e-3                       # px: a foot point off its segment (float32 pixels up to 128: 1e-5 at the worst; the oracle measures 4e-6)
DIST_SLACK = 1e-5                     # px: `distance` is tested on a float32 length of at most 10 px (10 x 2^-23 = 1.2e-6)
TIE_PX = 1e-4                         # px: a ray's segment is no further than the nearest run by this much; no ray is left out
BAR_DET_MID = 0.5                     # px: a detected segment's midpoint to the nearest projected edge
BAR_DET_MEAN = 0.25                   # px: each component of the mean offset: half of what a pixel-centre mix-up produces
BAR_TRI = 1e-4                        # world: between the restatement's 8e-7 and the 1e-2 of runs moved by half a pixel
COVER, COVERED = 0.8, {"box": 12, "lblock": 17}
CLOSEST_F64 = 1.2e-16                  # tests/closest_f64.py measures 1.11e-16 against the closed form at the 257 points (test_closed_loop_math)
BAR_CLOSEST = 4.0 * CLOSEST_F64


# ---- the camera, written out ----------------------------------------------------------------------------------------------------------
def project(K, pose, X):
    """World points X [...,3] -> ((column, row) [...,2], depth [...]): x = K R^T (X - C), division by depth."""
    K, pose, X = np.asarray(K, np.float64), np.asarray(pose, np.float64), np.asarray(X, np.float64)
    x = np.einsum("ij,jk,...k->...i", K[:3, :3], pose[:3, :3].T, X - pose[:3, 3])
    return x[..., :2] / x[..., 2:3], x[..., 2]


def pixel_ray(K, pose, uv):
    """Pixels (column, row) [...,2] -> (origin [3], unit directions [...,3]) in the world: the inverse of `project` as it is written,
    (R^T)^-1 K^-1 (column, row, 1).  The poses hold float32 values, so R is orthonormal to 2^-24 only and R itself in place of (R^T)^-1
    would already move a pixel by 2.5e-6 px."""
    K, pose, uv = np.asarray(K, np.float64), np.asarray(pose, np.float64), np.asarray(uv, np.float64)
    p = np.concatenate([uv, np.ones(uv.shape[:-1] + (1,))], axis=-1)
    d = np.einsum("ij,jk,...k->...i", np.linalg.inv(pose[:3, :3].T), np.linalg.inv(K[:3, :3]), p)
    return pose[:3, 3].copy(), d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- distances, any dimension ---------------------------------------------------------------------------------------------------------
def point_segment(p, a, b):
    """p [...,d] to the segments a, b [...,d] (broadcast) -> (distance [...], foot [...,d])."""
    p, a, b = (np.asarray(v, np.float64) for v in (p, a, b))
    e = b - a
    ee = (e * e).sum(-1)
    s = np.clip(((p - a) * e).sum(-1) / np.where(ee > 0.0, ee, 1.0), 0.0, 1.0)
    foot = a + s[..., None] * e
    return np.linalg.norm(p - foot, axis=-1), foot


def point_line(p, a, b):
    """p [...,d] to the infinite lines through a and b -> (distance [...], parameter [...]: 0 at a, 1 at b)."""
    p, a, b = (np.asarray(v, np.float64) for v in (p, a, b))
    e = b - a
    s = ((p - a) * e).sum(-1) / (e * e).sum(-1)
    return np.linalg.norm(p - (a + s[..., None] * e), axis=-1), s


# ---- the box in closed form -----------------------------------------------------------------------------------------------------------
def box_half(verts):
    """The half extents of a box centred at the origin."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    assert np.array_equal(v.max(0), -v.min(0))
    return v.max(0)


def box_sdf(p, h):
    """The signed distance: q = |p| - h, |max(q, 0)| + min(max(q), 0)."""
    q = np.abs(np.asarray(p, np.float64)) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def box_slab(o, d, h):
    """Rays o + t d, d [...,3] -> t [...] of the first point of the box with t >= 0, +inf on a miss (the slab form)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - o) / d, (h - o) / d
    near, far = np.fmax.reduce(np.minimum(t1, t2), axis=-1), np.fmin.reduce(np.maximum(t1, t2), axis=-1)
    return np.where((near <= far) & (far >= 0.0), np.where(near >= 0.0, near, far), np.inf)


def box_edge_visible(C, a, b, h):
    """The convex rule: the edge a-b of the box is seen from C iff one of its two faces looks at C.  Its faces are the two axes on which
    both ends sit on the same side; face (axis k, side s) looks at C iff s C[k] > h[k]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    axes = [k for k in range(3) if a[k] == b[k]]
    assert len(axes) == 2 and all(abs(a[k]) == h[k] for k in axes)
    return any(np.sign(a[k]) * C[k] > h[k] for k in axes)


# ---- lines against edges --------------------------------------------------------------------------------------------------------------
def nearest_edge_line(lines3d, J, E):
    """lines3d [L,2,3] -> (edge [L], distance [L]): the edge whose infinite line both end points lie nearest to (the larger of the two)."""
    L3 = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    a, b = J[E[:, 0]], J[E[:, 1]]
    d = point_line(L3[:, :, None, :], a[None, None], b[None, None])[0].max(axis=1)          # [L, nE]
    k = d.argmin(axis=1) if d.shape[0] else np.zeros(0, np.int64)
    return k, d[np.arange(d.shape[0]), k]


def edge_coverage(lines3d, J, E, bar=BAR_TRI):
    """float64 [nE]: the share of each edge's length that the lines within `bar` of its infinite line cover."""
    L3 = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    k, d = nearest_edge_line(L3, J, E)
    out = np.zeros(E.shape[0])
    for e in range(E.shape[0]):
        spans = []
        for l in np.nonzero((k == e) & (d <= bar))[0]:
            s = np.clip(point_line(L3[l], J[E[e, 0]], J[E[e, 1]])[1], 0.0, 1.0)
            spans.append((s.min(), s.max()))
        end = 0.0
        for lo, hi in sorted(spans):
            out[e] += max(0.0, hi - max(lo, end))
            end = max(end, hi)
    return out


def edges_2d(K, pose, J, E):
    """Every edge projected into one view -> (a [nE,2], b [nE,2])."""
    p = project(K, pose, J)[0]
    return p[E[:, 0]], p[E[:, 1]]


def offsets_to_edges(segments, K, pose, J, E):
    """segments [n,4] of one view -> (offset [n,2]: the midpoint minus its foot on the nearest projected edge; normal [n,2]: that
    edge's unit normal in the picture)."""
    s = np.asarray(segments, np.float64).reshape(-1, 4)
    mid = (s[:, :2] + s[:, 2:]) / 2.0
    a, b = edges_2d(K, pose, J, E)
    d, foot = point_segment(mid[:, None, :], a[None], b[None])
    k = d.argmin(axis=1) if d.shape[0] else np.zeros(0, np.int64)
    e = (b - a)[k]
    normal = np.stack([-e[:, 1], e[:, 0]], axis=1) / np.linalg.norm(e, axis=1, keepdims=True)
    return mid - foot[np.arange(mid.shape[0]), k], normal


# ---- the conditions both modules assert ---------------------------------------------------------------------------------------------
def check_runs(sc, idx, p2, p3, record):
    """The generator's leg: p2 is the projection of p3, p3 lies on its edge, and for the box the (view, edge) pairs with a run are the
    convex rule's."""
    J, E = sc["junctions"], sc["edges"]
    proj = np.stack([project(sc["K"][v], sc["poses"][v], x)[0] for v, x in zip(idx[:, 0], p3)]).reshape(-1, 4)
    e2 = record("p2", np.abs(proj - p2).max())
    e3 = record("p3", point_segment(p3, J[E[idx[:, 1], 0]][:, None], J[E[idx[:, 1], 1]][:, None])[0].max())
    assert e2 <= BAR_P2 and e3 <= BAR_P3, (e2, e3)
    if sc["name"] == "box":
        want = {(v, e) for v in range(VIEWS) for e in range(E.shape[0])
                if box_edge_visible(sc["poses"][v][:3, 3], J[E[e, 0]], J[E[e, 1]], sc["h"])}
        assert {(int(v), int(e)) for v, e in idx[:, :2]} == want


def check_detections(sc, lines, offsets, record):
    """Every midpoint within BAR_DET_MID of a projected edge; each component of the mean offset below BAR_DET_MEAN.  A segment shows
    only the part of a shift s that lies along its edge's normal n, (n.s) n, so over edges of all directions the mean offset is about
    s / 2: a half-pixel mix-up in both axes gives 0.23 and 0.29 px here, at the bar itself.  The shift is therefore solved for as well,
    (sum n n^T) s = sum n (n.offset), and held to the same bar, where the mix-up gives 0.5 px."""
    pairs = [offsets_to_edges(lines[offsets[v]:offsets[v + 1]], sc["K"][v], sc["poses"][v], sc["junctions"], sc["edges"]) for v in range(VIEWS)]
    off, n = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    assert off.shape[0] > 0
    worst = record("detect_midpoint", np.linalg.norm(off, axis=1).max())
    mean = off.mean(axis=0)
    shift = np.linalg.solve(np.einsum("ni,nj->ij", n, n), (n * (n * off).sum(1, keepdims=True)).sum(0))
    record("detect_mean_x", abs(mean[0])), record("detect_mean_y", abs(mean[1]))
    record("detect_shift_x", abs(shift[0])), record("detect_shift_y", abs(shift[1]))
    assert worst <= BAR_DET_MID, worst
    assert np.abs(mean).max() < BAR_DET_MEAN, mean
    assert np.abs(shift).max() < BAR_DET_MEAN, shift
    return off, shift


def check_lines3d(sc, lines3d, record, what):
    """Every line's two end points within BAR_TRI of one edge's infinite line, and the edges covered over COVER of their length."""
    J, E = sc["junctions"], sc["edges"]
    _, d = nearest_edge_line(lines3d, J, E)
    worst = record(what, d.max())
    covered = int((edge_coverage(lines3d, J, E) >= COVER).sum())
    assert worst <= BAR_TRI, worst
    assert covered >= COVERED[sc["name"]], covered


def closest_points(h, seed=7):
    """257 points in [-1, 1]^3: 200 anywhere, 40 inside the box, 17 on its faces."""
    rng = np.random.default_rng(seed)
    anywhere, inside, face = rng.uniform(-1.0, 1.0, (200, 3)), rng.uniform(-1.0, 1.0, (40, 3)) * h, rng.uniform(-1.0, 1.0, (17, 3)) * h
    for i in range(17):
        face[i, i % 3] = h[i % 3] * (1.0 if i % 2 else -1.0)
    return np.concatenate([anywhere, inside, face])


def camera_pixels(K, R, seed):
    """R integer pixels: the four corners, the principal point and seeded others, float64 [R,2]."""
    rng = np.random.default_rng(seed)
    fixed = np.array([[0, 0], [RES - 1, 0], [0, RES - 1], [RES - 1, RES - 1], [K[0, 2], K[1, 2]]], np.float64)
    return np.concatenate([fixed, rng.integers(0, RES, (R - 5, 2)).astype(np.float64)])


def check_attraction(segs, uv, uv_proj, lines2d, distance, record, what):
    """For the rays (uv, uv_proj, lines2d [n,>=4]) of one view with the runs segs [m,4] (float32 values): the foot lies on its segment
    and within `distance` of its pixel; the segment is one of the runs, and in float64 no run is nearer by TIE_PX or more.

    That last condition holds for EVERY ray and none is left out.  Where the nearest run leads by TIE_PX it says that the segment is the
    nearest run; where two runs tie it still ties the segment to the nearest distance.  Leaving the ties out would not do here: runs
    that end in a shared junction are equally far from every pixel of the sector beyond it, exactly, which is 6 to 7 % of a view's
    support (recorded), far over a 1 % allowance.  -> (the run of each ray, the share of rays with such a tie)."""
    segs, uv, uv_proj, seg = (np.asarray(x, np.float64) for x in (segs, uv, uv_proj, np.asarray(lines2d)[:, :4]))
    off = record(what + "_foot", point_segment(uv_proj, seg[:, :2], seg[:, 2:])[0].max())
    assert off <= BAR_FOOT, off
    assert (np.linalg.norm(uv_proj - uv, axis=1) <= distance + DIST_SLACK).all()
    same = (seg[:, None, :] == segs[None]).all(axis=2)
    assert same.any(axis=1).all()
    run = same.argmax(axis=1)
    d = point_segment(uv[:, None, :], segs[None, :, :2], segs[None, :, 2:])[0]
    order = np.sort(d, axis=1)
    tie = (order[:, 1] - order[:, 0] < TIE_PX) if segs.shape[0] > 1 else np.zeros(uv.shape[0], bool)
    lead = record(what + "_lead", (d[np.arange(uv.shape[0]), run] - order[:, 0]).max())
    assert lead < TIE_PX, lead
    assert (d.argmin(axis=1) == run)[~tie].all()                          # follows from the lead; kept as the condition is usually stated
    return run, record(what + "_ties", float(tie.mean()))


def merge_detections(refs):
    """detect_f64.detect's dicts of several picture sets -> the dict of the pictures stacked in that order (views are independent)."""
    out, views, kept = {}, 0, 0
    for k in ("lines", "width", "nfa", "n", "k", "part", "label", "cand_keep", "cand_judge", "grey"):
        out[k] = np.concatenate([r[k] for r in refs])
    view, cand, offsets = [], [], [np.zeros(1, np.int32)]
    for r in refs:
        view.append(r["view"] + views)
        cand.append(r["cand"] + np.array([views, 0, 0]))
        offsets.append(r["offsets"][1:] + kept)
        views, kept = views + len(r["offsets"]) - 1, kept + r["lines"].shape[0]
    out["view"], out["cand"], out["offsets"] = np.concatenate(view), np.concatenate(cand), np.concatenate(offsets).astype(np.int32)
    return out


def support_rays(sc, v, distance):
    """Every pixel of view v that supports its nearest run, as a batch would hand it: (uv [n,2], uv_proj [n,2], lines2d [n,4]) from the
    attraction oracle's maps."""
    from oracle import attraction_oracle as A
    lmap = sc["lmap"][v]
    mask, foot = A.support(lmap, distance)
    ys, xs = np.nonzero(mask)
    return np.stack([xs, ys], 1).astype(np.float64), foot[ys, xs].astype(np.float64), sc["segs"][v][sc["label"][v][ys, xs]]


def pixel_grid():
    """Every pixel (column, row), column fastest: the datasets' order, float32 [RES RES, 2]."""
    ys, xs = np.mgrid[0:RES, 0:RES]
    return np.stack([xs, ys], -1).reshape(-1, 2).astype(np.float32)


def check_pictures(sc, v, o, d, t, record, what):
    """The rays (o [3], d [n,3], float32 values) of every pixel of view v and their hit depths t [n] (+inf: a miss): a pixel whose
    sub-samples all hit must hit, one with none must miss; for the box the depth is the slab form's.  Pixels with a partial count are
    left out, PARTIAL_CAP of the picture at most."""
    hits = sc["hits"][v].reshape(-1)
    full, none = hits == SS * SS, hits == 0
    share = record(what + "_partial", 1.0 - (full | none).mean())
    assert share <= PARTIAL_CAP, share
    t = np.asarray(t, np.float64).reshape(-1)
    assert np.isfinite(t[full]).all() and np.isinf(t[none]).all() and full.any() and none.any()
    if sc["name"] == "box":
        want = box_slab(np.asarray(o, np.float64), np.asarray(d, np.float64), sc["h"])
        assert np.isfinite(want[full]).all() and np.isinf(want[none]).all()
        err = record(what + "_depth", np.abs(t[full] - want[full]).max())
        assert err <= BAR_DEPTH, err


def check_camera(sc, v, uv, o, d, record, what):
    """Rays (o [n,3] or [3], d [n,3]; float32 values) through the pixels uv [n,2] of view v: the truth's projection of o + t d is uv."""
    o, d, uv = (np.asarray(x, np.float64) for x in (o, d, uv))
    err = max(np.abs(project(sc["K"][v], sc["poses"][v], o + t * d)[0] - uv).max() for t in (0.5, 2.0, 5.0))
    record(what, err)
    return err


def view_runs(sc, v):
    """(p2 [n,4], p3 [n,2,3]) of view v's runs, float64."""
    r = sc["runs"]
    m = r["idx"][:, 0] == v
    return r["p2"][m], r["p3"][m]


# ---- the shared case --------------------------------------------------------------------------------------------------------------
_scenes = {}


def scene(name):
    """-> dict, read-only, built once per process.  Inputs: verts, faces, junctions, edges (normalised), K [V,3,3], poses [V,4,4], h (box).
    The restatements' outputs: runs (scenegen_f64.visible_edges), segs (per view, the runs' p2 rounded to float32 as the dataset hands
    them), rgb, mask, hits (pictures with counts), det (detect_f64.detect of rgb), tri_runs and tri_det (triangulate_f64.lines),
    lmap and label (attraction_oracle.encode_lines, views 0 and 7)."""
    if name in _scenes:
        return _scenes[name]
    from neat_amd import scenegen
    from oracle import attraction_oracle as A
    from tests import detect_f64 as D
    from tests import scenegen_f64 as G
    from tests import triangulate_f64 as T
    verts, faces, junctions, edges = scenegen.shapes[name]
    verts, junctions = scenegen.normalise(verts, junctions)
    faces, edges = faces.copy(), edges.copy()
    K, poses = scenegen.cameras(VIEWS, RES)
    sc = {"name": name, "verts": verts, "faces": faces, "junctions": junctions, "edges": edges, "K": K, "poses": poses}
    if name == "box":
        sc["h"] = box_half(verts)
    d = scenegen.DEFAULTS
    sc["runs"] = G.visible_edges(verts, faces, junctions, edges, K, poses, RES, RES, step=d["step"], min_len=d["min_len"], bias=d["bias"],
                                 near=d["near"])
    sc["segs"] = [sc["runs"]["p2"][sc["runs"]["idx"][:, 0] == v].astype(np.float32).astype(np.float64) for v in range(VIEWS)]
    sc["rgb"], sc["mask"], sc["hits"] = G.pictures(verts, faces, K, poses, RES, RES, ss=SS, counts=True)
    sc["det"] = D.detect(sc["rgb"], 1.0)
    off = sc["det"]["offsets"]
    sc["det_segs"] = [sc["det"]["lines"][off[v]:off[v + 1]] for v in range(VIEWS)]
    sc["tri_runs"] = T.lines(sc["segs"], K, poses)
    sc["tri_det"] = T.lines(sc["det_segs"], K, poses)
    sc["attraction_views"] = (0, 7)
    sc["lmap"], sc["label"] = {}, {}
    for v in sc["attraction_views"]:
        sc["lmap"][v], sc["label"][v], _ = A.encode_lines(sc["segs"][v].astype(np.float32), RES, RES)
    for x in sc.values():
        for y in (x.values() if isinstance(x, dict) else x if isinstance(x, list) else [x]):
            if isinstance(y, np.ndarray):
                y.setflags(write=False)
    _scenes[name] = sc
    return sc
