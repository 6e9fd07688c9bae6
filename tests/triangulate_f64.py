"""The triangulation rule of DESIGN 3k in numpy float64: the definition that neat_amd.triangulate (csrc/kernels_triangulate.hpp) must
reproduce.  Every product, sum and quotient stands alone in the order written here (numpy fuses nothing), which is the order of the
kernels, so the depths of a hypothesis are the same bits on both sides; the only transcendental function is the exp of the score.

    hypotheses(segments, Ks, poses, ...)  -> dict: rows int32 [H,4] = a, i, m, j; depths [H,2]; neighbours [V,M]; offsets [V+1]; margin
    lines(segments, Ks, poses, ...)       -> dict with the keys of triangulate.lines, and `margins`

`margin` / `margins` say how close the input comes to flipping a decision; tests/test_triangulate_math.py asserts them for every scene
the device is compared on."""
import math

import numpy as np

DEFAULTS = {"neighbours": 6, "angle_min": 5.0, "overlap_min": 0.25, "sigma_px": 2.5, "min_score": 1.5, "min_views": 3}


def cameras(Ks, poses):
    """-> dict of float64 arrays per view: Kinv, R (world -> camera), t, K, P = K [R|t], C."""
    K = np.asarray(Ks, dtype=np.float64).reshape(-1, 3, 3)
    T = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    V = K.shape[0]
    C = T[:, :3, 3].copy()
    R = T[:, :3, :3].transpose(0, 2, 1).copy()
    t = np.zeros((V, 3))
    for r in range(3):
        t[:, r] = -((R[:, r, 0] * C[:, 0] + R[:, r, 1] * C[:, 1]) + R[:, r, 2] * C[:, 2])
    fx, sk, cx, fy, cy = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    Kinv = np.zeros((V, 3, 3))
    Kinv[:, 0, 0] = 1.0 / fx
    Kinv[:, 0, 1] = -sk / (fx * fy)
    Kinv[:, 0, 2] = (sk * cy - cx * fy) / (fx * fy)
    Kinv[:, 1, 1] = 1.0 / fy
    Kinv[:, 1, 2] = -cy / fy
    Kinv[:, 2, 2] = 1.0
    Rt = np.concatenate([R, t[:, :, None]], axis=2)
    P = np.zeros((V, 3, 4))
    for r in range(3):
        for c in range(4):
            P[:, r, c] = (K[:, r, 0] * Rt[:, 0, c] + K[:, r, 1] * Rt[:, 1, c]) + K[:, r, 2] * Rt[:, 2, c]
    return {"Kinv": Kinv, "R": R, "t": t, "K": K, "P": P, "C": C}


def neighbour_table(C, M):
    """The M nearest other views of each view, nearest first, ties to the lower index; M is clipped to V - 1."""
    V = C.shape[0]
    M = max(0, min(int(M), V - 1))
    nb = np.zeros((V, M), dtype=np.int32)
    for a in range(V):
        d = C[a][None, :] - C
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        dist[a] = np.inf
        nb[a] = np.argsort(dist, kind="stable")[:M]
    return nb


def norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def segment_constants(seg, cam, v):
    """seg [n,4] of view v -> its viewing rays d1, d2 [n,3], the unit normal na [n,3] of their plane, the back-projected plane pi [n,4],
    q1 [n,2], u [n,2], uu [n], |pi_xyz| [n]."""
    x1, y1, x2, y2 = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    Ki, R, P = cam["Kinv"][v], cam["R"][v], cam["P"][v]
    d = []
    for x, y in ((x1, y1), (x2, y2)):
        r = [(Ki[q, 0] * x + Ki[q, 1] * y) + Ki[q, 2] for q in range(3)]
        d.append(np.stack([(R[0, q] * r[0] + R[1, q] * r[1]) + R[2, q] * r[2] for q in range(3)], axis=1))
    d1, d2 = d
    n = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2], d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], axis=1)
    na = n / norm3(n[:, 0], n[:, 1], n[:, 2])[:, None]
    l0, l1, l2 = y1 - y2, x2 - x1, x1 * y2 - y1 * x2
    pi = np.stack([(P[0, q] * l0 + P[1, q] * l1) + P[2, q] * l2 for q in range(4)], axis=1)
    ux, uy = x2 - x1, y2 - y1
    return {"d1": d1, "d2": d2, "na": na, "pi": pi, "q1": np.stack([x1, y1], axis=1), "u": np.stack([ux, uy], axis=1), "uu": ux * ux + uy * uy,
            "norm": norm3(pi[:, 0], pi[:, 1], pi[:, 2])}


def pair_test(A, B, cam, a, b, cos_min, overlap_min):
    """Every segment of a (rows) against every segment of b (columns) -> (ok bool [na,nb], s1, s2 [na,nb], margin: the least distance of a
    quantity from the threshold it is compared with, over the comparisons that no earlier one had already failed)."""
    C, R, t, K = cam["C"][a], cam["R"][b], cam["t"][b], cam["K"][b]
    pi, col = B["pi"], lambda x: x[None, :]
    row = lambda x: x[:, None]
    c = np.abs((row(A["na"][:, 0]) * col(pi[:, 0]) + row(A["na"][:, 1]) * col(pi[:, 1])) + row(A["na"][:, 2]) * col(pi[:, 2])) / col(B["norm"])
    e = ((pi[:, 0] * C[0] + pi[:, 1] * C[1]) + pi[:, 2] * C[2]) + pi[:, 3]
    ok = c <= cos_min
    margin = [np.abs(c - cos_min)[np.isfinite(c)]]
    s, ts = [], []
    front = np.ones_like(ok)
    for d in (A["d1"], A["d2"]):
        sk = -col(e) / ((col(pi[:, 0]) * row(d[:, 0]) + col(pi[:, 1]) * row(d[:, 1])) + col(pi[:, 2]) * row(d[:, 2]))
        s.append(sk)
    pos = (s[0] > 0.0) & (s[1] > 0.0) & np.isfinite(s[0]) & np.isfinite(s[1])
    margin.append(np.minimum(np.abs(s[0]), np.abs(s[1]))[ok & np.isfinite(s[0]) & np.isfinite(s[1])])
    ok = ok & pos
    for sk, d in zip(s, (A["d1"], A["d2"])):
        X = [C[q] + sk * row(d[:, q]) for q in range(3)]
        x = [((R[r, 0] * X[0] + R[r, 1] * X[1]) + R[r, 2] * X[2]) + t[r] for r in range(3)]
        front = front & (x[2] > 0.0)
        margin.append(np.abs(x[2])[ok])
        y0 = ((K[0, 0] * x[0] + K[0, 1] * x[1]) + K[0, 2] * x[2]) / x[2]
        y1 = ((K[1, 0] * x[0] + K[1, 1] * x[1]) + K[1, 2] * x[2]) / x[2]
        ts.append(((y0 - col(B["q1"][:, 0])) * col(B["u"][:, 0]) + (y1 - col(B["q1"][:, 1])) * col(B["u"][:, 1])) / col(B["uu"]))
    ok = ok & front & np.isfinite(ts[0]) & np.isfinite(ts[1])
    lo, hi = np.minimum(ts[0], ts[1]), np.maximum(ts[0], ts[1])
    inter = np.minimum(hi, 1.0) - np.maximum(lo, 0.0)
    uni = np.maximum(hi, 1.0) - np.minimum(lo, 0.0)
    margin.append(np.abs(inter - overlap_min * uni)[ok])
    ok = ok & (inter >= overlap_min * uni)
    return ok, s[0], s[1], min((float(m.min()) for m in margin if m.size), default=np.inf)


def _prepare(segments, Ks, poses):
    segments = [np.asarray(s, dtype=np.float64).reshape(-1, 4) for s in segments]
    cam = cameras(Ks, poses)
    assert cam["C"].shape[0] == len(segments)
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in segments])]).astype(np.int32)
    return segments, cam, offsets


def hypotheses(segments, Ks, poses, neighbours=DEFAULTS["neighbours"], angle_min=DEFAULTS["angle_min"], overlap_min=DEFAULTS["overlap_min"], **_):
    segments, cam, offsets = _prepare(segments, Ks, poses)
    V = len(segments)
    nb = neighbour_table(cam["C"], neighbours)
    cos_min = math.cos(float(angle_min) * math.pi / 180.0)
    rows, depths, margin = [], [], np.inf
    with np.errstate(all="ignore"):                       # a NaN is an answer here: it fails every comparison
        consts = [segment_constants(s, cam, v) for v, s in enumerate(segments)]
        for a in range(V):
            per_slot = []
            for m in range(nb.shape[1]):
                b = int(nb[a, m])
                ok, s1, s2, mg = pair_test(consts[a], consts[b], cam, a, b, cos_min, float(overlap_min))
                margin = min(margin, mg)
                i, j = np.nonzero(ok)                     # row-major: (i, j) ascending
                per_slot.append((i, np.full_like(i, m), j, s1[ok], s2[ok]))
            if not per_slot:
                continue
            i, m, j, s1, s2 = (np.concatenate(p) for p in zip(*per_slot))
            order = np.lexsort((j, m, i))                 # the hypotheses of one segment together, in (m, j) order
            rows.append(np.stack([np.full_like(i, a), i, m, j], axis=1)[order])
            depths.append(np.stack([s1, s2], axis=1)[order])
    rows = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)
    depths = np.concatenate(depths) if depths else np.zeros((0, 2))
    return {"rows": rows.reshape(-1, 4), "depths": depths.reshape(-1, 2), "neighbours": nb, "offsets": offsets, "margin": margin,
            "consts": consts, "cam": cam}


def line_dist(p, a, b):
    """Distance of point p to the infinite line through a and b."""
    w, d = p - a, b - a
    return norm3(w[1] * d[2] - w[2] * d[1], w[2] * d[0] - w[0] * d[2], w[0] * d[1] - w[1] * d[0]) / norm3(d[0], d[1], d[2])


def lines(segments, Ks, poses, neighbours=DEFAULTS["neighbours"], angle_min=DEFAULTS["angle_min"], overlap_min=DEFAULTS["overlap_min"],
          sigma_px=DEFAULTS["sigma_px"], min_score=DEFAULTS["min_score"], min_views=DEFAULTS["min_views"]):
    hyp = hypotheses(segments, Ks, poses, neighbours, angle_min, overlap_min)
    rows, depths, nb, offsets, cam, consts = (hyp[k] for k in ("rows", "depths", "neighbours", "offsets", "cam", "consts"))
    S, V = int(offsets[-1]), len(offsets) - 1
    view = np.repeat(np.arange(V), np.diff(offsets))
    seg_of = offsets[rows[:, 0]] + rows[:, 1] if rows.size else np.zeros(0, np.int64)
    hoff = np.searchsorted(seg_of, np.arange(S + 1))
    estimate, score, radius = np.zeros((S, 2, 3)), np.zeros(S), np.zeros(S)
    kept = np.zeros(S, dtype=bool)
    margins = {"pair": hyp["margin"], "score": np.inf, "top2": np.inf, "link": np.inf}
    with np.errstate(all="ignore"):
        # ---- score: the best hypothesis of every segment
        for g in range(S):
            h0, h1 = hoff[g], hoff[g + 1]
            if h1 == h0:
                continue
            a = view[g]
            f = cam["K"][a][0, 0]
            m, s = rows[h0:h1, 2], depths[h0:h1]
            sg = (sigma_px * s) / f
            w = 1.0 / (2.0 * (sg * sg))                   # one reciprocal a hypothesis, products in the pair loop
            e = s[:, None, :] - s[None, :, :]
            q = (e[..., 0] * e[..., 0]) * w[:, None, 0] + (e[..., 1] * e[..., 1]) * w[:, None, 1]       # sim = exp(-q)
            sc = np.zeros(h1 - h0)
            for slot in np.unique(m):                     # ascending: slot order
                best = np.exp(-np.fmin.reduce(q[:, m == slot], axis=1, initial=np.inf))                 # max of exp(-q) = exp(-min q)
                sc = sc + np.where(m != slot, best, 0.0)
            h = int(np.argmax(sc))                        # the first of equal maxima
            i = g - offsets[a]
            d = (consts[a]["d1"][i], consts[a]["d2"][i])
            r = 0.0
            for k in range(2):
                estimate[g, k] = cam["C"][a] + s[h, k] * d[k]
                r = max(r, ((sigma_px * s[h, k]) / f) * norm3(d[k][0], d[k][1], d[k][2]))
            score[g], radius[g], kept[g] = sc[h], r, sc[h] >= min_score
            margins["score"] = min(margins["score"], abs(sc[h] - min_score))
            if sc.size > 1 and sc[h] > 0.0:               # a best score of 0 is a sum of no terms: that tie is exact on every side
                margins["top2"] = min(margins["top2"], (sc[h] - np.sort(sc)[-2]) / sc[h])
        # ---- link: union-find over the kept estimates; the label is the lowest member
        parent = np.arange(S)

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for g in np.nonzero(kept)[0]:
            a = view[g]
            for h in range(hoff[g], hoff[g + 1]):
                p = int(offsets[nb[a, rows[h, 2]]] + rows[h, 3])
                if not kept[p]:
                    continue
                tol = 2.0 * max(radius[g], radius[p])
                e, f = estimate[g], estimate[p]
                dist = [line_dist(f[0], e[0], e[1]), line_dist(f[1], e[0], e[1]), line_dist(e[0], f[0], f[1]), line_dist(e[1], f[0], f[1])]
                margins["link"] = min([margins["link"]] + [abs(x - tol) / tol for x in dist if np.isfinite(x)])
                if all(x <= tol for x in dist):
                    rg, rp = find(g), find(p)
                    parent[max(rg, rp)] = min(rg, rp)
        labels = np.array([find(g) if kept[g] else -1 for g in range(S)], dtype=np.int32).reshape(S)
        # ---- lines: the components with enough distinct views, in label order
        members = np.full(S, -1, dtype=np.int32)
        out_lines, out_views, out_support = [], [], []
        for r in np.unique(labels[labels >= 0]):
            mem = np.nonzero(labels == r)[0]
            nv = np.unique(view[mem]).size
            if nv < min_views:
                continue
            ax = mem[int(np.argmax(score[mem]))]
            A, B = estimate[ax]
            bd = B - A
            u = bd / norm3(bd[0], bd[1], bd[2])
            P = estimate[mem].reshape(-1, 3)
            tau = ((P[:, 0] - A[0]) * u[0] + (P[:, 1] - A[1]) * u[1]) + (P[:, 2] - A[2]) * u[2]
            members[mem] = len(out_lines)
            out_lines.append(np.stack([A + tau.min() * u, A + tau.max() * u]))
            out_views.append(nv)
            out_support.append(score[ax])
    return {"lines3d": np.asarray(out_lines, dtype=np.float64).reshape(-1, 2, 3), "views": np.asarray(out_views, dtype=np.int32),
            "support": np.asarray(out_support, dtype=np.float64), "members": members, "labels": labels, "estimate": estimate, "score": score,
            "kept": kept, "rows": rows, "depths": depths, "offsets": offsets, "neighbours": nb, "margins": margins}


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """A camera-to-world pose [4,4] at `eye` looking at `target` (x right, y down, z forward)."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, up)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose


def ring_cameras(V, radius=4.0, height=1.5, f=600.0, c=256.0, seed=0):
    """V cameras on a jittered ring around the origin -> (Ks [V,3,3], poses [V,4,4])."""
    rng = np.random.default_rng(seed)
    poses = []
    for v in range(V):
        ang = 2.0 * math.pi * (v + 0.3 * rng.random()) / max(V, 1)
        poses.append(look_at((radius * math.cos(ang), radius * math.sin(ang), height + 0.5 * rng.random())))
    K = np.array([[f, 0.0, c], [0.0, f, c], [0.0, 0.0, 1.0]])
    return np.repeat(K[None], V, axis=0), np.asarray(poses).reshape(-1, 4, 4)


def project(lines3d, K, pose):
    """lines3d [n,2,3] -> exact projections [n,4] and the depths [n,2] in the view."""
    R, C = pose[:3, :3].T, pose[:3, 3]
    x = (np.asarray(lines3d, dtype=np.float64).reshape(-1, 3) - C) @ R.T
    y = x @ K.T
    return (y[:, :2] / y[:, 2:3]).reshape(-1, 4), x[:, 2].reshape(-1, 2)


def random_scene(counts, M_lines=40, seed=0, length=None):
    """len(counts) ring cameras; view v sees counts[v] segments: projections of shared random 3-D segments (cycled, with a sub-pixel
    jitter that keeps repeated ones distinct) -> (segments list, Ks, poses).  length: the 3-D segments keep their first end and their
    direction and get this length (default: both ends uniform in the cube)."""
    rng = np.random.default_rng(seed)
    V = len(counts)
    Ks, poses = ring_cameras(V, seed=seed)
    world = rng.uniform(-1.0, 1.0, (M_lines, 2, 3))
    if length is not None:
        d = world[:, 1] - world[:, 0]
        world[:, 1] = world[:, 0] + length * d / np.linalg.norm(d, axis=1, keepdims=True)
    segments = []
    for v, n in enumerate(counts):
        p, _ = project(world, Ks[v], poses[v])
        idx = np.arange(n) % M_lines
        segments.append(p[idx] + 0.5 * rng.standard_normal((n, 4)) * (np.arange(n)[:, None] >= M_lines) + 0.05 * rng.standard_normal((n, 4)))
    return segments, Ks, poses


def cube_scene(V=12, extra=8, seed=1):
    """The 12 edges of a cube and `extra` random segments seen from V ring cameras, exact projections -> (segments, Ks, poses, world
    [12 + extra, 2, 3])."""
    rng = np.random.default_rng(seed)
    c = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    edges = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.sum(c[i] != c[j]) == 1]
    world = np.concatenate([np.array([[c[i], c[j]] for i, j in edges]), rng.uniform(-1.2, 1.2, (extra, 2, 3))])
    Ks, poses = ring_cameras(V, seed=seed)
    segments = [project(world, Ks[v], poses[v])[0] for v in range(V)]
    return segments, Ks, poses, world


def fixture_segments(fx):
    """The arrays of tests/golden/triangulate_abc_00075213.npz -> one float64 [n_v,4] per view: the edges whose weight is above 0.05, as
    WireframeGraph.line_segments(0.05) gives them."""
    out = []
    for v in range(len(fx["view_ids"])):
        vert = fx["vertices"][fx["vertex_off"][v]:fx["vertex_off"][v + 1]]
        e0, e1 = fx["edge_off"][v], fx["edge_off"][v + 1]
        e = fx["edges"][e0:e1][fx["weights"][e0:e1] > np.float32(0.05)]
        out.append(np.concatenate([vert[e[:, 0]], vert[e[:, 1]]], axis=1).astype(np.float64).reshape(-1, 4))
    return out


def fixture_scene():
    import os
    fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "triangulate_abc_00075213.npz")))
    return fixture_segments(fx), fx["intrinsics"], fx["extrinsics"], fx


# the scenes the device is compared on (tests/test_triangulate_gpu.py); tests/test_triangulate_math.py asserts their margins.  The
# segment counts straddle the wavefront (63, 64, 65) and the tile of the pair kernel (255, 256, 257); seeds are chosen so that no
# decision of the rule lies at its threshold
GPU_SCENES = {
    "v2": lambda: random_scene([65, 255], 300, seed=11),
    "v3": lambda: random_scene([255, 257, 64], 300, seed=12),
    "v7": lambda: random_scene([256, 0, 1, 63, 64, 65, 257], 300, seed=13),
    "capacity": lambda: capacity_scene(),
    "fixture": lambda: fixture_scene()[:3],
    "fixture_slice": lambda: tuple(part[3:17] for part in fixture_scene()[:3]),
    "f32": lambda: float32_scene(),
}


def float32_scene():
    """Segments rounded to float32, as the datasets give them (the values are then exact in float64)."""
    seg, Ks, poses = random_scene([4, 4, 4], 4, seed=3)
    return [s.astype(np.float32).astype(np.float64) for s in seg], Ks, poses
_scenes, _refs = {}, {}


def scene(name):
    """(segments, Ks, poses) of a named scene, built once; read-only."""
    if name not in _scenes:
        seg, Ks, poses = GPU_SCENES[name]()
        for a in list(seg) + [Ks, poses]:
            a.setflags(write=False)
        _scenes[name] = (seg, Ks, poses)
    return _scenes[name]


def reference(name, what="lines", **kw):
    """The reference's answer on a named scene, computed once per set of arguments."""
    key = (name, what, tuple(sorted(kw.items())))
    if key not in _refs:
        _refs[key] = (lines if what == "lines" else hypotheses)(*scene(name), **kw)
    return _refs[key]


def capacity_scene(V=70, partners=16, seed=2):
    """Capacity edges of the kernels.  One 3-D line along the ring's axis, seen as one segment in each of V views (a component of more
    than 64 members); the six views nearest to view 0 see it `partners` times, as collinear segments with different ends, so the segment
    of view 0 has 6 * partners > 64 hypotheses.  A tenth of a pixel of noise keeps the scores apart."""
    rng = np.random.default_rng(seed)
    Ks, poses = ring_cameras(V, radius=5.0, seed=seed)
    A, B = np.array([0.05, -0.03, -0.8]), np.array([-0.02, 0.04, 0.9])
    near = neighbour_table(np.asarray(poses)[:, :3, 3], 6)[0]
    segments = []
    for v in range(V):
        n = partners if v in near else 1
        lo, hi = rng.uniform(0.0, 0.1, n), rng.uniform(0.9, 1.0, n)
        world = np.stack([A + lo[:, None] * (B - A), A + hi[:, None] * (B - A)], axis=1)
        segments.append(project(world, Ks[v], poses[v])[0] + 0.1 * rng.standard_normal((n, 4)))
    return segments, Ks, poses
