"""The closest point on a triangle mesh, restated in float64 (neat_amd/raycast.py closest, csrc/kernels_closest.hpp): the rule
for one triangle, the brute force over all triangles with the tie rule (closest_one, closest_all), and candidate_distance, a second
formula for the distance alone that shares nothing with the rule.  This file is the definition; the scenes are tests/raycast_f64.py's.

The rule (Ericson, Real-Time Collision Detection, 5.1.5).  Query p and triangle (a, b, c) float64; every operation below is one float64
operation, every product rounded on its own (numpy never fuses a product into an addition), a dot product is (x x' + y y') + z z':
    ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
    d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
    vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
    regions, the first that holds:                                         q                           (u, v)
      A    d1 <= 0 and d2 <= 0                                             a                           (0, 0)
      B    d3 >= 0 and d4 <= d3                                            b                           (1, 0)
      AB   vc <= 0 and d1 >= 0 and d3 <= 0          s = d1 / (d1 - d3)     a + s ab                    (s, 0)
      C    d6 >= 0 and d5 <= d6                                            c                           (0, 1)
      AC   vb <= 0 and d2 >= 0 and d6 <= 0          s = d2 / (d2 - d6)     a + s ac                    (0, s)
      BC   va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0
                              s = (d4 - d3) / ((d4 - d3) + (d5 - d6))      b + s (c - b)               (1 - s, s)
      in   otherwise    den = (va + vb) + vc, s = vb / den, t = vc / den   (a + s ab) + t ac           (s, t)
    q = (1 - u - v) a + u b + v c up to rounding;  d = p - q,  d2 = (dx dx + dy dy) + dz dz
    a triangle with a non-finite vertex or (b - a) x (c - a) == 0 in every component is never closest (raycast_f64.valid_triangles)
    accepted iff d2 <= max_d2 (inclusive; +inf: no bound; a NaN never is)
    result: the accepted triangle of the smallest d2, ties to the lowest face index; a query with a non-finite coordinate, an empty mesh
    or nothing accepted is a miss: d2 = +inf, tri = -1, q = 0, uv = 0.
"""
import numpy as np

from tests.raycast_f64 import box, fan, icosphere, strips, valid_triangles  # noqa: F401  (the scenes of the tests)

INF = float("inf")
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "in")


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def rule(tv, p):
    """tv [..., 3, 3] and p [..., 3], broadcast against each other -> (d2 [...], q [..., 3], uv [..., 2], region [...] int: the index in
    REGIONS).  No validity, no bound: the caller applies them."""
    tv, p = np.asarray(tv, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        a, b, c = tv[..., 0, :], tv[..., 1, :], tv[..., 2, :]
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        region = np.select(conds, list(range(6)), 6)
        s_ab, s_ac, s_bc = d1 / (d1 - d3), d2 / (d2 - d6), e43 / (e43 + e56)
        den = (va + vb) + vc
        s_in, t_in = vb / den, vc / den
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        u = np.select([region == k for k in range(6)], [zero, one, s_ab, zero, zero, 1.0 - s_bc], s_in)
        v = np.select([region == k for k in range(6)], [zero, zero, zero, one, s_ac, s_bc], t_in)
        r3 = region[..., None]
        shape = np.broadcast(a, p).shape
        full = lambda x: np.broadcast_to(x, shape)
        q = np.select([r3 == k for k in range(6)],
                      [full(a), full(b), a + s_ab[..., None] * ab, full(c), a + s_ac[..., None] * ac, b + s_bc[..., None] * bc],
                      (a + s_in[..., None] * ab) + t_in[..., None] * ac)
        d = p - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return dist2, q, np.stack([u, v], -1), region


def closest_one(tv, valid, p, max_d2=INF):
    """One query p [3] against all triangles tv [nf,3,3] (valid bool [nf]) -> (d2, tri, q [3], uv [2])."""
    p = np.asarray(p, np.float64).reshape(3)
    miss = (INF, -1, np.zeros(3), np.zeros(2))
    if tv.shape[0] == 0 or not np.isfinite(p).all():
        return miss
    d2, q, uv, _ = rule(tv, p)
    with np.errstate(invalid="ignore"):
        acc = valid & (d2 <= max_d2)
    if not acc.any():
        return miss
    best = d2[acc].min()
    k = int(np.argmax(acc & (d2 == best)))               # the lowest index among the ties
    return float(d2[k]), k, q[k].copy(), uv[k].copy()


def closest_all(verts, faces, points, max_d2=INF, chunk=256):
    """Brute force over all triangles -> (d2 float64 [N], +inf on a miss; tri int32 [N], -1 on a miss; q float64 [N,3] and uv float64 [N,2],
    zero on a miss).  A face index outside the vertices is the refused tree: every query misses."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    N, nf = pts.shape[0], faces.shape[0]
    out_d2, tri, out_q, out_uv = np.full(N, INF), np.full(N, -1, np.int32), np.zeros((N, 3)), np.zeros((N, 2))
    if nf == 0 or N == 0 or faces.min() < 0 or faces.max() >= verts.shape[0]:
        return out_d2, tri, out_q, out_uv
    tv, valid = verts[faces], valid_triangles(verts, faces)
    finite = np.isfinite(pts).all(axis=1)
    chunk = max(1, min(chunk, (1 << 21) // nf))
    for i in range(0, N, chunk):
        p = pts[i:i + chunk]
        d2, q, uv, _ = rule(tv[None], p[:, None, :])                  # [n, nf]
        with np.errstate(invalid="ignore"):
            acc = valid[None] & (d2 <= max_d2) & finite[i:i + chunk, None]
        key = np.where(acc, d2, INF)
        k = np.argmax(acc & (key == key.min(axis=1, keepdims=True)), axis=1)      # the lowest index among the ties
        rows = np.arange(p.shape[0])
        hit = acc[rows, k]
        sel = i + rows[hit]
        out_d2[sel], tri[sel], out_q[sel], out_uv[sel] = d2[rows, k][hit], k[hit], q[rows, k][hit], uv[rows, k][hit]
    return out_d2, tri, out_q, out_uv


def candidate_distance(tv, p):
    """The distance from p [3] to each triangle of tv [nf,3,3] without the region rule: the foot of the perpendicular on the plane if it
    lies inside the triangle, else the smallest distance to the three edges, each by projection on its line clamped to [0, 1]."""
    tv, p = np.asarray(tv, np.float64), np.asarray(p, np.float64).reshape(3)
    a, b, c = tv[:, 0], tv[:, 1], tv[:, 2]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(1)
    h = ((p - a) * n).sum(1) / nn
    foot = p - h[:, None] * n
    inside = np.ones(tv.shape[0], bool)
    for x, y in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(y - x, foot - x) * n).sum(1) >= 0
    best = np.full(tv.shape[0], INF)
    for x, y in ((a, b), (b, c), (c, a)):
        e = y - x
        s = np.clip(((p - x) * e).sum(1) / (e * e).sum(1), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (x + s[:, None] * e), axis=1))
    return np.where(inside, np.abs(h) * np.sqrt(nn), best)


def mesh_edges(faces):
    """The undirected edges of the faces, sorted, int64 [ne,2]."""
    f = np.asarray(faces).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0).astype(np.int64)


def line_samples(lines3d, samples):
    """The sample points of raycast.line_distance: a t + b (1 - t), t = linspace(0, 1, samples), float64 [n, samples, 3]
    (evaluation/eval-lsr-scannet.py :94-95)."""
    lines = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    t = np.linspace(0.0, 1.0, samples)[None, :, None]
    return lines[:, :1] * t + lines[:, 1:] * (1.0 - t)
