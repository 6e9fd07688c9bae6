"""The definition of the 3-D wireframe builder (neat_amd/csrc/kernels_wireframe3d.hpp implements it, triangulate.wireframe calls
it): the triangulated 3-D lines of a scene and the views' 2-D graphs -> one 3-D graph whose lines share their junctions.  Plain numpy
float64, every sum written out: each product, sum and quotient below is one IEEE operation in the order it stands in, three-term sums
are (a + b) + c, there is no np.linalg and no transcendental function but the one square root of `spread`, and numpy contracts nothing
into a fused multiply-add.  The device forms the same operations in the same order without contraction, so its vertices are these bits
and its decisions are these decisions.

    build(lines3d [N,2,3], support [N], members [S], estimate [S,2,3], endv [S,2], view [S], V, ...) -> dict       # the device's arrays
    wireframe(vertices, edges, Ks, poses, ...) -> dict       # triangulate_f64.lines of vertices[edges], then build

endv[g,k] is the 2-D vertex of end k of segment g, numbered over all views (a vertex belongs to one view); view[g] is the segment's view.

1. Ends.  Segment g with L = members[g] >= 0: (A, B) = lines3d[L], u = B - A, tau_k = ((estimate[g,k] - A) . u) / (u . u).  End k is at
   line end e = 0 iff tau_k <= end_frac, at e = 1 iff tau_k >= 1 - end_frac, else it carries nothing (a NaN fails both).  q = 2 L + e.
2. Votes.  The set of end ids carried by the segment ends at one 2-D vertex; every pair q < q' of different lines in it is one vote of
   the vertex's view; votes(q, q') = the distinct views that vote.
3. Geometry.  a = u.u, b = u.u', c = u'.u', r = A' - A, d = u.r, e_ = u'.r, w = u x u'.  Refused iff w.w < sin_min^2 (a c).
   den = a c - b b, s = (c d - b e_) / den, t = (b d - a e_) / den, X = A + s u, X' = A' + t u', delta2 = |X - X'|^2.  Accepted iff
   |s - e| <= reach, |t - e'| <= reach and delta2 <= reach^2 min(a, c).
4. Link iff votes >= min_votes and accepted; components by union-find, the root the lowest end id.
5. One vertex per component in ascending root.  One end: a free end (kind 0) at that line end, bit for bit.  More: a junction (kind 1)
   at the solution of M J = y, M = sum (I - u u^T / u.u), y = sum (I - u u^T / u.u) A in ascending end id, by the adjugate; the mean of
   the members' end points when det M is not finite or <= 0.  degree: the ends; votes: the largest vote count of its links; spread:
   the largest distance from J to a member's end point.
6. One edge per line in line order, (vertex of end 0, vertex of end 1); a line whose ends are one vertex is dropped; of several lines
   between the same two vertices the largest support stays, the lowest index on a tie.  esrc = the line.

`margins` says how far the input is from flipping a decision: `ends` |tau - threshold|, and over the pairs with enough votes `angle`
|w.w / (a c) - sin_min^2|, `reach` the least | |s - e| - reach | and | |t - e'| - reach | of the pairs the angle lets through,
`delta` |sqrt(delta2 / min(a, c)) - reach| of those, and `det` the least det M of a junction.
"""
import math

import numpy as np

from tests import triangulate_f64 as T

DEFAULTS = {"end_frac": 0.2, "reach": 0.25, "min_votes": 2, "angle": 10.0}


def sin_min(angle):
    """What the host hands to the kernels for the angle."""
    return math.sin(float(angle) * math.pi / 180.0)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def end_ids(lines3d, members, estimate, end_frac):
    """-> (q int64 [S,2]: the end id each segment end carries, -1 for none; the least distance of a tau from its thresholds)."""
    S, N = members.shape[0], lines3d.shape[0]
    q = np.full((S, 2), -1, dtype=np.int64)
    ok = (members >= 0) & (members < N)
    L = np.where(ok, members, 0)
    if S == 0 or N == 0:
        return q, np.inf
    with np.errstate(all="ignore"):
        A = lines3d[L, 0]
        u = lines3d[L, 1] - A
        uu = dot3(u, u)
        hi = 1.0 - end_frac
        margin = np.inf
        for k in range(2):
            tau = dot3(estimate[:, k] - A, u) / uu
            q[:, k] = np.where(ok & (tau <= end_frac), 2 * L, np.where(ok & (tau >= hi), 2 * L + 1, -1))
            m = np.minimum(np.abs(tau - end_frac), np.abs(tau - hi))[ok & np.isfinite(tau)]
            margin = min(margin, float(m.min()) if m.size else np.inf)
    return q, margin


def pair_geometry(lines3d, q0, q1, smin, reach):
    """Pairs of end ids (arrays, q0 < q1) -> (accepted bool [P], margins of the three tests)."""
    with np.errstate(all="ignore"):
        A, A_ = lines3d[q0 >> 1, 0], lines3d[q1 >> 1, 0]
        u, u_ = lines3d[q0 >> 1, 1] - A, lines3d[q1 >> 1, 1] - A_
        a, b, c = dot3(u, u), dot3(u, u_), dot3(u_, u_)
        r = A_ - A
        d, e_ = dot3(u, r), dot3(u_, r)
        w = np.stack([u[:, 1] * u_[:, 2] - u[:, 2] * u_[:, 1], u[:, 2] * u_[:, 0] - u[:, 0] * u_[:, 2], u[:, 0] * u_[:, 1] - u[:, 1] * u_[:, 0]], axis=1)
        ww = dot3(w, w)
        thr = (smin * smin) * (a * c)
        den = a * c - b * b
        s, t = (c * d - b * e_) / den, (b * d - a * e_) / den
        X, X_ = A + s[:, None] * u, A_ + t[:, None] * u_
        D = X - X_
        delta2 = dot3(D, D)
        ds, dt = np.abs(s - (q0 & 1)), np.abs(t - (q1 & 1))
        least = np.where(a < c, a, c)
        angle_ok = ~(ww < thr)
        reach_ok = (ds <= reach) & (dt <= reach)
        accepted = angle_ok & reach_ok & (delta2 <= (reach * reach) * least)
        fin = lambda x, m: float(x[m & np.isfinite(x)].min()) if (m & np.isfinite(x)).any() else np.inf
        every = np.ones(q0.shape[0], dtype=bool)
        margins = {"angle": fin(np.abs(ww / (a * c) - smin * smin), every),
                   "reach": min(fin(np.abs(ds - reach), angle_ok), fin(np.abs(dt - reach), angle_ok)),
                   "delta": fin(np.abs(np.sqrt(delta2 / least) - reach), angle_ok & reach_ok)}
    return accepted, margins


def solve(lines3d, mem):
    """The junction of the ends `mem` (ascending) -> (J [3], det)."""
    m00 = m01 = m02 = m11 = m12 = m22 = y0 = y1 = y2 = np.float64(0.0)
    sx = sy = sz = np.float64(0.0)
    with np.errstate(all="ignore"):
        for q in mem:
            A, B = lines3d[q >> 1, 0], lines3d[q >> 1, 1]
            ux, uy, uz = B[0] - A[0], B[1] - A[1], B[2] - A[2]
            uu = (ux * ux + uy * uy) + uz * uz
            p00, p01, p02 = 1.0 - (ux * ux) / uu, -((ux * uy) / uu), -((ux * uz) / uu)
            p11, p12, p22 = 1.0 - (uy * uy) / uu, -((uy * uz) / uu), 1.0 - (uz * uz) / uu
            m00, m01, m02, m11, m12, m22 = m00 + p00, m01 + p01, m02 + p02, m11 + p11, m12 + p12, m22 + p22
            y0 = y0 + ((p00 * A[0] + p01 * A[1]) + p02 * A[2])
            y1 = y1 + ((p01 * A[0] + p11 * A[1]) + p12 * A[2])
            y2 = y2 + ((p02 * A[0] + p12 * A[1]) + p22 * A[2])
            E = lines3d[q >> 1, q & 1]
            sx, sy, sz = sx + E[0], sy + E[1], sz + E[2]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        if np.isfinite(det) and det > 0.0:
            return np.array([((c00 * y0 + c01 * y1) + c02 * y2) / det, ((c01 * y0 + c11 * y1) + c12 * y2) / det,
                             ((c02 * y0 + c12 * y1) + c22 * y2) / det]), float(det)
        n = np.float64(len(mem))
        return np.array([sx / n, sy / n, sz / n]), float(det)


def build(lines3d, support, members, estimate, endv, view, V, end_frac=DEFAULTS["end_frac"], reach=DEFAULTS["reach"],
          min_votes=DEFAULTS["min_votes"], angle=DEFAULTS["angle"]):
    """-> dict: junctions3d float64 [J,3], degree, kind, votes int32 [J], spread float64 [J], edges3d int32 [E,2], esrc int32 [E],
    lines3d_wf float64 [E,2,3]; links (the pairs linked), pairs (the votes cast, a view's repeated vote counted once), margins."""
    lines3d = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    support = np.asarray(support, np.float64).reshape(-1)
    members = np.asarray(members, np.int64).reshape(-1)
    estimate = np.asarray(estimate, np.float64).reshape(-1, 2, 3)
    endv = np.asarray(endv, np.int64).reshape(-1, 2)
    view = np.asarray(view, np.int64).reshape(-1)
    N, S = lines3d.shape[0], members.shape[0]
    if not (0.0 < end_frac < 0.5 and 0.0 < reach <= 1.0 and 0.0 < angle <= 90.0 and min_votes >= 1):
        raise ValueError(f"wireframe: end_frac {end_frac} in (0, 0.5), reach {reach} in (0, 1], angle {angle} in (0, 90], min_votes {min_votes} >= 1")
    assert support.shape[0] == N and estimate.shape[0] == S == endv.shape[0] == view.shape[0]
    assert S == 0 or (0 <= view.min() and view.max() < V and endv.min() >= 0)
    smin = sin_min(angle)
    q, m_ends = end_ids(lines3d, members, estimate, float(end_frac))
    # ---- 2. votes: the end ids at every 2-D vertex, then the pairs of different lines, each with the views that cast it
    at, owner = {}, {}
    for g in range(S):
        for k in range(2):
            assert owner.setdefault(int(endv[g, k]), int(view[g])) == view[g], "a 2-D vertex belongs to one view"
            if q[g, k] >= 0:
                at.setdefault(int(endv[g, k]), set()).add(int(q[g, k]))
    voters = {}
    for gv, ids in at.items():
        ids = sorted(ids)
        for i, qa in enumerate(ids):
            for qb in ids[i + 1:]:
                if qa >> 1 != qb >> 1:
                    voters.setdefault((qa, qb), set()).add(owner[gv])
    pairs = sorted(voters)
    enough = [p for p in pairs if len(voters[p]) >= min_votes]
    # ---- 3. and 4. the links and the components
    q0, q1 = (np.array([p[k] for p in enough], dtype=np.int64).reshape(-1) for k in range(2))
    accepted, margins = pair_geometry(lines3d, q0, q1, smin, float(reach))
    margins["ends"] = m_ends
    parent = list(range(2 * N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    links = [p for p, ok in zip(enough, accepted) if ok]
    lvotes = np.zeros(2 * N, dtype=np.int32)
    for qa, qb in links:
        ra, rb = find(qa), find(qb)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
        n = len(voters[(qa, qb)])
        lvotes[qa], lvotes[qb] = max(lvotes[qa], n), max(lvotes[qb], n)
    root = np.array([find(e) for e in range(2 * N)], dtype=np.int64).reshape(-1)
    roots = np.nonzero(root == np.arange(2 * N))[0]
    vidx = np.full(2 * N, -1, dtype=np.int64)
    vidx[roots] = np.arange(roots.shape[0])
    mem = [[] for _ in roots]
    for e in range(2 * N):
        mem[vidx[root[e]]].append(e)
    # ---- 5. the vertices
    J = np.zeros((len(mem), 3))
    degree, kind, votes = (np.zeros(len(mem), dtype=np.int32) for _ in range(3))
    spread = np.zeros(len(mem))
    margins["det"] = np.inf
    for v, ends in enumerate(mem):
        degree[v] = len(ends)
        if len(ends) == 1:
            J[v] = lines3d[ends[0] >> 1, ends[0] & 1]
            continue
        J[v], det = solve(lines3d, ends)
        margins["det"] = min(margins["det"], det if np.isfinite(det) else -np.inf)
        kind[v], votes[v] = 1, max(lvotes[e] for e in ends)
        for e in ends:
            D = J[v] - lines3d[e >> 1, e & 1]
            spread[v] = max(spread[v], math.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]))
    # ---- 6. the edges
    ev = vidx[root].reshape(N, 2)
    best = {}
    for L in range(N):
        if ev[L, 0] == ev[L, 1]:
            continue
        key = (min(ev[L]), max(ev[L]))
        if key not in best or support[L] > support[best[key]]:
            best[key] = L
    esrc = np.array(sorted(best.values()), dtype=np.int32).reshape(-1)
    edges3d = ev[esrc].astype(np.int32).reshape(-1, 2)
    return {"junctions3d": J, "degree": degree, "kind": kind, "votes": votes, "spread": spread, "edges3d": edges3d, "esrc": esrc,
            "lines3d_wf": J[edges3d].reshape(-1, 2, 3), "links": links, "pairs": sum(len(v) for v in voters.values()), "margins": margins}


def graph_arrays(edges, counts=None):
    """The views' edges [e_v,2] (and their vertex counts; default: the largest index + 1) -> (endv int32 [S,2], view int32 [S], NV)."""
    edges = [np.asarray(e, np.int64).reshape(-1, 2) for e in edges]
    if counts is None:
        counts = [int(e.max()) + 1 if e.size else 0 for e in edges]
    voff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    endv = np.concatenate([e + voff[v] for v, e in enumerate(edges)] + [np.zeros((0, 2), np.int64)]).astype(np.int32)
    view = np.concatenate([np.full(e.shape[0], v) for v, e in enumerate(edges)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return endv, view, int(voff[-1])


def wireframe(vertices, edges, Ks, poses, end_frac=DEFAULTS["end_frac"], reach=DEFAULTS["reach"], min_votes=DEFAULTS["min_votes"],
              angle=DEFAULTS["angle"], **thresholds):
    """The views' graphs -> the dict of triangulate_f64.lines, plus build's keys; margins holds both sets."""
    vertices = [np.asarray(v, np.float64).reshape(-1, 2) for v in vertices]
    edges = [np.asarray(e, np.int64).reshape(-1, 2) for e in edges]
    segments = [v[e].reshape(-1, 4) for v, e in zip(vertices, edges)]
    R = T.lines(segments, Ks, poses, **thresholds)
    endv, view, _ = graph_arrays(edges, [v.shape[0] for v in vertices])
    W = build(R["lines3d"], R["support"], R["members"], R["estimate"], endv, view, len(vertices), end_frac, reach, min_votes, angle)
    out = dict(R)
    out.update({k: W[k] for k in W if k != "margins"})
    out["margins"] = dict(R["margins"], **W["margins"])
    return out


def weld(segments):
    """One view's segments [n,4] -> (vertices [m,2], edges [n,2]): end points with equal coordinates are one vertex, numbered in the order
    they first appear."""
    seg = np.asarray(segments, np.float64).reshape(-1, 4)
    index, verts, edges = {}, [], np.zeros((seg.shape[0], 2), dtype=np.int64)
    for i in range(seg.shape[0]):
        for k in range(2):
            p = (float(seg[i, 2 * k]), float(seg[i, 2 * k + 1]))
            if p not in index:
                index[p] = len(verts)
                verts.append(p)
            edges[i, k] = index[p]
    return np.asarray(verts, np.float64).reshape(-1, 2), edges


# ---- inputs with a known answer, as the device's arrays: every view sees every line as one segment whose estimate is the line's own
# end points moved along it by a few per cent, and the 2-D vertices are the nodes' numbers (no camera is needed for the rule) ---------------
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])          # a rotation with exact entries


def _observe(world, node_of_end, n_nodes, V, shrink, seed):
    """world [N,2,3] between nodes; node_of_end int [N,2] -> the arrays of build(): lines shrunk by `shrink` of their length at both
    ends, V views each seeing every line once with its ends jittered by up to 3 % along it."""
    rng = np.random.default_rng(seed)
    N = world.shape[0]
    d = world[:, 1] - world[:, 0]
    lines3d = np.stack([world[:, 0] + shrink * d, world[:, 1] - shrink * d], axis=1)
    u = lines3d[:, 1] - lines3d[:, 0]
    est, endv, view, members = [], [], [], []
    for v in range(V):
        j = rng.uniform(-0.03, 0.03, (N, 2))
        est.append(np.stack([lines3d[:, 0] + j[:, :1] * u, lines3d[:, 1] + j[:, 1:] * u], axis=1))
        endv.append(node_of_end + v * n_nodes)
        view.append(np.full(N, v))
        members.append(np.arange(N))
    cat = lambda x, *shape: np.concatenate(x).reshape(-1, *shape) if x else np.zeros((0, *shape))
    return {"lines3d": lines3d, "support": 1.0 + 0.001 * (np.arange(N) % 13), "members": cat(members).astype(np.int32),
            "estimate": cat(est, 2, 3), "endv": cat(endv, 2).astype(np.int32), "view": cat(view).astype(np.int32), "V": V, "NV": V * n_nodes}


def lattice(rods, V=4, n=None, shrink=0.05, seed=5):
    """The first `rods` rods of a rotated cubic lattice of n^3 nodes (default: the smallest that holds them), rods of a node's +x, +y, +z
    neighbours in node order -> (arrays of build(), nodes [n^3,3], rod ends int [rods,2])."""
    if n is None:
        n = 2
        while 3 * n * n * (n - 1) < rods:
            n += 1
    idx = lambda i, j, k: (i * n + j) * n + k
    nodes = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)], dtype=np.float64) * 0.37 @ ROT.T + np.array([0.11, -0.23, 0.05])
    ends = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                for di, dj, dk in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    if i + di < n and j + dj < n and k + dk < n:
                        ends.append((idx(i, j, k), idx(i + di, j + dj, k + dk)))
    ends = np.array(ends[:rods], dtype=np.int64).reshape(-1, 2)
    assert ends.shape[0] == rods
    return _observe(nodes[ends], ends, n ** 3, V, shrink, seed), nodes, ends


def fan(m, V=3, seed=9):
    """m lines that leave one point in seeded directions of the upper half space, lengths 1 to 1.5 -> the arrays of build(): one 2-D
    vertex a view holds m ends, one component holds m ends."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((m, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.05
    d = d / np.sqrt(dot3(d, d))[:, None] * rng.uniform(1.0, 1.5, (m, 1))
    centre = np.array([0.21, -0.13, 0.4])
    world = np.stack([np.repeat(centre[None], m, axis=0), centre + d], axis=1)
    ends = np.stack([np.zeros(m, np.int64), 1 + np.arange(m)], axis=1)
    return _observe(world, ends, m + 1, V, 0.04, seed)


def written(lines, segs, V, support=None):
    """A case written out: lines [N,2,3]; segs: (view, line, (2-D vertex of end 0, of end 1), (tau of end 0, of end 1)) per segment, the
    2-D vertices numbered over all views; an estimate is A + tau (B - A) -> the arrays of build()."""
    lines3d = np.asarray(lines, np.float64).reshape(-1, 2, 3)
    N = lines3d.shape[0]
    est = [[lines3d[L, 0] + t * (lines3d[L, 1] - lines3d[L, 0]) for t in taus] for _, L, _, taus in segs]
    return {"lines3d": lines3d, "support": np.asarray(support, np.float64) if support is not None else 1.0 + 0.5 * np.arange(N),
            "members": np.array([s[1] for s in segs], np.int32).reshape(-1), "estimate": np.asarray(est, np.float64).reshape(-1, 2, 3),
            "endv": np.array([s[2] for s in segs], np.int32).reshape(-1, 2), "view": np.array([s[0] for s in segs], np.int32).reshape(-1), "V": V,
            "NV": 1 + max([max(s[2]) for s in segs], default=-1)}


CORNER = [[[0.05, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.05, 0.001], [0.0, 1.0, 0.001]]]          # two lines that pass 0.001 apart at the origin


def twice():
    """Three views of CORNER.  View 0 votes for (end 0 of line 0, end 0 of line 1) three times: two segments of line 0 and one of line 1
    end in its vertex 0, and a second pair of segments meets in its vertex 5.  View 1 votes once, view 2 not at all: 2 votes."""
    return written(CORNER, [(0, 0, (0, 1), (0.0, 1.0)), (0, 0, (0, 2), (0.01, 0.7)), (0, 1, (0, 3), (0.0, 1.0)), (0, 0, (5, 6), (0.02, 0.9)),
                            (0, 1, (5, 7), (0.03, 0.95)), (1, 0, (8, 9), (0.0, 1.0)), (1, 1, (8, 10), (0.0, 1.0)), (2, 0, (11, 12), (0.0, 1.0)),
                            (2, 1, (13, 14), (0.0, 1.0))], 3)


def cases():
    """name -> (arrays of build(), its thresholds): what tests/test_wireframe3d_gpu.py runs on the device and tests/test_wireframe3d_math.py
    asserts the margins of.  Rod and line counts straddle the wavefront (63, 64, 65) and the workgroup (255, 256, 257)."""
    out = {f"lattice_{n}": (lattice(n)[0], {}) for n in (63, 64, 65, 255, 256, 257)}
    out["two_views"] = (lattice(54, V=2)[0], {"min_votes": 2})
    out["twice_2"] = (twice(), {"min_votes": 2})
    out["twice_3"] = (twice(), {"min_votes": 3})
    out["fan_65"] = (fan(65), {})
    out["fan_257"] = (fan(257), {})
    out["thresholds"] = (lattice(100, V=3, shrink=0.12)[0], {"end_frac": 0.3, "reach": 0.4, "min_votes": 3, "angle": 25.0})
    none = lattice(20)[0]
    out["no_members"] = (dict(none, members=np.full_like(none["members"], -1)), {})
    out["no_segments"] = (dict(none, members=np.zeros(0, np.int32), estimate=np.zeros((0, 2, 3)), endv=np.zeros((0, 2), np.int32),
                               view=np.zeros(0, np.int32), V=0, NV=0), {})
    out["no_lines"] = (dict(none, lines3d=np.zeros((0, 2, 3)), support=np.zeros(0), members=np.full_like(none["members"], -1)), {})
    out["nothing"] = (written(np.zeros((0, 2, 3)), [], 0), {})
    return out


def arrays_of(a):
    """The positional arguments of build() from a dict of arrays."""
    return a["lines3d"], a["support"], a["members"], a["estimate"], a["endv"], a["view"], a["V"]
