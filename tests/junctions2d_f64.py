"""The definition of the 2-D wireframe builder (neat_amd/csrc/kernels_wireframe2d.hpp implements it, detect.junctions calls it):
the 2-D segments of many views -> per view a graph whose segments share their junctions.  Plain numpy float64, every sum written out:
each product, sum, quotient and square root below is one IEEE operation in the order it stands in, three-term sums are (a + b) + c,
there is no transcendental function, and numpy contracts nothing into a fused multiply-add.  The device forms the same operations in
the same order without contraction, so its vertices are these bits and its decisions are these decisions.

    build(segments [S,4], segoff int32 [V+1], weight [S], gap=4.0, frac=0.4, angle=10.0, t_junctions=True) -> dict

Per segment i of a view (indices are the view's own): p, q its ends, d = q - p, L = sqrt(d.d), u = d / L, g = min(gap, frac L).  A segment
whose L is zero or not finite takes part in nothing; its ends stay free.  End k of segment i is endpoint 2 i + k, at e = p (k = 0) or q
(k = 1), with the outward direction o = -u or +u.

1. The pair (i, j), i < j, the lower index always the first operand: c = u_i x u_j, refused unless |c| >= sin_min; w = p_j - p_i,
   t = (w x u_j) / c, X = p_i + t u_i.  End e of i and end f of j meet iff -g_i <= (X - e).o_e <= g_i and -g_j <= (X - f).o_f <= g_j.
2. The components of the endpoints under "meet"; a component's root is its smallest endpoint.
3. A component of m >= 2 ends is a junction (kind 1) at the least-squares point of its members' supporting lines n.x = c, n = (-u.y, u.x),
   c = n.p: the five sums a11, a12, a22, b1, b2 from 0 in ascending endpoint order, det = a11 a22 - a12 a12,
   X = ((a22 b1 - a12 b2) / det, (a11 b2 - a12 b1) / det).  degree = m, score = the largest member weight, spread = the largest |X - e|.
4. A lone end e of i, with t_junctions: among the j != i that pass |c| with |a| <= g_i, a = (X - e).o_e, and g_j < (X - p_j).u_j < L_j - g_j
   (X of the pair, lower index first), the smallest |a|, the lowest j on a tie: the vertex moves to X, kind 2, t_edge = j, spread = |X - e|.
   Every other lone end stays where it is, kind 0, t_edge = -1.  A lone end has degree 1 and its segment's weight as score.
5. The vertices of a view in ascending root endpoint; ends [S,2] = the vertex of each end (the view's own numbering).  A segment is an
   edge unless both ends are one vertex, or another segment of the view joins the same unordered pair of vertices with a larger weight
   (the lower index on equal weights).  The edges in segment order: edges [E,2], eweight [E], esrc [E] = the segment in its view.

`margin` in the result is the smallest amount by which any decision of steps 1 and 4 could be flipped: for a conjunction that holds,
the least slack of its terms; for one that fails, the largest shortfall among the terms that fail (a NaN term never flips).
"""
import math

import numpy as np

DEFAULTS = {"gap": 4.0, "frac": 0.4, "angle": 10.0, "t_junctions": True}
DBL_MAX = np.finfo(np.float64).max


def sin_min(angle):
    """What the host hands to the kernels for --angle."""
    return math.sin(float(angle) * math.pi / 180.0)


def _slack(terms):
    """terms: arrays of (value - threshold), >= 0 where the term holds -> the amount that flips the conjunction, per element."""
    t = np.stack([np.where(np.isnan(x), -np.inf, x) for x in terms])
    return np.abs(t.min(axis=0))


def _view(seg, weight, gap, frac, smin, t_junctions):
    """One view -> (dict of the view's arrays, margin)."""
    n = seg.shape[0]
    px, py, qx, qy = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    with np.errstate(all="ignore"):
        dx, dy = qx - px, qy - py
        L = np.sqrt(dx * dx + dy * dy)
        ok = (L > 0.0) & (L <= DBL_MAX)
        ux, uy = dx / L, dy / L
        g = np.minimum(gap, frac * L)
        ii, jj = np.arange(n)[:, None], np.arange(n)[None, :]
        # ---- the pair's intersection, lower index first: [i, j] is valid for i < j
        c = ux[:, None] * uy[None, :] - uy[:, None] * ux[None, :]
        wx, wy = px[None, :] - px[:, None], py[None, :] - py[:, None]
        t = (wx * uy[None, :] - wy * ux[None, :]) / c
        Xl, Yl = px[:, None] + t * ux[:, None], py[:, None] + t * uy[:, None]
        upper = ii < jj
        okp = ok[:, None] & ok[None, :]
        cterm = np.abs(c) - smin                      # >= 0: the angle test holds (a NaN fails)
        # ---- 1. meet
        margin = np.inf
        ex, ey = np.stack([px, qx]), np.stack([py, qy])                   # [k, n]
        ox, oy = np.stack([-ux, ux]), np.stack([-uy, uy])
        pairs = []
        for ki in range(2):
            a = (Xl - ex[ki][:, None]) * ox[ki][:, None] + (Yl - ey[ki][:, None]) * oy[ki][:, None]
            for kj in range(2):
                b = (Xl - ex[kj][None, :]) * ox[kj][None, :] + (Yl - ey[kj][None, :]) * oy[kj][None, :]
                terms = [cterm, a + g[:, None], g[:, None] - a, b + g[None, :], g[None, :] - b]
                meet = upper & okp & (np.abs(c) >= smin) & (a >= -g[:, None]) & (a <= g[:, None]) & (b >= -g[None, :]) & (b <= g[None, :])
                live = upper & okp
                if live.any():
                    margin = min(margin, float(_slack(terms)[live].min()))
                i_, j_ = np.nonzero(meet)
                pairs += [(2 * int(i) + ki, 2 * int(j) + kj) for i, j in zip(i_, j_)]
    # ---- 2. components, the root the smallest member
    parent = list(range(2 * n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a_, b_ in pairs:
        ra, rb = find(a_), find(b_)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(e) for e in range(2 * n)], dtype=np.int64).reshape(-1)
    roots = np.nonzero(root == np.arange(2 * n))[0]
    nv = roots.shape[0]
    vidx = np.full(2 * n, -1, dtype=np.int64)
    vidx[roots] = np.arange(nv)
    members = [[] for _ in range(nv)]
    for e in range(2 * n):
        members[vidx[root[e]]].append(e)
    vertices, degree, kind = np.zeros((nv, 2)), np.zeros(nv, np.int32), np.zeros(nv, np.int32)
    score, spread, t_edge = np.zeros(nv), np.zeros(nv), np.full(nv, -1, np.int32)
    exf, eyf = seg[:, [0, 2]].reshape(-1), seg[:, [1, 3]].reshape(-1)       # by endpoint
    with np.errstate(all="ignore"):
        # ---- 4. the T candidates of every end: [k][i, j]
        Xf, Yf = np.where(upper, Xl, Xl.T), np.where(upper, Yl, Yl.T)
        cf = np.where(upper, c, c.T)
        s = (Xf - px[None, :]) * ux[None, :] + (Yf - py[None, :]) * uy[None, :]
        tee = []
        for k in range(2):
            a = (Xf - ex[k][:, None]) * ox[k][:, None] + (Yf - ey[k][:, None]) * oy[k][:, None]
            live = okp & (ii != jj)
            cand = live & (np.abs(cf) >= smin) & (np.abs(a) <= g[:, None]) & (s > g[None, :]) & (s < (L - g)[None, :])
            slack = _slack([np.abs(cf) - smin, g[:, None] - np.abs(a), s - g[None, :], (L - g)[None, :] - s])
            tee.append((cand, np.abs(a), np.where(live, slack, np.inf)))
        # ---- 3. and 4. the vertices
        for v, mem in enumerate(members):
            if len(mem) >= 2:
                a11 = a12 = a22 = b1 = b2 = 0.0
                for e in mem:
                    i = e >> 1
                    nx, ny = -uy[i], ux[i]
                    cc = nx * px[i] + ny * py[i]
                    a11, a12, a22 = a11 + nx * nx, a12 + nx * ny, a22 + ny * ny
                    b1, b2 = b1 + nx * cc, b2 + ny * cc
                det = a11 * a22 - a12 * a12
                X, Y = (a22 * b1 - a12 * b2) / det, (a11 * b2 - a12 * b1) / det
                vertices[v] = X, Y
                degree[v], kind[v] = len(mem), 1
                score[v] = max(weight[e >> 1] for e in mem)
                spread[v] = max(math.sqrt((X - exf[e]) * (X - exf[e]) + (Y - eyf[e]) * (Y - eyf[e])) for e in mem)
                continue
            e = mem[0]
            i, k = e >> 1, e & 1
            vertices[v] = exf[e], eyf[e]
            degree[v], score[v] = 1, weight[i]
            if not (t_junctions and ok[i]):
                continue
            cand, absa, slack = tee[k]
            if n > 1:
                margin = min(margin, float(slack[i].min()))
            best = np.where(cand[i], absa[i], np.inf)
            j = int(best.argmin()) if n else 0                      # the first of the smallest: the lowest j on a tie
            if n and best[j] < np.inf:
                X, Y = Xf[i, j], Yf[i, j]
                vertices[v] = X, Y
                kind[v], t_edge[v] = 2, j
                spread[v] = math.sqrt((X - exf[e]) * (X - exf[e]) + (Y - eyf[e]) * (Y - eyf[e]))
    # ---- 5. ends and edges
    ends = vidx[root].reshape(n, 2).astype(np.int32)
    lo, hi = ends.min(axis=1), ends.max(axis=1)
    same = (lo[:, None] == lo[None, :]) & (hi[:, None] == hi[None, :]) & (ii != jj)
    beats = same & ((weight[None, :] > weight[:, None]) | ((weight[None, :] == weight[:, None]) & (jj < ii)))      # [i, j]: j beats i
    keep = (lo != hi) & ~beats.any(axis=1)
    esrc = np.nonzero(keep)[0].astype(np.int32)
    return {"vertices": vertices, "degree": degree, "kind": kind, "score": score, "spread": spread, "t_edge": t_edge, "ends": ends,
            "edges": ends[esrc], "eweight": weight[esrc], "esrc": esrc}, margin


def build(segments, segoff, weight, gap=DEFAULTS["gap"], frac=DEFAULTS["frac"], angle=DEFAULTS["angle"], t_junctions=DEFAULTS["t_junctions"]):
    """-> dict: vertices float64 [N,2], degree, kind int32 [N], score, spread float64 [N], t_edge int32 [N], voff int32 [V+1];
    ends int32 [S,2]; edges int32 [E,2], eweight float64 [E], esrc int32 [E], eoff int32 [V+1]; margin.  All views concatenated, every
    index the view's own."""
    segments = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    weight = np.asarray(weight, dtype=np.float64).reshape(-1)
    segoff = np.asarray(segoff, dtype=np.int64).reshape(-1)
    if not (gap > 0.0 and 0.0 < frac < 0.5 and 0.0 < angle <= 90.0):
        raise ValueError(f"junctions: gap {gap} > 0, frac {frac} in (0, 0.5), angle {angle} in (0, 90]")
    assert segoff[0] == 0 and segoff[-1] == segments.shape[0] == weight.shape[0] and (np.diff(segoff) >= 0).all()
    smin = sin_min(angle)
    views, margin = [], np.inf
    for v in range(segoff.shape[0] - 1):
        r, m = _view(segments[segoff[v]:segoff[v + 1]], weight[segoff[v]:segoff[v + 1]], float(gap), float(frac), smin, bool(t_junctions))
        views.append(r)
        margin = min(margin, m)
    empty = {"vertices": np.zeros((0, 2)), "degree": np.zeros(0, np.int32), "kind": np.zeros(0, np.int32), "score": np.zeros(0),
             "spread": np.zeros(0), "t_edge": np.zeros(0, np.int32), "ends": np.zeros((0, 2), np.int32), "edges": np.zeros((0, 2), np.int32),
             "eweight": np.zeros(0), "esrc": np.zeros(0, np.int32)}
    out = {k: np.concatenate([r[k] for r in views] + [empty[k]]) for k in empty}
    out["voff"] = np.concatenate([[0], np.cumsum([r["vertices"].shape[0] for r in views])]).astype(np.int32)
    out["eoff"] = np.concatenate([[0], np.cumsum([r["edges"].shape[0] for r in views])]).astype(np.int32)
    out["margin"] = margin
    return out


def view_of(res, v):
    """The arrays of view v of a build() result (or of detect.junctions' arrays on the host)."""
    a, b, c, d = res["voff"][v], res["voff"][v + 1], res["eoff"][v], res["eoff"][v + 1]
    out = {k: res[k][a:b] for k in ("vertices", "degree", "kind", "score", "spread", "t_edge")}
    out.update({k: res[k][c:d] for k in ("edges", "eweight", "esrc")})
    return out


def members(res, v, segoff):
    """The junctions (degree >= 2) of view v as sets of the view's endpoints 2 i + k -> {frozenset: vertex}."""
    ends = res["ends"][segoff[v]:segoff[v + 1]].reshape(-1)
    out = {}
    for q in np.nonzero(res["degree"][res["voff"][v]:res["voff"][v + 1]] >= 2)[0]:
        out[frozenset(np.nonzero(ends == q)[0].tolist())] = int(q)
    return out


# ---- the smallest inputs that can go wrong (tests/test_junctions2d_math.py states their answers, tests/test_junctions2d_gpu.py runs them) ------
TILE = 256          # the pair kernels' tile of segments


def filler(n, y0=1000.0):
    """n horizontal segments far from everything and parallel to each other: they take part in nothing."""
    return [[10.0, y0 + 3.0 * i, 30.0, y0 + 3.0 * i] for i in range(n)]


def star(m, centre=(200.0, 200.0)):
    """m segments that leave one point in 24 directions of 15 degrees' spacing (opposite and repeated rays are parallel and reach the
    junction through the others), each starting 1 px from it: one junction of m ends."""
    out = []
    for i in range(m):
        th = math.radians(15.0 * (i % 24))
        d = np.array([math.cos(th), math.sin(th)])
        c = np.asarray(centre)
        out.append(np.concatenate([c + 1.0 * d, c + (12.0 + i // 24) * d]))
    return out


def cases():
    """name -> (segments [S,4], segoff [V+1], weight [S]).  Everything a view needs is said in tests/test_junctions2d_math.py."""
    corner = [[10.0, 50.0, 49.0, 50.0], [50.0, 51.0, 50.0, 90.0]]                      # an L: ends 1 px short of (50, 50)
    out = {}

    def add(name, views, weight=None):
        seg = np.array([s for v in views for s in v], dtype=np.float64).reshape(-1, 4)
        off = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int32)
        out[name] = (seg, off, np.asarray(weight, np.float64) if weight is not None else 0.5 + 0.001 * (np.arange(seg.shape[0]) % 7))

    add("no_views", [])
    add("tiny_views", [[], [corner[0]], corner])
    add("degenerate", [[corner[0], [5.0, 5.0, 5.0, 5.0], [np.nan, 1.0, 2.0, 3.0], corner[1], [1.0, 2.0, np.inf, 2.0], [49.5, 50.0, 49.5, 50.0]]])
    add("parallel", [[[10.0, 20.0, 40.0, 20.0], [41.0, 20.0, 70.0, 20.0], [10.0, 30.0, 40.0, 30.0], [41.0, 30.5, 70.0, 30.5]]])
    for n in (TILE - 1, TILE, TILE + 1):
        # a corner between the first and the last segment, a T from the second onto the last but one
        bar, stem = [100.0, 200.0, 160.0, 200.0], [130.0, 150.0, 130.0, 198.0]
        add(f"tile_{n}", [[corner[0], stem] + filler(n - 4) + [bar, corner[1]]])
    # a chain over three tiles: a and c are 6 degrees apart and never meet each other, both meet b
    a = [50.0 - 40.0 * math.cos(math.radians(3.0)), 50.0 - 40.0 * math.sin(math.radians(3.0)), 50.0 - math.cos(math.radians(3.0)), 50.0 - math.sin(math.radians(3.0))]
    c = [50.0 - 40.0 * math.cos(math.radians(3.0)), 50.0 + 40.0 * math.sin(math.radians(3.0)), 50.0 - math.cos(math.radians(3.0)), 50.0 + math.sin(math.radians(3.0))]
    add("chain", [[a] + filler(TILE + 10) + [corner[1]] + filler(TILE + 10, 3000.0) + [c]])
    for m in (63, 64, 65):
        add(f"star_{m}", [star(m)])
    add("ragged", [lattice(2, 1)[0].tolist(), lattice(1, 1)[0].tolist(), [], lattice(3, 2)[0].tolist(), corner])
    # a square whose top side is there twice, with equal weights and then with the second the heavier
    square = [[11.0, 10.0, 39.0, 10.0], [11.0, 10.2, 39.0, 10.1], [40.0, 11.0, 40.0, 39.0], [39.0, 40.0, 11.0, 40.0], [10.0, 39.0, 10.0, 11.0]]
    add("duplicate_equal", [square], [0.7, 0.7, 0.6, 0.6, 0.6])
    add("duplicate_heavier", [square], [0.7, 0.8, 0.6, 0.6, 0.6])
    # a short segment between the two arms of a corner: both its ends reach the corner's junction through the arms
    add("collapsed", [[[-20.0, 0.0, -1.5, 0.0], [0.0, -20.0, 0.0, -1.5], [-1.5, -0.3, -0.3, -1.5]]])
    # a stem that stops before three bars: 3 px before the first, 2 px before the second and the third, which are one line
    add("tee_two_bars", [[[0.0, 51.0, 100.0, 51.0], [0.0, 50.0, 100.0, 50.0], [5.0, 50.0, 95.0, 50.0], [50.0, 20.0, 50.0, 48.0]]])
    return out


# ---- inputs with a known answer --------------------------------------------------------------------------------------------------------------
def lattice(m, n, cell=10.0, theta=0.3, shrink=1.0, origin=(20.0, 15.0)):
    """m x n cells of `cell` px rotated by theta, every unit segment shrunk by `shrink` at both ends -> (segments [m (n+1) + n (m+1), 4],
    nodes [(m+1)(n+1), 2])."""
    ct, st = math.cos(theta), math.sin(theta)
    node = lambda i, j: np.array([origin[0] + cell * (i * ct - j * st), origin[1] + cell * (i * st + j * ct)])
    segs = []
    for j in range(n + 1):
        for i in range(m):
            segs.append((node(i, j), node(i + 1, j)))
    for i in range(m + 1):
        for j in range(n):
            segs.append((node(i, j), node(i, j + 1)))
    out = []
    for a, b in segs:
        d = (b - a) / np.linalg.norm(b - a)
        out.append(np.concatenate([a + shrink * d, b - shrink * d]))
    nodes = np.array([node(i, j) for j in range(n + 1) for i in range(m + 1)])
    return np.array(out), nodes
