"""The crease rule of DESIGN 3n restated in plain float64: dicts, loops and np.unique, nothing shared with neat_amd/creases.py or its
kernels.  Python floats are IEEE float64 and `a * b + c` is two roundings here, which is what the device does with every product
rounded on its own.  Also the solids of the crease tests."""
import math

import numpy as np

from neat_amd import scenegen


# ------------------------------------------------------------------ the rule
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _cross2(a, b):
    c = _cross(a, b)
    return _dot(c, c)


def constants(verts, angle, turn, deviation):
    """What the host hands over: cos(angle), sin^2(turn), the deviation as a length."""
    c = math.cos(math.radians(float(angle)))
    s2 = math.sin(math.radians(float(turn))) ** 2
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if verts.shape[0] == 0:
        return c, s2, 0.0
    d = verts.max(axis=0) - verts.min(axis=0)
    return c, s2, float(deviation) * math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))


def empty(status=0):
    return {"status": status, "junctions": np.zeros((0, 3)), "lines": np.zeros((0, 2), np.int32), "kind": np.zeros(0, np.uint8),
            "curved": np.zeros(0, bool), "vertex": np.zeros(0, np.int32),
            "stats": {"status": status, "welded": 0, "dropped_faces": 0, "edges": 0, "creases": 0, "boundary": 0, "non_manifold": 0, "chains": 0}}


def lines(verts, faces, angle=30.0, turn=1.0, deviation=1e-6, boundary=True, drop_curved=False, min_len=0.0):
    """-> dict(status, junctions float64 [J,3], lines int32 [L,2], kind uint8 [L], curved bool [L], vertex int32 [J], stats)."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv, nf = verts.shape[0], faces.shape[0]
    if nf and (faces.min() < 0 or faces.max() >= nv):
        return empty(1)
    if not np.isfinite(verts).all():
        return empty(2)
    c, s2, dev = constants(verts, angle, turn, deviation)
    # 1. weld: equal coordinates (-0.0 as 0.0), the lowest index stands for the group
    first, weld = {}, []
    for i in range(nv):
        key = tuple(float(x) + 0.0 for x in verts[i])            # -0.0 + 0.0 = 0.0
        weld.append(first.setdefault(key, i))
    P = [tuple(float(x) for x in v) for v in verts]
    # 2. faces, 3. half-edges in (face, corner) order
    normal, dropped, halves = {}, 0, {}
    for f in range(nf):
        w = [weld[int(i)] for i in faces[f]]
        n = _cross(_sub(P[w[1]], P[w[0]]), _sub(P[w[2]], P[w[0]]))
        q = _dot(n, n)
        if w[0] == w[1] or w[1] == w[2] or w[2] == w[0] or q == 0.0:
            dropped += 1
            continue
        normal[f] = (n, q)
        for k in range(3):
            a, b = w[k], w[(k + 1) % 3]
            halves.setdefault((min(a, b), max(a, b)), []).append((f, a == min(a, b)))
    # 4. kinds; the feature edges in key order
    edges = []
    for (lo, hi) in sorted(halves):
        h = halves[(lo, hi)]
        if len(h) == 1:
            if boundary:
                edges.append((lo, hi, 1))
        elif len(h) >= 3:
            edges.append((lo, hi, 2))
        else:
            (f1, fwd1), (f2, fwd2) = h
            (n1, q1), (n2, q2) = normal[f1], normal[f2]
            d = _dot(n1, n2)
            if fwd1 == fwd2:
                d = -d
            s = (c * c) * (q1 * q2)
            if (d < 0.0 or d * d < s) if c >= 0.0 else (d < 0.0 and d * d > s):
                edges.append((lo, hi, 0))
    E = len(edges)
    stats = {"status": 0, "welded": len(set(weld)), "dropped_faces": dropped, "edges": E, "creases": sum(k == 0 for _, _, k in edges),
             "boundary": sum(k == 1 for _, _, k in edges), "non_manifold": sum(k == 2 for _, _, k in edges), "chains": 0}
    # 5. pass-through vertices
    at = {}
    for e, (lo, hi, _) in enumerate(edges):
        at.setdefault(lo, []).append(e)
        at.setdefault(hi, []).append(e)
    end = {}
    parent = list(range(E))

    def find(e):
        while parent[e] != e:
            e = parent[e]
        return e
    for v in sorted(at):
        inc = at[v]
        through = False
        if len(inc) == 2 and edges[inc[0]][2] == edges[inc[1]][2]:
            far = [edges[e][0] if edges[e][1] == v else edges[e][1] for e in inc]
            u, w = _sub(P[far[0]], P[v]), _sub(P[far[1]], P[v])
            through = _dot(u, w) < 0.0 and _cross2(u, w) <= s2 * (_dot(u, u) * _dot(w, w))
        end[v] = not through
        if through:                                              # 6. union: the smaller root stays
            a, b = find(inc[0]), find(inc[1])
            parent[max(a, b)] = min(a, b)
    chains = {}
    for e in range(E):
        chains.setdefault(find(e), []).append(e)
    stats["chains"] = len(chains)
    out = []                                                     # (a, b, kind, curved)
    for label in sorted(chains):
        members = chains[label]
        kind = edges[members[0]][2]
        ends = [v for e in members for v in edges[e][:2] if end[v]]
        straight = len(ends) == 2 and ends[0] != ends[1]
        if straight:
            a, b = min(ends), max(ends)
            d = _sub(P[b], P[a])
            bound = (dev * dev) * _dot(d, d)
            straight = all(_cross2(_sub(P[v], P[a]), d) <= bound for e in members for v in edges[e][:2])
        if straight:
            out.append((a, b, kind, 0))
        else:
            out += [(edges[e][0], edges[e][1], kind, 1) for e in members]
    out.sort()                                                   # 7. ascending (a, b), kind, curved
    # the filters, applied afterwards
    if drop_curved:
        out = [l for l in out if not l[3]]
    if min_len > 0.0:
        m2 = float(min_len) * float(min_len)
        out = [l for l in out if not _dot(_sub(P[l[1]], P[l[0]]), _sub(P[l[1]], P[l[0]])) < m2]
    vertex = np.unique(np.asarray([v for l in out for v in l[:2]], dtype=np.int32))
    index = {int(v): j for j, v in enumerate(vertex)}
    return {"status": 0, "junctions": verts[vertex].reshape(-1, 3), "lines": np.asarray([(index[a], index[b]) for a, b, _, _ in out], np.int32).reshape(-1, 2),
            "kind": np.asarray([l[2] for l in out], np.uint8), "curved": np.asarray([l[3] for l in out], bool), "vertex": vertex.astype(np.int32),
            "stats": stats}


# ------------------------------------------------------------------ the solids
def roof(n, bend=0.0):
    """A ridge of n steps along x: vertices (i, -1, 0), (i, 0, 1 + bend i^2), (i, 1, 0), two triangles per step on each side."""
    verts = [(float(i), y, z) for i in range(n + 1) for y, z in ((-1.0, 0.0), (0.0, 1.0 + bend * i * i), (1.0, 0.0))]
    faces = []
    for i in range(n):
        a0, r0, b0, a1, r1, b1 = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3, 3 * i + 4, 3 * i + 5
        faces += [(a0, a1, r1), (a0, r1, r0), (r0, r1, b1), (r0, b1, b0)]
    return np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int32)


def ngon_prism(n, half):
    """A prism over the regular n-gon of radius 0.5 (half: over its upper half, closed by the diameter), caps as fans about vertex 0."""
    m = n // 2 + 1 if half else n
    outline = [(0.5 * math.cos(2.0 * math.pi * i / n), 0.5 * math.sin(2.0 * math.pi * i / n)) for i in range(m)]
    verts, faces, _, _ = scenegen._prism(outline, -0.25, 0.25, [(0, i, i + 1) for i in range(1, m - 1)])
    return verts, faces


def open_box():
    """The box without the two faces of its top cap."""
    verts, faces, _, _ = scenegen.shapes["box"]
    return verts.copy(), faces[[i for i in range(len(faces)) if i not in (2, 3)]].copy()


def fin():
    """The box and one more triangle on its edge (0, 1)."""
    verts, faces, _, _ = scenegen.shapes["box"]
    return np.concatenate([verts, [[0.0, -0.875, -0.75]]]), np.concatenate([faces, [[0, 1, len(verts)]]]).astype(np.int32)


def soup(verts, faces):
    """Every face with three vertices of its own."""
    faces = np.asarray(faces).reshape(-1, 3)
    return np.asarray(verts)[faces.reshape(-1)].copy(), np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)


def reverse_third(faces):
    faces = np.asarray(faces).copy()
    faces[::3] = faces[::3, ::-1]
    return faces


def rotated(verts, seed=0, scale=0.37, shift=0.1):
    """-> (verts', the map applied to any points): a QR of seeded normals, a scale and a shift."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))

    def move(x):
        return (np.asarray(x, dtype=np.float64) @ q.T) * scale + shift
    return move(verts), move


def coordinate_pairs(junctions, lines):
    """The lines as a set of unordered pairs of coordinate triples."""
    J = [tuple(float(x) + 0.0 for x in p) for p in np.asarray(junctions).reshape(-1, 3)]
    return {frozenset((J[int(a)], J[int(b)])) for a, b in np.asarray(lines).reshape(-1, 2)}
