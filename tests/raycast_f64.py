"""Ray casting against a triangle mesh, restated in float64 (neat_amd/raycast.py, csrc/kernels_raycast.hpp): the scenes of
the tests, the rule of intersection by brute force over all triangles (cast_all), a plain-Python model of the implicit tree (Tree: sort,
pad, refit, walk, with the nodes and triangles a ray costs) and the judge of rays too close to a tie to compare.

The rule (Woop, Benthin, Wald 2013).  Ray (o, d) float32 widened exactly, triangle (v0, v1, v2) float64; every operation below is one
float64 operation, every product rounded on its own (numpy and Python floats never fuse a product into an addition):
    kz = argmax |d| (lowest on a tie), kx = kz + 1, ky = kx + 1 (mod 3), kx <-> ky when d[kz] < 0
    Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
    A = v0 - o;  Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz];  B, C likewise from v1, v2
    U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax
    accepted iff (U, V, W all >= 0 or all <= 0) and det = (U + V) + W != 0 and t_min <= t < t_max,
    t = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det;  uv = (V / det, W / det)
    a triangle with a non-finite vertex or (v1 - v0) x (v2 - v0) == 0 is never hit
    closest hit: the smallest t, ties to the lowest face index.
"""
import math

import numpy as np

INF = float("inf")


# ------------------------------------------------------------------------------------------------------------------------ scenes
def icosphere(level):
    """-> (verts float64 [nv,3] on the unit sphere, faces int32 [20 * 4^level, 3], outward winding)."""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    verts = [np.asarray(x, np.float64) / math.sqrt(1.0 + p * p) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[key[0]] + verts[key[1]]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.stack(verts), np.asarray(faces, np.int32)


def box(lo=(-0.5, -0.4, -0.3), hi=(0.5, 0.4, 0.3)):
    """An axis-aligned box: 8 corners (corner i: bit 0 = x, bit 1 = y, bit 2 = z), 12 triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts = np.stack([np.where([(i >> a) & 1 for a in range(3)], hi, lo) for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return verts, np.asarray(faces, np.int32)


BOX_EDGES = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]


def strips(n=64):
    """Two parallel unit squares (z = 0 and z = 1), each cut into n strips of two sliver triangles: the CAD case.  4 n triangles."""
    verts, faces = [], []
    for z in (0.0, 1.0):
        base = len(verts)
        for i in range(n + 1):
            verts += [(i / n, 0.0, z), (i / n, 1.0, z)]
        for i in range(n):
            a, b, c, d = base + 2 * i, base + 2 * i + 1, base + 2 * i + 2, base + 2 * i + 3
            faces += [(a, c, d), (a, d, b)]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int32)


def fan(seed, n, centre=(0.0, 0.0, 0.0), distance=3.0, spread=0.6):
    """n rays from outside: origins on a sphere of `distance` about `centre`, aimed at points within `spread` of the centre, so that hits
    and misses mix.  -> (origins, dirs) float32 [n,3], unit to float32."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.asarray(centre) + distance * u
    target = np.asarray(centre) + spread * rng.uniform(-1.0, 1.0, (n, 3)) * np.array([2.0, 2.0, 2.0])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ the rule
def valid_triangles(verts, faces):
    """bool [nf]: every vertex finite and (v1 - v0) x (v2 - v0) != 0 in some component."""
    tv = np.asarray(verts, np.float64)[np.asarray(faces).reshape(-1, 3)]
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.isfinite(tv).all(axis=(1, 2)) & ((nx != 0) | (ny != 0) | (nz != 0))


def ray_axes(d):
    """d: three floats -> (kx, ky, kz)."""
    kz, m = 0, abs(d[0])
    if abs(d[1]) > m:
        kz, m = 1, abs(d[1])
    if abs(d[2]) > m:
        kz = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d[kz] < 0.0:
        kx, ky = ky, kx
    return kx, ky, kz


def _limits(t_min, t_max, R):
    t_min = np.zeros(R) if t_min is None else np.asarray(t_min, np.float32).astype(np.float64).reshape(R)
    t_max = np.full(R, INF) if t_max is None else np.asarray(t_max, np.float32).astype(np.float64).reshape(R)
    return t_min, t_max


def rule_one_ray(tv, valid, o, d, t_min, t_max):
    """The rule for one ray against all triangles tv [nf,3,3] -> (accepted bool [nf], t, u, v float64 [nf], bary_min [nf]: the smallest of
    the three normalised edge values, NaN where det == 0; in_range bool [nf])."""
    kx, ky, kz = ray_axes(d)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = np.float64(d[kx]) / np.float64(d[kz]), np.float64(d[ky]) / np.float64(d[kz]), np.float64(1.0) / np.float64(d[kz])
        P = tv - o                                       # [nf, 3 vertices, 3 axes]
        Pz = P[:, :, kz]
        X = P[:, :, kx] - Sx * Pz
        Y = P[:, :, ky] - Sy * Pz
        Ax, Bx, Cx = X[:, 0], X[:, 1], X[:, 2]
        Ay, By, Cy = Y[:, 0], Y[:, 1], Y[:, 2]
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        sign = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        det = (U + V) + W
        Z = Sz * Pz
        T = (U * Z[:, 0] + V * Z[:, 1]) + W * Z[:, 2]
        t = T / det
        in_range = (t >= t_min) & (t < t_max)
        acc = valid & sign & (det != 0) & in_range
        u, v = V / det, W / det
        bary_min = np.minimum(np.minimum(U / det, u), v)
    return acc, t, u, v, bary_min, in_range & valid


def cast_all(verts, faces, origins, dirs, t_min=None, t_max=None):
    """Brute force over all triangles -> (t float64 [R], +inf on a miss; tri int32 [R], -1 on a miss; uv float64 [R,2], 0 on a miss)."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    o64, d64 = np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    R = o64.shape[0]
    t_min, t_max = _limits(t_min, t_max, R)
    t_out, tri, uv = np.full(R, INF), np.full(R, -1, np.int32), np.zeros((R, 2))
    if faces.shape[0] == 0:
        return t_out, tri, uv
    tv, valid = verts[faces], valid_triangles(verts, faces)
    for r in range(R):
        acc, t, u, v, _, _ = rule_one_ray(tv, valid, o64[r], d64[r], t_min[r], t_max[r])
        if acc.any():
            tt = np.where(acc, t, INF)
            k = int(np.argmax(tt == tt.min()))           # the lowest index among the ties
            t_out[r], tri[r], uv[r] = t[k], k, (u[k], v[k])
    return t_out, tri, uv


def judge(verts, faces, origins, dirs, t_min=None, t_max=None, tol=1e-9):
    """bool [R]: the ray is excluded from a comparison: its two smallest accepted t on different triangles differ by less than
    tol (1 + t), or a candidate (a triangle in range whose smallest barycentric is >= -tol, with t no further than that window behind
    the closest hit) has its smallest barycentric within tol of zero."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    o64, d64 = np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    R = o64.shape[0]
    t_min, t_max = _limits(t_min, t_max, R)
    out = np.zeros(R, bool)
    if faces.shape[0] == 0:
        return out
    tv, valid = verts[faces], valid_triangles(verts, faces)
    for r in range(R):
        acc, t, _, _, bmin, in_range = rule_one_ray(tv, valid, o64[r], d64[r], t_min[r], t_max[r])
        with np.errstate(invalid="ignore"):
            cand = in_range & (bmin >= -tol)
        if not cand.any():
            continue
        tbest = np.where(acc, t, INF).min() if acc.any() else INF
        with np.errstate(invalid="ignore"):
            window = cand & ((t <= tbest + tol * (1.0 + abs(tbest))) if math.isfinite(tbest) else True)
        if (np.abs(bmin[window]) < tol).any():
            out[r] = True
        ts = np.sort(t[acc])
        if ts.size >= 2 and ts[1] - ts[0] < tol * (1.0 + ts[0]):
            out[r] = True
    return out


# ------------------------------------------------------------------------------------------------------------------------ the tree
def _spread21(x):
    x = x & 0x1fffff
    x = (x | (x << 32)) & 0x1f00000000ffff
    x = (x | (x << 16)) & 0x1f0000ff0000ff
    x = (x | (x << 8)) & 0x100f00f00f00f00f
    x = (x | (x << 4)) & 0x10c30c30c30c30c3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


KEY_LAST = 0x7fffffffffffffff


def morton_keys(verts, faces):
    """The 63-bit Morton key of each triangle's centroid in the box of the valid centroids (21 bits an axis); invalid triangles: KEY_LAST."""
    tv, valid = np.asarray(verts, np.float64)[faces], valid_triangles(verts, faces)
    keys = [KEY_LAST] * faces.shape[0]
    if not valid.any():
        return keys
    with np.errstate(all="ignore"):
        c = ((tv[:, 0] + tv[:, 1]) + tv[:, 2]) / 3.0
    lo, hi = c[valid].min(axis=0), c[valid].max(axis=0)
    for g in np.nonzero(valid)[0]:
        k = 0
        for a in range(3):
            ext = hi[a] - lo[a]
            q = (c[g, a] - lo[a]) / ext * 2097152.0 if ext > 0 else 0.0
            q = q if q >= 0.0 else 0.0
            q = q if q <= 2097151.0 else 2097151.0
            k |= _spread21(int(q)) << a
        keys[g] = k
    return keys


def _down32(x):
    f = np.float32(x)
    return float(np.nextafter(f, np.float32(-np.inf))) if float(f) > x else float(f)


def _up32(x):
    f = np.float32(x)
    return float(np.nextafter(f, np.float32(np.inf))) if float(f) < x else float(f)


EMPTY = (INF, INF, INF, -INF, -INF, -INF)
PAD = 2.0 ** -26


class Tree:
    """The implicit complete binary tree over the Morton-sorted triangles: L = the power of two >= max(nf, 1) leaves, node k has children
    2k and 2k + 1, leaf L + i holds sorted triangle i; float32 boxes rounded outwards; empty boxes for padding and invalid triangles."""

    def __init__(self, verts, faces):
        self.verts, self.faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
        nf = self.nf = self.faces.shape[0]
        if nf and (self.faces.min() < 0 or self.faces.max() >= self.verts.shape[0]):
            raise ValueError("face index out of range")
        self.valid = valid_triangles(self.verts, self.faces) if nf else np.zeros(0, bool)
        keys = morton_keys(self.verts, self.faces) if nf else []
        self.order = sorted(range(nf), key=lambda g: keys[g])          # stable, as the radix sort
        L = 1
        while L < nf:
            L *= 2
        self.L = L
        self.box = [EMPTY] * (2 * L)
        self.tv = self.verts[self.faces] if nf else np.zeros((0, 3, 3))
        for i, g in enumerate(self.order):
            if self.valid[g]:
                lo, hi = self.tv[g].min(axis=0), self.tv[g].max(axis=0)
                self.box[L + i] = tuple(_down32(x) for x in lo) + tuple(_up32(x) for x in hi)
        for k in range(L - 1, 0, -1):
            a, b = self.box[2 * k], self.box[2 * k + 1]
            self.box[k] = tuple(min(a[j], b[j]) for j in range(3)) + tuple(max(a[j], b[j]) for j in range(3, 6))

    def _box(self, k, o, d, t_min, best):
        """-> (may hold a hit, entry distance): the slab test on the box widened by PAD of its largest distance from the origin."""
        b = self.box[k]
        if not (b[0] <= b[3] and b[1] <= b[4] and b[2] <= b[5]):
            return False, INF
        lo = [b[a] - o[a] for a in range(3)]
        hi = [b[3 + a] - o[a] for a in range(3)]
        pad = max(max(abs(x) for x in lo), max(abs(x) for x in hi)) * PAD
        en, ex = -INF, INF
        for a in range(3):
            la, ha = lo[a] - pad, hi[a] + pad
            if d[a] == 0.0:
                if not (la <= 0.0 and ha >= 0.0):
                    return False, INF
                continue
            inv = 1.0 / d[a]
            t1, t2 = la * inv, ha * inv
            en, ex = max(en, min(t1, t2)), min(ex, max(t1, t2))
        return (en <= ex and en <= best and ex >= t_min), en

    def _hit(self, g, o, d, axes, S, t_min, t_max):
        kx, ky, kz = axes
        Sx, Sy, Sz = S
        P = [[float(self.tv[g][c][a]) - o[a] for a in range(3)] for c in range(3)]
        X = [P[c][kx] - Sx * P[c][kz] for c in range(3)]
        Y = [P[c][ky] - Sy * P[c][kz] for c in range(3)]
        U = X[2] * Y[1] - Y[2] * X[1]
        V = X[0] * Y[2] - Y[0] * X[2]
        W = X[1] * Y[0] - Y[1] * X[0]
        if not ((U >= 0 and V >= 0 and W >= 0) or (U <= 0 and V <= 0 and W <= 0)):
            return None
        det = (U + V) + W
        if det == 0.0 or det != det:
            return None
        T = (U * (Sz * P[0][kz]) + V * (Sz * P[1][kz])) + W * (Sz * P[2][kz])
        t = T / det
        if not (t >= t_min and t < t_max):
            return None
        return t, V / det, W / det

    def walk(self, o, d, t_min=0.0, t_max=INF, any_hit=False):
        """One ray (o, d: three floats each, float32 values) -> (t, tri, (u, v), nodes tested, triangles tested); near child first, a box
        is left out only when its entry distance is > the best t; the state is the node and a bit trail."""
        o, d = [float(x) for x in o], [float(x) for x in d]
        axes = ray_axes(d)
        kx, ky, kz = axes
        try:
            S = (d[kx] / d[kz], d[ky] / d[kz], 1.0 / d[kz])
        except ZeroDivisionError:
            return INF, -1, (0.0, 0.0), 1, 0
        L = self.L
        best, best_id, best_uv = t_max, -1, (0.0, 0.0)
        n_nodes, n_tris = 1, 0
        node, trail = 1, 0
        alive, _ = self._box(1, o, d, t_min, best)
        while alive:
            descend = False
            if node >= L:
                i = node - L
                if i < self.nf:
                    n_tris += 1
                    g = self.order[i]
                    h = self._hit(g, o, d, axes, S, t_min, t_max) if self.valid[g] else None
                    if h is not None and (h[0] < best or (h[0] == best and g < best_id)):
                        best, best_id, best_uv = h[0], g, (h[1], h[2])
                        if any_hit:
                            break
            else:
                n_nodes += 2
                h0, e0 = self._box(2 * node, o, d, t_min, best)
                h1, e1 = self._box(2 * node + 1, o, d, t_min, best)
                if h0 or h1:
                    both = h0 and h1
                    right = (1 if e1 < e0 else 0) if both else (1 if h1 else 0)
                    node = 2 * node + right
                    trail = (trail << 1) | (1 if both else 0)
                    descend = True
            if descend:
                continue
            while True:
                if trail == 0:
                    alive = False
                    break
                s = (trail & -trail).bit_length() - 1
                node >>= s
                trail >>= s
                node ^= 1
                trail ^= 1
                n_nodes += 1
                if self._box(node, o, d, t_min, best)[0]:
                    break
        if best_id < 0:
            return INF, -1, (0.0, 0.0), n_nodes, n_tris
        return best, best_id, best_uv, n_nodes, n_tris

    def cast(self, origins, dirs, t_min=None, t_max=None, any_hit=False):
        """-> (t float64 [R], tri int32 [R], uv float64 [R,2], counts int64 [R,2])."""
        o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
        R = o32.shape[0]
        t_min, t_max = _limits(t_min, t_max, R)
        t, tri, uv, counts = np.full(R, INF), np.full(R, -1, np.int32), np.zeros((R, 2)), np.zeros((R, 2), np.int64)
        for r in range(R):
            t[r], tri[r], uv[r], counts[r, 0], counts[r, 1] = self.walk(o32[r], d32[r], float(t_min[r]), float(t_max[r]), any_hit)
        return t, tri, uv, counts
