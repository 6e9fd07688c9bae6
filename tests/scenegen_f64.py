"""Scene generation restated in float64 numpy (neat_amd/scenegen.py, csrc/kernels_scenegen.hpp): the pictures and the visible
runs of the edges by brute force over all triangles with the rule of tests/raycast_f64.py.  Every operation is one float64 operation,
every product rounded on its own, divisions and square roots correctly rounded: the device equals these results byte for byte.

Cameras: K [3,3] (fx, skew, cx / fy, cy), pose [4,4] camera-to-world [R | c].
    pixel (u, v) -> ray    yl = (v - cy) / fy, xl = ((u - cx) - skew yl) / fx, d = (R[:,0] xl + R[:,1] yl) + R[:,2], origin c
    world X -> camera      Xc[a] = (R[0,a] (X - c)[0] + R[1,a] (X - c)[1]) + R[2,a] (X - c)[2]
    camera -> picture      x = (fx (Xc[0] / Xc[2]) + skew (Xc[1] / Xc[2])) + cx, y = fy (Xc[1] / Xc[2]) + cy
"""
import numpy as np

from tests import raycast_f64 as rc

INF = float("inf")
MAX_SAMPLES = 1 << 16


# ------------------------------------------------------------------------------------------------------------------------ the rule, many rays
def _rule(tv, valid, o, D, t_max):
    """The rule of raycast_f64.rule_one_ray for the rays (o, D[r]) with 0 <= t < t_max[r] against all triangles tv [nf,3,3]
    -> (accepted bool [R,nf], t float64 [R,nf])."""
    R = D.shape[0]
    rows = np.arange(R)
    kz = np.argmax(np.abs(D), axis=1)                    # the first of the largest: the lowest axis on a tie
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    swap = D[rows, kz] < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        dk = D[rows, kz]
        Sx, Sy, Sz = D[rows, kx] / dk, D[rows, ky] / dk, 1.0 / dk
        P = tv - o                                        # [nf, 3 vertices, 3 axes]
        Pt = np.ascontiguousarray(np.moveaxis(P, 2, 0))   # [3 axes, nf, 3 vertices]
        Pz = Pt[kz]                                       # [R, nf, 3]
        X = Pt[kx] - Sx[:, None, None] * Pz
        Y = Pt[ky] - Sy[:, None, None] * Pz
        Ax, Bx, Cx = X[..., 0], X[..., 1], X[..., 2]
        Ay, By, Cy = Y[..., 0], Y[..., 1], Y[..., 2]
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        sign = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        det = (U + V) + W
        Z = Sz[:, None, None] * Pz
        T = (U * Z[..., 0] + V * Z[..., 1]) + W * Z[..., 2]
        t = T / det
        acc = valid[None, :] & sign & (det != 0) & (t >= 0.0) & (t < t_max[:, None])
    return acc, t


def closest(verts, faces, o, D, chunk=128):
    """Closest hit of the rays (o, D[r]), t in [0, inf), ties to the lowest face index -> (t float64 [R], +inf on a miss; tri int32 [R])."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    D = np.asarray(D, np.float64).reshape(-1, 3)
    R = D.shape[0]
    t_out, tri = np.full(R, INF), np.full(R, -1, np.int32)
    if faces.shape[0] == 0 or R == 0:
        return t_out, tri
    tv, valid = verts[faces], rc.valid_triangles(verts, faces)
    for a in range(0, R, chunk):
        acc, t = _rule(tv, valid, np.asarray(o, np.float64), D[a:a + chunk], np.full(min(chunk, R - a), INF))
        tt = np.where(acc, t, INF)
        best = tt.min(axis=1)
        k = np.argmax(tt == best[:, None], axis=1)         # the lowest index among the ties
        hit = acc.any(axis=1)
        t_out[a:a + chunk] = np.where(hit, best, INF)
        tri[a:a + chunk] = np.where(hit, k, -1)
    return t_out, tri


def any_hit(verts, faces, o, D, t_max, chunk=128):
    """bool [R]: the ray (o, D[r]) meets a triangle with 0 <= t < t_max[r]."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    D, t_max = np.asarray(D, np.float64).reshape(-1, 3), np.asarray(t_max, np.float64).reshape(-1)
    R = D.shape[0]
    out = np.zeros(R, bool)
    if faces.shape[0] == 0 or R == 0:
        return out
    tv, valid = verts[faces], rc.valid_triangles(verts, faces)
    for a in range(0, R, chunk):
        out[a:a + chunk] = _rule(tv, valid, np.asarray(o, np.float64), D[a:a + chunk], t_max[a:a + chunk])[0].any(axis=1)
    return out


# ------------------------------------------------------------------------------------------------------------------------ pictures
def _norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def sample_rays(K, pose, H, W, ss, i, j):
    """The rays of sub-sample (i, j) of every pixel, x fastest -> D float64 [H W, 3]."""
    K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = (xs.reshape(-1) + (np.float64(i) + 0.5) / np.float64(ss)) - 0.5
    v = (ys.reshape(-1) + (np.float64(j) + 0.5) / np.float64(ss)) - 0.5
    yl = (v - cy) / fy
    xl = ((u - cx) - sk * yl) / fx
    return np.stack([(pose[r, 0] * xl + pose[r, 1] * yl) + pose[r, 2] for r in range(3)], axis=1)


def pictures(verts, faces, K, poses, H, W, ss=3, albedo=0.7, ambient=0.25, background=1.0, counts=False):
    """-> (rgb uint8 [V,H,W,3], mask uint8 [V,H,W]); with counts also the hits int32 [V,H,W] of each pixel's ss^2 sub-samples."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    K, poses = np.asarray(K, np.float64).reshape(-1, 3, 3), np.asarray(poses, np.float64).reshape(-1, 4, 4)
    V = poses.shape[0]
    rgb, mask, hits = np.zeros((V, H, W, 3), np.uint8), np.zeros((V, H, W), np.uint8), np.zeros((V, H, W), np.int32)
    albedo, ambient, background = np.float64(albedo), np.float64(ambient), np.float64(background)
    k1 = np.float64(1.0) - ambient
    tv = verts[faces] if faces.shape[0] else np.zeros((0, 3, 3))
    e1, e2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    for f in range(V):
        total, nhit = np.zeros(H * W), np.zeros(H * W, np.int32)
        for j in range(ss):
            for i in range(ss):
                D = sample_rays(K[f], poses[f], H, W, ss, i, j)
                _, tri = closest(verts, faces, poses[f, :3, 3], D)
                hit = tri >= 0
                nn = n[np.where(hit, tri, 0)] if faces.shape[0] else np.ones((H * W, 3))
                with np.errstate(all="ignore"):
                    nd = (nn[:, 0] * D[:, 0] + nn[:, 1] * D[:, 1]) + nn[:, 2] * D[:, 2]
                    den = _norm3(nn[:, 0], nn[:, 1], nn[:, 2]) * _norm3(D[:, 0], D[:, 1], D[:, 2])
                    col = albedo * (ambient + k1 * (np.abs(nd) / den))
                total = total + np.where(hit, col, background)
                nhit += hit
        q = np.floor(np.float64(255.0) * (total / np.float64(ss * ss)) + 0.5)
        byte = np.where(q >= 255.0, 255, np.where(q >= 0.0, q, 0)).astype(np.uint8)
        rgb[f] = np.repeat(byte.reshape(H, W, 1), 3, axis=2)
        mask[f] = np.where(nhit > 0, 255, 0).reshape(H, W)
        hits[f] = nhit.reshape(H, W)
    return (rgb, mask, hits) if counts else (rgb, mask)


# ------------------------------------------------------------------------------------------------------------------------ edges
def to_camera(pose, X):
    pose, X = np.asarray(pose, np.float64), np.asarray(X, np.float64)
    d = X - pose[:3, 3]
    return np.array([(pose[0, a] * d[0] + pose[1, a] * d[1]) + pose[2, a] * d[2] for a in range(3)])


def project(K, Xc):
    K = np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        ix, iy = Xc[0] / Xc[2], Xc[1] / Xc[2]
        return (K[0, 0] * ix + K[0, 1] * iy) + K[0, 2], K[1, 1] * iy + K[1, 2]


def _clip(p, q, t):
    """One Liang-Barsky boundary on t = [t0, t1] -> False: the segment lies outside."""
    if p == 0.0:
        return not q < 0.0
    with np.errstate(all="ignore"):
        r = q / p
    if p < 0.0:
        if r > t[1]:
            return False
        if r > t[0]:
            t[0] = r
    else:
        if r < t[0]:
            return False
        if r < t[1]:
            t[1] = r
    return True


class Edge:
    """One edge in one view: n samples (0: nothing), the cut flags, the cut segment in the picture and in the world."""

    def __init__(self, K, pose, P0, P1, H, W, step, near):
        K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
        P0, P1 = np.asarray(P0, np.float64), np.asarray(P1, np.float64)
        step, near = np.float64(step), np.float64(near)
        self.n, self.cut0, self.cut1 = 0, False, False
        self.Aw, self.Bw, self.c = P0.copy(), P1.copy(), pose[:3, 3].copy()
        A, B = to_camera(pose, P0), to_camera(pose, P1)
        if not A[2] >= near and not B[2] >= near:
            return
        with np.errstate(all="ignore"):
            if not A[2] >= near:
                s = (near - A[2]) / (B[2] - A[2])
                A = np.array([A[0] + s * (B[0] - A[0]), A[1] + s * (B[1] - A[1]), near])
                self.Aw = P0 + s * (P1 - P0)
                self.cut0 = True
            elif not B[2] >= near:
                s = (near - B[2]) / (A[2] - B[2])
                B = np.array([B[0] + s * (A[0] - B[0]), B[1] + s * (A[1] - B[1]), near])
                self.Bw = P1 + s * (P0 - P1)
                self.cut1 = True
        self.Az, self.Bz = A[2], B[2]
        (self.ax, self.ay), (self.bx, self.by) = project(K, A), project(K, B)
        dx, dy = self.bx - self.ax, self.by - self.ay
        t = [np.float64(0.0), np.float64(1.0)]
        ok = (_clip(-dx, self.ax - (-0.5), t) and _clip(dx, (np.float64(W) - 0.5) - self.ax, t) and
              _clip(-dy, self.ay - (-0.5), t) and _clip(dy, (np.float64(H) - 0.5) - self.ay, t))
        self.t0, self.t1 = t
        if not ok:
            return
        self.cut0 = self.cut0 or self.t0 > 0.0
        self.cut1 = self.cut1 or self.t1 < 1.0
        p0, p1 = self.point2(np.array([self.t0])), self.point2(np.array([self.t1]))
        with np.errstate(all="ignore"):
            q = np.ceil(length2(p0[0], p1[0]) / step)
        if not q >= 0.0:
            return
        self.n = MAX_SAMPLES if q >= MAX_SAMPLES - 1 else int(q) + 1

    def tau(self):
        n = self.n
        if n == 1:
            return np.array([self.t0])
        t = self.t0 + (self.t1 - self.t0) * (np.arange(n, dtype=np.float64) / np.float64(n - 1))
        t[0], t[n - 1] = self.t0, self.t1
        return t

    def point2(self, tau):
        """[m] parameters -> [m,2]; tau = 1 is the end itself."""
        x = np.where(tau == 1.0, self.bx, self.ax + tau * (self.bx - self.ax))
        y = np.where(tau == 1.0, self.by, self.ay + tau * (self.by - self.ay))
        return np.stack([x, y], axis=1)

    def point3(self, tau):
        """[m] parameters -> [m,3] by the perspective-correct parameter sigma; sigma = 1 is the end itself."""
        wa, wb = tau * self.Az, (1.0 - tau) * self.Bz
        sigma = wa / (wa + wb)
        return np.where((sigma == 1.0)[:, None], self.Bw[None], self.Aw[None] + sigma[:, None] * (self.Bw - self.Aw)[None])


def length2(p, q):
    dx, dy = q[0] - p[0], q[1] - p[1]
    return np.sqrt(dx * dx + dy * dy)


def visible_samples(verts, faces, e, bias):
    """bool [e.n]: sample k is visible from the camera centre."""
    X = e.point3(e.tau())
    d = X - e.c
    dist = _norm3(d[:, 0], d[:, 1], d[:, 2])
    with np.errstate(all="ignore"):
        D = d / dist[:, None]
    ok = dist > bias
    D = np.where(ok[:, None], D, np.array([0.0, 0.0, 1.0]))
    return ok & ~any_hit(verts, faces, e.c, D, np.where(ok, dist - np.float64(bias), 0.0))


def visible_edges(verts, faces, junctions, edges, K, poses, H, W, step=1.0, min_len=0.0, bias=0.0, near=0.05, all_runs=False):
    """-> dict(idx int32 [N,4] = view, edge, first, last; p2 float64 [N,4]; p3 float64 [N,2,3]; junc uint8 [N,2]) in (view, edge, run) order.
    all_runs: every run whatever its length, with `length` float64 [N] as well."""
    junctions, edges = np.asarray(junctions, np.float64).reshape(-1, 3), np.asarray(edges).reshape(-1, 2)
    K, poses = np.asarray(K, np.float64).reshape(-1, 3, 3), np.asarray(poses, np.float64).reshape(-1, 4, 4)
    idx, p2, p3, junc, lens = [], [], [], [], []
    for f in range(poses.shape[0]):
        for j, (a, b) in enumerate(edges):
            e = Edge(K[f], poses[f], junctions[a], junctions[b], H, W, step, near)
            if e.n == 0:
                continue
            vis = visible_samples(verts, faces, e, bias)
            tau = e.tau()
            k = 0
            while k < e.n:
                if not vis[k]:
                    k += 1
                    continue
                first = k
                while k < e.n and vis[k]:
                    k += 1
                last = k - 1
                ends2 = e.point2(tau[[first, last]])
                length = length2(ends2[0], ends2[1])
                if all_runs or length >= min_len:
                    idx.append((f, j, first, last))
                    p2.append(ends2.reshape(4))
                    p3.append(e.point3(tau[[first, last]]))
                    junc.append((int(first == 0 and not e.cut0), int(last == e.n - 1 and not e.cut1)))
                    lens.append(length)
    out = {"idx": np.asarray(idx, np.int32).reshape(-1, 4), "p2": np.asarray(p2, np.float64).reshape(-1, 4),
           "p3": np.asarray(p3, np.float64).reshape(-1, 2, 3), "junc": np.asarray(junc, np.uint8).reshape(-1, 2)}
    if all_runs:
        out["length"] = np.asarray(lens, np.float64)
    return out
