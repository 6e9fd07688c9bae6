"""The picture of neat_amd.show restated in numpy float64 (neat_amd/csrc/kernels_show.hpp): brute force over pixels x
primitives, one numpy operation per rounded device operation and in the same order (numpy never contracts a product into a sum).  Only
for the small frames of the tests.

    render(lines, cams, H, W, verts=None, faces=None, points=None, **style) -> dict per frame-stack:
        depth float32 [F,H,W], index int64 [F,H,W] (-1: uncovered), cov / covp float32 [F,H,W], rgb uint8 [F,H,W,3],
        second: the runner-up key's depth (float32, inf if none), edge_margin: min |E| / |A| of the winner (inf if uncovered)
"""
import numpy as np

COORD_MAX = 2.0 ** 40
STYLE = dict(width=1.5, radius=2.5, near=0.05, bias=0.01, hidden_alpha=0.0, bg=(1.0, 1.0, 1.0), line_color=(0.0, 0.0, 0.0),
             point_color=(0.0, 0.0, 1.0), mesh_color=(0.8, 0.8, 0.8))


def split_cam(cam):
    """cam [21] -> fx, fy, cx, cy, R [3,3], T [3]."""
    cam = np.asarray(cam, dtype=np.float64)
    K, RT = cam[:9].reshape(3, 3), cam[9:].reshape(3, 4)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2], RT[:, :3], RT[:, 3]


def to_cam(cam, X):
    """X [...,3] -> Xc [...,3]: ((R0 X0 + R1 X1) + R2 X2) + T per row."""
    _, _, _, _, R, T = split_cam(cam)
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(X.shape, dtype=np.float64)
    for r in range(3):
        out[..., r] = ((R[r, 0] * X[..., 0] + R[r, 1] * X[..., 1]) + R[r, 2] * X[..., 2]) + T[r]
    return out


def project(cam, Xc):
    """-> x, y, ok (finite and within 2^40)."""
    fx, fy, cx, cy, _, _ = split_cam(cam)
    with np.errstate(all="ignore"):
        x = (fx * Xc[..., 0]) / Xc[..., 2] + cx
        y = (fy * Xc[..., 1]) / Xc[..., 2] + cy
        ok = (np.abs(x) <= COORD_MAX) & (np.abs(y) <= COORD_MAX)
    return x, y, ok


def _pixels(H, W):
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return j, i          # px, py


def _f32_bits(z):
    return np.asarray(z, dtype=np.float32).view(np.uint32).astype(np.uint64)


def mesh_depth(cam, verts, faces, H, W, near):
    """-> depth f32 [H,W], index [H,W], second f32 [H,W], edge_margin [H,W]."""
    px, py = _pixels(H, W)
    clear = np.uint64(0x7f800000ffffffff)
    best = np.full((H, W), clear, dtype=np.uint64)
    second = np.full((H, W), clear, dtype=np.uint64)
    margin = np.full((H, W), np.inf)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    for k, (i0, i1, i2) in enumerate(faces):
        V = verts[[i0, i1, i2]]
        if not np.isfinite(V).all():
            continue
        C = to_cam(cam, V)
        if not np.isfinite(C).all() or (C[:, 2] < near).any():
            continue
        x, y, ok = project(cam, C)
        if not ok.all():
            continue
        (ax, bx, cx), (ay, by, cy), (za, zb, zc) = x, y, C[:, 2]

        def edge(ux, uy, vx, vy, qx, qy):
            return (vx - ux) * (qy - uy) - (vy - uy) * (qx - ux)
        A = edge(ax, ay, bx, by, cx, cy)
        if not (A != 0.0) or not np.isfinite(A):
            continue
        eab, ebc, eca = edge(ax, ay, bx, by, px, py), edge(bx, by, cx, cy, px, py), edge(cx, cy, ax, ay, px, py)
        inside = ((eab >= 0) & (ebc >= 0) & (eca >= 0)) if A > 0 else ((eab <= 0) & (ebc <= 0) & (eca <= 0))
        with np.errstate(all="ignore"):
            la, lb, lc = ebc / A, eca / A, eab / A
            iz = (la / za + lb / zb) + lc / zc
            zf = (1.0 / iz).astype(np.float32)
        inside &= zf > 0
        key = (_f32_bits(zf) << np.uint64(32)) | np.uint64(k)
        key = np.where(inside, key, clear)
        m = np.minimum(np.minimum(np.abs(eab), np.abs(ebc)), np.abs(eca)) / abs(A)
        wins = key < best
        second = np.where(wins, best, np.minimum(second, key))
        margin = np.where(wins, m, margin)
        best = np.where(wins, key, best)
    depth = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = (best & np.uint64(0xffffffff)).astype(np.int64)
    index[index == 0xffffffff] = -1
    return depth, index, (second >> np.uint64(32)).astype(np.uint32).view(np.float32), margin


def clip_segment(cam, P, near):
    """P [2,3] world -> (x0, y0, z0, x1, y1, z1) on the screen, or None if dropped."""
    P = np.asarray(P, dtype=np.float64).reshape(2, 3)
    if not np.isfinite(P).all():
        return None
    C = to_cam(cam, P)
    if not np.isfinite(C).all():
        return None
    behind = C[:, 2] < near
    if behind.all():
        return None
    if behind.any():
        e, o = (0, 1) if behind[0] else (1, 0)
        t = (near - C[e, 2]) / (C[o, 2] - C[e, 2])
        C[e, 0] = C[e, 0] + t * (C[o, 0] - C[e, 0])
        C[e, 1] = C[e, 1] + t * (C[o, 1] - C[e, 1])
        C[e, 2] = near
    x, y, ok = project(cam, C)
    if not ok.all():
        return None
    return x[0], y[0], C[0, 2], x[1], y[1], C[1, 2]


def _cover(seg, px, py, hw, depth, bias, alpha):
    """The float32 value of every pixel under one screen segment (a point is a zero-length one)."""
    x0, y0, z0, x1, y1, z1 = seg
    dx, dy = x1 - x0, y1 - y0
    l2 = dx * dx + dy * dy
    if l2 > 0.0:
        u = np.minimum(np.maximum(((px - x0) * dx + (py - y0) * dy) / l2, 0.0), 1.0)
    else:
        u = np.zeros_like(px)
    qx, qy = x0 + u * dx, y0 + u * dy
    ex, ey = px - qx, py - qy
    d = np.sqrt(ex * ex + ey * ey)
    cov = np.minimum(np.maximum(hw - d, 0.0), 1.0)
    with np.errstate(all="ignore"):
        z = 1.0 / ((1.0 - u) / z0 + u / z1)
        visible = z <= depth.astype(np.float64) + bias
    return np.where(visible, cov, cov * alpha).astype(np.float32)


def line_coverage(cam, lines, H, W, depth, width, near, bias, alpha):
    px, py = _pixels(H, W)
    C = np.zeros((H, W), dtype=np.float32)
    for P in np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3):
        seg = clip_segment(cam, P, near)
        if seg is not None:
            C = np.maximum(C, _cover(seg, px, py, width / 2.0 + 0.5, depth, bias, alpha))
    return C


def point_coverage(cam, points, H, W, depth, radius, near, bias, alpha):
    px, py = _pixels(H, W)
    C = np.zeros((H, W), dtype=np.float32)
    for P in np.asarray(points, dtype=np.float64).reshape(-1, 3):
        if not np.isfinite(P).all():
            continue
        c = to_cam(cam, P)
        if not np.isfinite(c).all() or c[2] < near:
            continue
        x, y, ok = project(cam, c)
        if ok:
            C = np.maximum(C, _cover((x, y, c[2], x, y, c[2]), px, py, radius + 0.5, depth, bias, alpha))
    return C


def shade(cam, verts, face):
    a, b, c = to_cam(cam, np.asarray(verts, dtype=np.float64)[list(face)])
    u, v = b - a, c - a
    nx, ny, nz = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return 0.25 + 0.75 * (abs(nz) / ln if ln > 0 else 0.0)


def compose(cam, verts, faces, index, C, Cp, bg, line_color, point_color, mesh_color):
    """-> rgb uint8 [H,W,3] and the float64 255 rgb + 0.5 before the floor."""
    H, W = index.shape
    base = np.empty((H, W, 3))
    base[:] = np.asarray(bg, dtype=np.float64)
    for k in np.unique(index[index >= 0]):
        s = shade(cam, verts, np.asarray(faces).reshape(-1, 3)[k])
        base[index == k] = np.asarray(mesh_color, dtype=np.float64) * s
    c, cp = C.astype(np.float64)[..., None], Cp.astype(np.float64)[..., None]
    rgb = base * (1.0 - c) + np.asarray(line_color, dtype=np.float64) * c
    rgb = rgb * (1.0 - cp) + np.asarray(point_color, dtype=np.float64) * cp
    pre = 255.0 * rgb + 0.5
    return np.clip(np.floor(pre), 0, 255).astype(np.uint8), pre


def render(lines, cams, H, W, verts=None, faces=None, points=None, **style):
    st = dict(STYLE)
    st.update(style)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 21)
    out = {k: [] for k in ("depth", "index", "second", "edge_margin", "cov", "covp", "rgb", "pre")}
    nf = 0 if faces is None else len(np.asarray(faces).reshape(-1, 3))
    for cam in cams:
        if nf:
            depth, index, second, margin = mesh_depth(cam, verts, faces, H, W, st["near"])
        else:
            depth = np.full((H, W), np.inf, dtype=np.float32)
            index, second, margin = np.full((H, W), -1, dtype=np.int64), depth.copy(), np.full((H, W), np.inf)
        n_lines = 0 if lines is None else np.asarray(lines).size
        C = line_coverage(cam, lines, H, W, depth, st["width"], st["near"], st["bias"], st["hidden_alpha"]) if n_lines \
            else np.zeros((H, W), dtype=np.float32)
        n_pts = 0 if points is None else np.asarray(points).size
        Cp = point_coverage(cam, points, H, W, depth, st["radius"], st["near"], st["bias"], st["hidden_alpha"]) if n_pts \
            else np.zeros((H, W), dtype=np.float32)
        rgb, pre = compose(cam, verts, faces, index, C, Cp, st["bg"], st["line_color"], st["point_color"], st["mesh_color"])
        for k, v in (("depth", depth), ("index", index), ("second", second), ("edge_margin", margin), ("cov", C), ("covp", Cp), ("rgb", rgb),
                     ("pre", pre)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}
