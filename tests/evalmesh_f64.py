"""Plain numpy float64 restatement of the evaluation-mesh definitions (csrc/kernels_evalmesh.hpp), written from the
definitions and not from the kernels: oriented grid points, surface moments and the principal frame, affine rows and bounds, the
aligned grid as a literal use of numpy.linspace / numpy.arange, and the cut of a mesh by planes with welded cut vertices.  An
independent unwelded polygon clip (Sutherland-Hodgman per triangle) checks the cut's area."""
import numpy as np

from tests import mesh_f64 as M


# ---- oriented grid points -----------------------------------------------------------------------------------------------------------
def axis_f64(b0, b1, n):
    """The linspace rule before its rounding to float32: b0 + i (b1 - b0) / (n - 1) in float64, the last node exactly b1."""
    b0, b1 = float(b0), float(b1)
    x = np.arange(n, dtype=np.float64) * ((b1 - b0) / (n - 1)) + b0
    x[-1] = b1
    return x


def oriented_points(shape, lo, hi, R, c):
    """-> float32 [N, 3], x slowest: x_a = float32(c_a + ((R_0a p_0 + R_1a p_1) + R_2a p_2)), every operation a float64 numpy op."""
    R, c = np.asarray(R, dtype=np.float64), np.asarray(c, dtype=np.float64)
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (3,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (3,))
    p0, p1, p2 = [g.reshape(-1) for g in np.meshgrid(*[axis_f64(lo[a], hi[a], shape[a]) for a in range(3)], indexing="ij")]
    cols = [c[a] + ((R[0, a] * p0 + R[1, a] * p1) + R[2, a] * p2) for a in range(3)]
    return np.stack(cols, axis=1).astype(np.float32)


# ---- moments and frame --------------------------------------------------------------------------------------------------------------------
def triangle_moments(a, b, c):
    """Per triangle, vertices [n, 3] float64 relative to the origin -> (area [n], first [n, 3], second [n, 3, 3]): exact integrals."""
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    g = (a + b + c) / 3.0
    outer = lambda u: u[:, :, None] * u[:, None, :]
    second = (area / 12.0)[:, None, None] * (outer(a) + outer(b) + outer(c) + 9.0 * outer(g))
    return area, area[:, None] * g, second


def moments(verts, faces, o):
    """-> float64 [10]: area, first moments, second moments (xx, xy, xz, yy, yz, zz) about o; triangles of zero area add nothing."""
    v = np.asarray(verts, dtype=np.float64) - np.asarray(o, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    area, first, second = triangle_moments(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    ok = area > 0
    s = second[ok].sum(axis=0)
    return np.concatenate([[area[ok].sum()], first[ok].sum(axis=0), [s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]]])


def frame_of(mom, o):
    """Moments about o -> (R, mean): rows of R the eigenvectors of the surface covariance by ascending eigenvalue, the largest-magnitude
    entry of each row positive, rows 1 and 2 swapped if det R < 0."""
    A = mom[0]
    m = mom[1:4] / A
    S = np.array([[mom[4], mom[5], mom[6]], [mom[5], mom[7], mom[8]], [mom[6], mom[8], mom[9]]]) / A
    w, vec = np.linalg.eigh(S - np.outer(m, m))
    R = vec[:, np.argsort(w, kind="stable")].T.copy()
    for r in range(3):
        R[r] *= np.sign(R[r, np.argmax(np.abs(R[r]))])
    if np.linalg.det(R) < 0:
        R[[1, 2]] = R[[2, 1]]
    return R, np.asarray(o, dtype=np.float64) + m


def principal_frame(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    o = 0.5 * (v.min(axis=0) + v.max(axis=0))
    return frame_of(moments(v, faces, o), o)


# ---- affine rows and bounds -------------------------------------------------------------------------------------------------------------
def affine_f64(v, A):
    """Rows -> ((A_r0 x + A_r1 y) + A_r2 z) + A_r3 in float64 [n, 3]."""
    v, A = np.asarray(v, dtype=np.float64), np.asarray(A, dtype=np.float64).reshape(3, 4)
    return np.stack([((A[r, 0] * v[:, 0] + A[r, 1] * v[:, 1]) + A[r, 2] * v[:, 2]) + A[r, 3] for r in range(3)], axis=1)


def affine_rows(v, A):
    return affine_f64(v, A).astype(np.float32)


def affine_bounds(v, A):
    y = affine_f64(v, A)
    return np.concatenate([y.min(axis=0), y.max(axis=0)])


# ---- the aligned grid, literally ------------------------------------------------------------------------------------------------------------
def aligned_axes_literal(lo, hi, resolution, eps):
    """The three node arrays as get_grid builds them: numpy.linspace on the shortest axis, numpy.arange with its spacing on the others."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    s = int(np.argmin(hi - lo))
    short = np.linspace(lo[s] - eps, hi[s] + eps, resolution)
    length = np.max(short) - np.min(short)
    step = length / (short.shape[0] - 1)
    return [short if a == s else np.arange(lo[a] - eps, hi[a] + step + eps, step) for a in range(3)]


# ---- the cut --------------------------------------------------------------------------------------------------------------------------------
def cut_plane(verts, faces, axis, value, sign, round32=True):
    """The part of the mesh with sign (x[axis] - float32(value)) >= 0 -> (verts float64 holding float32 values, faces int64).
    One inside vertex i (j, k next in the face's order): (i, c_ij, c_ik).  Two inside, o outside (i, j next in order): (i, j, c_jo),
    (i, c_jo, c_io).  c_ab = float32(a + t (b - a)), t = d_a / (d_a - d_b), its `axis` coordinate the plane value; one per (a, b).
    Order: used old vertices ascending, then cut vertices ascending by (a, b); faces by source face, then emitted triangle.
    round32=False keeps the cut vertices in float64 (the geometric identities of the CPU tests hold to float64 then)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    value = float(np.float32(value))
    d = sign * (v[:, axis] - value)
    inside = d >= 0
    records = []
    for fi in range(len(f)):
        idx = [int(t) for t in f[fi]]
        ins = [bool(inside[t]) for t in idx]
        n_in = sum(ins)
        if n_in == 3:
            records.append(tuple(idx))
        elif n_in == 1:
            s = ins.index(True)
            i, j, k = idx[s], idx[(s + 1) % 3], idx[(s + 2) % 3]
            records.append((i, (i, j), (i, k)))
        elif n_in == 2:
            o = ins.index(False)
            i, j, out = idx[(o + 1) % 3], idx[(o + 2) % 3], idx[o]
            records.append((i, j, (j, out)))
            records.append((i, (j, out), (i, out)))
    if not records:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    used = sorted({r for rec in records for r in rec if not isinstance(r, tuple)})
    cuts = sorted({r for rec in records for r in rec if isinstance(r, tuple)})
    name = {old: new for new, old in enumerate(used)}
    name.update({key: len(used) + n for n, key in enumerate(cuts)})
    new = [v[used]]
    if cuts:
        a, b = np.array([c[0] for c in cuts]), np.array([c[1] for c in cuts])
        t = d[a] / (d[a] - d[b])
        p = v[a] + t[:, None] * (v[b] - v[a])
        if round32:
            p = p.astype(np.float32).astype(np.float64)
        p[:, axis] = value
        new.append(p)
    return np.concatenate(new, axis=0), np.array([[name[r] for r in rec] for rec in records], dtype=np.int64)


BOX_PLANES = [(0, 0, 1), (0, 1, -1), (1, 0, 1), (1, 1, -1), (2, 0, 1), (2, 1, -1)]      # (axis, lo or hi, sign) in the order applied


def clip_box(verts, faces, lo, hi, round32=True):
    box = (np.broadcast_to(np.asarray(lo, dtype=np.float64), (3,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (3,)))
    for axis, side, sign in BOX_PLANES:
        verts, faces = cut_plane(verts, faces, axis, box[side][axis], sign, round32)
    return verts, faces


# ---- an independent check of the cut: every triangle clipped on its own, nothing shared ---------------------------------------------------
def polygon_clip_area(verts, faces, planes):
    """Sum over the triangles of the area of (triangle intersected with all half-spaces), planes = [(axis, value, sign)]."""
    v = np.asarray(verts, dtype=np.float64)
    total = 0.0
    for tri in np.asarray(faces, dtype=np.int64):
        poly = [v[t] for t in tri]
        for axis, value, sign in planes:
            value = float(np.float32(value))
            nxt = []
            for n in range(len(poly)):
                p, q = poly[n], poly[(n + 1) % len(poly)]
                dp, dq = sign * (p[axis] - value), sign * (q[axis] - value)
                if dp >= 0:
                    nxt.append(p)
                if (dp >= 0) != (dq >= 0):
                    nxt.append(p + (dp / (dp - dq)) * (q - p))
            poly = nxt
            if not poly:
                break
        for n in range(1, len(poly) - 1):
            total += 0.5 * np.linalg.norm(np.cross(poly[n] - poly[0], poly[n + 1] - poly[0]))
    return total


def mesh_area(verts, faces):
    return 0.5 * np.linalg.norm(M.face_normals(verts, faces), axis=1).sum()


def open_edges(faces):
    """The undirected edges that are not in exactly two faces with opposite directions [n, 2]."""
    _, ok, edges = M.edge_report(faces)
    return edges[~ok]
