"""Plain numpy float64 restatement of the marching-tetrahedra extraction, written from the definitions and not from the
kernels: the tetrahedra come from the axis permutations and a determinant, the 16-case table from a parity rule (the kernels carry both
as literal tables; tests/test_mesh_math.py checks that the two agree).

Definitions
  * nodes [nx][ny][nz], x slowest; node linear index (i ny + j) nz + k; a cell is named by its lowest node
  * inside iff v < level (NaN is outside); an edge carries a vertex iff its two nodes differ in that predicate and both are finite
  * 7 edge classes per node, class c joins the node to the node at offset (dx, dy, dz) = the bits (4, 2, 1) of c + 1
  * the vertex sits at a + t (b - a), t = (level - va) / (vb - va), from the inside node a towards the outside node b
  * a cell = the six tetrahedra 0 -> e_p -> e_p + e_q -> (1,1,1), (p, q, r) the permutations of (x, y, z) in lexicographic order;
    a tetrahedron with a non-finite corner emits nothing
  * vertex order: ascending (node, class); face order: ascending (cell, tetrahedron, triangle)
"""
import itertools

import numpy as np


def linspace_f32(b0, b1, n):
    """Node coordinates of one axis: float32(b0 + i (b1 - b0) / (n - 1)) in float64, the last node exactly b1."""
    b0, b1 = float(b0), float(b1)
    step = (b1 - b0) / (n - 1)
    x = np.arange(n, dtype=np.float64) * step + b0
    x[-1] = b1
    return x.astype(np.float32)


def _corner_vec(c):
    return np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], dtype=np.float64)


def tetrahedra():
    """Six corner quadruples (cell corner codes, bit 4 = x, 2 = y, 1 = z), each positively oriented."""
    out = []
    for p, q, _ in itertools.permutations((4, 2, 1)):
        t = [0, p, p | q, 7]
        m = np.stack([_corner_vec(t[1]), _corner_vec(t[2]), _corner_vec(t[3])])
        if np.linalg.det(m) < 0:
            t[1], t[2] = t[2], t[1]
        out.append(tuple(t))
    return out


def _even(perm):
    inv = sum(1 for i in range(len(perm)) for j in range(i + 1, len(perm)) if perm[i] > perm[j])
    return inv % 2 == 0


def case_table():
    """mask (bit l = local corner l inside) -> list of triangles, each three local corner pairs (a < b), oriented so that the normal
    leaves the inside corners when the tetrahedron (0, 1, 2, 3) is positively oriented."""
    table = []
    pair = lambda a, b: (min(a, b), max(a, b))
    for mask in range(16):
        ins = [c for c in range(4) if (mask >> c) & 1]
        outs = [c for c in range(4) if not (mask >> c) & 1]
        if len(ins) in (0, 4):
            table.append([])
        elif len(ins) == 1 or len(outs) == 1:
            p = ins[0] if len(ins) == 1 else outs[0]
            q = [c for c in range(4) if c != p]
            tri = [pair(p, q[0]), pair(p, q[1]), pair(p, q[2])]
            # (p, q0, q1, q2) positively oriented <=> the triangle's normal points away from p
            if (len(ins) == 1) != _even((p, q[0], q[1], q[2])):
                tri[1], tri[2] = tri[2], tri[1]
            table.append([tuple(tri)])
        else:
            p1, p2 = ins
            q1, q2 = outs
            A, B, C, D = pair(p1, q1), pair(p1, q2), pair(p2, q2), pair(p2, q1)
            if _even((p1, p2, q1, q2)):
                table.append([(A, B, C), (A, C, D)])
            else:
                table.append([(A, C, B), (A, D, C)])
    return table


def _offsets(c):
    return (c >> 2) & 1, (c >> 1) & 1, c & 1


def extract(grid, b0, b1, level=0.0):
    """grid [nx, ny, nz] (any float dtype; used as float64), b0 / b1 the bounds per axis (scalars or 3-vectors).
    -> verts float64 [nv, 3], faces int64 [nf, 3]."""
    g = np.asarray(grid, dtype=np.float64)
    nx, ny, nz = g.shape
    b0 = np.broadcast_to(np.asarray(b0, dtype=np.float64), (3,))
    b1 = np.broadcast_to(np.asarray(b1, dtype=np.float64), (3,))
    axes = [linspace_f32(b0[a], b1[a], g.shape[a]).astype(np.float64) for a in range(3)]
    level = float(level)
    inside = g < level
    finite = np.isfinite(g)
    cross = np.zeros((nx, ny, nz, 7), dtype=bool)
    for c in range(7):
        dx, dy, dz = _offsets(c + 1)
        lo = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        hi = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        cross[lo + (c,)] = (inside[lo] != inside[hi]) & finite[lo] & finite[hi]
    flat = cross.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int64) - 1).reshape(nx, ny, nz, 7)
    sel = np.nonzero(flat)[0]
    node, cls = sel // 7, sel % 7
    i, j, k = node // (ny * nz), (node // nz) % ny, node % nz
    d = np.array([_offsets(c + 1) for c in range(7)], dtype=np.int64)[cls]
    i2, j2, k2 = i + d[:, 0], j + d[:, 1], k + d[:, 2]
    pa = np.stack([axes[0][i], axes[1][j], axes[2][k]], axis=1)
    pb = np.stack([axes[0][i2], axes[1][j2], axes[2][k2]], axis=1)
    va, vb = g[i, j, k], g[i2, j2, k2]
    a_in = va < level
    ps, pe = np.where(a_in[:, None], pa, pb), np.where(a_in[:, None], pb, pa)
    vs, ve = np.where(a_in, va, vb), np.where(a_in, vb, va)
    t = (level - vs) / (ve - vs)
    verts = ps + t[:, None] * (pe - ps)

    cx, cy, cz = nx - 1, ny - 1, nz - 1
    if min(cx, cy, cz) < 1:
        return verts, np.zeros((0, 3), dtype=np.int64)
    corner_in, corner_fin = [], []
    for c in range(8):
        dx, dy, dz = _offsets(c)
        s = (slice(dx, dx + cx), slice(dy, dy + cy), slice(dz, dz + cz))
        corner_in.append(inside[s])
        corner_fin.append(finite[s])
    table = case_table()
    ntri = np.array([len(t_) for t_ in table])
    lut = np.zeros((16, 2, 3, 2), dtype=np.int64)
    for m, tris in enumerate(table):
        for s, tri in enumerate(tris):
            for v, (a, b) in enumerate(tri):
                lut[m, s, v] = (a, b)
    ci, cj, ck = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    faces = np.zeros((cx, cy, cz, 6, 2, 3), dtype=np.int64)
    valid = np.zeros((cx, cy, cz, 6, 2), dtype=bool)
    for ti, tet in enumerate(tetrahedra()):
        mask = sum(corner_in[tet[l]].astype(np.int64) << l for l in range(4))
        fin = corner_fin[tet[0]] & corner_fin[tet[1]] & corner_fin[tet[2]] & corner_fin[tet[3]]
        tet_a = np.array(tet, dtype=np.int64)
        for s in range(2):
            ok = fin & (ntri[mask] > s)
            valid[..., ti, s] = ok
            for v in range(3):
                ca, cb = tet_a[lut[mask, s, v, 0]], tet_a[lut[mask, s, v, 1]]
                lo, hi = np.minimum(ca, cb), np.maximum(ca, cb)
                oi, oj, ok_ = ci + ((lo >> 2) & 1), cj + ((lo >> 1) & 1), ck + (lo & 1)
                idx = vid[oi, oj, ok_, np.maximum((lo ^ hi) - 1, 0)]
                faces[..., ti, s, v] = np.where(ok, idx, 0)
    return verts, faces[valid]


# ---- mesh analysis shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def edge_report(faces):
    """-> (number of undirected edges, mask over them: in exactly two faces with opposite directions, the undirected edges [ne, 2])."""
    e = directed_edges(faces)
    und = np.sort(e, axis=1)
    sign = np.where(e[:, 0] < e[:, 1], 1, -1)
    uniq, inv = np.unique(und, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    count = np.bincount(inv, minlength=len(uniq))
    ssum = np.bincount(inv, weights=sign, minlength=len(uniq))
    return len(uniq), (count == 2) & (ssum == 0), uniq


def euler(nv, faces):
    ne, _, _ = edge_report(faces)
    return int(nv) - ne + len(faces)


def components(nv, faces):
    """Label per vertex = the lowest vertex index of its connected component (min-label propagation over the faces)."""
    f = np.asarray(faces, dtype=np.int64)
    label = np.arange(nv, dtype=np.int64)
    while True:
        m = label[f].min(axis=1)
        new = label.copy()
        for c in range(3):
            np.minimum.at(new, f[:, c], m)
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def face_normals(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def read_ply(path):
    """Minimal reader of the binary little-endian PLY that neat_amd.ply.write_ply writes -> (verts, normals or None, faces)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    nv = nf = 0
    props, element = [], None
    for ln in lines:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nf = int(w[2])
        elif w[0] == "property" and element == "vertex":
            assert w[1] == "float", ln
            props.append(w[2])
        elif w[0] == "property" and element == "face":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"], ln
    body = data[end:]
    vbytes = nv * len(props) * 4
    v = np.frombuffer(body[:vbytes], dtype="<f4").reshape(nv, len(props))
    rec = np.frombuffer(body[vbytes:], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert len(rec) == nf and len(body) == vbytes + nf * 13 and (rec["n"] == 3).all()
    assert props[:3] == ["x", "y", "z"]
    normals = v[:, 3:6].copy() if props[3:6] == ["nx", "ny", "nz"] else None
    return v[:, :3].copy(), normals, rec["i"].copy()
