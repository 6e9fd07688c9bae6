"""PLY and OBJ files: the one reader of the tools, the mesh writers (neat_amd.mesh, the trainer's --vis_mesh, neat_amd.scenegen) and the
cloud writer (neat_amd.evaluate).  tests/mesh_f64.read_ply is the tests' own, independent reader."""
import numpy as np
import torch

from .run_io import replace_file


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """-> dict(points float64 [n,3], faces int32 [m,3] or None, normals / colors or None).  ascii and binary little-endian; vertex
    properties beyond x y z are read by name (nx ny nz, red green blue); faces are a list property of 3 indices each."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elements = None, []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append({"name": tok[1], "count": int(tok[2]), "props": []})
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1]["props"].append(("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]], tok[4]))
                else:
                    elements[-1]["props"].append(("scalar", _PLY_TYPES[tok[1]], None, tok[2]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError("%s: format %s is not read (ascii, binary_little_endian)" % (path, fmt))
        out = {"points": None, "faces": None, "normals": None, "colors": None}
        ascii_rows = fh.read().decode("ascii").split("\n") if fmt == "ascii" else None
        row = 0
        for el in elements:
            n, props = el["count"], el["props"]
            has_list = any(p[0] == "list" for p in props)
            if not has_list:
                dt = np.dtype([(p[3], "<" + p[1]) for p in props])
                if fmt == "ascii":
                    tab = np.array([r.split() for r in ascii_rows[row:row + n]], dtype=np.float64).reshape(n, len(props))
                    row += n
                    col = {p[3]: tab[:, k] for k, p in enumerate(props)}
                else:
                    rec = np.frombuffer(fh.read(dt.itemsize * n), dtype=dt, count=n)
                    col = {p[3]: rec[p[3]] for p in props}
                if el["name"] == "vertex":
                    out["points"] = np.stack([col["x"], col["y"], col["z"]], 1).astype(np.float64)
                    if all(k in col for k in ("nx", "ny", "nz")):
                        out["normals"] = np.stack([col["nx"], col["ny"], col["nz"]], 1).astype(np.float64)
                    if all(k in col for k in ("red", "green", "blue")):
                        out["colors"] = np.stack([col["red"], col["green"], col["blue"]], 1)
            else:
                if len(props) != 1:
                    raise ValueError("%s: element %s mixes a list with other properties" % (path, el["name"]))
                _, ct, it, _ = props[0]
                if fmt == "ascii":
                    rows = [r.split() for r in ascii_rows[row:row + n]]
                    row += n
                    if any(int(r[0]) != 3 for r in rows):
                        raise ValueError("%s: only triangles are read" % path)
                    lists = np.array([r[1:4] for r in rows], dtype=np.int64).reshape(n, 3)
                else:
                    dt = np.dtype([("n", "<" + ct), ("i", "<" + it, (3,))])
                    rec = np.frombuffer(fh.read(dt.itemsize * n), dtype=dt, count=n)
                    if n and not (rec["n"] == 3).all():
                        raise ValueError("%s: only triangles are read" % path)
                    lists = rec["i"]
                if el["name"] == "face":
                    out["faces"] = lists.astype(np.int32).reshape(n, 3)
        if out["points"] is None:
            raise ValueError("%s: no vertex element" % path)
        return out


def read_obj(path):
    """A Wavefront OBJ -> (verts float64 [nv,3], faces int32 [nf,3], zero-based).  `v x y z [...]` and `f` records are read, everything else
    is skipped; an index is `i`, `i/j`, `i//k` or `i/j/k` (the vertex index is the first), a negative one counts back from the vertices
    read so far; a polygon becomes the fan about its first corner."""
    verts, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    if i == 0:
                        raise ValueError("%s: OBJ indices start at 1" % path)
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)


def read_mesh(path):
    """A .ply or .obj mesh -> (verts float64 [nv,3], faces int32 [nf,3])."""
    if path.lower().endswith(".obj"):
        return read_obj(path)
    m = read_ply(path)
    if m["faces"] is None:
        raise ValueError("%s: no faces" % path)
    return m["points"], m["faces"]


def write_obj(path, verts, faces):
    """A Wavefront OBJ that read_obj reads back to the same float64 values."""
    def write(tmp):
        with open(tmp, "w") as fh:
            fh.write("# neat_amd.scenegen\n")
            fh.writelines("v %r %r %r\n" % tuple(float(x) for x in v) for v in np.asarray(verts, dtype=np.float64).reshape(-1, 3))
            fh.writelines("f %d %d %d\n" % tuple(int(i) + 1 for i in f) for f in np.asarray(faces).reshape(-1, 3))
    replace_file(path, write)


def write_ply(path, verts, faces, normals=None):
    """Binary little-endian PLY: float32 x y z [nx ny nz] per vertex, `uchar 3 + 3 x int32` per face."""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    cols = [v]
    header = ["ply", "format binary_little_endian 1.0", "comment neat_amd.mesh: SDF level surface, marching tetrahedra",
              "element vertex %d" % v.shape[0], "property float x", "property float y", "property float z"]
    if normals is not None:
        n = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("write_ply: one normal per vertex")
        cols.append(n)
        header += ["property float nx", "property float ny", "property float nz"]
    header += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"] = 3
    rec["i"] = f

    def write(tmp):
        with open(tmp, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(np.concatenate(cols, axis=1).astype("<f4").tobytes())
            fh.write(rec.tobytes())
    replace_file(path, write)


def write_ply_cloud(path, points, colors=None):
    """Binary little-endian PLY of a cloud: double x y z and, given colours in [0, 1], uchar red green blue (what open3d writes)."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64)).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    header = ["ply", "format binary_little_endian 1.0", "comment neat_amd.evaluate", "element vertex %d" % p.shape[0],
              "property double x", "property double y", "property double z"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(p.shape[0], dtype=fields)
    rec["x"], rec["y"], rec["z"] = p[:, 0], p[:, 1], p[:, 2]
    if colors is not None:
        c = np.floor(np.clip(np.asarray(colors, dtype=np.float64).reshape(-1, 3), 0, 1) * 255.0 + 0.5).astype(np.uint8)      # rounded, as open3d does
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
