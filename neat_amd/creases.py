"""The crease lines of a triangle mesh, made on the device: the junctions and straight edges of a model read from its triangles alone, in
the format of a scene's lines.json, which scenegen (--lines), raycast analysis and evaluate abc start from.

    python -m neat_amd.creases --mesh M.obj|M.ply --out lines.json [--angle 30] [--turn 1] [--deviation 1e-6] [--no-boundary]
            [--drop-curved] [--min-len 0] [--ply creases.ply] [--gpu 0] [--overwrite]

    res = creases.lines(verts, faces, angle=30.0, turn=1.0, deviation=1e-6)      # Creases, on the device
    creases.write_lines("lines.json", res)                                        # junctions, lines, kind, curved

An edge of two faces is a crease (kind 0) when their normals differ by more than `angle`, an edge of one face is a boundary (kind 1,
kept with `boundary`), an edge of three and more is non-manifold (kind 2).  Feature edges that meet two by two within `turn` degrees of
straight are joined into chains; a chain between two ends whose vertices stay within `deviation` (relative to the diagonal of the
vertices' box) of the segment between them is one line, any other chain comes out edge by edge, marked `curved`.  Vertices are welded by
exact coordinates only.  The rule is DESIGN 3n; csrc/kernels_crease.hpp implements it and tests/creases_f64.py restates it in float64
numpy, which the device equals array for array.  There is no host fallback.
"""
import argparse
import collections
import math
import os
import sys

import numpy as np
import torch

from . import _lib, ply, run_io

KINDS = ("crease", "boundary", "non_manifold")      # the meaning of `kind` 0, 1, 2
DEFAULTS = {"angle": 30.0, "turn": 1.0, "deviation": 1e-6}

Creases = collections.namedtuple("Creases", ["junctions", "lines", "kind", "curved", "vertex", "stats"])
Creases.__doc__ = """On the device: junctions float64 [J,3] (the coordinates as given), in ascending `vertex`; lines int32 [L,2] into them, in
ascending (vertex a, vertex b), then kind, then curved; kind uint8 [L] (0 crease, 1 boundary, 2 non-manifold); curved bool [L]: a piece
of a chain that is not one straight line; vertex int32 [J]: the original vertex index (the lowest of its welded group).  stats: dict
(status, welded, dropped_faces, edges, creases, boundary, non_manifold, chains): status 1 = a face index outside the vertices, 2 = a
non-finite coordinate; everything is then empty."""


def _empty(dev, stats):
    return Creases(torch.zeros(0, 3, device=dev, dtype=torch.float64), torch.zeros(0, 2, device=dev, dtype=torch.int32),
                   torch.zeros(0, device=dev, dtype=torch.uint8), torch.zeros(0, device=dev, dtype=torch.bool),
                   torch.zeros(0, device=dev, dtype=torch.int32), stats)


def _filter(res, keep):
    """The lines with keep [L]; the junctions that one of them still ends at, in their order."""
    lines = res.lines[keep]
    used = torch.unique(lines.reshape(-1).long())                                  # ascending
    index = torch.searchsorted(used, lines.reshape(-1).long()).to(torch.int32).reshape(-1, 2)
    return Creases(res.junctions[used], index, res.kind[keep], res.curved[keep], res.vertex[used], res.stats)


@torch.no_grad()
def lines(verts, faces, angle=DEFAULTS["angle"], turn=DEFAULTS["turn"], deviation=DEFAULTS["deviation"], boundary=True, drop_curved=False,
          min_len=0.0, device=None):
    """verts [nv,3], faces [nf,3] -> Creases on `device`: the one named, else that of a tensor `verts`, else (arrays, lists) the current
    one; a CPU device raises.  angle in (0, 180) degrees, turn in [0, 90], deviation >= 0 relative to the diagonal of the vertices' box;
    drop_curved and min_len (a line with |b - a|^2 < min_len^2 goes) filter the finished list.  Three read-backs: the counts of the
    edges, the box, the counts of the lines."""
    if not (0.0 < float(angle) < 180.0) or not (0.0 <= float(turn) <= 90.0) or not (float(deviation) >= 0.0 and math.isfinite(float(deviation))) or \
            not float(min_len) >= 0.0:
        raise ValueError("creases.lines: 0 < angle < 180, 0 <= turn <= 90, deviation >= 0 and finite, min_len >= 0")
    if device is not None:
        dev = torch.device(device)
    else:
        dev = verts.device if torch.is_tensor(verts) else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("neat_amd.creases runs on the device (there is no CPU path)")
    v = torch.as_tensor(verts).detach().to(dev, torch.float64).reshape(-1, 3).contiguous()
    f = torch.as_tensor(faces).detach().to(dev, torch.int32).reshape(-1, 3).contiguous()
    nv, nf = int(v.shape[0]), int(f.shape[0])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        size = lib.neat_crease_scratch_bytes(nv, nf)
        if size == 0:
            raise ValueError(f"creases.lines: {nv} vertices and {nf} faces are more than the workspace is laid out for")
        ws = torch.empty(size, device=dev, dtype=torch.uint8)
        counts = torch.zeros(8, device=dev, dtype=torch.int32)
        _lib.check(lib.neat_crease_edges(_lib.ptr(v), nv, _lib.ptr(f), nf, math.cos(math.radians(float(angle))), int(bool(boundary)), _lib.ptr(ws),
                                         _lib.ptr(counts), _lib.stream()), "neat_crease_edges")
        status, welded, dropped, E, k0, k1, k2 = (int(x) for x in counts[:7].tolist())
        stats = {"status": status, "welded": welded, "dropped_faces": dropped, "edges": E, "creases": k0, "boundary": k1, "non_manifold": k2, "chains": 0}
        if status != 0 or E == 0:
            return _empty(dev, stats)
        d = [float(x) for x in (v.max(dim=0).values - v.min(dim=0).values).tolist()]
        length = float(deviation) * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        _lib.check(lib.neat_crease_chains(_lib.ptr(v), nv, nf, E, math.sin(math.radians(float(turn))) ** 2, length, _lib.ptr(ws), _lib.ptr(counts),
                                          _lib.stream()), "neat_crease_chains")
        stats["chains"], L, J = (int(x) for x in counts[:3].tolist())
        junctions = torch.empty(J, 3, device=dev, dtype=torch.float64)
        vertex = torch.empty(J, device=dev, dtype=torch.int32)
        pairs = torch.empty(L, 2, device=dev, dtype=torch.int32)
        kind, curved = torch.empty(L, device=dev, dtype=torch.uint8), torch.empty(L, device=dev, dtype=torch.uint8)
        _lib.check(lib.neat_crease_fill(_lib.ptr(v), nv, nf, E, _lib.ptr(ws), L, J, _lib.ptr(junctions), _lib.ptr(vertex), _lib.ptr(pairs),
                                        _lib.ptr(kind), _lib.ptr(curved), _lib.stream()), "neat_crease_fill")
        res = Creases(junctions, pairs, kind, curved != 0, vertex, stats)
        if drop_curved:
            res = _filter(res, ~res.curved)
        if float(min_len) > 0.0:
            e = res.junctions[res.lines[:, 1].long()] - res.junctions[res.lines[:, 0].long()]
            res = _filter(res, ~((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] < float(min_len) * float(min_len)))
    return res


# ------------------------------------------------------------------ files
def _host(x):
    return np.asarray(torch.as_tensor(x).detach().cpu().numpy())


def write_lines(path, res):
    """lines.json: `junctions` [J,3] and `lines` [L,2] as scenegen.read_lines, raycast.scan_wireframe and evaluate abc read them, and
    `kind`, `curved` [L] beside them.  Floats are written with repr, so they read back to the same float64.  Written to a .tmp beside
    the file and moved into place."""
    run_io.write_json(path, {"junctions": [[float(x) for x in p] for p in _host(res.junctions).reshape(-1, 3)],
                             "lines": [[int(a), int(b)] for a, b in _host(res.lines).reshape(-1, 2)],
                             "kind": [int(k) for k in _host(res.kind).reshape(-1)], "curved": [bool(c) for c in _host(res.curved).reshape(-1)]})


def write_tubes(path, res, radius):
    """The lines as a triangle mesh, a three-sided tube of `radius` around each, through ply.write_ply: what show --mesh reads."""
    J, pairs = _host(res.junctions).reshape(-1, 3), _host(res.lines).reshape(-1, 2)
    a, b = J[pairs[:, 0]], J[pairs[:, 1]]
    axis = b - a
    axis = axis / np.maximum(np.linalg.norm(axis, axis=1, keepdims=True), 1e-300)
    helper = np.where(np.abs(axis[:, :1]) < 0.9, np.asarray([[1.0, 0.0, 0.0]]), np.asarray([[0.0, 1.0, 0.0]]))
    u = np.cross(axis, helper)
    u = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-300)
    w = np.cross(axis, u)
    ring = [math.cos(2.0 * math.pi * k / 3.0) * u + math.sin(2.0 * math.pi * k / 3.0) * w for k in range(3)]
    verts = np.stack([a + radius * r for r in ring] + [b + radius * r for r in ring], axis=1).reshape(-1, 3)      # six per line
    local = [(0, 2, 1), (3, 4, 5)] + [t for k in range(3) for t in ((k, (k + 1) % 3, 3 + (k + 1) % 3), (k, 3 + (k + 1) % 3, 3 + k))]
    faces = (6 * np.arange(len(pairs))[:, None, None] + np.asarray(local)[None]).reshape(-1, 3)
    ply.write_ply(path, verts, faces)


# ------------------------------------------------------------------ command line
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.creases", description="the crease lines of a triangle mesh as a lines.json, on the device")
    ap.add_argument("--mesh", type=str, required=True, help="a .obj or .ply triangle mesh")
    ap.add_argument("--out", type=str, required=True, help="the lines.json to write")
    ap.add_argument("--angle", type=float, default=DEFAULTS["angle"], help="degrees between the normals of two faces from which their edge is a crease")
    ap.add_argument("--turn", type=float, default=DEFAULTS["turn"], help="degrees by which a chain may turn at a vertex and go on")
    ap.add_argument("--deviation", type=float, default=DEFAULTS["deviation"],
                    help="how far a straight chain's vertices may lie from its segment, relative to the diagonal of the mesh's box")
    ap.add_argument("--no-boundary", default=False, action="store_true", help="leave out the edges of one face")
    ap.add_argument("--drop-curved", default=False, action="store_true", help="leave out the pieces of chains that are not straight")
    ap.add_argument("--min-len", type=float, default=0.0, help="leave out lines shorter than this")
    ap.add_argument("--ply", type=str, default=None, help="also write the lines as thin tubes, a .ply that show --mesh reads")
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    ap.add_argument("--overwrite", default=False, action="store_true", help="replace an existing --out")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    if os.path.splitext(opt.mesh)[1].lower() not in (".ply", ".obj"):
        ap.error("--mesh is a .ply or an .obj file")
    if opt.ply is not None and os.path.splitext(opt.ply)[1].lower() != ".ply":
        ap.error("--ply is a .ply file")
    if not 0.0 < opt.angle < 180.0:
        ap.error("0 < --angle < 180")
    if not 0.0 <= opt.turn <= 90.0 or not (opt.deviation >= 0.0 and math.isfinite(opt.deviation)) or not opt.min_len >= 0.0 or opt.gpu < 0:
        ap.error("0 <= --turn <= 90, --deviation >= 0, --min-len >= 0, --gpu >= 0")
    return opt


def main(argv=None):
    opt = parse_args(argv)
    if run_io.skip_existing(opt.out, opt.overwrite):
        return 0
    _lib.lib()
    verts, faces = ply.read_mesh(opt.mesh)
    torch.cuda.set_device(opt.gpu)
    res = lines(verts, faces, angle=opt.angle, turn=opt.turn, deviation=opt.deviation, boundary=not opt.no_boundary, drop_curved=opt.drop_curved,
                min_len=opt.min_len, device=torch.device("cuda", opt.gpu))
    if res.stats["status"] != 0:
        raise ValueError("the mesh: " + ("a face index lies outside the vertices" if res.stats["status"] == 1 else "a coordinate is not finite"))
    write_lines(opt.out, res)
    if opt.ply is not None:
        span = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
        write_tubes(opt.ply, res, 0.002 * float(np.linalg.norm(span.max(axis=0) - span.min(axis=0))) if len(span) else 0.0)
    s = res.stats
    print("{}: {} lines ({} curved) between {} junctions from {} triangles: {} creases, {} boundary and {} non-manifold edges in {} chains; "
          "{} vertices welded to {}, {} faces dropped".format(opt.out, int(res.lines.shape[0]), int(res.curved.sum().item()), int(res.junctions.shape[0]),
                                                              int(np.asarray(faces).reshape(-1, 3).shape[0]), s["creases"], s["boundary"], s["non_manifold"],
                                                              s["chains"], int(np.asarray(verts).reshape(-1, 3).shape[0]), s["welded"], s["dropped_faces"]),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
