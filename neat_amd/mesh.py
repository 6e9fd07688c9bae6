"""The surface the SDF network learnt, as a triangle mesh (the reference's plots.get_surface_trace, code/utils/plots.py:101-138, which
training writes as `plots/surface_{epoch}.ply`; its evaluation scripts build the 512^3 version, :140-218):

    python -m neat_amd.mesh --conf <run>/runconf.conf [--checkpoint latest] [--resolution 100] [--grid-boundary -1.5 1.5] [--level 0]
                            [--largest-component] [--expdir <run>] [--gpu 0] [--precision fp32] [--overwrite]

The grid is evaluated on the device in chunks whose query points are written straight into the SDF kernels' layout (no [N, 3] point
tensor), and the level set is extracted on the device by marching tetrahedra (csrc/kernels_mesh.hpp) -- not the reference's
marching cubes (skimage, host): the two meshes are iso-surfaces of two interpolants of the same grid values, within one cell diagonal
of each other, and are not equal vertex for vertex.  There is no host fallback.

Defaults of resolution and grid_boundary are the conf's `plot` block (100 and [-1.5, 1.5] in every shipped conf).  The checkpoint is read
from `<run>/checkpoints/ModelParameters/<checkpoint>.pth` (run = the conf's directory, or --expdir); the file written is
`<run>/plots/surface_{epoch}.ply` (binary little-endian PLY: vertices, optional unit normals = the normalised SDF gradient at the
vertices, triangles).  A grid whose values are all above or all below the level writes nothing and says so (plots.py:110).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

DEFAULT_RESOLUTION = 100
DEFAULT_BOUNDARY = (-1.5, 1.5)
DEFAULT_CHUNK = 262144          # grid nodes per SDF query


def linspace_f32(b0, b1, n):
    """Node coordinates of one axis on the host: float32(b0 + i (b1 - b0) / (n - 1)) evaluated in float64, the last node exactly b1
    (= numpy.linspace(b0, b1, n).astype(float32), get_grid_uniform, plots.py:322-324; the device kernels use the same arithmetic)."""
    if n < 2:
        raise ValueError("an axis needs at least 2 nodes")
    b0, b1 = float(b0), float(b1)
    x = np.arange(n, dtype=np.float64) * ((b1 - b0) / (n - 1)) + b0
    x[-1] = b1
    return x.astype(np.float32)


def _shape3(resolution):
    if isinstance(resolution, (int, np.integer)):
        return (int(resolution),) * 3
    shape = tuple(int(v) for v in resolution)
    if len(shape) != 3:
        raise ValueError("resolution: an int or (nx, ny, nz)")
    return shape


def _bounds3(grid_boundary):
    """(lo, hi) scalars as in the conf's plot block, or ((x0, y0, z0), (x1, y1, z1)) -> two tuples of three floats."""
    lo, hi = grid_boundary
    three = lambda v: tuple(float(e) for e in v) if hasattr(v, "__len__") else (float(v),) * 3
    lo, hi = three(lo), three(hi)
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("grid_boundary: (lo, hi) with scalars or 3-vectors")
    return lo, hi


def _implicit(model):
    return getattr(model, "implicit_network", model)


@torch.no_grad()
def sdf_grid(model, resolution=DEFAULT_RESOLUTION, grid_boundary=DEFAULT_BOUNDARY, chunk=DEFAULT_CHUNK):
    """get_sdf_vals on the nodes of a uniform grid -> float32 device tensor [nx, ny, nz] (x slowest), in the model's own precision.
    `chunk` nodes per query (rounded up to the SDF kernels' point tile); the workspace is sized once, for one chunk."""
    from . import ops
    net = _implicit(model)
    shape = _shape3(resolution)
    lo, hi = _bounds3(grid_boundary)
    if min(shape) < 2:
        raise ValueError("sdf_grid: every axis needs at least 2 nodes")
    handle = net.handle()
    dev = next(net.parameters()).device
    total = shape[0] * shape[1] * shape[2]
    grid = torch.empty(shape, device=dev, dtype=torch.float32)
    flat = grid.view(-1)
    ws, ldp = ops.sdf_query_workspace(handle, max(1, min(int(chunk), total)), dev)
    chunk = ldp                                             # a whole multiple of the point tile
    for first in range(0, total, chunk):
        count = min(chunk, total - first)
        stride = ldp if count == chunk else ops._lib.lib().neat_sdf_ldp(count, handle.precision)      # the ragged last chunk: its own stride
        ops.grid_points(ws, stride, first, count, shape, lo, hi)
        ops.sdf_values_laid_out(handle, ws, count, net.sdf_bounding_sphere, net.sphere_scale, out=flat[first:first + count])
    return grid


def extract(grid, b0, b1, level=0.0):
    """Marching tetrahedra on ANY float32 device grid [nx, ny, nz] whose node (i, j, k) sits at linspace_f32 per axis over [b0, b1]
    (scalars or 3-vectors) -> (verts [nv, 3] float32, faces [nf, 3] int32) on the device.  Vertices ascend by (node, edge class), faces
    by (cell, tetrahedron, triangle); face normals point towards increasing values.  Two runs give the same bytes."""
    from . import ops
    return ops.mesh_extract(grid, b0, b1, level)


def face_components(faces, n_verts):
    """Label per face = the lowest vertex index of its connected component (min-label propagation over the faces, integer ops on the
    device; a few dozen rounds of pointer jumping)."""
    f = faces.long()
    label = torch.arange(n_verts, device=faces.device)
    while True:
        m = label[f].min(dim=1).values
        new = label.clone()
        for c in range(3):
            new.scatter_reduce_(0, f[:, c], m, reduce="amin")
        new = new[new]
        if torch.equal(new, label):
            return label[f[:, 0]]
        label = new


def keep_largest_component(verts, faces):
    """The connected component with the largest area (plots.py:163-166), vertices re-indexed in their order -> (verts, faces, kept vertex index)."""
    if faces.shape[0] == 0:
        return verts, faces, torch.arange(verts.shape[0], device=verts.device)
    lab = face_components(faces, verts.shape[0])
    v = verts.double()
    f = faces.long()
    area = 0.5 * torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).norm(dim=1)
    total = torch.zeros(verts.shape[0], device=verts.device, dtype=torch.float64).index_add_(0, lab, area)
    keep_f = lab == torch.argmax(total)
    f = f[keep_f]
    used = torch.zeros(verts.shape[0], device=verts.device, dtype=torch.bool)
    used[f.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    return verts[used].contiguous(), new_index[f].to(torch.int32).contiguous(), torch.nonzero(used).flatten()


def vertex_normals(model, verts, chunk=65536):
    """Unit normals = the SDF network's gradient at the vertices (ops.sdf_point_normals), normalised on the device."""
    from . import ops
    net = _implicit(model)
    out = torch.empty_like(verts)
    with torch.no_grad():
        for i0 in range(0, verts.shape[0], chunk):
            _, g = ops.sdf_point_normals(net.handle(), verts[i0:i0 + chunk].contiguous(), net.sdf_bounding_sphere, net.sphere_scale)
            out[i0:i0 + chunk] = g
    return ops.unit_rows3_(out) if out.shape[0] else out


def surface(model, resolution=None, grid_boundary=None, level=0.0, largest_component=False, normals=True, plot_conf=None,
            chunk=DEFAULT_CHUNK, timings=None):
    """-> dict(verts, faces, normals or None) on the device, or None if no cell of the grid crosses the level (plots.py:110).
    resolution / grid_boundary default to plot_conf (the conf's `plot` block), then to 100 and [-1.5, 1.5]."""
    plot_conf = plot_conf or {}
    if resolution is None:
        resolution = int(plot_conf.get("resolution", DEFAULT_RESOLUTION))
    if grid_boundary is None:
        grid_boundary = tuple(plot_conf.get("grid_boundary", DEFAULT_BOUNDARY))
    lo, hi = _bounds3(grid_boundary)
    dev = next(_implicit(model).parameters()).device
    sync = (lambda: torch.cuda.synchronize(dev)) if timings is not None else (lambda: None)
    sync()
    t0 = time.perf_counter()
    grid = sdf_grid(model, resolution, (lo, hi), chunk=chunk)
    sync()
    t1 = time.perf_counter()
    verts, faces = extract(grid, lo, hi, level)         # (its read of the two counts is the synchronisation)
    t2 = time.perf_counter()
    if timings is not None:
        timings.update(grid_s=t1 - t0, extract_s=t2 - t1)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return None
    if largest_component:
        verts, faces, _ = keep_largest_component(verts, faces)
    nrm = vertex_normals(model, verts) if normals else None
    return {"verts": verts, "faces": faces, "normals": nrm}


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
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(np.concatenate(cols, axis=1).astype("<f4").tobytes())
        fh.write(rec.tobytes())
    os.replace(tmp, path)


def out_path(run_dir, epoch):
    """`<run>/plots/surface_{epoch}.ply`: the reference's name (plots.py:37-38, :131-134)."""
    return os.path.join(run_dir, "plots", "surface_{}.ply".format(epoch))


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.mesh")
    ap.add_argument("--conf", type=str, required=True)
    ap.add_argument("--checkpoint", default="latest", type=str, help="the trained model checkpoint to mesh")
    ap.add_argument("--resolution", default=None, type=int, help="grid nodes per axis (default: the conf's plot.resolution)")
    ap.add_argument("--grid-boundary", default=None, type=float, nargs=2, metavar=("LO", "HI"), help="default: the conf's plot.grid_boundary")
    ap.add_argument("--level", default=0.0, type=float)
    ap.add_argument("--largest-component", default=False, action="store_true", help="keep the component with the largest area")
    ap.add_argument("--no-normals", default=False, action="store_true", help="write no vertex normals")
    ap.add_argument("--expdir", default=None, help="run directory holding checkpoints/ (default: the conf's directory)")
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    ap.add_argument("--precision", choices=["fp32", "bf16", "bf16x3", "fp16", "fp16x3"], default=None)
    ap.add_argument("--overwrite", default=False, action="store_true", help="write even if the .ply exists")
    return ap


def plot_block(conf):
    """The conf's `plot` block as a plain dict (empty if absent)."""
    return dict(conf.get("plot", None) or {})


def load(conf_path, checkpoint, device, expdir=None, precision=None):
    """-> (model with the checkpoint loaded strictly, its epoch, run directory, the conf's plot block)."""
    from . import conf as conf_mod
    from .general import get_class
    from .runner import CLASS_MAP
    conf = conf_mod.parse_file(conf_path)
    root = expdir or os.path.dirname(os.path.abspath(conf_path))
    name = conf.get_string("train.model_class")
    model = get_class(CLASS_MAP.get(name, name))(conf=conf.get_config("model")).to(device)
    if precision is not None:
        model.set_precision(precision)
    path = os.path.join(root, "checkpoints", "ModelParameters", str(checkpoint) + ".pth")
    print("Checkpoint: {}".format(path), flush=True)
    state = torch.load(path, map_location=device)
    model.load_state_dict(state["model_state_dict"], strict=True)
    model.eval()
    return model, state["epoch"], root, plot_block(conf)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    model, epoch, root, plot = load(opt.conf, opt.checkpoint, device, opt.expdir, opt.precision)
    path = out_path(root, epoch)
    if os.path.exists(path) and not opt.overwrite:
        print("exists: {} (--overwrite to replace it)".format(path), flush=True)
        return 0
    timings = {}
    res = surface(model, opt.resolution, tuple(opt.grid_boundary) if opt.grid_boundary else None, level=opt.level,
                  largest_component=opt.largest_component, normals=not opt.no_normals, plot_conf=plot, timings=timings)
    if "grid_s" in timings:
        print("grid evaluation {:.3f} s, extraction {:.3f} s".format(timings["grid_s"], timings["extract_s"]), flush=True)
    if res is None:
        print("the grid does not cross level {}: no surface, nothing written".format(opt.level), flush=True)
        return 0
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_ply(path, res["verts"], res["faces"], res["normals"])
    print("{}: {} vertices, {} faces".format(path, res["verts"].shape[0], res["faces"].shape[0]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
