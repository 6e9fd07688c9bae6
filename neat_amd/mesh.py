"""The surface the SDF network learnt, as a triangle mesh (the reference's plots.get_surface_trace, code/utils/plots.py:101-138, which
training writes as `plots/surface_{epoch}.ply`; its evaluation scripts build the 512^3 version, :140-218):

    python -m neat_amd.mesh --conf <run>/runconf.conf [--checkpoint latest] [--resolution 100] [--grid-boundary -1.5 1.5] [--level 0]
                            [--largest-component] [--expdir <run>] [--gpu 0] [--precision fp32] [--overwrite]
    python -m neat_amd.mesh --conf <run>/runconf.conf --eval [--resolution 512] [--bbox bbs.npz --scan_id N | --bbox-values x0 y0 z0 x1 y1 z1]
                            [--cams cameras.npz] [--no-world] [--all-components] [--normals]

--eval writes the mesh the reference's evaluation scores (eval_surface below; evaluation/eval.py:132-162) as `<run>/{epoch}/scan{id}.ply`,
ready for `python -m neat_amd.evaluate dtu-mesh --data`.

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

from . import ply
from ._lib import PRECISIONS
from .run_io import implicit_network_of, load_model, skip_existing

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


@torch.no_grad()
def sdf_grid(model, resolution=DEFAULT_RESOLUTION, grid_boundary=DEFAULT_BOUNDARY, chunk=DEFAULT_CHUNK, frame=None):
    """get_sdf_vals on the nodes of a uniform grid -> float32 device tensor [nx, ny, nz] (x slowest), in the model's own precision.
    `chunk` nodes per query (rounded up to the SDF kernels' point tile); the workspace is sized once, for one chunk.
    frame = (R [3,3], c [3]) float64 on the host: the grid is laid out in the local coordinates p of that frame and node p is queried at
    c + R^T p (ops.grid_points_affine); without it the nodes are queried where they are."""
    from . import ops
    net = implicit_network_of(model)
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
        if frame is None:
            ops.grid_points(ws, stride, first, count, shape, lo, hi)
        else:
            ops.grid_points_affine(ws, stride, first, count, shape, lo, hi, frame[0], frame[1])
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
    net = implicit_network_of(model)
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
    dev = next(implicit_network_of(model).parameters()).device
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


# ---- the evaluation mesh (plots.get_surface_high_res_mesh :140-218 / get_surface_by_grid(higher_res=True) :221-316, eval.py:132-162) ----
EVAL_RESOLUTION = 512
COARSE_RESOLUTION = 100          # the first mesh, which gives the frame (plots.py:142, :229)
DTU_BBOX_QUIRK = np.array([[1.5], [1.0]])      # get_surface_by_grid multiplies the npz's min row by 1.5 and its max row by 1.0 (plots.py:222)


def principal_frame(verts, faces):
    """The principal axes of a surface -> (R [3,3], mean [3]) float64 on the host.  The moments are the exact surface integrals
    (ops.mesh_moments; the reference estimates them from 10 000 unseeded random surface samples, plots.py:168-175) about the vertex
    bounding-box centre o: C = M2 / A - m m^T, mean = o + m.  Rows of R = eigenvectors of C by ascending eigenvalue, each with its
    largest-magnitude entry positive; if det R < 0 rows 1 and 2 are swapped (plots.py:176-177)."""
    from . import ops
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("principal_frame: an empty mesh has no frame")
    box = ops.affine_bounds3(verts, np.eye(3, 4)).cpu().numpy()
    o = 0.5 * (box[:3] + box[3:])
    return frame_from_moments(ops.mesh_moments(verts, faces, o), o)


def frame_from_moments(mom, o):
    """(area, first moments [3], second moments xx xy xz yy yz zz) about o -> (R, mean); the host half of principal_frame."""
    mom, o = np.asarray(mom, dtype=np.float64), np.asarray(o, dtype=np.float64)
    area = mom[0]
    if not area > 0:
        raise ValueError("principal_frame: the mesh has no area")
    m = mom[1:4] / area
    xx, xy, xz, yy, yz, zz = mom[4:10] / area
    C = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - np.outer(m, m)
    _, vec = np.linalg.eigh(C)                               # ascending eigenvalues, eigenvectors in columns
    R = vec.T.copy()
    for r in range(3):
        if R[r, np.argmax(np.abs(R[r]))] < 0:
            R[r] = -R[r]
    if np.linalg.det(R) < 0:
        R = R[[0, 2, 1]]
    return R, o + m


def _aligned_axes(lo, hi, resolution, eps):
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or any(not h > l for l, h in zip(lo, hi)):
        raise ValueError("aligned_grid: a box with three positive extents")
    if resolution < 2:
        raise ValueError("aligned_grid: the shortest axis needs at least 2 nodes")
    s = int(np.argmin([h - l for l, h in zip(lo, hi)]))
    start_s, stop_s = lo[s] - eps, hi[s] + eps
    h = (stop_s - start_s) / (resolution - 1)
    shape, lo3, hi3 = [0] * 3, [0.0] * 3, [0.0] * 3
    for a in range(3):
        if a == s:
            shape[a], lo3[a], hi3[a] = int(resolution), start_s, stop_s
        else:
            start, stop = lo[a] - eps, hi[a] + h + eps
            shape[a] = int(np.ceil((stop - start) / h))      # numpy.arange's length rule
            lo3[a], hi3[a] = start, start + (shape[a] - 1) * h
    return tuple(shape), tuple(lo3), tuple(hi3)


def aligned_grid(lo, hi, resolution, eps):
    """get_grid (plots.py:331-362) -> (shape, lo3, hi3): the shortest axis of the box [lo, hi] gets `resolution` nodes over
    [lo_s - eps, hi_s + eps] (numpy.linspace), spacing h; every other axis starts at lo_a - eps and has numpy.arange's
    ceil(((hi_a + h + eps) - (lo_a - eps)) / h) nodes, the last one at lo3_a + (n_a - 1) h.  The nodes of the long axes follow the
    linspace rule of the kernels over [lo3_a, hi3_a], not arange's start + i h: equal within one float32 ulp.
    A grid of 2^31 nodes or more raises, naming the largest resolution that fits."""
    shape, lo3, hi3 = _aligned_axes(lo, hi, int(resolution), float(eps))
    nodes = lambda r: int(np.prod([int(n) for n in _aligned_axes(lo, hi, r, float(eps))[0]], dtype=object))
    if nodes(int(resolution)) >= 2 ** 31:
        fit, top = 2, int(resolution)
        while top - fit > 1:                                 # nodes(r) grows with r
            mid = (fit + top) // 2
            fit, top = (mid, top) if nodes(mid) < 2 ** 31 else (fit, mid)
        raise ValueError("aligned_grid: resolution {} gives a grid of {} x {} x {} nodes, 2^31 or more; the largest resolution that fits "
                         "this box is {}".format(resolution, shape[0], shape[1], shape[2], fit))
    return shape, lo3, hi3


def clip_box(verts, faces, lo, hi):
    """The part of a mesh inside the axis-aligned box [lo, hi] (float32 values), uncapped (trimesh's slice_plane(cap=False),
    plots.py:307-314): six half-spaces one after the other, x >= lo, x <= hi, y >= lo, y <= hi, z >= lo, z <= hi (ops.mesh_cut).
    -> (verts, faces); an empty result is ([0,3], [0,3])."""
    from . import ops
    lo, hi = _bounds3((lo, hi))
    for axis in range(3):
        for value, sign in ((lo[axis], 1), (hi[axis], -1)):
            verts, faces = ops.mesh_cut(verts, faces, axis, value, sign)
    return verts, faces


def _affine34(M3, t):
    A = np.zeros((3, 4), dtype=np.float64)
    A[:, :3], A[:, 3] = M3, t
    return A


def eval_surface(model, resolution=EVAL_RESOLUTION, grid_boundary=None, level=0.0, bbox=None, take_components=True, scale_mat=None,
                 normals=False, plot_conf=None, timings=None, chunk=DEFAULT_CHUNK):
    """The mesh the reference's evaluation scores (eval.py:132-162) -> dict(verts, faces, normals or None, frame) on the device, or None
    if a grid does not cross the level.  frame = dict(R, mean, shape, lo3, hi3): the principal frame of the coarse mesh and the fine grid
    aligned to it.
    Without bbox (get_surface_high_res_mesh): coarse cubic 100-node grid over grid_boundary -> its mesh -> the largest component (if
    take_components) -> frame -> aligned grid, eps 0.1 -> mesh -> model frame.  With bbox [2,3] (get_surface_by_grid(higher_res=True)): the
    coarse grid is aligned_grid(bbox, 100, eps 0), the largest component is always taken, eps is 0.01, and the mesh is cut by the box.
    Then scale_mat [4,4] (model -> world) if given, and the largest component by area.  Normals (at the model-frame vertices) need
    scale_mat's 3x3 part to be a positive multiple of the identity."""
    from . import ops
    plot_conf = plot_conf or {}
    if grid_boundary is None:
        grid_boundary = tuple(plot_conf.get("grid_boundary", DEFAULT_BOUNDARY))
    S = None
    if scale_mat is not None:
        S = np.asarray(torch.as_tensor(scale_mat).detach().cpu().numpy(), dtype=np.float64)
        if S.shape != (4, 4) or not np.isfinite(S).all():
            raise ValueError("eval_surface: scale_mat [4, 4]")
        if normals and not (S[0, 0] > 0 and np.array_equal(S[:3, :3], S[0, 0] * np.eye(3))):
            raise ValueError("eval_surface: normals need scale_mat's 3x3 part to be a positive multiple of the identity")
    dev = next(implicit_network_of(model).parameters()).device
    t = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize(dev)
            t.append(time.perf_counter())
            timings[name] = timings.get(name, 0.0) + t[-1] - t[-2]

    if timings is not None:
        torch.cuda.synchronize(dev)
        t[0] = time.perf_counter()
    if bbox is None:
        cshape, clo, chi = _shape3(COARSE_RESOLUTION), *_bounds3(grid_boundary)
        eps = 0.1
    else:
        bbox = np.asarray(torch.as_tensor(bbox).detach().cpu().numpy(), dtype=np.float32).astype(np.float64)      # the box as float32 values
        if bbox.shape != (2, 3):
            raise ValueError("eval_surface: bbox [2, 3] = (min, max)")
        cshape, clo, chi = aligned_grid(bbox[0], bbox[1], COARSE_RESOLUTION, 0.0)
        eps = 0.01
    grid = sdf_grid(model, cshape, (clo, chi), chunk=chunk)
    verts, faces = extract(grid, clo, chi, level)
    del grid
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return None
    if take_components or bbox is not None:
        verts, faces, _ = keep_largest_component(verts, faces)
    lap("coarse_s")
    R, mean = principal_frame(verts, faces)
    box = ops.affine_bounds3(verts, _affine34(R, -R @ mean)).cpu().numpy()
    shape, lo3, hi3 = aligned_grid(box[:3], box[3:], resolution, eps)
    del verts, faces
    lap("frame_s")
    grid = sdf_grid(model, shape, (lo3, hi3), chunk=chunk, frame=(R, mean))
    gmin, gmax = torch.aminmax(grid)
    crosses = not (float(gmin) > level or float(gmax) < level)      # plots.py:199
    lap("grid_s")
    frame = {"R": R, "mean": mean, "shape": shape, "lo3": lo3, "hi3": hi3}
    if not crosses:
        return None
    verts, faces = extract(grid, lo3, hi3, level)
    del grid
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return None
    ops.affine_rows3_(verts, _affine34(R.T, mean))          # local -> model frame
    lap("extract_s")
    if bbox is not None:
        verts, faces = clip_box(verts, faces, bbox[0], bbox[1])
        lap("cut_s")
        if faces.shape[0] == 0:
            return None
    world = verts
    if S is not None:
        world = ops.affine_rows3_(verts.clone(), S[:3])
    world, faces, kept = keep_largest_component(world, faces)
    lap("components_s")
    nrm = vertex_normals(model, verts[kept].contiguous()) if normals else None
    return {"verts": world, "faces": faces, "normals": nrm, "frame": frame}


def eval_out_path(run_dir, epoch, scan_id=None):
    """`<run>/{epoch}/scan{scan_id}.ply` (eval.py:160-162 under the run directory); `scan.ply` without an id."""
    return os.path.join(run_dir, str(epoch), "scan{}.ply".format("" if scan_id is None else scan_id))


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
    ap.add_argument("--precision", choices=list(PRECISIONS), default=None)
    ap.add_argument("--overwrite", default=False, action="store_true", help="write even if the .ply exists")
    ev = ap.add_argument_group("evaluation mesh (eval_surface)")
    ev.add_argument("--eval", default=False, action="store_true", help="the mesh the evaluation scores: aligned fine grid, box cut, world frame "
                    "(--resolution then defaults to %d and no normals are written unless --normals)" % EVAL_RESOLUTION)
    ev.add_argument("--bbox", default=None, type=str, metavar="FILE.npz", help="bounding boxes by scan id (DTU's bbs.npz); needs --scan_id; "
                    "its min row is multiplied by 1.5 as the reference does")
    ev.add_argument("--bbox-values", default=None, type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="the box, taken as given")
    ev.add_argument("--scan_id", default=None, type=int)
    ev.add_argument("--cams", default=None, type=str, metavar="cameras.npz", help="its scale_mat_0 moves the mesh to world coordinates")
    ev.add_argument("--no-world", default=False, action="store_true", help="stay in the model's frame even with --cams")
    ev.add_argument("--all-components", default=False, action="store_true", help="no component selection on the coarse mesh (no-bbox route)")
    ev.add_argument("--normals", default=False, action="store_true", help="write vertex normals")
    return ap


def plot_block(conf):
    """The conf's `plot` block as a plain dict (empty if absent)."""
    return dict(conf.get("plot", None) or {})


def eval_bbox(opt):
    """--bbox FILE.npz --scan_id N: npz[str(N)] * [[1.5], [1.0]], the reference's own scaling of the DTU boxes (plots.py:222), which
    applies to this route only; --bbox-values: the six numbers as given.  -> float64 [2,3] or None."""
    if opt.bbox is not None and opt.bbox_values is not None:
        raise SystemExit("--bbox and --bbox-values exclude each other")
    if opt.bbox is not None:
        if opt.scan_id is None:
            raise SystemExit("--bbox needs --scan_id")
        with np.load(opt.bbox) as npz:
            return np.asarray(npz[str(opt.scan_id)], dtype=np.float64).reshape(2, 3) * DTU_BBOX_QUIRK
    if opt.bbox_values is not None:
        return np.asarray(opt.bbox_values, dtype=np.float64).reshape(2, 3)
    return None


def main_eval(opt, model, epoch, root, plot):
    path = eval_out_path(root, epoch, opt.scan_id)
    if skip_existing(path, opt.overwrite):
        return 0
    scale_mat = None
    if opt.cams is not None and not opt.no_world:
        with np.load(opt.cams) as npz:
            scale_mat = np.asarray(npz["scale_mat_0"], dtype=np.float64)
    timings = {}
    res = eval_surface(model, opt.resolution or EVAL_RESOLUTION, tuple(opt.grid_boundary) if opt.grid_boundary else None, level=opt.level,
                       bbox=eval_bbox(opt), take_components=not opt.all_components, scale_mat=scale_mat, normals=opt.normals, plot_conf=plot,
                       timings=timings)
    print(", ".join("{} {:.3f} s".format(name, timings[key]) for name, key in (("coarse", "coarse_s"), ("frame", "frame_s"), ("fine grid", "grid_s"),
          ("extraction", "extract_s"), ("cut", "cut_s"), ("components", "components_s")) if key in timings), flush=True)
    if res is None:
        print("a grid does not cross level {} (or the box cuts everything away): no surface, nothing written".format(opt.level), flush=True)
        return 0
    ply.write_ply(path, res["verts"], res["faces"], res["normals"])
    print("{}: {} vertices, {} faces, aligned grid {} x {} x {}".format(path, res["verts"].shape[0], res["faces"].shape[0], *res["frame"]["shape"]),
          flush=True)
    return 0


def main(argv=None):
    opt = build_parser().parse_args(argv)
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    model, epoch, root, conf = load_model(opt.conf, opt.checkpoint, device, opt.expdir, opt.precision)
    plot = plot_block(conf)
    if opt.eval:
        return main_eval(opt, model, epoch, root, plot)
    path = out_path(root, epoch)
    if skip_existing(path, opt.overwrite):
        return 0
    timings = {}
    res = surface(model, opt.resolution, tuple(opt.grid_boundary) if opt.grid_boundary else None, level=opt.level,
                  largest_component=opt.largest_component, normals=not opt.no_normals, plot_conf=plot, timings=timings)
    if "grid_s" in timings:
        print("grid evaluation {:.3f} s, extraction {:.3f} s".format(timings["grid_s"], timings["extract_s"]), flush=True)
    if res is None:
        print("the grid does not cross level {}: no surface, nothing written".format(opt.level), flush=True)
        return 0
    ply.write_ply(path, res["verts"], res["faces"], res["normals"])
    print("{}: {} vertices, {} faces".format(path, res["verts"].shape[0], res["faces"].shape[0]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
