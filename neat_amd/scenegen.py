"""A training scene from a mesh and its wireframe, made on the device: shaded anti-aliased views, cameras.npz, the per-view 2-D wireframe
of the visible parts of the ground-truth edges, the mesh, the lines and offset_scale.txt.  The directory loads without a hand edit in
BlenderDataset, detect, triangulate, raycast analysis and evaluate abc, and its 3-D answer is exact.

    python -m neat_amd.scenegen (--mesh M.obj|M.ply --lines lines.json | --shape box|lblock) --out DIR [--views 100] [--res 512]
            [--focal 560] [--radius 2.0] [--ss 3] [--name gt] [--step 1] [--min-len 2] [--bias 0.002] [--subdivide 0] [--gpu 0] [--overwrite]

writes DIR/images/image_%04d.png, mask/%04d.png, cameras.npz, <name>/image_%04d.json, mesh.obj, lines.json and offset_scale.txt; a conf
then says `dataset.line_detector = <name>`.  lines.json holds `junctions` [J,3] and `lines` [E,2], straight edges.

    K, poses = scenegen.cameras(n, res, focal=560.0, radius=2.0)
    verts, faces, junctions, edges = scenegen.shapes["lblock"];  verts, faces = scenegen.subdivide(verts, faces, 2)
    verts, junctions = scenegen.normalise(verts, junctions, extent=1.0)
    scene = raycast.build(verts, faces)
    rgb, mask = scenegen.pictures(scene, K, poses, H, W, ss=3)                        # uint8 [V,H,W,3], [V,H,W] on the device
    runs = scenegen.visible_edges(scene, junctions, edges, K, poses, H, W)             # Runs, in (view, edge, run) order
    graphs = scenegen.to_wireframes(runs, len(poses), H, W)                            # one WireframeGraph per view

The rule is DESIGN 3l; csrc/kernels_scenegen.hpp implements it with the walk and the intersection rule of kernels_raycast.hpp, and
tests/scenegen_f64.py restates it in float64 numpy, which the device equals byte for byte.  There is no host fallback.
"""
import argparse
import collections
import ctypes
import math
import os
import sys

import numpy as np
import torch

from . import _lib, ply, raycast, run_io
from .synth import look_at_pose
from .wireframe import WireframeGraph

MAX_SS = 16                # sub-samples per pixel axis
MAX_SAMPLES = 1 << 16      # samples of one edge in one view
DEFAULTS = {"step": 1.0, "min_len": 2.0, "bias": 0.002, "near": 0.05}

Runs = collections.namedtuple("Runs", ["idx", "p2", "p3", "junction"])
Runs.__doc__ = """The visible runs in (view, edge, run) order, on the device: idx int32 [N,4] = view, edge, first and last sample;
p2 float64 [N,4] = x1 y1 x2 y2 in the picture; p3 float64 [N,2,3] the ends in the world; junction bool [N,2]: the end is the edge's own
junction, not an occlusion or a cut."""


# ------------------------------------------------------------------ cameras, shapes
def cameras(n, res, focal=560.0, radius=2.0):
    """-> (intrinsics float64 [n,3,3], extrinsics float64 [n,4,4] camera-to-world): what BlenderDataset reads from cameras.npz.  The centres
    lie on a Fibonacci spiral over the sphere of `radius` (z = 1 - (2 i + 1) / n, the golden angle between neighbours) and look at the
    origin through synth.look_at_pose, whose float32 values are kept, so a float32 reader loses nothing.  `focal` is stated at 512 pixels
    and scales with res, the principal point is res / 2: the defaults are the reference's ABC cameras (560 at 512, distance 2)."""
    n, res = int(n), int(res)
    K = np.zeros((n, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = float(focal) * res / 512.0
    K[:, 0, 2] = K[:, 1, 2] = res / 2.0
    K[:, 2, 2] = 1.0
    poses = np.zeros((n, 4, 4))
    golden = math.pi * (3.0 - math.sqrt(5.0))
    for i in range(n):
        z = 1.0 - (2.0 * i + 1.0) / n
        r = math.sqrt(max(0.0, 1.0 - z * z))
        poses[i] = look_at_pose((radius * r * math.cos(golden * i), radius * r * math.sin(golden * i), radius * z)).astype(np.float64)
    return K, poses


def _prism(outline, z0, z1, caps):
    """A polygon `outline` (counter-clockwise, [(x, y)]) between z0 and z1 -> (verts, faces, junctions, edges); `caps`: its triangulation."""
    m = len(outline)
    verts = np.asarray([(x, y, z0) for x, y in outline] + [(x, y, z1) for x, y in outline], dtype=np.float64)
    faces = [(a, c, b) for a, b, c in caps] + [(m + a, m + b, m + c) for a, b, c in caps]
    edges = []
    for i in range(m):
        j = (i + 1) % m
        faces += [(i, j, m + j), (i, m + j, m + i)]
        edges += [(i, j), (m + i, m + j), (i, m + i)]
    return verts, np.asarray(faces, dtype=np.int32), verts.copy(), np.asarray(sorted(edges), dtype=np.int32)


def _shapes():
    box = _prism([(-0.5, -0.375), (0.5, -0.375), (0.5, 0.375), (-0.5, 0.375)], -0.25, 0.25, [(0, 1, 2), (0, 2, 3)])
    # an L: the fan about its reflex corner (3) is its triangulation
    lblock = _prism([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.0), (0.0, 0.0), (0.0, 0.5), (-0.5, 0.5)], -0.25, 0.25,
                    [(3, 4, 5), (3, 5, 0), (3, 0, 1), (3, 1, 2)])
    return {"box": box, "lblock": lblock}


shapes = _shapes()      # name -> (verts float64 [nv,3], faces int32 [nf,3], junctions float64 [J,3], edges int32 [E,2]): every sharp edge


def subdivide(verts, faces, n):
    """Every triangle into four (its edge mid points), n times -> (verts, faces).  No point of the surface moves.  Triangle g becomes
    4 g .. 4 g + 3, so the face order is kept."""
    verts = [tuple(v) for v in np.asarray(verts, dtype=np.float64).reshape(-1, 3)]
    faces = [tuple(int(i) for i in f) for f in np.asarray(faces).reshape(-1, 3)]
    for _ in range(int(n)):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                verts.append(tuple((np.asarray(verts[key[0]]) + np.asarray(verts[key[1]])) / 2.0))
                cache[key] = len(verts) - 1
            return cache[key]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)


def normalise(verts, junctions, extent=1.0):
    """The centre of the mesh's box to the origin and its largest extent to `extent`: one transform for mesh and junctions
    -> (verts, junctions) float64.  Everything is then written in that frame, so offset_scale.txt is `0 0 0 1`."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    junctions = np.asarray(junctions, dtype=np.float64).reshape(-1, 3)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    centre, scale = (lo + hi) / 2.0, float(extent) / float((hi - lo).max())
    return (verts - centre) * scale, (junctions - centre) * scale


# ------------------------------------------------------------------ the device calls
def _cams(K, poses, dev):
    K = torch.as_tensor(np.asarray(torch.as_tensor(K).detach().cpu().numpy(), dtype=np.float64)).reshape(-1, 3, 3)
    poses = torch.as_tensor(np.asarray(torch.as_tensor(poses).detach().cpu().numpy(), dtype=np.float64)).reshape(-1, 4, 4)
    if K.shape[0] != poses.shape[0]:
        raise ValueError(f"scenegen: {K.shape[0]} intrinsics for {poses.shape[0]} poses")
    return K.contiguous().to(dev), poses.contiguous().to(dev)


def _scene(scene):
    if not isinstance(scene, raycast.Scene) or scene.device.type != "cuda":
        raise RuntimeError("neat_amd.scenegen needs a raycast.Scene on the device (there is no CPU path)")
    return scene.device


@torch.no_grad()
def pictures(scene, K, poses, H, W, ss=3, albedo=0.7, ambient=0.25, background=1.0):
    """scene: a raycast.Scene; K [V,3,3], poses [V,4,4] camera-to-world -> (rgb uint8 [V,H,W,3], mask uint8 [V,H,W]) on the device.  Pixel
    centres are at integer coordinates; a pixel is the mean of its ss x ss sub-samples, each albedo (ambient + (1 - ambient) |cos|) of
    the closest triangle or `background`; mask is 255 where any sub-sample hit."""
    dev = _scene(scene)
    K, poses = _cams(K, poses, dev)
    V, H, W = int(poses.shape[0]), int(H), int(W)
    rgb = torch.empty(V, H, W, 3, device=dev, dtype=torch.uint8)
    mask = torch.empty(V, H, W, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().neat_scenegen_shade(_lib.ptr(scene.bvh), scene.nf, _lib.ptr(K), _lib.ptr(poses), V, H, W, int(ss), float(albedo),
                                                  float(ambient), float(background), _lib.ptr(rgb), _lib.ptr(mask), _lib.stream()),
                   "neat_scenegen_shade")
    return rgb, mask


@torch.no_grad()
def visible_edges(scene, junctions, edges, K, poses, H, W, step=DEFAULTS["step"], min_len=DEFAULTS["min_len"], bias=DEFAULTS["bias"],
                  near=DEFAULTS["near"]):
    """junctions [J,3], edges [E,2] -> Runs: the maximal sequences of visible samples of each edge in each view whose 2-D length is at
    least min_len pixels.  An edge is cut at z = near and at the border of the picture, sampled every `step` pixels at most, and a
    sample is visible by raycast.visible_points' rule in float64 (no triangle with 0 <= t < distance - bias).  One synchronisation:
    the count of the runs."""
    dev = _scene(scene)
    K, poses = _cams(K, poses, dev)
    V, H, W = int(poses.shape[0]), int(H), int(W)
    J = torch.as_tensor(np.asarray(torch.as_tensor(junctions).detach().cpu().numpy(), dtype=np.float64)).reshape(-1, 3).contiguous().to(dev)
    e = np.ascontiguousarray(np.asarray(torch.as_tensor(edges).detach().cpu().numpy()).reshape(-1, 2), dtype=np.int32)
    E, nJ = int(e.shape[0]), int(J.shape[0])
    lib = _lib.lib()
    args = (float(step), float(min_len), float(bias), float(near))
    with torch.cuda.device(dev):
        ws = torch.empty(max(lib.neat_scenegen_scratch_bytes(V, E), 8), device=dev, dtype=torch.uint8)
        total = torch.empty(1, device=dev, dtype=torch.int64)
        _lib.check(lib.neat_scenegen_edge_count(_lib.ptr(scene.bvh), scene.nf, _lib.ptr(J), nJ, e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), E,
                                                _lib.ptr(K), _lib.ptr(poses), V, H, W, *args, _lib.ptr(ws), _lib.ptr(total), _lib.stream()),
                   "neat_scenegen_edge_count")
        N = int(total.item())                       # the one read-back: the list's length
        idx = torch.empty(N, 4, device=dev, dtype=torch.int32)
        p2, p3 = torch.empty(N, 4, device=dev, dtype=torch.float64), torch.empty(N, 2, 3, device=dev, dtype=torch.float64)
        junc = torch.empty(N, 2, device=dev, dtype=torch.uint8)
        _lib.check(lib.neat_scenegen_edge_fill(_lib.ptr(scene.bvh), scene.nf, _lib.ptr(J), nJ, E, _lib.ptr(K), _lib.ptr(poses), V, H, W, *args,
                                               _lib.ptr(ws), N, _lib.ptr(idx), _lib.ptr(p2), _lib.ptr(p3), _lib.ptr(junc), _lib.stream()),
                   "neat_scenegen_edge_fill")
    return Runs(idx, p2, p3, junc != 0)


def to_wireframes(runs, views, H, W, edges=None):
    """Runs (or its four arrays, anywhere) -> one WireframeGraph per view, on the host.  A run end that is the edge's own junction becomes
    one 2-D junction per (view, junction index), shared by every run that ends there; `edges` [E,2] names the junction of each end (without
    it such ends stay apart too).  Every other end, an occlusion T-junction or a cut at the border, is a junction of its own.
    Confidences and weights are 1."""
    idx, p2, _, junc = (np.asarray(torch.as_tensor(x).detach().cpu().numpy()) for x in runs)
    idx, p2, junc = idx.reshape(-1, 4), p2.reshape(-1, 4).astype(np.float64), junc.reshape(-1, 2).astype(bool)
    edges = None if edges is None else np.asarray(torch.as_tensor(edges).detach().cpu().numpy()).reshape(-1, 2)
    out = []
    for v in range(int(views)):
        verts, pairs, shared = [], [], {}
        for r in np.nonzero(idx[:, 0] == v)[0]:
            ends = []
            for s in range(2):
                key = int(edges[idx[r, 1], s]) if (edges is not None and junc[r, s]) else None
                if key is not None and key in shared:
                    ends.append(shared[key])
                    continue
                verts.append((p2[r, 2 * s], p2[r, 2 * s + 1]))
                ends.append(len(verts) - 1)
                if key is not None:
                    shared[key] = ends[-1]
            pairs.append(ends)
        out.append(WireframeGraph(torch.tensor(verts, dtype=torch.float32).reshape(-1, 2), torch.ones(len(verts)),
                                  torch.tensor(pairs, dtype=torch.long).reshape(-1, 2), torch.ones(len(pairs)), frame_width=int(W), frame_height=int(H)))
    return out


# ------------------------------------------------------------------ files
def image_name(i):
    return "image_%04d" % i


def scene_paths(out, views, name="gt"):
    """Every file of a scene directory -> dict(images, masks, wireframes: lists of `views` paths; cameras, mesh, lines, offset_scale)."""
    return {"images": [os.path.join(out, "images", image_name(i) + ".png") for i in range(views)],
            "masks": [os.path.join(out, "mask", "%04d.png" % i) for i in range(views)],
            "wireframes": [os.path.join(out, name, image_name(i) + ".json") for i in range(views)],
            "cameras": os.path.join(out, "cameras.npz"), "mesh": os.path.join(out, "mesh.obj"), "lines": os.path.join(out, "lines.json"),
            "offset_scale": os.path.join(out, "offset_scale.txt")}


write_obj = ply.write_obj              # its home is neat_amd.ply


def write_static(paths, verts, faces, junctions, edges, K, poses):
    """cameras.npz, mesh.obj, lines.json and offset_scale.txt (`0 0 0 1`: everything is in the one normalised frame)."""
    run_io.replace_file(paths["cameras"], lambda tmp: np.savez(tmp, intrinsics=np.asarray(K, dtype=np.float64),
                                                               extrinsics=np.asarray(poses, dtype=np.float64)))
    write_obj(paths["mesh"], verts, faces)
    run_io.write_json(paths["lines"], {"junctions": np.asarray(junctions, dtype=np.float64).reshape(-1, 3).tolist(),
                                       "lines": np.asarray(edges).reshape(-1, 2).astype(int).tolist()})

    def offset(tmp):
        with open(tmp, "w") as fh:
            fh.write("0 0 0 1\n")
    run_io.replace_file(paths["offset_scale"], offset)


def read_lines(path):
    """lines.json -> (junctions float64 [J,3], edges int32 [E,2])."""
    junctions, edges = run_io.read_lines_json(path)
    return junctions, edges.astype(np.int32)


# ------------------------------------------------------------------ command line
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.scenegen", description="make a training scene from a mesh and its wireframe on the device")
    ap.add_argument("--mesh", type=str, default=None, help="a .obj or .ply triangle mesh")
    ap.add_argument("--lines", type=str, default=None, help="lines.json: junctions [J,3] and lines [E,2], in the mesh's frame")
    ap.add_argument("--shape", type=str, default=None, choices=sorted(shapes), help="a built-in model instead of --mesh and --lines")
    ap.add_argument("--out", type=str, required=True, help="the scene directory")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=512, help="pictures are res x res pixels")
    ap.add_argument("--focal", type=float, default=560.0, help="focal length in pixels at 512 pixels")
    ap.add_argument("--radius", type=float, default=2.0, help="distance of the cameras from the origin")
    ap.add_argument("--ss", type=int, default=3, help="sub-samples per pixel axis")
    ap.add_argument("--name", type=str, default="gt", help="directory of the 2-D wireframes: the conf's dataset.line_detector")
    ap.add_argument("--step", type=float, default=DEFAULTS["step"], help="pixels between the samples of an edge, at most")
    ap.add_argument("--min-len", type=float, default=DEFAULTS["min_len"], help="least 2-D length of a visible run, pixels")
    ap.add_argument("--bias", type=float, default=DEFAULTS["bias"], help="a visibility ray stops this far in front of its sample")
    ap.add_argument("--subdivide", type=int, default=0, help="split every triangle into four, this many times")
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    ap.add_argument("--overwrite", default=False, action="store_true", help="write into a directory that already holds a cameras.npz")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    if (opt.shape is None) == (opt.mesh is None) or (opt.mesh is None) != (opt.lines is None):
        ap.error("either --shape, or --mesh and --lines")
    if opt.mesh is not None and os.path.splitext(opt.mesh)[1].lower() not in (".ply", ".obj"):
        ap.error("--mesh is a .ply or an .obj file")
    if opt.views < 1 or opt.res < 2 or not 1 <= opt.ss <= MAX_SS or not opt.step > 0.0 or not opt.bias >= 0.0 or opt.subdivide < 0 or \
            not opt.focal > 0.0 or not opt.radius > 0.0:
        ap.error("--views >= 1, --res >= 2, 1 <= --ss <= %d, --step > 0, --bias >= 0, --subdivide >= 0, --focal > 0, --radius > 0" % MAX_SS)
    if math.ceil(math.hypot(opt.res, opt.res) / opt.step) + 2 > MAX_SAMPLES:
        ap.error("--step is too small for --res: an edge may take %d samples at most" % MAX_SAMPLES)
    return opt


def main(argv=None):
    opt = parse_args(argv)
    _lib.lib()
    paths = scene_paths(opt.out, opt.views, opt.name)
    if run_io.skip_existing(paths["cameras"], opt.overwrite):
        return 0
    if opt.shape is not None:
        verts, faces, junctions, edges = shapes[opt.shape]
    else:
        verts, faces = ply.read_mesh(opt.mesh)
        junctions, edges = read_lines(opt.lines)
    if edges.size and (edges.min() < 0 or edges.max() >= junctions.shape[0]):
        raise ValueError("lines.json: a line names a junction outside the list")
    verts, faces = subdivide(verts, faces, opt.subdivide)
    verts, junctions = normalise(verts, junctions)
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    K, poses = cameras(opt.views, opt.res, opt.focal, opt.radius)
    scene = raycast.build(verts, faces, device)
    if scene.status != 0:
        raise ValueError("the mesh: a face index lies outside the vertices")
    rgb, mask = pictures(scene, K, poses, opt.res, opt.res, ss=opt.ss)
    runs = visible_edges(scene, junctions, edges, K, poses, opt.res, opt.res, step=opt.step, min_len=opt.min_len, bias=opt.bias)
    graphs = to_wireframes(runs, opt.views, opt.res, opt.res, edges)
    rgb, mask = rgb.cpu().numpy(), mask.cpu().numpy()
    write_static(paths, verts, faces, junctions, edges, K, poses)
    for i in range(opt.views):
        run_io.write_png(paths["images"][i], rgb[i])
        run_io.write_png(paths["masks"][i], mask[i])
        run_io.write_wireframe_json(paths["wireframes"][i], graphs[i])
    print("{}: {} views of {} x {}, {} triangles, {} edges, {} visible runs".format(opt.out, opt.views, opt.res, opt.res, scene.nf,
                                                                                      int(edges.shape[0]), int(runs.idx.shape[0])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
