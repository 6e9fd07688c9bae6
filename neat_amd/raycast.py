"""Where a ray meets a triangle mesh: a tree over the triangles built and walked on the device.

    from neat_amd import raycast
    scene = raycast.build(verts, faces)                                  # device-resident; scene.nf, scene.status
    t, tri, uv = raycast.cast(scene, origins, dirs, t_min=None, t_max=None, any_hit=False, counts=None)
    depth, normal, tri = raycast.view(scene, pose, intrinsics, H, W)
    seen = raycast.visible_points(scene, points, cams, bias=0.01)        # bool [F, N]
    frac = raycast.visible_lines(scene, lines3d, cams, samples=16)       # float32 [F, N]
    dist, tri, point, uv = raycast.closest(scene, points, max_dist=inf)  # float64: the closest point of the surface
    dist = raycast.line_distance(scene, lines3d, samples=32)             # float64 [n, samples]

    python -m neat_amd.raycast check --mesh M.ply|M.obj --data X-wfi.npz|X-neat.pth (--conf <run>/runconf.conf | --cams cameras.npz)
        [--min-views 5] [--min-frac 0.5] [--bias 0.01] [--samples 16] [--data_root ../data] [--gpu 0] [--json] [--overwrite]
    python -m neat_amd.raycast analysis --conf <conf> --scan <dir with lines.json, offset_scale.txt, mesh.obj> [--data_root ../data]
        [--gpu 0] [--json]
    python -m neat_amd.raycast distance --mesh M.ply|M.obj (--data X.npz | --points P.ply) [--samples 32] [--threshold 0.05] [--max-dist d]
        [--scale-file offset_scale.txt] [--gpu 0] [--json] [--overwrite]

The mesh may be ground truth, a surface_*.ply of neat_amd.mesh or anyone's reconstruction; no checkpoint is needed.  The rule of
intersection (Woop, Benthin, Wald 2013, decided in float64: both windings, edges inclusive, a hit has t_min <= t < t_max, ties in t go to
the lowest face index), the tree and the walk are the kernels of csrc/kernels_raycast.hpp behind neat_raycast_* (include/neat_hip.h;
DESIGN 3h; tests/raycast_f64.py restates them in float64): the answer is the brute-force minimum over all triangles.  A triangle with a
non-finite vertex or zero area is never hit.  A face index outside the vertices sets scene.status = 1; the tree is then empty and
every ray misses.  There is no host fallback.

`check` is `python -m neat_amd.trace check` with the mesh as the occluder: the same keep rule (a line is kept when at least --min-views
cameras see at least --min-frac of its --samples points) and the same three arrays, written to `<data stem>_occlmesh.npz`.
`analysis` is the reference's occlusion-aware ceiling (evaluation/abc-analysis.py :58-182): which ground-truth junctions and lines of an
ABC scan each camera really sees past the ground-truth mesh, and how many of those the 2-D detections of the view recover.
`distance` asks how far things are from the surface itself, not from its vertices (the closest point on the mesh by the region
rule of Ericson 5.1.5 in float64, the brute-force minimum over all triangles, ties to the lowest face index).  With --data it samples
every line as evaluation/eval-lsr-scannet.py :94-95 does and writes `<data stem>_dist.npz`: dist [n,samples], mean [n], max [n], tri
[n,samples], on_surface [n] (max <= --threshold).  With --points the vertices of a PLY are the queries and `<stem>_dist.npz` holds dist,
tri and point; it prints Acc (the mean distance), the median and Prec (the share nearer than --threshold); run it both ways round for
the two-sided figures.  A mesh with a face index outside its vertices is an error (exit code 1), not a result.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import _lib, ply, run_io, visibility


class Scene:
    """A mesh and its tree on the device.  nf = its triangles; status = 0, or 1 after a face index outside [0, nv) (read from the device
    on first use: one synchronisation)."""

    def __init__(self, verts, faces, bvh):
        self.verts, self.faces, self.bvh = verts, faces, bvh
        self.nv, self.nf = int(verts.shape[0]), int(faces.shape[0])
        self._status = None

    @property
    def device(self):
        return self.bvh.device

    @property
    def status(self):
        if self._status is None:
            self._status = int(self.bvh[:4].view(torch.int32).item())
        return self._status


def _device_of(x, device):
    if device is not None:
        return torch.device(device)
    if torch.is_tensor(x) and x.is_cuda:
        return x.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def build(verts, faces, device=None):
    """verts [nv,3], faces [nf,3] (arrays or tensors, anywhere) -> Scene on `device` (that of verts, or the current one)."""
    from . import ops
    dev = _device_of(verts, device)
    v = torch.as_tensor(verts).detach().to(dev, torch.float64).reshape(-1, 3).contiguous()
    f = torch.as_tensor(faces).detach().to(dev, torch.int32).reshape(-1, 3).contiguous()
    with torch.cuda.device(dev):
        return Scene(v, f, ops.raycast_build(v, f))


@torch.no_grad()
def cast(scene, origins, dirs, t_min=None, t_max=None, any_hit=False, counts=None):
    """origins, dirs [R,3] float32 on the scene's device (t is in units of |dir|), t_min / t_max [R] or None (0, +inf) -> (t [R] float32,
    +inf on a miss; tri [R] int32, the face index, -1 on a miss; uv [R,2] float32 barycentrics, hit = (1 - u - v) v0 + u v1 + v v2).
    any_hit: the first accepted hit the walk meets instead of the closest (t is finite iff something lies in [t_min, t_max)).
    counts: a [R,2] tensor of 4-byte integers on the device receives (node boxes tested, triangles tested) per ray."""
    from . import ops
    with torch.cuda.device(scene.device):
        return ops.raycast_cast(scene.bvh, scene.nf, origins, dirs, t_min, t_max, any_hit, counts)


@torch.no_grad()
def view(scene, pose, intrinsics, H, W):
    """One view of H x W pixels: pose [4,4] camera-to-world, intrinsics [4,4] or [3,3] -> (depth [H,W] float32, the distance along the
    ray, NaN on a miss; normal [H,W,3], the geometric unit normal of the triangle turned towards the camera, zero on a miss; tri [H,W]
    int32, -1 on a miss).  Rays are neat_camera_rays', as trace.view makes them."""
    from . import ops
    dev = scene.device
    pose = torch.as_tensor(pose).detach().to(dev, torch.float32).reshape(1, 4, 4).contiguous()
    K = torch.as_tensor(intrinsics).detach().to(dev, torch.float32)
    K = K.reshape(1, *K.shape[-2:]).contiguous()
    with torch.cuda.device(dev):
        dirs, _, origins = ops.camera_rays(ops.pixel_grid(H, W, dev)[None], pose, K, with_origins=True)
        dirs = dirs.reshape(-1, 3)
        t, tri, _ = cast(scene, origins, dirs)
        hit = tri >= 0
        depth = torch.where(hit, t, torch.full_like(t, float("nan")))
        normal = torch.zeros(H * W, 3, device=dev)
        idx = torch.nonzero(hit).flatten()
        if idx.numel():
            tv = scene.verts[scene.faces[tri[idx]].long()]                       # [n, 3, 3] float64
            n = torch.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0], dim=-1)
            n = n / n.norm(dim=-1, keepdim=True)
            away = (n * dirs[idx].double()).sum(-1) > 0
            normal[idx] = torch.where(away[:, None], -n, n).float()
    return depth.view(H, W), normal.view(H, W, 3), tri.view(H, W)


def _visible(scene, rows, cams, samples, bias):
    # neat_trace_target_rays refuses targets outside a sphere: one that holds every centre and target (float64, on the host)
    def radius(centres, rows):
        far = max(float(np.linalg.norm(centres, axis=1).max()), float(rows.double().reshape(-1, 3).norm(dim=1).max().item()))
        return 2.0 * far + 1.0
    return visibility.visible(scene.device, rows, cams, samples, bias, radius, 0.0,
                              lambda o, d, t_end: torch.isinf(cast(scene, o, d, t_max=t_end, any_hit=True)[0]))


@torch.no_grad()
def visible_points(scene, points, cams, *, bias=0.01):
    """points [N,3], cams [F,4,4] world-to-camera -> bool [F,N] on the device: point p is visible from the camera centre c iff the ray
    from c towards p meets no triangle with 0 <= t < |p - c| - bias.  A point nearer to c than bias is not visible.  The view frustum is
    not tested."""
    return _visible(scene, points, cams, 1, bias)[..., 0]


@torch.no_grad()
def visible_lines(scene, lines3d, cams, *, samples=16, bias=0.01):
    """lines3d [N,2,3], cams [F,4,4] -> float32 [F,N]: the visible fraction of the `samples` points linspace(0, 1, samples) of each segment."""
    if samples < 2:
        raise ValueError("raycast.visible_lines: samples >= 2")
    return _visible(scene, lines3d, cams, int(samples), bias).float().mean(dim=-1)


@torch.no_grad()
def closest(scene, points, max_dist=float("inf"), counts=None):
    """points [N,3] (any float type, on the scene's device; they are widened to float64) -> (dist [N] float64, the distance to the closest
    point of the mesh, +inf on a miss; tri [N] int32, its face index, -1 on a miss; point [N,3] float64, the closest point; uv [N,2]
    float64, its barycentrics, point = (1 - u - v) v0 + u v1 + v v2: both zero on a miss).  A triangle further than max_dist is not
    accepted (the bound is inclusive on the squared distance, max_dist^2 in float64).  A point with a non-finite coordinate misses, and
    so does every point when scene.status = 1.  counts: a [N,2] tensor of 4-byte integers on the device receives (node boxes tested,
    triangles tested) per query.  The rule: DESIGN 3m, tests/closest_f64.py."""
    from . import ops
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError("raycast.closest: max_dist >= 0")
    max_d2 = max_dist * max_dist
    dev = scene.device
    pts = torch.as_tensor(points).detach().to(dev, torch.float64).reshape(-1, 3).contiguous()
    with torch.cuda.device(dev):
        # the queries go in the order given: sorting them along a Morton curve first was measured and is not worth its code
        d2, tri, point, uv = ops.raycast_closest(scene.bvh, scene.nf, pts, max_d2, counts)
        return torch.sqrt(d2), tri, point, uv


def line_points(lines3d, samples):
    """lines3d [n,2,3] float64 tensor -> the sample points a t + b (1 - t), t = linspace(0, 1, samples), [n, samples, 3]
    (evaluation/eval-lsr-scannet.py :94-95: the first sample is the second end point)."""
    t = torch.from_numpy(np.linspace(0.0, 1.0, samples)).to(lines3d.device).view(1, -1, 1)       # numpy's linspace, to the last bit
    return lines3d[:, :1] * t + lines3d[:, 1:] * (1.0 - t)


@torch.no_grad()
def line_distance(scene, lines3d, samples=32, max_dist=float("inf"), with_tri=False):
    """lines3d [n,2,3] -> dist float64 [n, samples] on the device: the distance of each sample point of line_points to the mesh
    (with_tri: also tri int32 [n, samples])."""
    if samples < 2:
        raise ValueError("raycast.line_distance: samples >= 2")
    lines = torch.as_tensor(lines3d).detach().to(scene.device, torch.float64).reshape(-1, 2, 3)
    n = int(lines.shape[0])
    dist, tri, _, _ = closest(scene, line_points(lines, int(samples)).reshape(-1, 3), max_dist)
    dist, tri = dist.view(n, samples), tri.view(n, samples)
    return (dist, tri) if with_tri else dist


# ------------------------------------------------------------------ command line
def out_path(data):
    """`<data stem>_occlmesh.npz` beside the input."""
    return os.path.splitext(data)[0] + "_occlmesh.npz"


read_mesh = ply.read_mesh              # its home is neat_amd.ply


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.raycast", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    ck = sub.add_parser("check", help="keep the lines of a wireframe that enough cameras see past a triangle mesh")
    ck.add_argument("--mesh", type=str, required=True, help="the occluder: a .ply or .obj triangle mesh")
    visibility.add_check_flags(ck, "--data")
    ck.add_argument("--conf", type=str, default=None, help="a run's conf: the cameras of its dataset")
    ck.add_argument("--cams", type=str, default=None, help="a cameras.npz (extrinsics: camera-to-world) or a cam.json (world-to-camera)")
    visibility.add_check_flags(ck, "--min-views", "--min-frac", "--bias", "--samples", "--data_root", "--gpu", "--json")
    ck.add_argument("--overwrite", default=False, action="store_true", help="rewrite an _occlmesh.npz that is already on disk")
    an = sub.add_parser("analysis", help="what the cameras see of a scan's ground-truth wireframe, and what the detections recover of it")
    an.add_argument("--conf", type=str, required=True)
    an.add_argument("--scan", type=str, required=True, help="directory with lines.json, offset_scale.txt and mesh.obj")
    an.add_argument("--data_root", default="../data", help="root of the dataset's data_dir")
    an.add_argument("--gpu", default=0, type=int, help="device index")
    an.add_argument("--json", default=False, action="store_true", help="print one JSON object with the six numbers")
    di = sub.add_parser("distance", help="how far the lines of a wireframe, or the points of a cloud, are from a triangle mesh")
    di.add_argument("--mesh", type=str, required=True, help="the surface: a .ply or .obj triangle mesh")
    di.add_argument("--data", type=str, default=None, help="a wireframe: an .npz with `lines3d`, or a -neat.pth")
    di.add_argument("--points", type=str, default=None, help="a .ply cloud or mesh: its vertices are the queries")
    di.add_argument("--samples", default=32, type=int, help="points per line")
    di.add_argument("--threshold", default=0.05, type=float, help="a line lies on the surface when no sample is further; Prec counts the points nearer")
    di.add_argument("--max-dist", default=float("inf"), type=float, help="nothing further than this is looked for: the distance is then inf")
    di.add_argument("--scale-file", type=str, default=None, help="an offset_scale.txt: the lines or points are x / scale - offset in the mesh's frame")
    di.add_argument("--gpu", default=0, type=int, help="device index")
    di.add_argument("--json", default=False, action="store_true", help="print one JSON object with the summary and the seconds")
    di.add_argument("--overwrite", default=False, action="store_true", help="rewrite a _dist.npz that is already on disk")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    if opt.command == "check":
        visibility.validate_check(ap, opt)
        if (opt.conf is None) == (opt.cams is None):
            ap.error("one of --conf and --cams")
        if os.path.splitext(opt.mesh)[1].lower() not in (".ply", ".obj"):
            ap.error("--mesh is a .ply or an .obj file")
    if opt.command == "distance":
        if opt.samples < 2 or not opt.threshold >= 0.0 or not opt.max_dist >= 0.0:
            ap.error("--samples >= 2, --threshold >= 0, --max-dist >= 0")
        if (opt.data is None) == (opt.points is None):
            ap.error("one of --data and --points")
        if os.path.splitext(opt.mesh)[1].lower() not in (".ply", ".obj"):
            ap.error("--mesh is a .ply or an .obj file")
        if opt.points is not None and not opt.points.lower().endswith(".ply"):
            ap.error("--points is a .ply file")
    return opt


def main_check(opt):
    _lib.lib()
    path = out_path(opt.data)
    if run_io.skip_existing(path, opt.overwrite):
        return 0
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    if opt.conf is not None:
        cams = run_io.dataset_cams(run_io.build_dataset(run_io.parse_conf(opt.conf), opt.data_root))
    else:
        cams = run_io.read_cams(opt.cams)
    verts, faces = read_mesh(opt.mesh)

    def fraction(lines3d):
        scene = build(verts, faces, device)
        if scene.status != 0:
            raise ValueError("%s: a face index lies outside the vertices" % opt.mesh)
        return visible_lines(scene, lines3d, cams, samples=opt.samples, bias=opt.bias).cpu().numpy(), {"triangles": scene.nf}
    return visibility.run_check(opt, path, device, cams, fraction, "casting", "cast_s")


# ---- analysis (evaluation/abc-analysis.py)
def project2d(K, R, T, X):
    """abc-analysis.py :28-42 in float64: K (R X + T) with the guarded division.  K [3,3], R [3,3], T [3], X [n,3] -> [n,2]."""
    x = (K @ (R @ X.T + T.reshape(3, 1))).T
    den = x[:, -1:]
    sign = np.where(den >= 0, 1.0, -1.0)
    eps = np.where(np.abs(den) < 1e-8, 1e-8, 0.0)
    return (x / (den + eps * sign))[:, :2]


def inside(p, width, height):
    """abc-analysis.py :127, :147."""
    return (p[:, 0] >= 0) & (p[:, 0] < width) & (p[:, 1] >= 0) & (p[:, 1] < height)


def cast_check(scene, points2d, points3d, intrinsics, pose, tol):
    """abc-analysis.py :44-56: the rays of the pixels points2d [n,2]; a target is seen when the closest hit lies within tol of it."""
    from . import ops
    dev = scene.device
    n = points2d.shape[0]
    if n == 0:
        return np.zeros(0, bool)
    uv = torch.from_numpy(np.ascontiguousarray(points2d, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        dirs, _, origins = ops.camera_rays(uv[None], pose.to(dev, torch.float32).reshape(1, 4, 4).contiguous(),
                                           intrinsics.to(dev, torch.float32)[None].contiguous(), with_origins=True)
        t, _, _ = cast(scene, origins, dirs.reshape(-1, 3))
    o, d, t = origins.cpu().numpy().astype(np.float64), dirs.reshape(-1, 3).cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.linalg.norm(o + d * t[:, None] - points3d, axis=-1) < tol


def scan_wireframe(scan):
    """<scan>/lines.json, offset_scale.txt -> (inv(scale_mat) float64 [4,4], junctions float32 [J,3] in the training frame, edges [L,2])."""
    junctions, edges = run_io.read_lines_json(os.path.join(scan, "lines.json"))
    off = run_io.read_offset_scale(os.path.join(scan, "offset_scale.txt"))
    s = 1.0 / float(off[-1])
    scale_mat = np.array([[s, 0, 0, -float(off[0])], [0, s, 0, -float(off[1])], [0, 0, s, -float(off[2])], [0, 0, 0, 1.0]])
    inv_scale = np.linalg.inv(scale_mat)
    junctions = (inv_scale[:3, :3] @ junctions.T + inv_scale[:3, 3:]).T
    return inv_scale, junctions.astype(np.float32), edges


def _assign(cost, device):
    """scipy's linear_sum_assignment on the device -> (rows, cols) of the matched pairs, on the host."""
    from . import ops
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    with torch.cuda.device(device):
        rows, cols, _ = ops.linear_sum_assignment(torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float32)).to(device))
    rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
    ok = (rows >= 0) & (cols >= 0)
    return rows[ok], cols[ok]


def analyse(scene, dataset, junctions, edges, device):
    """abc-analysis.py :107-172 -> dict(junctions_seen bool [F,J], lines_seen bool [F,L], junctions_hit int32 [J], lines_hit int32 [L],
    junction_rate, line_rate: the mean over the views of the recovered share of the seen junctions / lines)."""
    width, height = dataset.img_res             # as the reference unpacks the pair (:107)
    J64 = junctions.astype(np.float64)
    lines = J64[edges]                          # [L,2,3]
    F, nJ, nL = len(dataset), J64.shape[0], edges.shape[0]
    j_seen, l_seen = np.zeros((F, nJ), bool), np.zeros((F, nL), bool)
    j_hit, l_hit = np.zeros(nJ, np.int32), np.zeros(nL, np.int32)
    j_rate = l_rate = 0.0
    for i in range(F):
        _, sample, _ = dataset[i]
        K4, pose = sample["intrinsics"], sample["pose"]
        K = np.asarray(K4.numpy(), dtype=np.float64)[:3, :3]
        w2c = np.linalg.inv(np.asarray(pose.numpy(), dtype=np.float64))
        R, T = w2c[:3, :3], w2c[:3, 3]
        j2d = project2d(K, R, T, J64)
        valid = inside(j2d, width, height) & cast_check(scene, j2d, J64, K4, pose, 1e-4)
        j_seen[i] = valid
        wf = sample["wireframe"]
        pred = np.asarray(wf.vertices.detach().cpu().numpy(), dtype=np.float64).reshape(-1, 2)
        jdist = np.linalg.norm(pred[:, None] - j2d[None], axis=-1)
        rows, cols = _assign(jdist, device)
        hit = (jdist[rows, cols] < 20) & valid[cols]
        j_hit[cols[hit]] += 1
        j_rate += hit.sum() / max(int(valid.sum()), 1)
        l2d = project2d(K, R, T, lines.reshape(-1, 3)).reshape(-1, 4)
        is_in = inside(l2d[:, :2], width, height) & inside(l2d[:, 2:], width, height)
        is_in &= cast_check(scene, l2d[:, :2], lines[:, 0], K4, pose, 0.1) & cast_check(scene, l2d[:, 2:], lines[:, 1], K4, pose, 0.1)
        l_seen[i] = is_in
        det = np.asarray(wf.line_segments(0.05)[:, :-1].detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4)
        d1 = np.linalg.norm(det[:, None, :2] - l2d[None, :, :2], axis=-1) + np.linalg.norm(det[:, None, 2:] - l2d[None, :, 2:], axis=-1)
        d2 = np.linalg.norm(det[:, None, :2] - l2d[None, :, 2:], axis=-1) + np.linalg.norm(det[:, None, 2:] - l2d[None, :, :2], axis=-1)
        ldist = np.minimum(d1, d2) * 0.5
        rows, cols = _assign(ldist, device)
        hit = (ldist[rows, cols] < 20) & is_in[cols]
        l_hit[cols[hit]] += 1
        l_rate += hit.sum() / max(int(is_in.sum()), 1)
    return {"junctions_seen": j_seen, "lines_seen": l_seen, "junctions_hit": j_hit, "lines_hit": l_hit,
            "junction_rate": np.float64(j_rate / max(F, 1)), "line_rate": np.float64(l_rate / max(F, 1))}


def main_analysis(opt):
    _lib.lib()
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    dataset = run_io.build_dataset(run_io.parse_conf(opt.conf), opt.data_root, distance_threshold=1.0)
    inv_scale, junctions, edges = scan_wireframe(opt.scan)
    verts, faces = ply.read_obj(os.path.join(opt.scan, "mesh.obj"))
    verts = (inv_scale[:3, :3] @ verts.T + inv_scale[:3, 3:]).T
    scene = build(verts, faces, device)
    if scene.status != 0:
        raise ValueError("%s: a face index lies outside the vertices" % os.path.join(opt.scan, "mesh.obj"))
    res = analyse(scene, dataset, junctions, edges, device)
    # the reference's six numbers; its last is the lines with a hit count >= 0, which is every line
    six = [int(junctions.shape[0]), int(edges.shape[0]), int((res["junctions_hit"] > 0).sum()), float(res["junction_rate"]),
           float(res["line_rate"]), int((res["lines_hit"] >= 0).sum())]
    for x in six:
        print(x, flush=True)
    path = os.path.join(opt.scan, "wireframe_visibility.npz")
    run_io.replace_file(path, lambda tmp: np.savez(tmp, **res))
    if opt.json:
        print(json.dumps({"junctions": six[0], "lines": six[1], "junctions_hit": six[2], "junction_rate": six[3], "line_rate": six[4],
                          "lines_kept": six[5], "lines_hit": int((res["lines_hit"] > 0).sum()), "views": len(dataset), "path": path}), flush=True)
    return 0


# ---- distance
def dist_path(data):
    """`<stem>_dist.npz` beside the wireframe or the cloud."""
    return os.path.splitext(data)[0] + "_dist.npz"


def to_mesh_frame(x, scale_file):
    """x [..., 3] in the model frame -> the frame of the scan's mesh, x / scale - offset with the four numbers of offset_scale.txt (as
    evaluate.abc_scores maps the predictions)."""
    off = run_io.read_offset_scale(scale_file)
    return np.asarray(x, dtype=np.float64) * (1.0 / off[3]) - off[:3]


def main_distance(opt):
    _lib.lib()
    source = opt.data if opt.data is not None else opt.points
    path = dist_path(source)
    if run_io.skip_existing(path, opt.overwrite):
        return 0
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    verts, faces = read_mesh(opt.mesh)
    if opt.data is not None:
        queries = run_io.load_lines(opt.data)[0]
    else:
        queries = np.asarray(ply.read_ply(opt.points)["points"], dtype=np.float64).reshape(-1, 3)
    if opt.scale_file is not None:
        queries = to_mesh_frame(queries, opt.scale_file)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    scene = build(verts, faces, device)
    if scene.status != 0:
        print("error: {}: a face index lies outside the vertices".format(opt.mesh), file=sys.stderr, flush=True)
        return 1
    if opt.data is not None:
        dist, tri = line_distance(scene, torch.from_numpy(queries), opt.samples, opt.max_dist, with_tri=True)
        dist, tri = dist.cpu().numpy(), tri.cpu().numpy()
        query_s = time.perf_counter() - t0
        n = dist.shape[0]
        mean, worst = dist.mean(axis=1), dist.max(axis=1)
        on = worst <= opt.threshold
        run_io.replace_file(path, lambda tmp: np.savez(tmp, dist=dist, mean=mean, max=worst, tri=tri, on_surface=on))
        report = {"path": path, "lines": n, "on_surface": int(on.sum()), "mean": float(mean.mean()) if n else float("nan"),
                  "median": float(np.median(mean)) if n else float("nan"), "samples": opt.samples, "threshold": opt.threshold,
                  "triangles": scene.nf, "query_s": query_s}
        print("{}: {} / {} lines on the surface (every one of {} samples within {:g}); mean distance {:.6g}, median {:.6g} ({} triangles, {:.3f} s)".format(
            path, report["on_surface"], n, opt.samples, opt.threshold, report["mean"], report["median"], scene.nf, query_s), flush=True)
    else:
        dist, tri, point, _ = closest(scene, torch.from_numpy(queries), opt.max_dist)
        dist, tri, point = dist.cpu().numpy(), tri.cpu().numpy(), point.cpu().numpy()
        query_s = time.perf_counter() - t0
        n = dist.shape[0]
        run_io.replace_file(path, lambda tmp: np.savez(tmp, dist=dist, tri=tri, point=point))
        report = {"path": path, "points": n, "acc": float(dist.mean()) if n else float("nan"), "median": float(np.median(dist)) if n else float("nan"),
                  "prec": float((dist < opt.threshold).mean()) if n else float("nan"), "threshold": opt.threshold, "triangles": scene.nf,
                  "query_s": query_s}
        print("{}: {} points; Acc {:.6g}, median {:.6g}, Prec {:.4f} (nearer than {:g}) ({} triangles, {:.3f} s)".format(
            path, n, report["acc"], report["median"], report["prec"], opt.threshold, scene.nf, query_s), flush=True)
    if opt.json:
        print(json.dumps(report), flush=True)
    return 0


def main(argv=None):
    opt = parse_args(argv)
    return {"check": main_check, "analysis": main_analysis, "distance": main_distance}[opt.command](opt)


if __name__ == "__main__":
    sys.exit(main())
