"""Score a reconstruction against ground truth on the device (the reference's code/evaluation/eval-dtu.py, eval-lsr-dtu.py,
eval-wfr-dtu.py and eval-abc.py; those need open3d, sklearn, GPUtil and trimesh, none of which is imported here):

    python -m neat_amd.evaluate dtu-mesh      --data surface_2000.ply --scan 24 --dataset_dir <DTU> [--mode mesh|pcd] [--vis_out_dir DIR]
    python -m neat_amd.evaluate dtu-lines     --data <name>-wfi_checked.npz --scan 24 --cam cameras.npz --dataset_dir <DTU> [--score S]
    python -m neat_amd.evaluate dtu-junctions --data <name>-neat.pth --scan 24 --cam cameras.npz --dataset_dir <DTU>
    python -m neat_amd.evaluate abc           --data <name>-neat.pth | <name>-wf3d.npz --scan <scan dir with lines.json and offset_scale.txt>

Flags and defaults are the reference's; every sub-command also takes --seed (the permutation of the shuffle that precedes the thinning;
the reference draws an unseeded one), --gpu (a device index), --obs (an .npz with ObsMask, BB, Res, P instead of the two .mat files),
--stl (the ground-truth cloud instead of <dataset_dir>/Points/stl/stl{scan:03}_total.ply) and --json (one JSON object: the result and
the seconds per stage).  With the same permutation the numbers are the reference's: every decision is taken on float64 quantities
computed in its order (csrc/kernels_eval.hpp).  There is no host fallback.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

from . import _lib, ply, run_io
from ._lib import ptr as _p, stream as _stream

DENSE_MAX_FACTOR = 4          # a dense box is used while it has at most this many cells per point (and at least 4096 are always allowed)
MAX_DIM = 1 << 20             # cells per axis the kernels index
THIN_BATCH = 8                # thinning rounds between two reads of the undecided counters


# ------------------------------------------------------------------ files
def load_obs(dataset_dir=None, scan=None, npz=None):
    """-> dict(ObsMask [a,b,c], BB [2,3], Res, P [4]) from <dataset_dir>/ObsMask/ObsMask{scan}_10.mat and Plane{scan}.mat (scipy.io.loadmat),
    or from one .npz with the same four arrays."""
    if npz is not None:
        z = np.load(npz)
        missing = [k for k in ("ObsMask", "BB", "Res", "P") if k not in z.files]
        if missing:
            raise KeyError("%s: missing %s" % (npz, ", ".join(missing)))
        m = {k: z[k] for k in ("ObsMask", "BB", "Res", "P")}
    else:
        from scipy.io import loadmat
        a = loadmat(os.path.join(dataset_dir, "ObsMask", "ObsMask%d_10.mat" % scan))
        m = {k: a[k] for k in ("ObsMask", "BB", "Res")}
        m["P"] = loadmat(os.path.join(dataset_dir, "ObsMask", "Plane%d.mat" % scan))["P"]
    if np.asarray(m["ObsMask"]).ndim != 3 or np.asarray(m["BB"]).shape != (2, 3) or np.asarray(m["P"]).size != 4:
        raise ValueError("ObsMask [a,b,c], BB [2,3], Res scalar, P of four numbers expected")
    return {"ObsMask": np.asarray(m["ObsMask"]), "BB": np.asarray(m["BB"]), "Res": float(np.asarray(m["Res"]).reshape(-1)[0]),
            "P": np.asarray(m["P"], dtype=np.float64).reshape(4)}


# ------------------------------------------------------------------ device pieces
def _dev_points(x, device=None):
    """arrays and tensors -> contiguous float64 [n,3] on the device (no host fallback: a CPU tensor without a device to go to raises)."""
    t = torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = t.detach().to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    if not t.is_cuda:
        raise RuntimeError("neat_amd.evaluate runs on the device only")
    return t


def sample_mesh(verts, faces, density=0.2):
    """eval-dtu.py:48-71 -> float64 [nv + ns, 3] on the device: the vertices, then the lattice samples of every triangle of non-zero
    area in the reference's order."""
    v = _dev_points(verts)
    f = (torch.as_tensor(np.asarray(faces)) if not torch.is_tensor(faces) else faces).detach().to(device=v.device, dtype=torch.int32)
    f = f.reshape(-1, 3).contiguous()
    lib = _lib.lib()
    nv, nf = v.shape[0], f.shape[0]
    ws = torch.empty(max(int(lib.neat_eval_tri_ws_bytes(nf)), 8), device=v.device, dtype=torch.uint8)
    total = torch.empty(1, device=v.device, dtype=torch.int32)
    _lib.check(lib.neat_eval_tri_count(_p(v), nv, _p(f), nf, float(density), _p(ws), _p(total), _stream()), "neat_eval_tri_count")
    ns = int(total.item())          # the one read-back: the count sizes the output
    if ns < 0:
        raise RuntimeError("sample_mesh: a face index out of range, a triangle with more than 30000 lattice steps on a side, "
                           "or more samples than int32 indexes")
    out = torch.empty(nv + ns, 3, device=v.device, dtype=torch.float64)
    out[:nv] = v
    if ns:
        _lib.check(lib.neat_eval_tri_emit(_p(v), nv, _p(f), nf, float(density), _p(ws), ctypes.c_void_p(out.data_ptr() + 24 * nv), ns, _stream()),
                   "neat_eval_tri_emit")
    return out


class Grid:
    """A uniform cell grid over a device cloud (neat_eval_grid); keeps the tensors the descriptor points to alive."""

    def __init__(self, points, cell, min_cell=None):
        lib = _lib.lib()
        self.points = points
        n, dev = points.shape[0], points.device
        if n and not bool(torch.isfinite(points).all()):
            raise ValueError("a cloud with non-finite coordinates cannot be gridded")
        lo = points.min(0).values.tolist() if n else [0.0] * 3
        hi = points.max(0).values.tolist() if n else [0.0] * 3
        span = max(h - l for l, h in zip(lo, hi))
        cell = max(float(cell), span / (MAX_DIM - 2), np.finfo(np.float64).tiny)
        dim = [min(int((h - l) / cell) + 1, MAX_DIM) for l, h in zip(lo, hi)]
        cells = dim[0] * dim[1] * dim[2]
        self.dense = cells <= max(DENSE_MAX_FACTOR * n, 4096)
        buckets = cells if self.dense else 1 << max(int(2 * n - 1).bit_length(), 10)
        self.cell, self.dim, self.buckets = cell, dim, buckets
        self.start = torch.empty(buckets + 1, device=dev, dtype=torch.int32)
        self.sidx = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
        self.spts = torch.empty(max(n, 1), 3, device=dev, dtype=torch.float64)
        self.c = _lib.EvalGrid((ctypes.c_double * 3)(*lo), cell, (ctypes.c_int * 3)(*dim), buckets, int(self.dense), n,
                               self.start.data_ptr(), self.sidx.data_ptr(), self.spts.data_ptr())
        ws = torch.empty(max(int(lib.neat_eval_grid_ws_bytes(n, buckets)), 8), device=dev, dtype=torch.uint8)
        _lib.check(lib.neat_eval_grid(_p(points), ctypes.byref(self.c), _p(self.start), ctypes.c_void_p(self.sidx.data_ptr()),
                                      ctypes.c_void_p(self.spts.data_ptr()), _p(ws), _stream()), "neat_eval_grid")

    def occupancy(self):
        """mean points per non-empty bucket"""
        used = int((self.start[1:] != self.start[:-1]).sum().item())
        return self.points.shape[0] / max(used, 1)


def thin(points, radius, order=None, return_rounds=False):
    """eval-dtu.py:81-94 with the permutation given: the cloud is visited in the sequence points[order] (order None = as it is) and a
    point stays iff no earlier staying point lies within `radius` (<=, float64).  -> int64 indices into `points` of the staying points,
    in visiting order, on the device: points[thin(...)] is the reference's data_down."""
    pts = _dev_points(points)
    n, dev = pts.shape[0], pts.device
    if order is not None:
        order = torch.as_tensor(np.asarray(order) if not torch.is_tensor(order) else order).to(device=dev, dtype=torch.int64).reshape(-1)
        if order.shape[0] != n or (n and not torch.equal(torch.sort(order).values, torch.arange(n, device=dev))):
            raise ValueError("thin: order must be a permutation of the point indices")
        seq = pts[order].contiguous()
    else:
        seq = pts
    radius = float(radius)
    if not radius >= 0.0 or not np.isfinite(radius):
        raise ValueError("thin: a finite radius >= 0")
    if n == 0:
        kept = torch.zeros(0, device=dev, dtype=torch.int64)
        return (kept, 0) if return_rounds else kept
    lib = _lib.lib()
    grid = Grid(seq, radius * (1.0 + 1e-6))          # a cell a little over the radius: neighbours within it never sit two cells apart
    state = torch.zeros(n, device=dev, dtype=torch.uint8)
    counters = torch.empty(THIN_BATCH, device=dev, dtype=torch.int32)
    rounds, done = 0, False
    while not done:
        if rounds > n + THIN_BATCH:
            raise RuntimeError("thin: %d rounds for %d points: the rounds do not converge" % (rounds, n))
        counters.zero_()
        for k in range(THIN_BATCH):
            _lib.check(lib.neat_eval_thin_round(_p(seq), ctypes.byref(grid.c), radius, _p(state), ctypes.c_void_p(counters.data_ptr() + 4 * k),
                                                _stream()), "neat_eval_thin_round")
        left = counters.tolist()
        for k, c in enumerate(left):
            if c == 0:
                rounds += k + 1
                done = True
                break
        else:
            rounds += THIN_BATCH
    keep = torch.nonzero(state == 1).flatten()
    kept = order[keep] if order is not None else keep
    return (kept, rounds) if return_rounds else kept


def _nearest_cell(cloud):
    """A first cell edge from the cloud's density: about two points per cell if the cloud filled its box (build_nearest_grid shrinks it
    where the cloud is a surface or a curve and fills few cells of that box)."""
    n = cloud.shape[0]
    if n == 0:
        return 1.0
    ext = (cloud.max(0).values - cloud.min(0).values).tolist()
    pos = sorted(e for e in ext if e > 0)
    if not pos:
        return 1.0
    vol = float(np.prod(pos))
    return (2.0 * vol / n) ** (1.0 / len(pos))


def nearest(cloud, queries, max_dist=float("inf"), grid=None):
    """For every query the nearest point of `cloud` within max_dist -> (dist float64 [m], idx int32 [m]) on the device; inf and -1 where
    there is none.  Ties go to the lowest index.  The distance is sqrt(((dx dx) + dy dy) + dz dz) in float64."""
    c = _dev_points(cloud)
    q = _dev_points(queries, c.device)
    m, dev = q.shape[0], c.device
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError("nearest: max_dist >= 0")
    dist = torch.full((m,), float("inf"), device=dev, dtype=torch.float64)
    idx = torch.full((m,), -1, device=dev, dtype=torch.int32)
    if m == 0 or c.shape[0] == 0:
        return dist, idx
    if grid is None:
        grid = build_nearest_grid(c, max_dist)
    _lib.check(_lib.lib().neat_eval_nearest(ctypes.byref(grid.c), _p(q), m, max_dist, _p(dist), _p(idx), _stream()), "neat_eval_nearest")
    return dist, idx


def build_nearest_grid(cloud, max_dist=float("inf")):
    """The grid of a nearest-point query: the cell shrinks while the occupied buckets hold more than 8 points on average, but not under
    max_dist / 16: a query with nothing near walks max_dist / cell rings before it gives up."""
    cell = _nearest_cell(cloud)
    floor = max_dist / 16.0 if np.isfinite(max_dist) else 0.0
    grid = Grid(cloud, max(cell, min(floor, cell * 8.0)))
    for _ in range(4):
        occ = grid.occupancy()
        if occ <= 8.0 or grid.cell <= max(cell * 1e-3, floor):
            break
        grid = Grid(cloud, max(grid.cell / min(max(np.sqrt(occ / 3.0), 1.5), 8.0), floor))
    return grid


def obs_flags(points, obs_mask, bb, res, patch=60.0, f32_quotient=False):
    """eval-dtu.py:98-110 per point -> uint8 [n] on the device: bit 0 = inside the box padded by patch / 2 patch, bit 1 = also in an
    observed voxel.  f32_quotient: the voxel index rounds a float32 quotient (eval-lsr-dtu.py:106, eval-wfr-dtu.py:55)."""
    pts = _dev_points(points)
    dev = pts.device
    bb32 = np.asarray(bb).astype(np.float32)
    lo = (bb32[:1] - patch).astype(np.float64).reshape(3)            # float32 sums, as numpy forms them from a float32 array and a scalar
    hi = (bb32[1:] + patch * 2).astype(np.float64).reshape(3)
    bb0 = bb32[0].astype(np.float64)
    mask = torch.as_tensor(np.ascontiguousarray(np.asarray(obs_mask) != 0).astype(np.uint8)).to(dev) if not torch.is_tensor(obs_mask) \
        else (obs_mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    if mask.dim() != 3:
        raise ValueError("obs_flags: ObsMask [a, b, c]")
    flags = torch.empty(pts.shape[0], device=dev, dtype=torch.uint8)
    d3 = lambda a: (ctypes.c_double * 3)(*[float(v) for v in a])
    _lib.check(_lib.lib().neat_eval_obs_mask(_p(pts), pts.shape[0], d3(lo), d3(hi), d3(bb0), float(res), _p(mask),
                                             (ctypes.c_int * 3)(*mask.shape), int(bool(f32_quotient)), _p(flags), _stream()), "neat_eval_obs_mask")
    return flags


def _mean_below(dist, max_dist):
    sel = dist[dist < max_dist]
    if sel.numel() == 0:
        warnings.warn("Mean of empty slice.", RuntimeWarning, stacklevel=3)          # numpy's words for the same event
        return float("nan")
    return float(sel.mean().item())


def dtu_scores(points, stl, obs_mask, bb, res, plane, density=0.2, patch=60.0, max_dist=20.0, order=None, seed=0, f32_quotient=False,
               thinning=True, timings=None, details=None):
    """Steps 2 to 4 of the DTU scripts on a data cloud -> (mean data->stl, mean stl->data).  order: the permutation of the shuffle
    (None: numpy.random.default_rng(seed).permutation(n)).  thinning=False visits the shuffled cloud whole (eval-wfr-dtu.py:46).
    timings (a dict) receives the seconds per stage; details (a dict) the intermediate device tensors."""
    pts = _dev_points(points)
    dev = pts.device
    stl_d = _dev_points(stl, dev)
    n = pts.shape[0]
    if order is None:
        order = np.random.default_rng(seed).permutation(n)
    order_d = torch.as_tensor(np.asarray(order)).to(device=dev, dtype=torch.int64)

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t = time.perf_counter()
    if thinning:
        data_down = pts[thin(pts, density, order_d)]
    else:
        data_down = pts[order_d]
    t = lap("thin_s", t)
    flags = obs_flags(data_down, obs_mask, bb, res, patch, f32_quotient)
    data_in = data_down[(flags & 1) != 0]
    data_in_obs = data_down[(flags & 2) != 0]
    pl = torch.as_tensor(np.asarray(plane, dtype=np.float64).reshape(4)).to(dev)
    # (P * [x, y, z, 1]).sum(-1) > 0 in numpy's order, every product and sum rounded on its own
    above = (((pl[0] * stl_d[:, 0] + pl[1] * stl_d[:, 1]) + pl[2] * stl_d[:, 2]) + pl[3] * torch.ones_like(stl_d[:, 0])) > 0
    stl_above = stl_d[above]
    t = lap("mask_s", t)
    dist_d2s, _ = nearest(stl_d, data_in_obs, max_dist)
    mean_d2s = _mean_below(dist_d2s, max_dist)
    t = lap("d2s_s", t)
    dist_s2d, _ = nearest(data_in, stl_above, max_dist)
    mean_s2d = _mean_below(dist_s2d, max_dist)
    lap("s2d_s", t)
    if details is not None:
        details.update(data_down=data_down, flags=flags, above=above, dist_d2s=dist_d2s, dist_s2d=dist_s2d)
    return mean_d2s, mean_s2d


def line_cost(pred, gt, ends):
    """eval-abc.py:43 (ends = 1: points [n,3]) / :86-88 (ends = 2: lines [n,2,3]) -> cost float64 [n_pred, n_gt] on the device."""
    p = _dev_points(pred)
    g = _dev_points(gt, p.device)
    n_pred, n_gt = p.shape[0] // ends, g.shape[0] // ends
    cost = torch.empty(n_pred, n_gt, device=p.device, dtype=torch.float64)
    _lib.check(_lib.lib().neat_eval_line_cost(_p(p), n_pred, _p(g), n_gt, int(ends), _p(cost), _stream()), "neat_eval_line_cost")
    return cost


def _assigned_cost(cost):
    from . import ops
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return cost.new_zeros(0)
    rows, cols, n_match = ops.linear_sum_assignment(cost.float())
    k = int(n_match.item())
    return cost[rows[:k], cols[:k]]


ABC_THRESHOLDS = (0.01, 0.02, 0.05)


def abc_scores(junctions_pred, lines_pred, junctions_gt, edges_gt, offset_scale):
    """eval-abc.py -> dict(junctions_precision, junctions_recall, lines_precision, lines_recall: three numbers each, at 0.01, 0.02 and
    0.05 x scale; junctions_correct / lines_correct: the counts).  offset_scale: the four numbers of offset_scale.txt."""
    off = [float(v) for v in offset_scale]
    s = 1.0 / off[-1]
    scale_mat = np.array([[s, 0, 0, -off[0]], [0, s, 0, -off[1]], [0, 0, s, -off[2]], [0, 0, 0, 1.0]])
    jp = np.asarray(torch.as_tensor(junctions_pred).detach().cpu().numpy()).reshape(-1, 3)
    lp = np.asarray(torch.as_tensor(lines_pred).detach().cpu().numpy()).reshape(-1, 3)
    jg = np.asarray(junctions_gt, dtype=np.float64).reshape(-1, 3)
    lg = jg[np.asarray(edges_gt, dtype=np.int64).reshape(-1, 2)]
    jps = (jp @ scale_mat[:3, :3].T) + scale_mat[:3, 3]              # a few dozen rows: the reference's own numpy expression
    lps = ((lp @ scale_mat[:3, :3].T) + scale_mat[:3, 3]).reshape(-1, 2, 3)
    global_scale = scale_mat[0, 0]
    res = {}
    for name, pred, gt, ends, n_pred, n_gt in (("junctions", jps, jg, 1, jp.shape[0], jg.shape[0]),
                                               ("lines", lps, lg, 2, lps.shape[0], lg.shape[0])):
        cost = _assigned_cost(line_cost(pred, gt, ends))
        correct = [int((cost < th * global_scale).sum().item()) for th in ABC_THRESHOLDS]
        res[name + "_correct"] = correct
        res[name + "_precision"] = [c / n_pred if n_pred else float("nan") for c in correct]
        res[name + "_recall"] = [c / n_gt if n_gt else float("nan") for c in correct]
    return res


def abc_lines(res):
    """The two lines eval-abc.py prints: precision then recall at the three thresholds, '{:.3f}' joined by ' & '."""
    fmt = lambda v: " & ".join("{:.3f}".format(x) for x in v)
    return fmt(res["junctions_precision"] + res["junctions_recall"]), fmt(res["lines_precision"] + res["lines_recall"])


# ------------------------------------------------------------------ the four scripts
def _scale_points(scale_mat, x):
    """global_scale_mat @ [x, 1] rows 0..2 (eval-lsr-dtu.py:80-81), numpy's expression on the host (a few thousand rows)."""
    h = scale_mat @ np.concatenate([x, np.ones([x.shape[0], 1])], axis=-1).T
    return h[:3].transpose(1, 0)


def line_cloud(lines3d, scale_mat):
    """eval-lsr-dtu.py:64-81 -> (cloud float64 [32 n, 3], mean length after the scale matrix)."""
    lines3d = np.asarray(lines3d)
    e = np.concatenate((lines3d.reshape(-1, 3), np.ones((lines3d.shape[0] * 2, 1))), axis=1)
    e = scale_mat @ e.transpose()
    e = (e[:3] / e[3:]).transpose().reshape(-1, 2, 3)
    mean_length = float(np.mean(np.linalg.norm(e[:, 0] - e[:, 1], axis=1))) if lines3d.shape[0] else float("nan")
    t = np.linspace(0, 1, 32).reshape(1, -1, 1)
    pts = (lines3d[:, :1] * t) + (lines3d[:, 1:] * (1 - t))
    pts = pts.reshape(-1, 3)
    return np.ascontiguousarray(_scale_points(scale_mat, pts), dtype=np.float64), mean_length


def junction_cloud(lines3d, scale_mat):
    """eval-wfr-dtu.py:111-112 and :31-32: the unique end points (torch.unique's row order) through the scale matrix."""
    j = torch.as_tensor(np.asarray(lines3d) if not torch.is_tensor(lines3d) else lines3d).detach().cpu().reshape(-1, 3).unique(dim=0).numpy()
    return np.ascontiguousarray(_scale_points(scale_mat, j), dtype=np.float64), j.shape[0]


def _common(ap, dtu=True):
    ap.add_argument("--seed", type=int, default=0, help="the permutation of the shuffle before the thinning")
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    ap.add_argument("--json", default=False, action="store_true", help="print one JSON object: the result and the seconds per stage")
    if dtu:
        ap.add_argument("--obs", type=str, default=None, help="an .npz with ObsMask, BB, Res, P instead of the two .mat files")
        ap.add_argument("--stl", type=str, default=None, help="ground-truth cloud (default <dataset_dir>/Points/stl/stl{scan:03}_total.ply)")
        ap.add_argument("--downsample_density", type=float, default=0.2)
        ap.add_argument("--patch_size", type=float, default=60)
        ap.add_argument("--max_dist", type=float, default=20)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.evaluate")
    sub = ap.add_subparsers(dest="command", required=True)
    m = sub.add_parser("dtu-mesh", help="eval-dtu.py")
    m.add_argument("--data", type=str, default="data_in.ply")
    m.add_argument("--scan", type=int, default=1)
    m.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    m.add_argument("--dataset_dir", type=str, default=".")
    m.add_argument("--vis_out_dir", type=str, default=None, help="write vis_{scan:03}_d2s.ply and vis_{scan:03}_s2d.ply there")
    m.add_argument("--visualize_threshold", type=float, default=10)
    _common(m)
    for name, helptext in (("dtu-lines", "eval-lsr-dtu.py"), ("dtu-junctions", "eval-wfr-dtu.py")):
        s = sub.add_parser(name, help=helptext)
        s.add_argument("--data", type=str, required=True, help="the path of the reconstructed wireframe model")
        s.add_argument("--scan", type=int, default=1)
        s.add_argument("--cam", type=str, default=None, help="the path of cam")
        s.add_argument("--score", type=float, default=None)
        s.add_argument("--threshold", type=float, default=1., help="dist to surface threshold")
        s.add_argument("--dataset_dir", type=str, default="/home/xn/datasets/DTU")
        s.add_argument("--noscale", default=False, action="store_true")
        _common(s)
    a = sub.add_parser("abc", help="eval-abc.py")
    a.add_argument("--data", type=str, required=True, help="the path of the reconstructed wireframe model")
    a.add_argument("--scan", type=str, required=True, help="the path of the scan dir")
    _common(a, dtu=False)
    return ap


def _dtu_inputs(opt):
    obs = load_obs(opt.dataset_dir, opt.scan, opt.obs)
    stl_path = opt.stl or os.path.join(opt.dataset_dir, "Points", "stl", "stl%03d_total.ply" % opt.scan)
    return obs, ply.read_ply(stl_path)["points"]


def _scale_mat(opt):
    if opt.noscale:
        return np.eye(4)
    cam = opt.cam if opt.cam is not None else "../data/DTU/scan{}/cameras.npz".format(opt.scan)
    return np.load(cam)["scale_mat_0"]


def _averaged(details, max_dist):
    """the number of distances each of the two means averages"""
    return [int((details[k] < max_dist).sum().item()) for k in ("dist_d2s", "dist_s2d")]


def _emit(opt, result, timings, lines):
    if opt.json:
        print(json.dumps(dict(result, seconds=timings)), flush=True)
    else:
        for l in lines:
            print(l, flush=True)


def run_dtu_mesh(opt, dev):
    timings = {"sample_s": 0.0}
    data = ply.read_ply(opt.data)
    obs, stl = _dtu_inputs(opt)
    if opt.mode == "mesh":
        if data["faces"] is None:
            raise SystemExit("%s has no faces: --mode pcd evaluates a point cloud" % opt.data)
        t0 = time.perf_counter()
        cloud = sample_mesh(torch.as_tensor(data["points"]).to(dev), torch.as_tensor(data["faces"]).to(dev), opt.downsample_density)
        torch.cuda.synchronize(dev)
        timings["sample_s"] = time.perf_counter() - t0
    else:
        cloud = _dev_points(data["points"], dev)
    details = {}
    acc, comp = dtu_scores(cloud, stl, obs["ObsMask"], obs["BB"], obs["Res"], obs["P"], opt.downsample_density, opt.patch_size, opt.max_dist,
                           seed=opt.seed, timings=timings, details=details)
    overall = (acc + comp) / 2
    with open(opt.data[:-4] + ".txt", "w") as f:
        f.writelines("{}\t{}\t{}".format(acc, comp, overall))
    if opt.vis_out_dir:
        write_vis(opt, details, stl)
    _emit(opt, {"acc": acc, "comp": comp, "overall": overall, "points": int(cloud.shape[0]), "thinned": int(details["data_down"].shape[0]),
                "averaged": _averaged(details, opt.max_dist)}, timings, ["{} {} {}".format(acc, comp, overall)])
    return 0


def vis_colors(details, n_stl, visualize_threshold=10.0, max_dist=20.0):
    """eval-dtu.py:137-152 -> (colours of data_down, colours of the stl cloud), float64 [n,3] in [0, 1]: white to red up to the threshold,
    green at or beyond max_dist (the capped query answers inf there), blue = not scored."""
    R, G, B, W = (np.array([c], dtype=np.float64) for c in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]))
    out = []
    for n, sel, dist in ((details["data_down"].shape[0], (details["flags"] & 2) != 0, details["dist_d2s"]),
                         (n_stl, details["above"], details["dist_s2d"])):
        d = dist.cpu().numpy().reshape(-1, 1)
        color = np.tile(B, (n, 1))
        alpha = d.clip(max=visualize_threshold) / visualize_threshold
        where = np.where(sel.cpu().numpy())[0]
        color[where] = R * alpha + W * (1 - alpha)
        color[where[d[:, 0] >= max_dist]] = G
        out.append(color)
    return out


def write_vis(opt, details, stl):
    """The two clouds of eval-dtu.py:137-152 coloured by error: vis_{scan:03}_d2s.ply and vis_{scan:03}_s2d.ply under --vis_out_dir."""
    colors = vis_colors(details, stl.shape[0], opt.visualize_threshold, opt.max_dist)
    os.makedirs(opt.vis_out_dir, exist_ok=True)
    for name, pts, color in (("d2s", details["data_down"].cpu().numpy(), colors[0]), ("s2d", stl, colors[1])):
        ply.write_ply_cloud(os.path.join(opt.vis_out_dir, "vis_%03d_%s.ply" % (opt.scan, name)), pts, color)


def run_dtu_lines(opt, dev):
    lines3d, scores = run_io.load_lines(opt.data)          # float64: line_cloud computes in float64 whatever the file holds
    if opt.score is not None:
        if scores is None:
            raise SystemExit("--score needs the key `scores` in %s" % opt.data)
        lines3d = lines3d[scores < opt.score]
    obs, stl = _dtu_inputs(opt)
    cloud, mean_length = line_cloud(lines3d, _scale_mat(opt))
    timings, details = {"sample_s": 0.0}, {}
    acc, comp = dtu_scores(torch.as_tensor(cloud).to(dev), stl, obs["ObsMask"], obs["BB"], obs["Res"], obs["P"], opt.downsample_density,
                           opt.patch_size, opt.max_dist, seed=opt.seed, f32_quotient=True, timings=timings, details=details)
    n = int(lines3d.shape[0])
    _emit(opt, {"acc": acc, "comp": comp, "mean_length": mean_length, "num_lines": n, "averaged": _averaged(details, opt.max_dist)}, timings,
          ["ACC {}".format(acc), "COMP {}".format(comp), "mean length:  {}".format(mean_length), "num lines:  {}".format(n),
           str(acc), str(comp), str(mean_length), str(n)])
    return 0


def run_dtu_junctions(opt, dev):
    lines3d = run_io.load_lines(opt.data)[0]
    obs, stl = _dtu_inputs(opt)
    cloud, n = junction_cloud(lines3d, _scale_mat(opt))
    timings, details = {"sample_s": 0.0}, {}
    acc, comp = dtu_scores(torch.as_tensor(cloud).to(dev), stl, obs["ObsMask"], obs["BB"], obs["Res"], obs["P"], opt.downsample_density,
                           opt.patch_size, opt.max_dist, seed=opt.seed, f32_quotient=True, thinning=False, timings=timings, details=details)
    _emit(opt, {"acc": acc, "comp": comp, "num_junctions": n, "averaged": _averaged(details, opt.max_dist)}, timings,
          ["initial junctions: \t ACC = {} \t COMP = {}".format(acc, comp), "num junctions: {}".format(n)])
    return 0


def run_abc(opt, dev):
    if opt.data.lower().endswith(".npz"):           # triangulate --wireframe: the junctions and the edges' segments of a checkpoint-free wireframe
        with np.load(opt.data) as z:
            data = {"junctions3d_initial": np.asarray(z["junctions3d"], dtype=np.float64).reshape(-1, 3),
                    "lines3d_wfi_checked": np.asarray(z["lines3d"], dtype=np.float64).reshape(-1, 2, 3)}
    else:
        data = torch.load(opt.data, map_location="cpu")
    junctions, edges = run_io.read_lines_json(os.path.join(opt.scan, "lines.json"))
    offset_scale = run_io.read_offset_scale(os.path.join(opt.scan, "offset_scale.txt"))
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        res = abc_scores(data["junctions3d_initial"], data["lines3d_wfi_checked"], junctions, edges, offset_scale)
    torch.cuda.synchronize(dev)
    _emit(opt, res, {"abc_s": time.perf_counter() - t0}, abc_lines(res))
    return 0


def main(argv=None):
    opt = build_parser().parse_args(argv)
    _lib.lib()                      # a missing library is an error before any file is read
    torch.cuda.set_device(opt.gpu)
    dev = torch.device("cuda", opt.gpu)
    return {"dtu-mesh": run_dtu_mesh, "dtu-lines": run_dtu_lines, "dtu-junctions": run_dtu_junctions, "abc": run_abc}[opt.command](opt, dev)


if __name__ == "__main__":
    sys.exit(main())
