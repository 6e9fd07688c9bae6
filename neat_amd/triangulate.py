"""3-D line segments straight from calibrated views and their 2-D segments, on the device: no checkpoint, no training.  This is the
baseline the reference scores itself against (its L3dpp-*.npz files come from Line3D++, which it does not ship), a seconds-long check
that cameras.npz and the detections agree, and a line soup that post, raycast check, show and evaluate read.

    python -m neat_amd.triangulate --conf <conf> [--data_root ../data] [--scan_id N] [--views a:b:step]
            [--neighbours 6] [--min-views 3] [--min-score 1.5] [--sigma 2.5] [--overlap 0.25] [--angle 5] [--out PATH]

builds the conf's dataset and writes `<instance dir>/<line_detector>-l3d.npz` with lines3d [N,2,3], views [N] (the distinct views of a
line), support [N] (the consensus score of its axis member; not `scores`, which evaluate --score reads as lower-is-better) and cameras
[V,4,4] (the camera-to-world poses used).  One summary line: views, segments, hypotheses, estimates, lines, seconds.

    ... --wireframe [--end-frac 0.2] [--reach 0.25] [--min-votes 2] [--junction-angle 10]

reads the views as graphs (their 2-D junctions are shared: detect --junctions) and writes `<instance dir>/<line_detector>-wf3d.npz`
instead: the 3-D wireframe whose line ends that share a 2-D vertex in enough views are one junction.  lines3d [E,2,3] holds
the edges' segments, so every tool that reads the line soup reads this file, and its unique end points are the junctions; beside it
junctions3d [J,3], edges [E,2], degree, kind, votes [J], src [E] (the triangulated line of an edge), views, support [E], cameras.

    triangulate.lines(segments, Ks, poses, **thresholds)         # -> dict of device tensors
    triangulate.hypotheses(segments, Ks, poses, neighbours=6, angle_min=5.0, overlap_min=0.25)      # the pair test alone
    triangulate.wireframe(vertices, edges, Ks, poses, **thresholds, end_frac=0.2, reach=0.25, min_votes=2, angle=10.0)
    triangulate.junctions3d(lines3d, support, members, estimate, endv, view, V, NV, ...)            # the junction rule alone, on lines' arrays

segments: one device tensor [n_v,4] = x1 y1 x2 y2 in pixels per view; Ks [V,3,3]; poses [V,4,4] camera-to-world.  The rule is DESIGN 3k;
csrc/kernels_triangulate.hpp implements it and tests/triangulate_f64.py restates it.  There is no CPU path: CPU tensors are refused.
"""
import argparse
import functools
import math
import os
import sys
import time

import numpy as np
import torch

from . import _lib, run_io

DEFAULTS = {"neighbours": 6, "angle_min": 5.0, "overlap_min": 0.25, "sigma_px": 2.5, "min_score": 1.5, "min_views": 3}
CAM = 48                     # doubles per view in the camera block
MAX_HYPOTHESES = (2 ** 31 - 1) // 2
WIREFRAME_DEFAULTS = {"end_frac": 0.2, "reach": 0.25, "min_votes": 2, "angle": 10.0}
WIREFRAME_KEYS = ("junctions3d", "degree", "kind", "votes", "spread", "edges3d", "esrc", "lines3d_wf")


def _np64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    elif isinstance(x, (list, tuple)) and len(x) and torch.is_tensor(x[0]):
        x = np.stack([t.detach().cpu().numpy() for t in x])
    return np.asarray(x, dtype=np.float64)


def camera_block(Ks, poses):
    """Ks [V,3,3] (upper triangular, last row 0 0 1), poses [V,4,4] camera-to-world -> float64 [V,48]: K^-1 in closed form [9], R =
    pose[:3,:3]^T [9], t = -R C [3], K [9], P = K [R|t] [12], C = pose[:3,3] [3], 3 unused.  Every sum is written out in the order the
    reference writes it."""
    K = _np64(Ks).reshape(-1, 3, 3)
    T = _np64(poses).reshape(-1, 4, 4)
    if K.shape[0] != T.shape[0]:
        raise ValueError(f"triangulate: {K.shape[0]} intrinsics for {T.shape[0]} poses")
    V = K.shape[0]
    if V and (np.any(K[:, 1, 0] != 0.0) or np.any(K[:, 2, :2] != 0.0) or np.any(K[:, 2, 2] != 1.0)):
        raise ValueError("triangulate: intrinsics must be upper triangular with last row 0 0 1")
    C = T[:, :3, 3]
    R = np.ascontiguousarray(T[:, :3, :3].transpose(0, 2, 1))
    t = -((R[:, :, 0] * C[:, None, 0] + R[:, :, 1] * C[:, None, 1]) + R[:, :, 2] * C[:, None, 2])
    fx, sk, cx, fy, cy = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    Ki = np.zeros((V, 3, 3))
    Ki[:, 0, 0] = 1.0 / fx
    Ki[:, 0, 1] = -sk / (fx * fy)
    Ki[:, 0, 2] = (sk * cy - cx * fy) / (fx * fy)
    Ki[:, 1, 1] = 1.0 / fy
    Ki[:, 1, 2] = -cy / fy
    Ki[:, 2, 2] = 1.0
    Rt = np.concatenate([R, t[:, :, None]], axis=2)
    P = (K[:, :, 0, None] * Rt[:, None, 0, :] + K[:, :, 1, None] * Rt[:, None, 1, :]) + K[:, :, 2, None] * Rt[:, None, 2, :]
    cam = np.zeros((V, CAM))
    cam[:, 0:9] = Ki.reshape(V, 9)
    cam[:, 9:18] = R.reshape(V, 9)
    cam[:, 18:21] = t
    cam[:, 21:30] = K.reshape(V, 9)
    cam[:, 30:42] = P.reshape(V, 12)
    cam[:, 42:45] = C
    return cam


def neighbour_table(centres, M):
    """centres [V,3] -> int32 [V, min(M, V - 1)]: the nearest other views of each view, nearest first, ties to the lower index."""
    C = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    V = C.shape[0]
    M = max(0, min(int(M), V - 1))
    if M == 0:
        return np.zeros((V, 0), dtype=np.int32)
    d = C[:, None, :] - C[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    dist[np.arange(V), np.arange(V)] = np.inf
    return np.ascontiguousarray(np.argsort(dist, axis=1, kind="stable")[:, :M].astype(np.int32))


def _check_segments(segments, device):
    if torch.is_tensor(segments):
        raise RuntimeError("triangulate: segments is one tensor [n,4] per view, in a list")
    segments = list(segments)
    for s in segments:
        if not torch.is_tensor(s) or not s.is_cuda:
            raise RuntimeError("neat_amd.triangulate needs CUDA tensors (there is no CPU path)")
        if s.dim() != 2 or s.shape[1] != 4:
            raise RuntimeError(f"triangulate: segments [n,4] per view, got {tuple(s.shape)}")
    if segments:
        device = segments[0].device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return segments, torch.device(device)


class _Match:
    """The inputs on the device, the workspace and the hypothesis list of one call."""

    def __init__(self, segments, Ks, poses, neighbours, angle_min, overlap_min, device=None):
        segments, dev = _check_segments(segments, device)
        if dev.type != "cuda":
            raise RuntimeError("neat_amd.triangulate needs CUDA tensors (there is no CPU path)")
        cam = camera_block(Ks, poses)
        V = cam.shape[0]
        if V != len(segments):
            raise ValueError(f"triangulate: {len(segments)} views of segments for {V} cameras")
        if neighbours < 0:
            raise ValueError(f"triangulate: neighbours {neighbours} is negative")
        nb = neighbour_table(cam[:, 42:45], neighbours)
        counts = [int(s.shape[0]) for s in segments]
        self.V, self.M, self.S, self.nmax = V, int(nb.shape[1]), sum(counts), max(counts, default=0)
        self.device = dev
        self.cos_min = math.cos(float(angle_min) * math.pi / 180.0)
        self.overlap_min = float(overlap_min)
        lib = _lib.lib()
        nbytes = lib.neat_tri_scratch_bytes(self.V, self.S, self.M, self.nmax) if self.S < 2 ** 31 else 0
        if nbytes == 0 and self.S > 0:               # without segments the workspace is empty; the calls still check the counts
            raise RuntimeError(f"triangulate: {V} views of {self.S} segments with {self.M} neighbours are beyond what one call indexes; pass fewer views")
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            self.cam = torch.from_numpy(cam).to(dev)
            self.nb = torch.from_numpy(nb).to(dev)
            self.segoff = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
            self.seg = (torch.cat([s.to(torch.float64) for s in segments]) if segments else torch.empty(0, 4, device=dev, dtype=torch.float64)).contiguous()
            self.ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            self.view, self.hoff = i32(self.S), i32(self.S + 1)
            total = torch.empty(1, device=dev, dtype=torch.int64)
            _lib.check(lib.neat_tri_count(_lib.ptr(self.seg), _lib.ptr(self.segoff), self.V, self.S, self.nmax, _lib.ptr(self.nb), self.M,
                                          _lib.ptr(self.cam), self.cos_min, self.overlap_min, _lib.ptr(self.ws), _lib.ptr(self.view),
                                          _lib.ptr(self.hoff), _lib.ptr(total), _lib.stream()), "neat_tri_count")
            self.H = H = int(total.item())              # the one read-back before the end: the list's length
            if H > MAX_HYPOTHESES:
                raise RuntimeError(f"triangulate: {H} hypotheses are beyond what one call indexes; pass fewer views or neighbours")
            self.hyp_m, self.hyp_j = i32(H), i32(H)
            self.hyp_s = torch.empty(H, 2, device=dev, dtype=torch.float64)
            _lib.check(lib.neat_tri_fill(_lib.ptr(self.segoff), self.V, self.S, self.nmax, _lib.ptr(self.nb), self.M, _lib.ptr(self.cam),
                                         self.cos_min, self.overlap_min, _lib.ptr(self.ws), H, _lib.ptr(self.hyp_m), _lib.ptr(self.hyp_j),
                                         _lib.ptr(self.hyp_s), _lib.stream()), "neat_tri_fill")

    def rows(self):
        """int32 [H,4] = (view a, segment i of a, slot m, segment j of the slot's view), in list order."""
        counts = (self.hoff[1:] - self.hoff[:-1]).to(torch.int64)
        g = torch.repeat_interleave(torch.arange(self.S, device=self.device), counts, output_size=self.H)
        a = self.view[g].to(torch.int64)
        i = g - self.segoff[a].to(torch.int64)
        return torch.stack([a.to(torch.int32), i.to(torch.int32), self.hyp_m, self.hyp_j], dim=1)


def hypotheses(segments, Ks, poses, neighbours=DEFAULTS["neighbours"], angle_min=DEFAULTS["angle_min"], overlap_min=DEFAULTS["overlap_min"],
               device=None):
    """The pair test alone -> (rows int32 [H,4] = a, i, m, j; depths float64 [H,2] = s_1, s_2; neighbours int32 [V,M])."""
    mt = _Match(segments, Ks, poses, neighbours, angle_min, overlap_min, device)
    return mt.rows(), mt.hyp_s, mt.nb


def lines(segments, Ks, poses, neighbours=DEFAULTS["neighbours"], angle_min=DEFAULTS["angle_min"], overlap_min=DEFAULTS["overlap_min"],
          sigma_px=DEFAULTS["sigma_px"], min_score=DEFAULTS["min_score"], min_views=DEFAULTS["min_views"], device=None):
    """-> dict of device tensors.  Per line, in label order: lines3d float64 [N,2,3], views int32 [N], support float64 [N].  Per 2-D
    segment, in (view, index) order: estimate float64 [S,2,3], score float64 [S], kept bool [S], labels int32 [S] (the component's lowest
    kept segment, -1 when not kept), members int32 [S] (the segment's line, -1 for none).  Also rows [H,4], depths [H,2] of the
    hypotheses and offsets int32 [V+1].  Two synchronisations: the hypothesis count, and the line count at the end."""
    if not sigma_px > 0.0:
        raise ValueError(f"triangulate: sigma_px {sigma_px} must be positive")
    mt = _Match(segments, Ks, poses, neighbours, angle_min, overlap_min, device)
    dev, S = mt.device, mt.S
    f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
    estimate, score, kept, label, members = f64(S, 2, 3), f64(S), i32(S), i32(S), i32(S)
    lines3d, views, support, n_lines = f64(S, 2, 3), i32(S), f64(S), i32(1)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().neat_tri_lines(_lib.ptr(mt.segoff), mt.V, S, mt.nmax, _lib.ptr(mt.nb), mt.M, _lib.ptr(mt.cam), _lib.ptr(mt.ws),
                                             _lib.ptr(mt.view), _lib.ptr(mt.hoff), mt.H, _lib.ptr(mt.hyp_m), _lib.ptr(mt.hyp_j),
                                             _lib.ptr(mt.hyp_s), float(sigma_px), float(min_score), int(min_views), _lib.ptr(estimate),
                                             _lib.ptr(score), _lib.ptr(kept), _lib.ptr(label), _lib.ptr(members), _lib.ptr(lines3d),
                                             _lib.ptr(views), _lib.ptr(support), _lib.ptr(n_lines), _lib.stream()), "neat_tri_lines")
        N = int(n_lines.item())
    return {"lines3d": lines3d[:N].clone(), "views": views[:N].clone(), "support": support[:N].clone(), "members": members, "labels": label,
            "estimate": estimate, "score": score, "kept": kept != 0, "rows": mt.rows(), "depths": mt.hyp_s, "offsets": mt.segoff,
            "neighbours": mt.nb}


def check_wireframe_options(end_frac, reach, min_votes, angle):
    if not (0.0 < end_frac < 0.5 and 0.0 < reach <= 1.0 and 0.0 < angle <= 90.0 and int(min_votes) >= 1):
        raise ValueError(f"triangulate: end_frac {end_frac} in (0, 0.5), reach {reach} in (0, 1], angle {angle} in (0, 90] degrees, "
                         f"min_votes {min_votes} >= 1")


def junctions3d(lines3d, support, members, estimate, endv, view, V, NV, end_frac=WIREFRAME_DEFAULTS["end_frac"],
                reach=WIREFRAME_DEFAULTS["reach"], min_votes=WIREFRAME_DEFAULTS["min_votes"], angle=WIREFRAME_DEFAULTS["angle"], pairs_max=None):
    """The rule of DESIGN 3p on the arrays of lines(): lines3d [N,2,3], support [N], members int32 [S], estimate [S,2,3], with endv int32
    [S,2] the 2-D vertex of each segment end, numbered over all V views in [0, NV), and view int32 [S] -> dict of device tensors:
    junctions3d float64 [J,3], degree, kind, votes int32 [J], spread float64 [J], edges3d int32 [E,2], esrc int32 [E].
    pairs_max: the votes the workspace has room for (default: 8 per segment, what 2-D vertices of nine ends cast, and 4096 at least; a
    scene that casts more is run again with the room it asks for).  One synchronisation: the read of the two counts."""
    check_wireframe_options(end_frac, reach, min_votes, angle)
    tensors = (lines3d, support, members, estimate, endv, view)
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("neat_amd.triangulate needs CUDA tensors (there is no CPU path)")
    dev = lines3d.device
    lines3d, support, estimate = (t.to(torch.float64).contiguous() for t in (lines3d, support, estimate))
    members, endv, view = (t.to(torch.int32).contiguous() for t in (members, endv, view))
    N, S = int(support.shape[0]), int(members.shape[0])
    if tuple(lines3d.shape) != (N, 2, 3) or tuple(estimate.shape) != (S, 2, 3) or tuple(endv.shape) != (S, 2) or tuple(view.shape) != (S,):
        raise RuntimeError(f"triangulate: lines3d [N,2,3], support [N], members [S], estimate [S,2,3], endv [S,2], view [S]; got {[tuple(t.shape) for t in tensors]}")
    lib = _lib.lib()
    f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        out = {"junctions3d": f64(2 * N, 3), "degree": i32(2 * N), "kind": i32(2 * N), "votes": i32(2 * N), "spread": f64(2 * N),
               "edges3d": i32(N, 2), "esrc": i32(N)}
        counts = i32(2)
        room = max(8 * S, 4096) if pairs_max is None else int(pairs_max)
        while True:
            nbytes = lib.neat_wf3d_scratch_bytes(int(V), S, N, int(NV), room)
            if nbytes == 0:
                raise RuntimeError(f"triangulate: {V} views, {S} segments, {N} lines, {NV} vertices and {room} votes are beyond what one call indexes")
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _lib.check(lib.neat_wf3d_build(_lib.ptr(lines3d), _lib.ptr(support), N, _lib.ptr(members), _lib.ptr(estimate), _lib.ptr(endv), _lib.ptr(view),
                                           int(V), S, int(NV), room, float(end_frac), float(reach), math.sin(float(angle) * math.pi / 180.0),
                                           int(min_votes), _lib.ptr(ws), _lib.ptr(out["junctions3d"]), _lib.ptr(out["degree"]), _lib.ptr(out["kind"]),
                                           _lib.ptr(out["votes"]), _lib.ptr(out["spread"]), _lib.ptr(counts[0:1]), _lib.ptr(out["edges3d"]),
                                           _lib.ptr(out["esrc"]), _lib.ptr(counts[1:2]), _lib.stream()), "neat_wf3d_build")
            J, E = counts.tolist()                      # the one read-back: the two counts
            if J >= 0:
                break
            if E <= room:
                raise RuntimeError(f"triangulate: the views cast more votes than one call indexes ({E})")
            room = E                                    # more votes than there was room for: once more, with the room they need
    return {k: v[:E if k in ("edges3d", "esrc") else J].clone() for k, v in out.items()}


def wireframe(vertices, edges, Ks, poses, end_frac=WIREFRAME_DEFAULTS["end_frac"], reach=WIREFRAME_DEFAULTS["reach"],
              min_votes=WIREFRAME_DEFAULTS["min_votes"], angle=WIREFRAME_DEFAULTS["angle"], pairs_max=None, device=None, **thresholds):
    """The views as graphs -> the dict of lines(vertices[edges], ...), plus the 3-D wireframe (the rule: DESIGN 3p,
    tests/wireframe3d_f64.py): junctions3d float64 [J,3], degree, kind, votes int32 [J], spread float64 [J] per vertex; edges3d int32
    [E,2], esrc int32 [E] (the line of an edge), lines3d_wf float64 [E,2,3] = junctions3d[edges3d].

    vertices: one device tensor [n_v,2] per view; edges: one device integer tensor [e_v,2] per view, into the view's vertices.
    pairs_max: see junctions3d.  One synchronisation beyond lines': the read of the two counts."""
    check_wireframe_options(end_frac, reach, min_votes, angle)
    vertices, edges = list(vertices), list(edges)
    if len(vertices) != len(edges):
        raise ValueError(f"triangulate: {len(vertices)} views of vertices for {len(edges)} views of edges")
    for v, e in zip(vertices, edges):
        if not (torch.is_tensor(v) and torch.is_tensor(e) and v.is_cuda and e.is_cuda):
            raise RuntimeError("neat_amd.triangulate needs CUDA tensors (there is no CPU path)")
        if v.dim() != 2 or v.shape[1] != 2 or e.dim() != 2 or e.shape[1] != 2 or e.dtype.is_floating_point:
            raise RuntimeError(f"triangulate: vertices [n,2] and integer edges [e,2] per view, got {tuple(v.shape)} and {tuple(e.shape)}")
    segments = [torch.cat([v[e[:, 0].long()], v[e[:, 1].long()]], dim=1) for v, e in zip(vertices, edges)]
    res = lines(segments, Ks, poses, device=device, **thresholds)
    dev = res["estimate"].device
    voff = np.concatenate([[0], np.cumsum([int(v.shape[0]) for v in vertices])]).astype(np.int64)      # shapes: no read-back
    with torch.cuda.device(dev):
        endv = torch.cat([e.to(torch.int32) + int(voff[v]) for v, e in enumerate(edges)] + [torch.empty(0, 2, device=dev, dtype=torch.int32)])
        view = torch.from_numpy(np.repeat(np.arange(len(edges), dtype=np.int32), [int(e.shape[0]) for e in edges])).to(dev)
    res.update(junctions3d(res["lines3d"], res["support"], res["members"], res["estimate"], endv, view, len(vertices), int(voff[-1]), end_frac, reach,
                           min_votes, angle, pairs_max))
    res["lines3d_wf"] = res["junctions3d"][res["edges3d"].long()].reshape(-1, 2, 3)
    return res


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.triangulate",
                                 description="triangulate 3-D line segments from the views' 2-D segments on the device")
    ap.add_argument("--conf", type=str, required=True)
    ap.add_argument("--data_root", default="../data", help="root of the dataset's data_dir")
    ap.add_argument("--scan_id", type=int, default=-1, help="replaces the conf's scan_id")
    ap.add_argument("--views", type=str, default=None, help="a:b:step, a slice of the dataset's views")
    ap.add_argument("--neighbours", type=int, default=DEFAULTS["neighbours"], help="nearest views a view is paired with")
    ap.add_argument("--min-views", type=int, default=DEFAULTS["min_views"], help="distinct views a line needs")
    ap.add_argument("--min-score", type=float, default=DEFAULTS["min_score"], help="consensus score an estimate needs")
    ap.add_argument("--sigma", type=float, default=DEFAULTS["sigma_px"], help="depth uncertainty in pixels")
    ap.add_argument("--overlap", type=float, default=DEFAULTS["overlap_min"], help="least overlap of a pair along the partner")
    ap.add_argument("--angle", type=float, default=DEFAULTS["angle_min"], help="least angle between the two planes, degrees")
    ap.add_argument("--out", type=str, default=None, help="output file (default: <instance dir>/<line_detector>-l3d.npz)")
    ap.add_argument("--wireframe", action="store_true", help="read the views as graphs and write the 3-D wireframe with shared junctions (-wf3d.npz)")
    ap.add_argument("--end-frac", dest="end_frac", type=float, default=WIREFRAME_DEFAULTS["end_frac"],
                    help="--wireframe: how far from a line's end, as a share of its length, a segment end still is that end, in (0, 0.5)")
    ap.add_argument("--reach", type=float, default=WIREFRAME_DEFAULTS["reach"], help="--wireframe: how far beyond its end, likewise, a line may cross another")
    ap.add_argument("--min-votes", dest="min_votes", type=int, default=WIREFRAME_DEFAULTS["min_votes"], help="--wireframe: views that must share the 2-D vertex")
    ap.add_argument("--junction-angle", dest="junction_angle", type=float, default=WIREFRAME_DEFAULTS["angle"],
                    help="--wireframe: the least angle between two lines that meet, degrees")
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    return ap


parse_views = functools.partial(run_io.parse_views, step=True)              # 'a:b' or 'a:b:step'; its home is neat_amd.run_io


def out_path(opt, instance_dir, line_detector):
    """The output file of a parsed command line."""
    return opt.out or os.path.join(instance_dir, f"{line_detector}-{'wf3d' if getattr(opt, 'wireframe', False) else 'l3d'}.npz")


def write_lines(path, lines3d, views, support, cameras):
    """The tool's file, written through a temporary one."""
    run_io.replace_file(path, lambda tmp: np.savez(tmp, lines3d=np.asarray(lines3d, np.float64).reshape(-1, 2, 3), views=np.asarray(views, np.int32),
                                                   support=np.asarray(support, np.float64), cameras=np.asarray(cameras, np.float64).reshape(-1, 4, 4)))


def write_wireframe(path, res, cameras):
    """The file of --wireframe, written through a temporary one: lines3d are the edges' segments."""
    host = {k: res[k].cpu().numpy() for k in WIREFRAME_KEYS + ("views", "support")}
    src = host["esrc"].astype(np.int64)
    run_io.replace_file(path, lambda tmp: np.savez(
        tmp, lines3d=np.asarray(host["lines3d_wf"], np.float64).reshape(-1, 2, 3), junctions3d=np.asarray(host["junctions3d"], np.float64).reshape(-1, 3),
        edges=np.asarray(host["edges3d"], np.int32).reshape(-1, 2), degree=host["degree"], kind=host["kind"], votes=host["votes"],
        src=host["esrc"], views=np.asarray(host["views"][src], np.int32), support=np.asarray(host["support"][src], np.float64),
        cameras=np.asarray(cameras, np.float64).reshape(-1, 4, 4)))


def main_wireframe(opt, conf, dataset):
    """--wireframe: the views as graphs -> the -wf3d.npz."""
    try:
        check_wireframe_options(opt.end_frac, opt.reach, opt.min_votes, opt.junction_angle)
        vertices, edges, Ks, poses = run_io.dataset_graphs(dataset)
        picked = list(parse_views(opt.views, len(vertices)))
    except ValueError as err:
        print(err, file=sys.stderr, flush=True)
        return 2
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    t0 = time.perf_counter()
    Ks, poses = _np64([Ks[v] for v in picked]).reshape(-1, 3, 3), _np64([poses[v] for v in picked]).reshape(-1, 4, 4)
    res = wireframe([torch.as_tensor(vertices[v])[:, :2].to(device) for v in picked], [torch.as_tensor(edges[v]).to(device) for v in picked], Ks, poses,
                    neighbours=opt.neighbours, angle_min=opt.angle, overlap_min=opt.overlap, sigma_px=opt.sigma, min_score=opt.min_score,
                    min_views=opt.min_views, end_frac=opt.end_frac, reach=opt.reach, min_votes=opt.min_votes, angle=opt.junction_angle, device=device)
    torch.cuda.synchronize(device)
    seconds = time.perf_counter() - t0
    path = out_path(opt, dataset.instance_dir, conf.get_config("dataset").get("line_detector", "hawp"))
    write_wireframe(path, res, poses)
    print(f"{len(picked)} views, {res['estimate'].shape[0]} segments, {res['rows'].shape[0]} hypotheses, {int(res['kept'].sum())} estimates, "
          f"{res['lines3d'].shape[0]} lines, {res['junctions3d'].shape[0]} vertices, {int((res['kind'] == 1).sum())} junctions, "
          f"{res['edges3d'].shape[0]} edges, {seconds:.3f} s -> {path}", flush=True)
    return 0


def main(argv=None):
    opt = build_parser().parse_args(argv)
    conf = run_io.parse_conf(opt.conf)
    dataset = run_io.build_dataset(conf, opt.data_root, opt.scan_id)
    if opt.wireframe:
        return main_wireframe(opt, conf, dataset)
    segments, Ks, poses = run_io.dataset_views(dataset)
    try:
        picked = list(parse_views(opt.views, len(segments)))
    except ValueError as err:
        print(err, file=sys.stderr, flush=True)
        return 2
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    t0 = time.perf_counter()
    segs = [torch.as_tensor(segments[v])[:, :4].to(device) for v in picked]              # line_segments: x1 y1 x2 y2 score
    Ks, poses = _np64([Ks[v] for v in picked]).reshape(-1, 3, 3), _np64([poses[v] for v in picked]).reshape(-1, 4, 4)
    res = lines(segs, Ks, poses, neighbours=opt.neighbours, angle_min=opt.angle, overlap_min=opt.overlap, sigma_px=opt.sigma,
                min_score=opt.min_score, min_views=opt.min_views, device=device)
    torch.cuda.synchronize(device)
    seconds = time.perf_counter() - t0
    line_detector = conf.get_config("dataset").get("line_detector", "hawp")
    path = out_path(opt, dataset.instance_dir, line_detector)
    write_lines(path, res["lines3d"].cpu().numpy(), res["views"].cpu().numpy(), res["support"].cpu().numpy(), poses)
    print(f"{len(picked)} views, {res['estimate'].shape[0]} segments, {res['rows'].shape[0]} hypotheses, {int(res['kept'].sum())} estimates, "
          f"{res['lines3d'].shape[0]} lines, {seconds:.3f} s -> {path}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
