"""Data fixture of the triangulation tests: 25 views of the ABC scene 00075213 that the reference ships, as arrays.

    python tests/golden/make_triangulate_fixture.py <reference>/data/abc/00075213

writes tests/golden/triangulate_abc_00075213.npz from the scene's data files only (cameras.npz, hawp/*.json, lines.json):
  view_ids     int64 [25]           views 0, 4, ..., 96 of the scene's directory
  intrinsics   float64 [25,3,3]     cameras.npz intrinsics
  extrinsics   float64 [25,4,4]     cameras.npz extrinsics (camera-to-world)
  vertices     float32 [nv,2]       the HAWP junctions of all views, view v's at rows vertex_off[v]:vertex_off[v+1]
  edges        int64 [ne,2], weights float32 [ne]     the HAWP edges (vertex numbers within the view) and `edges-weights`, by edge_off
  gt_junctions float64 [12,3], gt_edges int64 [18,2]  lines.json, in its own frame X_gt = s X + o
  gt_scale, gt_offset               s and o, fitted here: a scale-plus-offset ICP of the end points that tests/triangulate_f64.py
                                    triangulates from these views to the junctions
  gt_lines     float64 [18,2,3]     the ground-truth lines in the cameras' frame, (junction - o) / s
Data only, no program text.  tests/triangulate_f64.fixture_segments turns the arrays into the per-view segments the datasets give
(edges with a weight above 0.05)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PATH = os.path.join(HERE, "triangulate_abc_00075213.npz")


def fit_scale_offset(points, junctions, rounds=50):
    """X_gt = s X + o by iterated closest junction: the points within a tenth of the junctions' extent of one, least squares for one scale
    and an offset per axis."""
    ext = np.linalg.norm(junctions.max(0) - junctions.min(0))
    s = ext / np.linalg.norm(points.max(0) - points.min(0))
    o = junctions.mean(0) - s * points.mean(0)
    for _ in range(rounds):
        y = s * points + o
        d = np.linalg.norm(y[:, None, :] - junctions[None, :, :], axis=2)
        near = d.argmin(1)
        keep = d.min(1) < 0.1 * ext
        x, t = points[keep], junctions[near[keep]]
        xc, tc = x - x.mean(0), t - t.mean(0)
        s = float((xc * tc).sum() / (xc * xc).sum())
        o = t.mean(0) - s * x.mean(0)
    return s, o, int(keep.sum())


def main(root):
    from tests import triangulate_f64 as T
    cams = np.load(os.path.join(root, "cameras.npz"))
    ids = list(range(0, 100, 4))
    vert, edges, weights, voff, eoff = [], [], [], [0], [0]
    for v in ids:
        wf = json.load(open(os.path.join(root, "hawp", f"image_{v:04d}.json")))
        vert.append(np.asarray(wf["vertices"], dtype=np.float32).reshape(-1, 2))
        edges.append(np.asarray(wf["edges"], dtype=np.int64).reshape(-1, 2))
        weights.append(np.asarray(wf["edges-weights"], dtype=np.float32).reshape(-1))
        voff.append(voff[-1] + vert[-1].shape[0])
        eoff.append(eoff[-1] + edges[-1].shape[0])
    gt = json.load(open(os.path.join(root, "lines.json")))
    out = {"view_ids": np.asarray(ids, dtype=np.int64), "intrinsics": cams["intrinsics"][ids].astype(np.float64)[:, :3, :3],
           "extrinsics": cams["extrinsics"][ids].astype(np.float64), "vertices": np.concatenate(vert), "vertex_off": np.asarray(voff, np.int64),
           "edges": np.concatenate(edges), "weights": np.concatenate(weights), "edge_off": np.asarray(eoff, np.int64),
           "gt_junctions": np.asarray(gt["junctions"], dtype=np.float64).reshape(-1, 3), "gt_edges": np.asarray(gt["lines"], dtype=np.int64).reshape(-1, 2)}
    res = T.lines(T.fixture_segments(out), out["intrinsics"], out["extrinsics"])
    s, o, used = fit_scale_offset(res["lines3d"].reshape(-1, 3), out["gt_junctions"])
    out["gt_scale"], out["gt_offset"] = np.float64(s), np.asarray(o, dtype=np.float64)
    out["gt_lines"] = (out["gt_junctions"][out["gt_edges"]] - o) / s
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes;", f"{res['rows'].shape[0]} hypotheses, {int(res['kept'].sum())} estimates, {res['lines3d'].shape[0]} lines;",
          f"s = {s:.4f}, o = {np.round(o, 4).tolist()} from {used} end points")


if __name__ == "__main__":
    main(sys.argv[1])
