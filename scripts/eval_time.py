"""Seconds per stage of `neat_amd.evaluate`'s dtu-mesh path on a large synthetic case at the reference's defaults (density 0.2,
max_dist 20), next to the reference's algorithm (tests/eval_f64.py with scipy's cKDTree and the sequential thinning loop) on the same
arrays and the same machine -> profiles/eval_time.txt.

    python scripts/eval_time.py [--radius 60] [--subdiv 7] [--stl 1000000] [--reps 3] [--no-host] [--out profiles/eval_time.txt]

The mesh is an octahedron subdivided `subdiv` times onto a sphere of `radius` mm with a little noise; the ground truth is `stl` noisy
points of the same sphere; everything is observed.  One warm-up run, then the median of `reps` runs per stage (device-synchronised).
"""
import argparse
import os
import statistics
import time

import numpy as np
import torch

from timing import ROOT


def sphere(radius, subdiv, seed=0):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int64)
    for _ in range(subdiv):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1) + len(v)
        v = np.concatenate([v, mid])
        f = np.concatenate([np.stack([f[:, 0], m[0], m[2]], 1), np.stack([m[0], f[:, 1], m[1]], 1), np.stack([m[2], m[1], f[:, 2]], 1),
                            np.stack([m[0], m[1], m[2]], 1)])
    rng = np.random.default_rng(seed)
    return v * radius + rng.normal(0, 0.02, v.shape), f.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=60.0)
    ap.add_argument("--subdiv", type=int, default=7)
    ap.add_argument("--stl", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_time.txt"))
    opt = ap.parse_args()
    from neat_amd import evaluate as E
    from tests import eval_f64 as F
    verts, faces = sphere(opt.radius, opt.subdiv)
    rng = np.random.default_rng(1)
    d = rng.normal(size=(opt.stl, 3))
    stl = d / np.linalg.norm(d, axis=1, keepdims=True) * opt.radius + rng.normal(0, 0.1, (opt.stl, 3))
    r = opt.radius
    bb = np.array([[-r - 5, -r - 5, -r - 5], [r + 5, r + 5, r + 5]])
    obs = np.ones((int(2 * r + 10) + 1,) * 3, dtype=np.uint8)
    plane = np.array([0.0, 0.0, 1.0, 0.5 * r])
    dev = torch.device("cuda", 0)
    vd, fd, sd = torch.tensor(verts).to(dev), torch.tensor(faces).to(dev), torch.tensor(stl).to(dev)
    stages = ("sample_s", "thin_s", "mask_s", "d2s_s", "s2d_s")
    runs, res = [], None
    for rep in range(opt.reps + 1):
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cloud = E.sample_mesh(vd, fd, 0.2)
        torch.cuda.synchronize()
        t["sample_s"] = time.perf_counter() - t0
        order = np.random.default_rng(0).permutation(cloud.shape[0])
        det = {}
        res = E.dtu_scores(cloud, sd, obs, bb, 1.0, plane, order=order, timings=t, details=det)
        if rep:
            runs.append(t)
    med = {k: statistics.median(x[k] for x in runs) for k in stages}
    n_cloud, n_down = int(cloud.shape[0]), int(det["data_down"].shape[0])
    lines = ["# scripts/eval_time.py on %s: sphere of radius %g mm, %d triangles, density 0.2, max_dist 20; %d sampled points, %d after thinning, "
             "%d ground-truth points; median of %d runs after one warm-up, seconds" % (torch.cuda.get_device_name(0), r, len(faces), n_cloud,
                                                                                         n_down, opt.stl, opt.reps),
             "# side     sample     thin     mask   data->stl   stl->data    total      acc        comp"]
    lines.append("device  %8.4f %8.4f %8.4f %10.4f %11.4f %8.4f   %.6f   %.6f" % (*(med[k] for k in stages), sum(med.values()), *res))
    with open(opt.out, "w") as fh:          # the device's line is kept even if the host's run is cut short
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    if not opt.no_host:
        t0 = time.perf_counter()
        host_cloud = F.sample_mesh(verts, faces, 0.2)
        t1 = time.perf_counter()
        ref = F.dtu_scores(host_cloud, stl, obs, bb, 1.0, plane, order=order, tree=True)
        t2 = time.perf_counter()
        lines.append("# host: tests/eval_f64.py, cKDTree with 16 workers and the sequential thinning loop (the reference's algorithm), one run; "
                     "thinning, masks and both queries are timed together")
        lines.append("host    %8.4f %39s %8.4f %8.4f   %.6f   %.6f" % (t1 - t0, "", t2 - t1, t2 - t0, *ref))
        print("\n".join(lines[-2:]), flush=True)
        with open(opt.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
