"""Time of the closest-point query against a triangle mesh (neat_amd.raycast.closest) -> profiles/closest_time.txt.

    timeout -k 10 900 python scripts/closest_time.py [--out profiles/closest_time.txt] [--reps 3]

Workloads, on an icosphere of 327 680 triangles (level 7), the tree already built:
  (a) 1 M queries within 0.05 of the surface (the lines of a wireframe, the points of a reconstruction);
  (b) 1 M queries uniform in the box [-1, 1]^3 of the mesh;
each in the order given (what raycast.closest does) and in the Morton order of the queries (sorted with torch on the device, the sort
and the un-sort inside the time: the measurement behind leaving the order alone), with the node boxes and triangles tested
per query.
Beside them the same answer by two other routes on a subset both can finish (20 480 triangles, 65 536 of the queries of (a) and (b)):
the rule of tests/closest_f64.py by brute force over all triangles in float64 torch on the same device, and tests/closest_f64.closest_all
on 16 CPU processes.  One process, one warm-up, the median of `reps` repetitions (device-synchronised wall time).  The kernel table is
from a run of its own: this script once more as a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run).
"""
import argparse
import multiprocessing
import os
import statistics
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from timing import ROOT, kernel_table, sync_time


def torch_brute_force(verts, faces, pts, chunk=128):
    """The rule of tests/closest_f64.py over all triangles in float64 torch (every product and sum a kernel of its own, so nothing is
    fused) -> (d2, tri) on the device."""
    import torch
    tv = verts[faces.long()]
    a, b, c = tv[None, :, 0], tv[None, :, 1], tv[None, :, 2]
    ab, ac, bc = b - a, c - a, c - b
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    N = pts.shape[0]
    d2_out = torch.empty(N, device=pts.device, dtype=torch.float64)
    tri = torch.empty(N, device=pts.device, dtype=torch.int64)
    for i in range(0, N, chunk):
        p = pts[i:i + chunk, None, :]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        den = (va + vb) + vc
        s_in, t_in = (vb / den)[..., None], (vc / den)[..., None]
        q = (a + s_in * ab) + t_in * ac
        for cond, point in reversed((((d1 <= 0) & (d2 <= 0), a), ((d3 >= 0) & (d4 <= d3), b),
                                     ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[..., None] * ab), ((d6 >= 0) & (d5 <= d6), c),
                                     ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[..., None] * ac),
                                     ((va <= 0) & (e43 >= 0) & (e56 >= 0), b + (e43 / (e43 + e56))[..., None] * bc))):
            q = torch.where(cond[..., None], point, q)                      # the first region that holds is applied last
        d = p - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = dist2.min(dim=1).values
        d2_out[i:i + chunk] = best
        tri[i:i + chunk] = (dist2 == best[:, None]).int().argmax(dim=1)   # the lowest index among the ties
    return d2_out, tri


def morton_order(points):
    """points [N,3] float64 on the device -> the permutation that sorts them by the 30-bit Morton code of their place in their own box."""
    import torch
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    cell = ((points - lo) / (hi - lo).clamp_min(1e-300) * 1024.0).clamp_(0.0, 1023.0).long()
    code = torch.zeros(points.shape[0], device=points.device, dtype=torch.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((cell[:, axis] >> bit) & 1) << (3 * bit + axis)
    return torch.argsort(code)


def _cpu_chunk(args):
    from tests import closest_f64 as CP
    verts, faces, pts = args
    return CP.closest_all(verts, faces, pts)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_time.txt"))
    ap.add_argument("--level", type=int, default=7, help="icosphere level of the workloads (7: 327 680 triangles)")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--sub-level", type=int, default=5, help="icosphere level of the comparison subset (5: 20 480 triangles)")
    ap.add_argument("--sub-queries", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run, no file")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("closest_time.py measures on the GPU: no device found")
    from neat_amd import ops, raycast
    from tests import closest_f64 as CP
    dev = torch.device("cuda:0")
    verts, faces = CP.icosphere(opt.level)
    rng = np.random.default_rng(0)
    u = rng.standard_normal((opt.queries, 3))
    near = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.95, 1.05, (opt.queries, 1))
    sets = {"(a) within 0.05 of the surface": torch.from_numpy(near).to(dev), "(b) uniform in the box": torch.from_numpy(rng.uniform(-1.0, 1.0, (opt.queries, 3))).to(dev)}
    scene = raycast.build(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev))

    if opt.kernel_run:
        for pts in sets.values():
            raycast.closest(scene, pts)
        torch.cuda.synchronize()
        return
    med = lambda x: statistics.median(x[1:])
    out = ["# scripts/closest_time.py on %s: icosphere level %d (%d triangles), %d queries, median of %d after one warm-up"
           % (torch.cuda.get_device_name(0), opt.level, faces.shape[0], opt.queries, opt.reps)]

    def sorted_query(pts):
        order = morton_order(pts)
        return tuple(torch.empty_like(x).index_copy_(0, order, x) for x in ops.raycast_closest(scene.bvh, scene.nf, pts[order]))

    for name, pts in sets.items():
        counts = torch.zeros(opt.queries, 2, device=dev, dtype=torch.int32)
        plain = [sync_time(lambda: ops.raycast_closest(scene.bvh, scene.nf, pts))[0] for _ in range(opt.reps + 1)]
        ordered = [sync_time(lambda: sorted_query(pts))[0] for _ in range(opt.reps + 1)]
        same = all(torch.equal(x, y) for x, y in zip(ops.raycast_closest(scene.bvh, scene.nf, pts, counts=counts), sorted_query(pts)))
        out.append("%s: as given %.4f s = %.1f M queries/s; in Morton order (sort and un-sort included) %.4f s = %.1f M queries/s, outputs %s; per query "
                   "%.1f node boxes and %.2f triangles tested" % (name, med(plain), opt.queries / med(plain) * 1e-6, med(ordered), opt.queries / med(ordered) * 1e-6,
                                                                "equal" if same else "DIFFER", counts[:, 0].float().mean().item(), counts[:, 1].float().mean().item()))
        print(out[-1], flush=True)
    # the subset both other routes can finish
    sv, sf = CP.icosphere(opt.sub_level)
    half = opt.sub_queries // 2
    sp = torch.cat([sets[k][:half] for k in sets])
    sv_dev, sf_dev = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    td, tq = [], []
    for rep in range(opt.reps + 1):
        s, sub = sync_time(lambda: raycast.build(sv_dev, sf_dev))
        td.append(s)
        s, (d2_dev, tri_dev, _, _) = sync_time(lambda: ops.raycast_closest(sub.bvh, sub.nf, sp))
        tq.append(s)
    tt = []
    for rep in range(2):
        s, (d2_t, tri_t) = sync_time(lambda: torch_brute_force(sv_dev, sf_dev, sp))
        tt.append(s)
    p_np = sp.cpu().numpy()
    t0 = time.perf_counter()
    with ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("spawn")) as pool:
        parts = list(pool.map(_cpu_chunk, [(sv, sf, p_np[i:i + 1024]) for i in range(0, p_np.shape[0], 1024)]))
    t_cpu = time.perf_counter() - t0
    d2_cpu, tri_cpu = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    tree = med(td) + med(tq)
    n = p_np.shape[0]
    out += ["subset: icosphere level %d (%d triangles), %d queries, half of (a) and half of (b)" % (opt.sub_level, sf.shape[0], n),
            "  neat_amd.raycast (build %.5f s + closest %.5f s)           %10.5f s" % (med(td), med(tq), tree),
            "  the rule by brute force, float64 torch, same device      %10.5f s   (x %.0f)" % (tt[-1], tt[-1] / tree),
            "  tests/closest_f64.closest_all, 16 CPU processes          %10.5f s   (x %.0f)" % (t_cpu, t_cpu / tree),
            "  agreement: triangle equal to closest_all's on %d of %d queries, to the torch form's on %d; d2 equal to the last bit on %d and %d"
            % (int((tri_dev.cpu().numpy() == tri_cpu).sum()), n, int((tri_dev.long() == tri_t).sum()),
               int((d2_dev.cpu().numpy() == d2_cpu).sum()), int((d2_dev == d2_t).sum()))]
    print("\n".join(out[-5:]), flush=True)
    out += kernel_table(__file__, ["--kernel-run", "--level", str(opt.level), "--queries", str(opt.queries)],
                        "the build, then (a) and (b) once each through raycast.closest; %d kernels, %.3f s of kernel time", 8)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
