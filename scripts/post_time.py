"""Time of `neat_amd.post` fuse / refine / snap on a synthetic soup: N = 50 000 lines, 64 views of 500 detections each, G = 512, against
the float32 torch form of the same rules (tests/post_f64.py: torch_fuse, torch_refine, torch_snap) on the same device and on 16 CPU
threads -> profiles/post_time.txt.

    timeout -k 10 900 python scripts/post_time.py [--out profiles/post_time.txt] [--lines 50000] [--views 64] [--dets 500] [--grid 512]

One process, one warm-up of the same shape, the median of `reps` repetitions of device-synchronised wall time (the one read-back at the end
of each call included).  The CPU form runs once (it takes seconds).  The kernel table is from a run of its own: this script once more as a
fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: one warm-up and one call of each subcommand).
"""
import argparse
import os
import statistics
import time

import numpy as np
import torch

from timing import ROOT, kernel_table
W, H, FOCAL = 640, 480, 600.0


def scene(n, V, m, seed=0):
    """n noisy copies (both orientations) of m/2 segments and outliers; V cameras on a ring; per view, detections on the segments' projections
    (scores on both sides of 0.5) filled up to m with clutter."""
    from tests.golden.make_parse_golden import look_at
    from tests.post_f64 import project
    rng = np.random.default_rng(seed)
    nseg = m // 2
    segs = rng.uniform(-0.6, 0.6, (nseg, 2, 3))
    lines = segs[rng.integers(0, nseg, n)] + rng.normal(0, 0.002, (n, 2, 3))
    flip = rng.random(n) < 0.5
    lines[flip] = lines[flip][:, [1, 0]]
    out = rng.random(n) < 0.1
    lines[out] = rng.uniform(-1, 1, (int(out.sum()), 2, 3))
    K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]], np.float32)
    views = []
    for v in range(V):
        ang = 2 * np.pi * v / V
        pose = look_at(np.array([3 * np.cos(ang), 3 * np.sin(ang), 1.0 + 0.5 * np.sin(3 * ang)])).astype(np.float32)
        det = np.zeros((m, 5), np.float32)
        det[:nseg, :4] = project(K, pose, segs) + rng.normal(0, 0.3, (nseg, 4))
        det[nseg:, :4] = rng.uniform(0, [W, H, W, H], (m - nseg, 4))
        det[:, 4] = np.where(rng.random(m) < 0.3, rng.uniform(0.05, 0.4, m), rng.uniform(0.6, 0.99, m))
        views.append({"K": K, "pose": pose, "det": det[rng.permutation(m)]})
    return lines.astype(np.float32), views


def timed(fn, reps, sync):
    ts = []
    for _ in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:]) if reps > 0 else ts[0], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_time.txt"))
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--dets", type=int, default=500)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run, no file")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("post_time.py measures on the GPU: no device found")
    from neat_amd import post
    from tests import post_f64 as F
    dev = torch.device("cuda:0")
    lines, views = scene(opt.lines, opt.views, opt.dets)
    pv = post.pack_views([torch.tensor(v["det"]) for v in views], [torch.tensor(v["K"]) for v in views], [torch.tensor(v["pose"]) for v in views],
                         (H, W), dev)
    dl = torch.tensor(lines).to(dev)
    calls = {"fuse": lambda: post.fuse(dl, pv)["lines3d"], "refine": lambda: post.refine(dl, pv), "snap": lambda: post.snap(dl, opt.grid)["junctions"]}
    if opt.kernel_run:
        for fn in list(calls.values()) * 2:
            fn()
        torch.cuda.synchronize()
        return
    tviews = {d: [{k: torch.tensor(v).to(d) for k, v in vw.items()} for vw in views] for d in (dev, torch.device("cpu"))}
    torch.set_num_threads(16)
    forms = {"fuse": lambda L, vs: F.torch_fuse(L, vs), "refine": lambda L, vs: F.torch_refine(L, vs, W, H),
             "snap": lambda L, vs: F.torch_snap(L, opt.grid)[0]}
    out = ["# scripts/post_time.py on %s: %d lines, %d views of %d detections, G = %d; median of %d after one warm-up (torch on 16 CPU threads: one run)"
           % (torch.cuda.get_device_name(0), opt.lines, opt.views, opt.dets, opt.grid, opt.reps),
           "# command   neat_amd.post s   torch fp32, same device s   torch fp32, 16 CPU threads s   rows out (post / torch device / torch cpu)"]
    for name, fn in calls.items():
        t_post, r = timed(fn, opt.reps, torch.cuda.synchronize)
        t_dev, rd = timed(lambda: forms[name](dl, tviews[dev]), opt.reps, torch.cuda.synchronize)
        t_cpu, rc = timed(lambda: forms[name](torch.tensor(lines), tviews[torch.device("cpu")]), 0, lambda: None)
        out.append("%-8s %17.4f %26.4f %30.3f     %d / %d / %d" % (name, t_post, t_dev, t_cpu, r.shape[0], rd.shape[0], rc.shape[0]))
        print(out[-1], flush=True)
    out += kernel_table(__file__, ["--kernel-run", "--lines", str(opt.lines), "--views", str(opt.views), "--dets", str(opt.dets), "--grid", str(opt.grid)],
                        "one warm-up and one call of fuse, refine and snap; %d kernels, %.3f s of kernel time", 16, limit=420)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
