"""Time of the triangulation of 3-D segments from the views' 2-D segments (neat_amd.triangulate) -> profiles/triangulate_time.txt.

    timeout -k 10 900 python scripts/triangulate_time.py [--out profiles/triangulate_time.txt] [--views 64] [--segments 500] [--neighbours 10]

Workload: tests/triangulate_f64.random_scene, `--views` ring cameras that each see `--segments` segments (projections of 400 shared
3-D segments of length 0.4 in a cube of side 2, with a twentieth of a pixel of noise, the rest of the segments repeat them half a pixel
off), `--neighbours` slots: views x slots x segments^2 pair tests.
One process, one warm-up, the median of `reps` repetitions of device-synchronised wall time, the two read-backs included.  Beside it:
the pair test alone (triangulate.hypotheses) and the same pair test written with float64 torch tensor operations on the same device
(one broadcast per (view, slot), the segment constants given; its hypothesis count must be the kernels'); and the whole rule by
tests/triangulate_f64.py on this machine's CPU (16 threads allowed; numpy uses what it uses) at `--host-views` x `--host-segments`,
a size the CPU finishes, with the device's time for that size.  The kernel table is from a run of its own: this script once more as
a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: the workload twice).  None of these times is a pass condition.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

from timing import ROOT, kernel_table, timed


def torch_pair_count(consts, cam, nb, cos_min, overlap_min):
    """The pair test of DESIGN 3k with float64 torch operations, one broadcast [n_a, n_b] per (view, slot) -> the number of hypotheses."""
    import torch
    total = torch.zeros((), dtype=torch.int64, device=cam["C"].device)
    col, row = (lambda x: x[None, :]), (lambda x: x[:, None])
    for a in range(nb.shape[0]):
        A = consts[a]
        for m in range(nb.shape[1]):
            b = int(nb[a, m])
            B, C, R, t, K = consts[b], cam["C"][a], cam["R"][b], cam["t"][b], cam["K"][b]
            pi = B["pi"]
            c = ((row(A["na"][:, 0]) * col(pi[:, 0]) + row(A["na"][:, 1]) * col(pi[:, 1])) + row(A["na"][:, 2]) * col(pi[:, 2])).abs() / col(B["norm"])
            e = ((pi[:, 0] * C[0] + pi[:, 1] * C[1]) + pi[:, 2] * C[2]) + pi[:, 3]
            ok = c <= cos_min
            ts = []
            for d in (A["d1"], A["d2"]):
                s = -col(e) / ((col(pi[:, 0]) * row(d[:, 0]) + col(pi[:, 1]) * row(d[:, 1])) + col(pi[:, 2]) * row(d[:, 2]))
                ok = ok & (s > 0.0) & torch.isfinite(s)
                X = [C[q] + s * row(d[:, q]) for q in range(3)]
                x = [((R[r, 0] * X[0] + R[r, 1] * X[1]) + R[r, 2] * X[2]) + t[r] for r in range(3)]
                ok = ok & (x[2] > 0.0)
                y0 = ((K[0, 0] * x[0] + K[0, 1] * x[1]) + K[0, 2] * x[2]) / x[2]
                y1 = ((K[1, 0] * x[0] + K[1, 1] * x[1]) + K[1, 2] * x[2]) / x[2]
                ts.append(((y0 - col(B["q1"][:, 0])) * col(B["u"][:, 0]) + (y1 - col(B["q1"][:, 1])) * col(B["u"][:, 1])) / col(B["uu"]))
            ok = ok & torch.isfinite(ts[0]) & torch.isfinite(ts[1])
            lo, hi = torch.minimum(ts[0], ts[1]), torch.maximum(ts[0], ts[1])
            inter = hi.clamp(max=1.0) - lo.clamp(min=0.0)
            uni = hi.clamp(min=1.0) - lo.clamp(max=0.0)
            total += (ok & (inter >= overlap_min * uni)).sum()
    return int(total.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_time.txt"))
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--segments", type=int, default=500)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--host-views", type=int, default=16)
    ap.add_argument("--host-segments", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true", help="the traced workload only; writes nothing")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 reference on the CPU")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch pair test")
    ap.add_argument("--no-trace", action="store_true", help="skip the kernel table")
    opt = ap.parse_args()
    import torch
    from neat_amd import triangulate
    from tests import triangulate_f64 as T
    assert torch.cuda.is_available(), "triangulate_time.py measures on the device"
    dev = torch.device("cuda:0")
    up = lambda seg: [torch.from_numpy(s).to(dev) for s in seg]
    seg, Ks, poses = T.random_scene([opt.segments] * opt.views, 400, seed=0, length=0.4)
    dseg = up(seg)
    M = opt.neighbours
    if opt.kernel_run:
        for _ in range(2):
            triangulate.lines(dseg, Ks, poses, neighbours=M)
        torch.cuda.synchronize()
        return 0
    med, lo, hi, res = timed(lambda: triangulate.lines(dseg, Ks, poses, neighbours=M), opt.reps)
    H = int(res["rows"].shape[0])
    pairs = opt.views * min(M, opt.views - 1) * opt.segments ** 2
    lines = ["# neat_amd.triangulate.lines on %d views of %d segments, %d neighbours: %.3g pair tests, float64; median (min .. max) of %d after one"
             % (opt.views, opt.segments, M, pairs, opt.reps), "# warm-up, device-synchronised wall time, the two read-backs (hypothesis and line counts) included",
             "lines:      %8.2f ms (%.2f .. %.2f);  %d hypotheses, %d estimates, %d lines" % (med * 1e3, lo * 1e3, hi * 1e3, H, int(res["kept"].sum()),
                                                                                           int(res["lines3d"].shape[0]))]
    med_h, lo_h, hi_h, _ = timed(lambda: triangulate.hypotheses(dseg, Ks, poses, neighbours=M), opt.reps)
    lines.append("hypotheses: %8.2f ms (%.2f .. %.2f)  = %.2f G pair tests/s, both passes (count and fill) counted once"
                 % (med_h * 1e3, lo_h * 1e3, hi_h * 1e3, pairs / med_h * 1e-9))
    if not opt.no_torch:
        with np.errstate(all="ignore"):
            cam_h = T.cameras(Ks, poses)
            consts = [{k: torch.from_numpy(v).to(dev) for k, v in T.segment_constants(s, cam_h, v_).items()} for v_, s in enumerate(seg)]
        cam = {k: torch.from_numpy(v).to(dev) for k, v in cam_h.items()}
        nb = T.neighbour_table(cam_h["C"], M)
        cos_min = math.cos(5.0 * math.pi / 180.0)
        med_t, lo_t, hi_t, count = timed(lambda: torch_pair_count(consts, cam, nb, cos_min, 0.25), max(2, opt.reps // 2))
        lines.append("the pair test with float64 torch operations, same device, constants given: %.1f ms (%.1f .. %.1f) = %.1f x the two kernel "
                     "passes; %d hypotheses, equal to the kernels': %s" % (med_t * 1e3, lo_t * 1e3, hi_t * 1e3, med_t / med_h, count, count == H))
    if not opt.no_host:
        hseg, hK, hP = T.random_scene([opt.host_segments] * opt.host_views, 160, seed=1, length=0.4)
        t0 = time.perf_counter()
        ref = T.lines(hseg, hK, hP, neighbours=6)
        t1 = time.perf_counter() - t0
        dh = up(hseg)
        med1, lo1, hi1, got = timed(lambda: triangulate.lines(dh, hK, hP, neighbours=6), opt.reps)
        same = np.array_equal(got["rows"].cpu().numpy(), ref["rows"]) and np.array_equal(got["lines3d"].cpu().numpy(), ref["lines3d"])
        lines.append("tests/triangulate_f64.lines on the CPU, %d views of %d segments, 6 neighbours: %.2f s; the device: %.2f ms (%.2f .. %.2f), %.0f x; "
                     "%d hypotheses, %d lines; equal to the device's: %s"
                     % (opt.host_views, opt.host_segments, t1, med1 * 1e3, lo1 * 1e3, hi1 * 1e3, t1 / med1, ref["rows"].shape[0], ref["lines3d"].shape[0], same))
    if not opt.no_trace:
        lines += kernel_table(__file__, ["--kernel-run", "--views", str(opt.views), "--segments", str(opt.segments), "--neighbours", str(M)],
                              "the workload twice; %d kernels, %.3f s of kernel time", 12)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
