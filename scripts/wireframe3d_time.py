"""Time of the 3-D wireframe builder (neat_amd.triangulate.junctions3d) -> profiles/wireframe3d_time.txt.

    timeout -k 10 900 python scripts/wireframe3d_time.py [--out profiles/wireframe3d_time.txt] [--views 64] [--segments 500 2000]

Workload: for every n of `--segments`, the first n rods of a rotated cubic lattice (tests/wireframe3d_f64.lattice), each seen as one
segment by every one of `--views` views, the segment ends a few per cent of the rod away from its ends: views x n segments, n lines,
junctions of three to six ends.  One process, one warm-up, the median of `reps` repetitions of device-synchronised wall time, the
allocations and the one read-back included.  Beside it: the same rule written with float64 torch tensor operations on the same device
(the records and the votes by torch.unique, the pairs of a 2-D vertex by shifted comparisons of the sorted records, the components by
min-label propagation until nothing changes, the junctions' sums by index_add, the duplicate edges by unique; its vertex, junction and
edge counts must be the kernels'), and tests/wireframe3d_f64.build on this machine's CPU, whose arrays must be the device's.  The kernel
table is from a run of its own: this script once more as a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: the
workload twice).  None of these times is a pass condition."""
import argparse
import os
import sys
import time

import numpy as np

from timing import ROOT, kernel_table, timed


def torch_rule(t, V, NV, end_frac, reach, smin, min_votes):
    """The rule of DESIGN 3p with float64 torch operations -> (vertices, junctions, edges, the junctions' positions by root)."""
    import torch
    lines3d, support, estimate = t["lines3d"], t["support"], t["estimate"]
    members, endv, view = t["members"].long(), t["endv"].long(), t["view"].long()
    N, dev = lines3d.shape[0], lines3d.device
    n2 = 2 * N
    A, U = lines3d[:, 0], lines3d[:, 1] - lines3d[:, 0]
    uu = (U * U).sum(1)
    ok = members >= 0
    L = members.clamp(min=0)
    tau = ((estimate - A[L][:, None, :]) * U[L][:, None, :]).sum(2) / uu[L][:, None]
    q = torch.where(ok[:, None] & (tau <= end_frac), 2 * L[:, None], torch.where(ok[:, None] & (tau >= 1.0 - end_frac), 2 * L[:, None] + 1, -1))
    vview = torch.zeros(NV, dtype=torch.int64, device=dev).scatter_reduce(0, endv.reshape(-1), view.repeat_interleave(2), "amax")
    valid = q >= 0
    rec = torch.unique(endv[valid] * n2 + q[valid])
    gv, rq = rec // n2, rec % n2
    most = int(torch.bincount(gv).max()) if rec.numel() else 0
    keys = []
    for d in range(1, most):
        same = gv[:-d] == gv[d:]
        qa, qb, g = rq[:-d][same], rq[d:][same], gv[:-d][same]
        keep = (qa >> 1) != (qb >> 1)
        keys.append((qa[keep] * n2 + qb[keep]) * V + vview[g[keep]])
    pk = torch.unique(torch.cat(keys)) if keys else torch.zeros(0, dtype=torch.int64, device=dev)
    pq, votes = torch.unique(pk // V, return_counts=True)
    pq = pq[votes >= min_votes]
    q0, q1 = pq // n2, pq % n2
    A0, A1, u, v = A[q0 >> 1], A[q1 >> 1], U[q0 >> 1], U[q1 >> 1]
    a, b, c = (u * u).sum(1), (u * v).sum(1), (v * v).sum(1)
    r = A1 - A0
    d_, e_ = (u * r).sum(1), (v * r).sum(1)
    w = torch.linalg.cross(u, v)
    den = a * c - b * b
    s, tt = (c * d_ - b * e_) / den, (b * d_ - a * e_) / den
    D = (A0 + s[:, None] * u) - (A1 + tt[:, None] * v)
    accepted = ~((w * w).sum(1) < smin * smin * (a * c)) & ((s - (q0 & 1)).abs() <= reach) & ((tt - (q1 & 1)).abs() <= reach) & \
        ((D * D).sum(1) <= reach * reach * torch.minimum(a, c))
    pa, pb = q0[accepted], q1[accepted]
    label = torch.arange(n2, device=dev)
    while True:                                   # min-label propagation over the links
        m = torch.minimum(label[pa], label[pb])
        new = label.scatter_reduce(0, torch.cat([pa, pb]), torch.cat([m, m]), "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    count = torch.bincount(label, minlength=n2)
    roots = label == torch.arange(n2, device=dev)
    P = torch.eye(3, dtype=torch.float64, device=dev)[None] - U[:, :, None] * U[:, None, :] / uu[:, None, None]
    Pe, Ae = P.repeat_interleave(2, dim=0), A.repeat_interleave(2, dim=0)
    M = torch.zeros(n2, 3, 3, dtype=torch.float64, device=dev).index_add_(0, label, Pe)
    y = torch.zeros(n2, 3, dtype=torch.float64, device=dev).index_add_(0, label, (Pe @ Ae[:, :, None])[:, :, 0])
    big = roots & (count >= 2)
    J = torch.linalg.solve(M[big], y[big])
    ev = label.reshape(N, 2)
    lo, hi = ev.min(dim=1).values, ev.max(dim=1).values
    _, inv = torch.unique(lo * n2 + hi, return_inverse=True)
    top = torch.full((int(inv.max()) + 1,), -np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, inv, support, "amax")
    idx = torch.arange(N, device=dev)
    first = torch.full_like(top, N, dtype=torch.int64).scatter_reduce(0, inv, torch.where(support == top[inv], idx, N), "amin")
    keep = (lo != hi) & (first[inv] == idx)
    return int(roots.sum()), int(big.sum()), int(keep.sum()), J


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wireframe3d_time.txt"))
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--segments", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true", help="the traced workload only; writes nothing")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 reference on the CPU")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch operations")
    ap.add_argument("--no-trace", action="store_true", help="skip the kernel table")
    opt = ap.parse_args()
    import torch
    from neat_amd import triangulate
    from tests import wireframe3d_f64 as W
    assert torch.cuda.is_available(), "wireframe3d_time.py measures on the device"
    dev = torch.device("cuda:0")
    D = W.DEFAULTS
    lines = []
    for n in opt.segments:
        a = W.lattice(n, V=opt.views)[0]
        t = {k: torch.from_numpy(np.ascontiguousarray(a[k])).to(dev) for k in ("lines3d", "support", "members", "estimate", "endv", "view")}
        run = lambda: triangulate.junctions3d(t["lines3d"], t["support"], t["members"], t["estimate"], t["endv"], t["view"], a["V"], a["NV"])
        if opt.kernel_run:
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            continue
        med, lo, hi, res = timed(run, opt.reps)
        got = {k: v.cpu().numpy() for k, v in res.items()}
        counts = (got["junctions3d"].shape[0], int((got["kind"] == 1).sum()), got["edges3d"].shape[0])
        lines += ["# neat_amd.triangulate.junctions3d on %d views of %d segments (%d lines), float64; median (min .. max) of %d after one warm-up,"
                  % (opt.views, n, n, opt.reps), "# device-synchronised wall time, the allocations and the one read-back included",
                  "junctions3d: %8.3f ms (%.3f .. %.3f);  %d vertices of %d ends, %d junctions, %d edges" % (med * 1e3, lo * 1e3, hi * 1e3, counts[0], 2 * n,
                                                                                                          counts[1], counts[2])]
        if not opt.no_torch:
            smin = W.sin_min(D["angle"])
            med_t, lo_t, hi_t, tc = timed(lambda: torch_rule(t, a["V"], a["NV"], D["end_frac"], D["reach"], smin, D["min_votes"]), max(2, opt.reps // 2))
            near = float((tc[3] - res["junctions3d"][res["kind"] == 1]).abs().max()) if tc[1] == counts[1] else float("nan")
            lines.append("the rule with float64 torch operations, same device: %.1f ms (%.1f .. %.1f) = %.1f x; its counts %s equal the kernels': %s; "
                         "its junctions within %.2g of them" % (med_t * 1e3, lo_t * 1e3, hi_t * 1e3, med_t / med, tc[:3], tuple(tc[:3]) == counts, near))
        if not opt.no_host:
            t0 = time.perf_counter()
            ref = W.build(*W.arrays_of(a))
            t1 = time.perf_counter() - t0
            same = all(got[k].tobytes() == ref[k].tobytes() for k in got)
            lines.append("tests/wireframe3d_f64.build on one CPU process: %.2f s = %.0f x; its arrays are the device's bytes: %s; least decision margin %.3g"
                         % (t1, t1 / med, same, min(ref["margins"].values())))
    if opt.kernel_run:
        return 0
    if not opt.no_trace:
        lines += kernel_table(__file__, ["--kernel-run", "--views", str(opt.views), "--segments"] + [str(n) for n in opt.segments],
                              "the workloads twice each; %d kernels, %.3f s of kernel time", 12, family=("3-D wireframe", "wf3_"))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
