"""Time of the 2-D wireframe builder (neat_amd.detect.junctions) -> profiles/junctions2d_time.txt.

    timeout -k 10 900 python scripts/junctions2d_time.py [--out profiles/junctions2d_time.txt] [--views 64] [--segments 500 2000]

Workload: `--views` views of n segments each, for every n of `--segments`: the unit segments of a rotated lattice of 10 px cells (as many
cells as give n segments at least, cut to n), a rotation of its own per view, every end pulled in by 0.5 to 1.5 px and moved by 0.05 px
of noise: mostly junctions of three and four ends, some free ends where the cut fell.  One process, one warm-up, the median of `reps`
repetitions of device-synchronised wall time, the one read-back included.  Beside it: the same rule written with float64 torch tensor
operations on the same device (the meet and T tests as one broadcast [V,n,n] each, the components by min-label propagation until nothing
changes, the junctions' sums by index_add, the duplicate edges by unique; its vertex, junction, T and edge counts must be the
kernels'), and tests/junctions2d_f64.build on this machine's CPU, a view a task over 16 processes, whose arrays must be the device's.  The kernel table is from a run of its own: this script once more as a fresh process under `rocprofv3 --kernel-trace --stats`
(--kernel-run: the workload twice).  With --fixture: the table of the eight fixture views from the device's output, and the rows
the junction matching sees per view.  None of these times is a pass condition."""
import argparse
import math
import os
import sys
import time

import numpy as np

from timing import ROOT, kernel_table, timed


def workload(views, n, seed=0):
    """-> (segments float64 [views n, 4], offsets int32 [views + 1])."""
    from tests import junctions2d_f64 as J
    rng = np.random.default_rng(seed)
    m = 1
    while 2 * m * (m + 1) < n:
        m += 1
    out = []
    for _ in range(views):
        seg, _ = J.lattice(m, m, theta=float(rng.uniform(0.0, math.pi / 2.0)), shrink=0.0, origin=(400.0, 50.0))
        seg = seg[:n]
        d = seg[:, 2:] - seg[:, :2]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        seg[:, :2] += rng.uniform(0.5, 1.5, (n, 1)) * d
        seg[:, 2:] -= rng.uniform(0.5, 1.5, (n, 1)) * d
        out.append(seg + rng.normal(0.0, 0.05, seg.shape))
    return np.concatenate(out), (np.arange(views + 1) * n).astype(np.int32)


def _cpu_view(args):
    from tests import junctions2d_f64 as J
    seg, weight = args
    return J.build(seg, [0, seg.shape[0]], weight)


def cpu_build(seg, off, weight):
    """tests/junctions2d_f64.build, a view a task over 16 processes (the views are independent) -> the arrays of all views, the margin."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("spawn")) as pool:
        parts = list(pool.map(_cpu_view, [(seg[off[v]:off[v + 1]], weight[off[v]:off[v + 1]]) for v in range(off.shape[0] - 1)]))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("vertices", "degree", "kind", "score", "spread", "t_edge", "ends", "edges", "eweight", "esrc")}
    out["voff"] = np.concatenate([[0], np.cumsum([p["vertices"].shape[0] for p in parts])]).astype(np.int32)
    out["eoff"] = np.concatenate([[0], np.cumsum([p["edges"].shape[0] for p in parts])]).astype(np.int32)
    return out, min(p["margin"] for p in parts)


def torch_build(seg, weight, V, n, gap, frac, smin):
    """The rule of DESIGN 3o with float64 torch operations for V views of n segments each -> (vertices, junctions, T ends, edges)."""
    import torch
    S = V * n
    s = seg.reshape(V, n, 4)
    p, q = s[..., :2], s[..., 2:]
    d = q - p
    L = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sqrt()
    u = d / L[..., None]
    g = torch.minimum(torch.full_like(L, gap), frac * L)
    row, col = (lambda x: x[:, :, None]), (lambda x: x[:, None, :])
    c = row(u[..., 0]) * col(u[..., 1]) - row(u[..., 1]) * col(u[..., 0])
    t = ((col(p[..., 0]) - row(p[..., 0])) * col(u[..., 1]) - (col(p[..., 1]) - row(p[..., 1])) * col(u[..., 0])) / c
    X, Y = row(p[..., 0]) + t * row(u[..., 0]), row(p[..., 1]) + t * row(u[..., 1])
    ar = torch.arange(n, device=seg.device)
    upper = (ar[:, None] < ar[None, :])[None]
    angle = c.abs() >= smin
    e, o = [p, q], [-u, u]
    along_i = [(X - row(e[k][..., 0])) * row(o[k][..., 0]) + (Y - row(e[k][..., 1])) * row(o[k][..., 1]) for k in range(2)]
    base = (torch.arange(V, device=seg.device) * n)[:, None, None]
    label = torch.arange(2 * S, device=seg.device)
    pa, pb = [], []
    for ki in range(2):
        for kj in range(2):
            b = (X - col(e[kj][..., 0])) * col(o[kj][..., 0]) + (Y - col(e[kj][..., 1])) * col(o[kj][..., 1])
            meet = upper & angle & (along_i[ki].abs() <= row(g)) & (b.abs() <= col(g))
            v, i, j = meet.nonzero(as_tuple=True)
            pa.append(2 * (v * n + i) + ki)
            pb.append(2 * (v * n + j) + kj)
    pa, pb = torch.cat(pa), torch.cat(pb)
    while True:                                   # min-label propagation over the meet pairs
        m = torch.minimum(label[pa], label[pb])
        new = label.scatter_reduce(0, torch.cat([pa, pb]), torch.cat([m, m]), "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    count = torch.bincount(label, minlength=2 * S)
    lone = count[label] == 1
    roots = label == torch.arange(2 * S, device=seg.device)
    uf, pf = u.reshape(S, 2), p.reshape(S, 2)
    nx, ny = (-uf[:, 1]).repeat_interleave(2), uf[:, 0].repeat_interleave(2)
    cc = nx * pf[:, 0].repeat_interleave(2) + ny * pf[:, 1].repeat_interleave(2)
    sums = [torch.zeros(2 * S, dtype=torch.float64, device=seg.device).index_add_(0, label, x) for x in (nx * nx, nx * ny, ny * ny, nx * cc, ny * cc)]
    det = sums[0] * sums[2] - sums[1] * sums[1]
    junction = torch.stack([(sums[2] * sums[3] - sums[1] * sums[4]) / det, (sums[0] * sums[4] - sums[1] * sums[3]) / det], dim=1)
    # the T ends
    Xf, Yf = torch.where(upper, X, X.transpose(1, 2)), torch.where(upper, Y, Y.transpose(1, 2))
    af = torch.where(upper, angle, angle.transpose(1, 2)) & (ar[:, None] != ar[None, :])[None]
    sj = (Xf - col(p[..., 0])) * col(u[..., 0]) + (Yf - col(p[..., 1])) * col(u[..., 1])
    inside = af & (sj > col(g)) & (sj < col(L - g))
    tees = 0
    for k in range(2):
        a = ((Xf - row(e[k][..., 0])) * row(o[k][..., 0]) + (Yf - row(e[k][..., 1])) * row(o[k][..., 1])).abs()
        best = torch.where(inside & (a <= row(g)), a, torch.full_like(a, math.inf)).min(dim=2)
        tees = tees + (lone.reshape(S, 2)[:, k].reshape(V, n) & (best.values < math.inf)).sum()
    # the edges: one per pair of vertices, the heaviest, then the lowest
    ends = label.reshape(S, 2)
    lo, hi = ends.min(dim=1).values, ends.max(dim=1).values
    _, inv = torch.unique(lo * (2 * S) + hi, return_inverse=True)
    top = torch.full((int(inv.max()) + 1,), -math.inf, dtype=torch.float64, device=seg.device).scatter_reduce(0, inv, weight, "amax")
    idx = torch.arange(S, device=seg.device)
    first = torch.full_like(top, 2 * S, dtype=torch.int64).scatter_reduce(0, inv, torch.where(weight == top[inv], idx, 2 * S), "amin")
    keep = (lo != hi) & (first[inv] == idx)
    return int(roots.sum()), int((roots & ~lone).sum()), int(tees), int(keep.sum()), junction


def fixture_table(dev):
    """The eight fixture views: segments, soup and built vertices, the stored junctions within 3 px of either -> the table's lines."""
    import torch
    from neat_amd import detect
    data = np.load(os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz"))
    images = torch.from_numpy(data["images"]).to(dev)
    lines, _, nfa, _, _, off = detect.lines(images)
    res = {k: v.cpu().numpy() for k, v in detect.junctions(lines.float(), detect.nfa_weight(nfa).to(dev), off).items()}
    off = off.cpu().numpy()
    soup = lines.float().cpu().numpy().reshape(-1, 2)
    out = ["# the eight fixture views, detect.lines at scale 1, gap 4 px: per view segments, soup vertices, built vertices (junctions, T ends), edges;",
           "# the rows of the junction matching are the vertices: soup against built"]
    for v in range(images.shape[0]):
        a, b = res["voff"][v], res["voff"][v + 1]
        out.append("  view %d: %3d segments, %3d soup vertices, %3d built (%2d junctions, %2d T), %3d edges"
                   % (v, off[v + 1] - off[v], 2 * (off[v + 1] - off[v]), b - a, int((res["kind"][a:b] == 1).sum()), int((res["kind"][a:b] == 2).sum()),
                      res["eoff"][v + 1] - res["eoff"][v]))
    out.append("  all:    %3d segments, %3d soup vertices, %3d built (%d junctions, %d T), %d edges"
               % (off[-1], 2 * off[-1], res["vertices"].shape[0], int((res["kind"] == 1).sum()), int((res["kind"] == 2).sum()), res["edges"].shape[0]))
    # the junctions the fixture stores (the reference's detector): the vertices on an edge of weight > 0.05, as the datasets keep them
    n_stored = n_soup = n_built = n_both = 0
    near = lambda x, pts: pts.shape[0] > 0 and float(np.linalg.norm(pts - x, axis=1).min()) <= 3.0
    for v, vid in enumerate(data["view_ids"]):
        used = np.unique(data["wf_%d_edges" % vid][data["wf_%d_weights" % vid] > 0.05])
        built = res["vertices"][res["voff"][v]:res["voff"][v + 1]]
        for x in data["wf_%d_vertices" % vid][used].astype(np.float64):
            s, b = near(x, soup[2 * off[v]:2 * off[v + 1]]), near(x, built)
            n_stored, n_soup, n_built, n_both = n_stored + 1, n_soup + s, n_built + b, n_both + (s and b)
    out.append("# the fixture's stored junctions on edges of weight > 0.05: %d; with a soup end point within 3 px: %d; with a built vertex within 3 px: %d; "
               "with both: %d" % (n_stored, n_soup, n_built, n_both))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "junctions2d_time.txt"))
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--segments", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true", help="the traced workload only; writes nothing")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 reference on the CPU")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch operations")
    ap.add_argument("--no-trace", action="store_true", help="skip the kernel table")
    ap.add_argument("--fixture", action="store_true", help="add the table of the eight fixture views")
    opt = ap.parse_args()
    import torch
    from neat_amd import detect
    from tests import junctions2d_f64 as J
    assert torch.cuda.is_available(), "junctions2d_time.py measures on the device"
    dev = torch.device("cuda:0")
    D = J.DEFAULTS
    lines = []
    for n in opt.segments:
        seg, off = workload(opt.views, n)
        weight = 0.5 + 0.4 * np.random.default_rng(1).random(seg.shape[0])
        dseg, dw = torch.from_numpy(seg).to(dev), torch.from_numpy(weight).to(dev)
        if opt.kernel_run:
            for _ in range(2):
                detect.junctions(dseg, dw, off)
            torch.cuda.synchronize()
            continue
        med, lo, hi, res = timed(lambda: detect.junctions(dseg, dw, off), opt.reps)
        got = {k: v.cpu().numpy() for k, v in res.items()}
        counts = (got["vertices"].shape[0], int((got["kind"] == 1).sum()), int((got["kind"] == 2).sum()), got["edges"].shape[0])
        lines += ["# neat_amd.detect.junctions on %d views of %d segments: 3 pair passes of %.3g pairs, float64; median (min .. max) of %d after one warm-up,"
                  % (opt.views, n, opt.views * n * n, opt.reps), "# device-synchronised wall time, the allocations and the one read-back included",
                  "junctions:  %8.3f ms (%.3f .. %.3f);  %d vertices of %d ends, %d junctions, %d T ends, %d edges" % ((med * 1e3, lo * 1e3, hi * 1e3, counts[0],
                                                                                                                     2 * seg.shape[0]) + counts[1:])]
        if not opt.no_torch:
            smin = J.sin_min(D["angle"])
            med_t, lo_t, hi_t, tc = timed(lambda: torch_build(dseg, dw, opt.views, n, D["gap"], D["frac"], smin), max(2, opt.reps // 2))
            lines.append("the rule with float64 torch operations, same device: %.1f ms (%.1f .. %.1f) = %.1f x; its counts %s equal the kernels': %s"
                         % (med_t * 1e3, lo_t * 1e3, hi_t * 1e3, med_t / med, tc[:4], tuple(tc[:4]) == counts))
        if not opt.no_host:
            t0 = time.perf_counter()
            ref, margin = cpu_build(seg, off, weight)
            t1 = time.perf_counter() - t0
            same = all(got[k].tobytes() == ref[k].tobytes() for k in got)
            lines.append("tests/junctions2d_f64.build, a view a task on 16 CPU processes: %.2f s = %.0f x; its arrays are the device's bytes: %s; "
                         "least decision margin %.3g" % (t1, t1 / med, same, margin))
    if opt.kernel_run:
        return 0
    if not opt.no_trace:
        lines += kernel_table(__file__, ["--kernel-run", "--views", str(opt.views), "--segments"] + [str(n) for n in opt.segments],
                              "the workloads twice each; %d kernels, %.3f s of kernel time", 12, family=("wireframe", "wf_"))
    if opt.fixture:
        lines += fixture_table(dev)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
