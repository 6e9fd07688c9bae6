"""Time of crease extraction (neat_amd.creases) -> profiles/creases_time.txt.

    timeout -k 10 900 python scripts/creases_time.py [--out profiles/creases_time.txt] [--reps 10]

Cases: the icosphere of 327 680 triangles that the other tools time (level 7: nothing is sharp at 30 degrees, so the welds, the sort
of the half-edges and the classification are all there is), and the L block subdivided to 20 480 and 327 680 triangles (18 chains of
2^5 and 2^7 edges each).  Beside creases.lines: the same rule as torch operations on the same device (torch_rule below: unique, sort,
scatter_reduce; the chains by min-label propagation with pointer jumping), whose counts are reported beside the tool's, and once the
float64 restatement tests/creases_f64.py on the CPU.  One process, one warm-up, the median of `reps` repetitions (device-synchronised
wall time, the host's read-backs included).  The kernel table is from a run of its own: this script once more as a fresh process under
`rocprofv3 --kernel-trace --stats` (--kernel-run: creases.lines once per case).
"""
import argparse
import os
import statistics
import time

import numpy as np

from timing import ROOT, kernel_table, sync_time


def torch_rule(v, f, c, s2, length, boundary=True):
    """DESIGN 3n as torch operations on the device of v -> (feature edges, chains, lines).  Sums of three products are torch's, so a
    decision on the last bit may differ from the tool's."""
    import torch
    nv, dev = v.shape[0], v.device
    _, inv = torch.unique(v + 0.0, dim=0, return_inverse=True)
    rep = torch.full((int(inv.max()) + 1,), nv, device=dev, dtype=torch.long).scatter_reduce(0, inv, torch.arange(nv, device=dev), "amin")
    w = rep[inv][f.long()]
    n = torch.cross(v[w[:, 1]] - v[w[:, 0]], v[w[:, 2]] - v[w[:, 0]], dim=-1)
    q = (n * n).sum(-1)
    keep = (w[:, 0] != w[:, 1]) & (w[:, 1] != w[:, 2]) & (w[:, 2] != w[:, 0]) & (q != 0.0)
    w, n, q = w[keep], n[keep], q[keep]
    p, r = w.reshape(-1), w[:, [1, 2, 0]].reshape(-1)
    skey, order = torch.sort((torch.minimum(p, r) << 32) | torch.maximum(p, r), stable=True)
    ukey, cnt = torch.unique_consecutive(skey, return_counts=True)
    start = torch.cumsum(cnt, 0) - cnt
    h1, h2 = order[start], order[(start + 1).clamp(max=order.numel() - 1)]
    lo, hi = ukey >> 32, ukey & 0xffffffff
    d = (n[h1 // 3] * n[h2 // 3]).sum(-1)
    d = torch.where((p[h1] == lo) == (p[h2] == lo), -d, d)
    s = (c * c) * (q[h1 // 3] * q[h2 // 3])
    crease = ((d < 0.0) | (d * d < s)) if c >= 0.0 else ((d < 0.0) & (d * d > s))
    kind = torch.where(cnt == 1, 1, torch.where(cnt >= 3, 2, 0))
    feat = ((cnt == 2) & crease) | (cnt >= 3) | ((cnt == 1) & bool(boundary))
    elo, ehi, ekind = lo[feat], hi[feat], kind[feat]
    E = int(elo.numel())
    if E == 0:
        return 0, 0, 0
    ids = torch.arange(E, device=dev)
    sk, _ = torch.sort((torch.cat([elo, ehi]) << 32) | torch.cat([ids, ids]))
    uv, cnt = torch.unique_consecutive(sk >> 32, return_counts=True)
    start = torch.cumsum(cnt, 0) - cnt
    se = sk & 0xffffffff
    e1, e2 = se[start], se[(start + 1).clamp(max=se.numel() - 1)]
    u = v[torch.where(elo[e1] == uv, ehi[e1], elo[e1])] - v[uv]
    t = v[torch.where(elo[e2] == uv, ehi[e2], elo[e2])] - v[uv]
    x = torch.cross(u, t, dim=-1)
    through = (cnt == 2) & (ekind[e1] == ekind[e2]) & ((u * t).sum(-1) < 0.0) & ((x * x).sum(-1) <= s2 * ((u * u).sum(-1) * (t * t).sum(-1)))
    is_end = torch.zeros(nv, device=dev, dtype=torch.bool)
    is_end[uv[~through]] = True
    a, b = e1[through], e2[through]
    label = ids.clone()
    while True:
        m = torch.minimum(label[a], label[b])
        new = label.scatter_reduce(0, a, m, "amin").scatter_reduce(0, b, m, "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    _, chain = torch.unique(label, return_inverse=True)
    C = int(chain.max()) + 1
    end_lo, end_hi = is_end[elo], is_end[ehi]
    ends = torch.zeros(C, device=dev, dtype=torch.long).index_add(0, chain, end_lo.long() + end_hi.long())
    first = torch.full((C,), nv, device=dev, dtype=torch.long)
    first = first.scatter_reduce(0, chain, torch.where(end_lo, elo, nv), "amin").scatter_reduce(0, chain, torch.where(end_hi, ehi, nv), "amin")
    last = torch.full((C,), -1, device=dev, dtype=torch.long)
    last = last.scatter_reduce(0, chain, torch.where(end_lo, elo, -1), "amax").scatter_reduce(0, chain, torch.where(end_hi, ehi, -1), "amax")
    straight = (ends == 2) & (first < last)
    A = v[first.clamp(max=nv - 1)]
    D = v[last.clamp(min=0)] - A
    bound = (length * length) * (D * D).sum(-1)
    off = torch.zeros(C, device=dev, dtype=torch.long)
    for end in (elo, ehi):
        x = torch.cross(v[end] - A[chain], D[chain], dim=-1)
        off = off.index_add(0, chain, ((x * x).sum(-1) > bound[chain]).long())
    straight &= off == 0
    return E, C, int(straight.sum()) + int((~straight[chain]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "creases_time.txt"))
    ap.add_argument("--level", type=int, default=7, help="icosphere level (7: 327 680 triangles)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run, no file")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("creases_time.py measures on the GPU: no device found")
    from neat_amd import creases, scenegen
    from tests import creases_f64 as F
    from tests import raycast_f64 as RC
    dev = torch.device("cuda:0")
    lv, lf = scenegen.shapes["lblock"][:2]
    cases = [("icosphere level %d" % opt.level,) + tuple(RC.icosphere(opt.level)), ("L block subdivided 5 times",) + tuple(scenegen.subdivide(lv, lf, 5)),
             ("L block subdivided 7 times",) + tuple(scenegen.subdivide(lv, lf, 7))]

    if opt.kernel_run:
        for _, verts, faces in cases:
            creases.lines(verts, faces, device=dev)
        torch.cuda.synchronize()
        return
    out = ["# scripts/creases_time.py on %s: angle 30, turn 1, deviation 1e-6; median of %d after one warm-up" % (torch.cuda.get_device_name(0), opt.reps)]
    for name, verts, faces in cases:
        v, f = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(dev)
        c, s2, length = F.constants(verts, 30.0, 1.0, 1e-6)
        tc, tt = [], []
        for _ in range(opt.reps + 1):
            s, res = sync_time(lambda: creases.lines(v, f))
            tc.append(s)
            s, counts = sync_time(lambda: torch_rule(v, f, c, s2, length))
            tt.append(s)
        t0 = time.perf_counter()
        want = F.lines(verts, faces)
        cpu = time.perf_counter() - t0
        same = all(np.array_equal(getattr(res, k).cpu().numpy(), want[k]) for k in ("junctions", "lines", "kind", "curved", "vertex")) and res.stats == want["stats"]
        med = lambda x: statistics.median(x[1:])
        out += ["%s: %d vertices, %d triangles -> %d feature edges, %d chains, %d lines (%d curved), %d junctions"
                % (name, verts.shape[0], faces.shape[0], res.stats["edges"], res.stats["chains"], res.lines.shape[0], int(res.curved.sum()),
                   res.junctions.shape[0]),
                "    creases.lines %.5f s (%.1f M triangles/s; min %.5f, max %.5f); the rule as torch operations %.5f s (x %.2f; edges, chains, lines "
                "%d, %d, %d); tests/creases_f64.py on the CPU %.2f s, once (x %.0f); equal to the device array for array: %s"
                % (med(tc), faces.shape[0] / med(tc) * 1e-6, min(tc[1:]), max(tc[1:]), med(tt), med(tt) / med(tc), counts[0], counts[1], counts[2], cpu,
                   cpu / med(tc), same)]
        print("\n".join(out[-2:]), flush=True)
    out += kernel_table(__file__, ["--kernel-run"], "creases.lines once per case (the uploads included); %d kernels, %.4f s of kernel time", 14)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
