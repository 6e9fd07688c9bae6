"""Time of ray casting against a triangle mesh (neat_amd.raycast) -> profiles/raycast_time.txt.

    timeout -k 10 1100 python scripts/raycast_time.py [--out profiles/raycast_time.txt] [--reps 3]

Workloads, on an icosphere of 327 680 triangles (level 7):
  (a) the build of the tree plus one 1200 x 1600 closest-hit view (raycast.build, raycast.view);
  (b) any-hit visibility of 50 000 lines x 16 samples from 64 views (raycast.visible_lines: 51.2 M rays).
Beside them the same answer by two other routes on a subset both can finish (20 480 triangles, 65 536 rays of the view): the rule of
tests/raycast_f64.py by brute force over all triangles in float64 torch on the same device, and tests/raycast_f64.cast_all on 16 CPU
processes.  One process, one warm-up, the median of `reps` repetitions (device-synchronised wall time).  The kernel table is from a run of
its own: this script once more as a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: workload (a) twice and a
sixteenth of workload (b)).
"""
import argparse
import os
import statistics
import time
from concurrent.futures import ProcessPoolExecutor
import multiprocessing

import numpy as np

from timing import ROOT, kernel_table, sync_time


def torch_brute_force(verts, faces, o, d, chunk=256):
    """The rule of tests/raycast_f64.py over all triangles in float64 torch -> (t, tri) on the device."""
    import torch
    tv = verts[faces.long()]                                        # [nf,3,3]
    R = o.shape[0]
    t_out = torch.full((R,), float("inf"), device=o.device, dtype=torch.float64)
    tri = torch.full((R,), -1, device=o.device, dtype=torch.int64)
    o, d = o.double(), d.double()
    kz = d.abs().argmax(dim=1)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = d.gather(1, kz[:, None])[:, 0] < 0
    kx, ky = torch.where(neg, ky, kx), torch.where(neg, kx, ky)
    for i in range(0, R, chunk):
        s = slice(i, i + chunk)
        P = tv[None] - o[s, None, None, :]                          # [r,nf,3,3]
        r = P.shape[0]
        pick = lambda k: P.gather(3, k[s].view(r, 1, 1, 1).expand(r, P.shape[1], 3, 1))[..., 0]
        dk = lambda k: d[s].gather(1, k[s, None])
        Pz, dz = pick(kz), dk(kz)
        Sx, Sy, Sz = (dk(kx) / dz)[:, :, None], (dk(ky) / dz)[:, :, None], (1.0 / dz)[:, :, None]
        X, Y = pick(kx) - Sx * Pz, pick(ky) - Sy * Pz
        U = X[..., 2] * Y[..., 1] - Y[..., 2] * X[..., 1]
        V = X[..., 0] * Y[..., 2] - Y[..., 0] * X[..., 2]
        W = X[..., 1] * Y[..., 0] - Y[..., 1] * X[..., 0]
        det = (U + V) + W
        Z = Sz * Pz
        t = ((U * Z[..., 0] + V * Z[..., 1]) + W * Z[..., 2]) / det
        acc = (((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))) & (det != 0) & (t >= 0)
        t = torch.where(acc, t, torch.full_like(t, float("inf")))
        best, idx = t.min(dim=1)
        t_out[s], tri[s] = best, torch.where(torch.isinf(best), torch.full_like(idx, -1), idx)
    return t_out, tri


def _cpu_chunk(args):
    from tests import raycast_f64 as RC
    verts, faces, o, d = args
    return RC.cast_all(verts, faces, o, d)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_time.txt"))
    ap.add_argument("--level", type=int, default=7, help="icosphere level of the workloads (7: 327 680 triangles)")
    ap.add_argument("--sub-level", type=int, default=5, help="icosphere level of the comparison subset (5: 20 480 triangles)")
    ap.add_argument("--sub-rays", type=int, default=65536)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run, no file")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raycast_time.py measures on the GPU: no device found")
    from neat_amd import ops, raycast, render, synth
    from tests import raycast_f64 as RC
    dev = torch.device("cuda:0")
    H, W = 1200, 1600
    verts, faces = RC.icosphere(opt.level)
    w2c = np.linalg.inv(synth.synth_scene(seed=1, n_rays=4, res=64, view=1)["pose"][0].astype(np.float64))
    w2c[:3, 3] *= 1.5                                              # the camera at distance 3 of the unit sphere
    uv, pose, K = render.camera_view(w2c, W, H, 40.0, dev)
    rng = np.random.default_rng(0)
    u = rng.standard_normal((opt.lines, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = u * rng.uniform(0.8, 1.3, (opt.lines, 1))
    lines = torch.from_numpy(np.stack([a, a + 0.1 * rng.standard_normal((opt.lines, 3))], 1)).float().to(dev)
    c = rng.standard_normal((opt.views, 3))
    c = 3.0 * c / np.linalg.norm(c, axis=1, keepdims=True)
    cams = np.stack([np.linalg.inv(synth.look_at_pose(tuple(x)).astype(np.float64)) for x in c])
    v_dev, f_dev = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)

    if opt.kernel_run:
        for _ in range(2):
            scene = raycast.build(v_dev, f_dev)
            raycast.view(scene, pose, K, H, W)
        raycast.visible_lines(scene, lines[:opt.lines // 16], cams)
        torch.cuda.synchronize()
        return
    out = ["# scripts/raycast_time.py on %s: icosphere level %d (%d triangles), median of %d after one warm-up"
           % (torch.cuda.get_device_name(0), opt.level, faces.shape[0], opt.reps)]
    tb, tv, tl = [], [], []
    for rep in range(opt.reps + 1):
        s, scene = sync_time(lambda: raycast.build(v_dev, f_dev))
        tb.append(s)
        s, (depth, _, tri) = sync_time(lambda: raycast.view(scene, pose, K, H, W))
        tv.append(s)
        s, frac = sync_time(lambda: raycast.visible_lines(scene, lines, cams))
        tl.append(s)
    dirs, _, origins = ops.camera_rays(uv, pose, K, with_origins=True)
    dirs = dirs.reshape(-1, 3)
    counts = torch.zeros(H * W, 2, device=dev, dtype=torch.int32)
    tc = [sync_time(lambda: raycast.cast(scene, origins, dirs, counts=counts))[0] for _ in range(opt.reps + 1)]
    med = lambda x: statistics.median(x[1:])
    nrays = opt.lines * 16 * opt.views
    out += ["(a) build %.4f s; one %d x %d closest-hit view %.4f s (the cast alone, with counts: %.4f s = %.1f M rays/s; %d hit pixels; per ray %.1f node"
            " boxes and %.2f triangles tested)" % (med(tb), W, H, med(tv), med(tc), H * W / med(tc) * 1e-6, int((tri >= 0).sum()),
                                                   counts[:, 0].float().mean().item(), counts[:, 1].float().mean().item()),
            "(b) any-hit visibility of %d lines x 16 samples from %d views (%.1f M rays, target rays included): %.4f s = %.1f M rays/s; mean visible"
            " fraction %.3f" % (opt.lines, opt.views, nrays * 1e-6, med(tl), nrays / med(tl) * 1e-6, frac.mean().item())]
    print("\n".join(out[1:]), flush=True)
    # the subset both other routes can finish
    sv, sf = RC.icosphere(opt.sub_level)
    pick = torch.from_numpy(np.sort(rng.choice(H * W, opt.sub_rays, replace=False))).to(dev)
    so, sd = origins[pick].contiguous(), dirs[pick].contiguous()
    sv_dev, sf_dev = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    td, tt = [], []
    for rep in range(opt.reps + 1):
        s, (t_dev, tri_dev, _) = sync_time(lambda: raycast.cast(raycast.build(sv_dev, sf_dev), so, sd))
        td.append(s)
    for rep in range(2):
        s, (t_t, tri_t) = sync_time(lambda: torch_brute_force(sv_dev, sf_dev, so, sd))
        tt.append(s)
    o_np, d_np = so.cpu().numpy(), sd.cpu().numpy()
    t0 = time.perf_counter()
    with ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("spawn")) as pool:
        parts = list(pool.map(_cpu_chunk, [(sv, sf, o_np[i:i + 1024], d_np[i:i + 1024]) for i in range(0, opt.sub_rays, 1024)]))
    t_cpu = time.perf_counter() - t0
    tri_cpu = np.concatenate([p[1] for p in parts])
    t_cpu64 = np.concatenate([p[0] for p in parts])
    same_t = int((tri_dev.cpu().numpy() == tri_cpu).sum())
    out += ["subset: icosphere level %d (%d triangles), %d rays of the view; build + closest hit" % (opt.sub_level, sf.shape[0], opt.sub_rays),
            "  neat_amd.raycast (build + cast)                          %10.5f s" % med(td),
            "  the rule by brute force, float64 torch, same device      %10.5f s   (x %.0f)" % (tt[-1], tt[-1] / med(td)),
            "  tests/raycast_f64.cast_all, 16 CPU processes             %10.5f s   (x %.0f)" % (t_cpu, t_cpu / med(td)),
            "  agreement: triangle equal to cast_all's on %d of %d rays, to the torch form's on %d; max |t - cast_all t| %.3g"
            % (same_t, opt.sub_rays, int((tri_dev.long() == tri_t).sum()), opt.sub_rays and float(np.nanmax(np.abs(np.where(
                tri_cpu >= 0, t_dev.cpu().numpy().astype(np.float64) - t_cpu64, 0.0)))))]
    print("\n".join(out[-5:]), flush=True)
    out += kernel_table(__file__, ["--kernel-run", "--level", str(opt.level)],
                        "the build and the view twice, 3 125 lines x 16 samples x 64 views; %d kernels, %.3f s of kernel time", 12, limit=420)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
