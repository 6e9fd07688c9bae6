"""Time of scene generation (neat_amd.scenegen) -> profiles/scenegen_time.txt.

    timeout -k 10 900 python scripts/scenegen_time.py [--out profiles/scenegen_time.txt] [--reps 3]

Workloads, on an icosphere of 327 680 triangles (level 7, as scripts/raycast_time.py) scaled to the unit box:
  (a) the pictures: 100 views of 512 x 512 at ss = 3 (235.9 M rays) in one launch of scenegen.pictures, and beside it the same pictures
      on the interface the tool replaces, in the same process: raycast.cast with nine float32 rays per pixel and torch operations for
      the normals, the shading and the resolve, view by view;
  (b) the edges: the 18 edges of the L block from the same 100 views at step 1 (scenegen.visible_edges: count, scan, fill), and beside it
      raycast.visible_lines with 16 samples per edge.
One process, one warm-up, the median of `reps` repetitions (device-synchronised wall time).  The kernel table is from a run of its
own: this script once more as a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: both workloads once).
"""
import argparse
import os
import statistics

import numpy as np

from timing import ROOT, kernel_table, sync_time


def parent_pictures(scene, K, poses, H, W, ss, albedo=0.7, ambient=0.25, background=1.0):
    """The pictures through raycast.cast: float32 rays, the shading and the resolve as torch operations -> (rgb, mask) as scenegen.pictures."""
    import torch
    from neat_amd import raycast
    dev = scene.device
    Kd, Pd = torch.from_numpy(K).to(dev), torch.from_numpy(poses).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    sub = (torch.arange(ss, device=dev, dtype=torch.float64) + 0.5) / ss - 0.5
    u = (xs[..., None, None] + sub[None, None, None, :]).expand(H, W, ss, ss).reshape(-1)
    v = (ys[..., None, None] + sub[None, None, :, None]).expand(H, W, ss, ss).reshape(-1)
    tv = scene.verts[scene.faces.long()]
    normals = torch.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0], dim=-1)
    normals = (normals / normals.norm(dim=-1, keepdim=True)).float()
    rgb = torch.empty(len(poses), H, W, 3, device=dev, dtype=torch.uint8)
    mask = torch.empty(len(poses), H, W, device=dev, dtype=torch.uint8)
    for f in range(len(poses)):
        yl = (v - Kd[f, 1, 2]) / Kd[f, 1, 1]
        xl = ((u - Kd[f, 0, 2]) - Kd[f, 0, 1] * yl) / Kd[f, 0, 0]
        d = (xl[:, None] * Pd[f, :3, 0] + yl[:, None] * Pd[f, :3, 1] + Pd[f, :3, 2]).float()
        o = Pd[f, :3, 3].float().expand_as(d).contiguous()
        _, tri, _ = raycast.cast(scene, o, d)
        hit = tri >= 0
        n = normals[tri.clamp(min=0).long()]
        cosv = (n * d).sum(-1).abs() / d.norm(dim=-1)
        col = torch.where(hit, albedo * (ambient + (1.0 - ambient) * cosv), torch.full_like(cosv, background))
        pix = col.view(H, W, ss * ss).mean(dim=-1)
        rgb[f] = torch.floor(255.0 * pix + 0.5).clamp(0, 255).to(torch.uint8)[..., None].expand(H, W, 3)
        mask[f] = hit.view(H, W, ss * ss).any(dim=-1).to(torch.uint8) * 255
    return rgb, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenegen_time.txt"))
    ap.add_argument("--level", type=int, default=7, help="icosphere level (7: 327 680 triangles)")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--ss", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run, no file")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scenegen_time.py measures on the GPU: no device found")
    from neat_amd import raycast, scenegen
    from tests import raycast_f64 as RC
    dev = torch.device("cuda:0")
    verts, faces = RC.icosphere(opt.level)
    _, _, J, E = scenegen.shapes["lblock"]
    verts, _ = scenegen.normalise(verts, J)                     # the sphere of radius 0.5; the L block pokes through it
    K, poses = scenegen.cameras(opt.views, opt.res)
    H = W = opt.res
    v_dev, f_dev = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    w2c = np.linalg.inv(poses)
    segs = torch.from_numpy(J[E]).float().to(dev)

    scene = raycast.build(v_dev, f_dev)
    if opt.kernel_run:
        scenegen.pictures(scene, K, poses, H, W, ss=opt.ss)
        scenegen.visible_edges(scene, J, E, K, poses, H, W)
        torch.cuda.synchronize()
        return
    out = ["# scripts/scenegen_time.py on %s: icosphere level %d (%d triangles), %d views of %d x %d, ss = %d, median of %d after one warm-up"
           % (torch.cuda.get_device_name(0), opt.level, faces.shape[0], opt.views, H, W, opt.ss, opt.reps)]
    tp, tq, te, tl = [], [], [], []
    for rep in range(opt.reps + 1):
        s, (rgb, mask) = sync_time(lambda: scenegen.pictures(scene, K, poses, H, W, ss=opt.ss))
        tp.append(s)
        s, (rgb_p, mask_p) = sync_time(lambda: parent_pictures(scene, K, poses, H, W, opt.ss))
        tq.append(s)
        s, runs = sync_time(lambda: scenegen.visible_edges(scene, J, E, K, poses, H, W))
        te.append(s)
        s, frac = sync_time(lambda: raycast.visible_lines(scene, segs, w2c, samples=16))
        tl.append(s)
    med = lambda x: statistics.median(x[1:])
    rays = opt.views * H * W * opt.ss * opt.ss
    diff = (rgb.int() - rgb_p.int()).abs()
    samples = int((runs.idx[:, 3] - runs.idx[:, 2] + 1).sum())
    out += ["(a) pictures, %.1f M rays: scenegen.pictures (one launch, float64 rays) %.4f s = %.1f M rays/s; raycast.cast + torch, view by view "
            "(float32 rays) %.4f s = %.1f M rays/s (x %.2f)" % (rays * 1e-6, med(tp), rays / med(tp) * 1e-6, med(tq), rays / med(tq) * 1e-6,
                                                                 med(tq) / med(tp)),
            "    %d of %d pixels hit; bytes that differ between the two routes: %d of %d, by %d at most; masks differ on %d pixels"
            % (int((mask > 0).sum()), mask.numel(), int((diff > 0).sum()), diff.numel(), int(diff.max()), int((mask != mask_p).sum())),
            "(b) edges, %d edges x %d views at step 1: scenegen.visible_edges (count, scan, fill) %.4f s, %d runs holding %d visible samples; "
            "raycast.visible_lines, 16 samples an edge (%d rays) %.4f s, mean visible fraction %.3f"
            % (E.shape[0], opt.views, med(te), runs.idx.shape[0], samples, E.shape[0] * opt.views * 16, med(tl), frac.mean().item())]
    print("\n".join(out[1:]), flush=True)
    out += kernel_table(__file__, ["--kernel-run", "--level", str(opt.level), "--views", str(opt.views), "--res", str(opt.res)],
                        "the build, the pictures and the edges once; %d kernels, %.3f s of kernel time", 10)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
