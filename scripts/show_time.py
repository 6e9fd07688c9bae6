"""Milliseconds per pass of `neat_amd.show` for a turntable and for one frame, with and without a large mesh behind the wireframe, next
to the reference's drawing path on the same machine -> profiles/show_time.txt.

    python scripts/show_time.py [--segments 3000] [--grid 512] [--frames 72] [--size 1024] [--no-host] [--out profiles/show_time.txt]

The wireframe is synthetic (segments between neighbouring points of a noisy sphere and box, inside the unit ball, the size of a parsed
scene's); the mesh is the zero level of a bumpy sphere sampled on a grid^3 lattice, extracted by neat_amd.mesh.  Per pass: HIP events,
3 warm-up renders, the median of 10.  Encoding (PNG + GIF through PIL) is timed once.  A cube's twelve frame-filling triangles are timed as the
other extreme of the mesh pass.  The host baseline draws what the reference's loop draws per frame (show.py:386-404: all projected segments as
0.03-point black lines on a figure-filling axes, saved as PNG at dpi = width) with matplotlib's Agg backend, the median of 5 frames.
"""
import argparse
import os
import statistics
import tempfile
import time

import numpy as np
import torch

from timing import ROOT


def wireframe(n, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    a = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 0.8, (n, 1))
    b = a + rng.normal(0, 0.12, (n, 3))
    return np.stack([a, b], 1)


def bumpy_sphere(grid, dev):
    from neat_amd import mesh as M
    ax = torch.linspace(-1.0, 1.0, grid, device=dev)
    g = torch.empty(grid, grid, grid, device=dev, dtype=torch.float32)
    for i in range(grid):          # a slab at a time: the whole lattice of coordinates would be three more grids
        x, y, z = ax[i], ax[:, None], ax[None, :]
        r = torch.sqrt(x * x + y * y + z * z)
        g[i] = r - 0.6 - 0.03 * torch.sin(9 * x) * torch.sin(7 * y) * torch.sin(8 * z)
    verts, faces = M.extract(g, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))[:2]
    return verts.to(torch.float64), faces


def host_frame(lines2d, width, height, path):
    """The baseline's frame in object-oriented matplotlib: a figure of width / height x 1 inches whose single axes fills it, pixel-centre
    limits with y downwards, every segment as a black line of 0.03 points, saved at dpi = width.  These are the artists, the canvas size
    and the resolution of the reference's drawing loop (Agg rasterises a LineCollection and a list of Line2D alike, path by path)."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.collections import LineCollection
    from matplotlib.figure import Figure
    fig = Figure(figsize=(width / height, 1.0))
    FigureCanvasAgg(fig)
    ax = fig.add_axes([0.0, 0.0, 1.0, 1.0])
    ax.axis("off")
    ax.set_xlim(-0.5, width - 0.5)
    ax.set_ylim(height - 0.5, -0.5)
    ax.add_collection(LineCollection(lines2d, colors="black", linewidths=0.03))
    fig.savefig(path, dpi=width)


def project(w2c, K, X):
    c = X @ w2c[:3, :3].T + w2c[:3, 3]
    return np.stack([K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2], K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]], -1)


def cube():
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=3000)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--frames", type=int, default=72)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "show_time.txt"))
    opt = ap.parse_args()
    from neat_amd import show
    dev = torch.device("cuda", 0)
    W = H = opt.size
    lines = wireframe(opt.segments)
    ld = torch.tensor(lines, device=dev)
    verts, faces = bumpy_sphere(opt.grid, dev)
    K = show.intrinsics(W, H, 60.0)
    passes = ("clear", "mesh", "lines", "resolve")
    out = ["# scripts/show_time.py on %s: %d segments, width 1.5; mesh of %d triangles (%d^3 lattice); %d x %d frames; HIP events, "
           "3 warm-ups, median of %d, milliseconds" % (torch.cuda.get_device_name(0), len(lines), len(faces), opt.grid, W, H, opt.reps),
           "# case                      frames    clear     mesh    lines  resolve    total  ms/frame"]
    frames = None
    for name, F, mesh in (("wireframe", opt.frames, None), ("wireframe + mesh", opt.frames, (verts, faces)), ("wireframe", 1, None),
                          ("wireframe + mesh", 1, (verts, faces)), ("wireframe + cube (12)", opt.frames, cube())):
        w2c = show.orbit(*show.POSES["dtu"], frames=F, step=5.0)
        runs = []
        for rep in range(3 + opt.reps):
            t = {}
            res = show.render(ld, w2c, K, W, H, mesh=mesh, timings=t)
            if rep >= 3:
                runs.append(t)
            if F > 1 and mesh is not None and len(mesh[1]) > 12:
                frames = res
        med = {k: statistics.median(r.get(k, 0.0) for r in runs) for k in passes}
        total = sum(med.values())
        out.append("%-26s %7d %8.3f %8.3f %8.3f %8.3f %8.3f %9.3f" % (name, F, *(med[k] for k in passes), total, total / F))
        print(out[-1], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        host = frames.cpu()
        t1 = time.perf_counter()
        show.write_frames(os.path.join(tmp, "video"), host, gif=os.path.join(tmp, "video.gif"))
        t2 = time.perf_counter()
        out.append("# encoding the %d frames: copy to the host %.3f s, PNG + GIF through PIL %.3f s (%.1f ms per frame)"
                   % (len(host), t1 - t0, t2 - t1, 1e3 * (t2 - t1) / len(host)))
        print(out[-1], flush=True)
        if not opt.no_host:
            w2c = show.orbit(*show.POSES["dtu"], frames=5, step=5.0)
            times = []
            for k in range(5):
                l2d = project(w2c[k], K, lines.reshape(-1, 3)).reshape(-1, 2, 2)
                t0 = time.perf_counter()
                host_frame(l2d, W, H, os.path.join(tmp, "%04d.png" % k))
                times.append(time.perf_counter() - t0)
            out.append("# host: the reference's drawing path (all segments as 0.03-point lines + savefig at dpi = width to PNG, matplotlib Agg, wireframe "
                       "only; it has no mesh path), median of 5 frames: %.1f ms per frame" % (1e3 * statistics.median(times)))
            print(out[-1], flush=True)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
