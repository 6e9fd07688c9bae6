"""Time of the sphere-traced surface frame (neat_amd.trace.view) on the synthetic geometric-initialisation model: one 1200 x 1600 view, the
seconds, the SDF evaluations per ray and per iteration, and the same view through neat_amd.render.view (the volumetric forward: sampler,
main pass, both heads) timed in the same process as the comparison -> profiles/trace_time.txt.

    timeout -k 10 900 python scripts/trace_time.py [--out profiles/trace_time.txt] [--width 1600] [--height 1200] [--reps 3]

One process, one warm-up of the same shape, the median of `reps` repetitions (device-synchronised wall time: the trace reads its active
count back once per iteration, so host time is part of what a user waits for).  The kernel table is from a run of its own: this script
once more as a fresh process under `rocprofv3 --kernel-trace --stats` (--kernel-run: one warm-up and one traced view in the default build).
"""
import argparse
import os
import statistics
import time

import numpy as np
import torch

from timing import ROOT, kernel_table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_time.txt"))
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--fov", type=float, default=40.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunksize", type=int, default=65536, help="pixels per chunk of render.view")
    ap.add_argument("--kernel-run", action="store_true", help="(internal) the body of the rocprofv3 run: a warm-up and one traced view, no file")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trace_time.py measures on the GPU: no device found")
    from neat_amd import networks, ops, render, synth, trace
    dev = torch.device("cuda:0")
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in synth.synth_state_dict(7, "init").items()})
    model.to(dev).eval()
    H, W = opt.height, opt.width
    w2c = np.linalg.inv(synth.synth_scene(seed=1, n_rays=4, res=64, view=1)["pose"][0].astype(np.float64))
    uv, pose, K = render.camera_view(w2c, W, H, opt.fov, dev)
    if opt.kernel_run:
        trace.view(model, pose, K, H, W)
        trace.view(model, pose, K, H, W)
        torch.cuda.synchronize()
        return
    lines = ["# scripts/trace_time.py on %s: synthetic 'init' model, one %d x %d view (fov %g), median of %d after one warm-up"
             % (torch.cuda.get_device_name(0), W, H, opt.fov, opt.reps),
             "# prec      trace s   evals/ray  iterations   hit px   unconverged px   render.view s (chunk %d)   render / trace" % opt.chunksize]
    for prec in ("fp16x3", "bf16", "fp32"):
        model.set_precision(prec)
        ts, rec = [], []
        for rep in range(opt.reps + 1):
            tm = {}
            depth, normal, state = trace.view(model, pose, K, H, W, timings=tm)
            ts.append(tm["trace_s"])
        # the iteration count: a second pass through trace.rays with a record (not timed)
        dirs, _, origins = ops.camera_rays(uv, pose, K, with_origins=True)
        trace.rays(model, origins, dirs.reshape(-1, 3), radius=float(model.implicit_network.sdf_bounding_sphere), record=rec)
        rs = []
        for rep in range(opt.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render.view(model, uv, pose, K, H, W, chunksize=opt.chunksize)
            torch.cuda.synchronize()
            rs.append(time.perf_counter() - t0)
        t_s, r_s = statistics.median(ts[1:]), statistics.median(rs[1:])
        counts = torch.bincount(state.reshape(-1).long(), minlength=4).tolist()
        lines.append("%-7s %9.4f %10.2f %11d %9d %15d %16.4f %26.1f" % (prec, t_s, tm["evals"] / (H * W), len(rec), counts[trace.HIT],
                                                                       counts[trace.UNCONVERGED], r_s, r_s / t_s))
        print(lines[-1], flush=True)
    lines += kernel_table(__file__, ["--kernel-run", "--width", str(opt.width), "--height", str(opt.height), "--fov", str(opt.fov)],
                          "one warm-up and one traced view, default build; %d kernels, %.3f s of kernel time", 14, limit=420, family=("trace", "trace_"))
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
