"""Seconds per frame of `neat_amd.render` on one 1200 x 1600 view (a DTU view's 1.92 M pixels) at three chunk sizes, split into
rendering, frame kernels and PNG encoding, next to the host route the reference takes on the same chunks -> profiles/render_time.txt.

    python scripts/render_time.py [--width 1600] [--height 1200] [--chunks 1024,10000,65536] [--reps 3] [--no-host] [--no-trace]
                                  [--out profiles/render_time.txt]

Synthetic weights (synth.synth_state_dict) and a camera of neat_amd.show's orbit through the --cam-json route (render.camera_view), so no
dataset is needed; the ground truth of the error sum is uniform noise.  Per case: one warm-up frame, the median of --reps frames, wall
clock around device-synchronised frames; the frame kernels' share is the sum of HIP-event intervals around their launches.
device route  render.view: render_pixels per chunk + one neat_frame_put, then the sum, the range and the grey pass; then the three PNGs.
host route    what eval.py does: model(s) per chunk (the eval forward with its junction and line block), torch.cat, .cpu().numpy(),
              (x * 255).astype(uint8) and a float32 torch.mean of the squares; its PNG is the same encoder and is not timed again.
The kernel table is from a run of its own: this script under `rocprofv3 --kernel-trace --stats` for one frame at the middle chunk size.
"""
import argparse
import os
import statistics
import tempfile
import time

import numpy as np
import torch

from timing import ROOT, kernel_table


def setup(width, height, dev):
    from neat_amd import networks, render, show, synth
    from neat_amd.wireframe import WireframeGraph
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in synth.synth_state_dict(7, "rough").items()})
    model.to(dev).eval()
    w2c = show.orbit(*show.POSES["dtu"], frames=1)[0]
    uv, pose, K = render.camera_view(w2c, width, height, 60.0, dev)
    gt = torch.rand(height * width, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    sc = synth.synth_scene(seed=3, n_rays=4)
    wf = WireframeGraph(torch.tensor(sc["wf_vertices"]), torch.tensor(sc["wf_vconf"]), torch.tensor(sc["wf_edges"]), torch.tensor(sc["wf_weights"]),
                        height, width)
    return model, uv, pose, K, gt, wf


def device_frame(model, uv, pose, K, gt, H, W, chunk, tmp):
    from neat_amd import render
    t = {}
    res = render.view(model, uv, pose, K, H, W, gt=gt, chunksize=chunk, timings=t)
    t0 = time.perf_counter()
    for name, key in (("eval", "rgb"), ("normal", "normal"), ("depth", "depth8")):
        render.write_png(os.path.join(tmp, name + ".png"), res[key])
    t["encode_s"] = time.perf_counter() - t0
    return t


def host_frame(model, uv, pose, K, gt, wf, H, W, chunk):
    """eval.py:100-126 on the same chunks: -> seconds (device-synchronised wall clock), without the PNG."""
    from neat_amd.general import split_input
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inp = {"uv": uv, "uv_proj": uv, "pose": pose, "intrinsics": K, "wireframe": [wf]}
    with torch.no_grad():
        res = [model(s)["rgb_values"].detach() for s in split_input(inp, H * W, n_pixels=chunk)]
        rgb = torch.cat(res, 0)
        img = (rgb.reshape(H, W, 3).cpu().numpy() * 255).astype(np.uint8)
        mse = torch.mean((rgb - gt) ** 2)
        psnr = (-10.0 * torch.log(mse) / np.log(10.0)).item()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, img, psnr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--chunks", default="1024,10000,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced", action="store_true", help="(internal) the body of the rocprofv3 run: frames only, no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.txt"))
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = opt.width, opt.height
    chunks = [int(c) for c in opt.chunks.split(",")]
    model, uv, pose, K, gt, wf = setup(W, H, dev)
    with tempfile.TemporaryDirectory() as tmp:
        if opt.traced:
            for _ in range(2):
                device_frame(model, uv, pose, K, gt, H, W, chunks[0], tmp)
            return
        from neat_amd import networks
        out = ["# scripts/render_time.py on %s: one %d x %d frame (%d pixels), synthetic weights, precision %s; 1 warm-up frame, median of %d, "
               "device-synchronised wall clock, seconds" % (torch.cuda.get_device_name(0), H, W, H * W, networks.DEFAULT_PRECISION, opt.reps),
               "# route    chunk   chunks    frame_s  rendering  frame kernels   encoding   (frame_s = rendering + frame kernels; encoding = 3 PNGs)"]
        for chunk in chunks:
            runs = [device_frame(model, uv, pose, K, gt, H, W, chunk, tmp) for _ in range(1 + opt.reps)][1:]
            med = {k: statistics.median(r[k] for r in runs) for k in ("render_s", "frame_s", "encode_s")}
            out.append("device %8d %8d %10.3f %10.3f %14.4f %10.3f" % (chunk, -(-H * W // chunk), med["render_s"], med["render_s"] - med["frame_s"],
                                                                    med["frame_s"], med["encode_s"]))
            print(out[-1], flush=True)
            if not opt.no_host:
                runs = [host_frame(model, uv, pose, K, gt, wf, H, W, chunk)[0] for _ in range(1 + opt.reps)][1:]
                out.append("host   %8d %8d %10.3f   (model(s) per chunk, torch.cat, .cpu().numpy(), numpy cast, float32 mean)"
                           % (chunk, -(-H * W // chunk), statistics.median(runs)))
                print(out[-1], flush=True)
    if not opt.no_trace:
        chunk = str(chunks[len(chunks) // 2])
        out += kernel_table(__file__, ["--traced", "--width", str(opt.width), "--height", str(opt.height), "--chunks", chunk],
                            "one warm-up and one timed frame at chunk " + chunk + "; %d kernels, %.3f s of kernel time", 14, limit=420,
                            family=("frame", "frame_"))
        print("\n".join(out[-18:]), flush=True)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
