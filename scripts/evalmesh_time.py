"""Time of the evaluation mesh (neat_amd.mesh.eval_surface) on the synthetic geometric-initialisation model at resolution 512: the
stages the CLI prints -- coarse mesh, frame, fine grid, extraction, cut, components -- without a box (get_surface_high_res_mesh) and with
one that cuts the surface (get_surface_by_grid), for bf16 and fp16x3 -> profiles/evalmesh_time.txt.

    timeout -k 10 900 python scripts/evalmesh_time.py [--out profiles/evalmesh_time.txt] [--resolution 512] [--reps 3]

One process.  Every figure is the mean of `reps` runs after one warm-up of the same shape; eval_surface synchronises around each stage
itself when it is given a timings dict, so the stages are wall-clock seconds between synchronisations and include their read-backs.
"""
import argparse
import os

import numpy as np
import torch

from timing import ROOT
STAGES = ("coarse_s", "frame_s", "grid_s", "extract_s", "cut_s", "components_s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalmesh_time.txt"))
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evalmesh_time.py measures on the GPU: no device found")
    from neat_amd import mesh, networks, synth
    dev = torch.device("cuda:0")
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in synth.synth_state_dict(7, "init").items()})
    model.to(dev).eval()
    lines = ["# scripts/evalmesh_time.py on %s: synthetic 'init' model, resolution %d, mean of %d runs after a warm-up, seconds between synchronisations"
             % (torch.cuda.get_device_name(0), opt.resolution, opt.reps),
             "# prec    route  grid              coarse     frame  fine grid   extract       cut  components     total   vertices      faces"]
    for prec in ("bf16", "fp16x3"):
        model.set_precision(prec)
        probe = mesh.eval_surface(model, resolution=64)["verts"]
        lo, hi = probe.min(dim=0).values.cpu().numpy() - 0.1, probe.max(dim=0).values.cpu().numpy() + 0.1
        hi[0] = 0.5 * (lo[0] + hi[0]) + 0.2 * (hi[0] - lo[0])        # a box that cuts the surface
        for route, bbox in (("free", None), ("box", np.stack([lo, hi]))):
            mesh.eval_surface(model, resolution=opt.resolution, bbox=bbox)
            total = {}
            for _ in range(opt.reps):
                t = {}
                res = mesh.eval_surface(model, resolution=opt.resolution, bbox=bbox, timings=t)
                for k, v in t.items():
                    total[k] = total.get(k, 0.0) + v / opt.reps
            lines.append("%-8s %-5s %-15s " % (prec, route, "x".join(str(n) for n in res["frame"]["shape"]))
                         + " ".join("%9.4f" % total.get(k, 0.0) for k in STAGES)
                         + " %11.4f %10d %10d" % (sum(total.values()), res["verts"].shape[0], res["faces"].shape[0]))
            print(lines[-1], flush=True)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
