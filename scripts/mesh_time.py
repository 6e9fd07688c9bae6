"""Time of the surface mesh path (neat_amd.mesh) on the synthetic geometric-initialisation model (one closed sphere-like surface): grid evaluation and extraction separately, at 100^3,
256^3 and 512^3, for bf16 and fp16x3 -> profiles/mesh_time.txt.

    timeout -k 10 900 python scripts/mesh_time.py [--out profiles/mesh_time.txt] [--sizes 100 256 512] [--reps 5]

One process.  Every figure is the mean of `reps` repetitions between two device events after one warm-up of the same shape.  The grid
evaluation is set against secondary.sdf_mlp_forward_<precision> of profiles/r06_bench_bf16.json (the same fused values-mode kernel on
131 072 points); the extraction's algorithmic bytes (the grid read twice, the edge bits and vertex bases written and read, vertices and
faces written) against the 6.29 TB/s float4 copy rate of the MI355X.  The extraction includes its one read-back of the two counts.
"""
import argparse
import json
import os

import torch

from timing import ROOT
COPY_RATE = 6.29e12      # bytes/s, float4 copy measured on MI355X


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 256, 512])
    ap.add_argument("--reps", type=int, default=5)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_time.py measures on the GPU: no device found")
    from neat_amd import mesh, networks, synth
    ref = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_bf16.json")))["secondary"]
    dev = torch.device("cuda:0")
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in synth.synth_state_dict(7, "init").items()})
    model.to(dev).eval()
    lines = ["# scripts/mesh_time.py on %s: synthetic 'init' model, grid [-1.5, 1.5]^3, chunk %d nodes, mean of %d repetitions between device events"
             % (torch.cuda.get_device_name(0), mesh.DEFAULT_CHUNK, opt.reps),
             "# prec      n   grid ms   Mquery/s  of sdf_mlp_forward   extract ms   nv        nf        alg. MB    GB/s   of 6.29 TB/s copy"]
    for prec in ("bf16", "fp16x3"):
        model.set_precision(prec)
        ref_rate = ref["sdf_mlp_forward_" + prec]["value"]
        for n in opt.sizes:
            nodes = n ** 3
            g_ms, grid = timed(lambda: mesh.sdf_grid(model, n, (-1.5, 1.5)), opt.reps)
            x_ms, (verts, faces) = timed(lambda: mesh.extract(grid, -1.5, 1.5), opt.reps)
            nv, nf = verts.shape[0], faces.shape[0]
            nbytes = 2 * 4 * nodes + 2 * (1 + 4) * nodes + 12 * nv + 12 * nf
            rate = nodes / (g_ms * 1e-3)
            lines.append("%-7s %5d %9.3f %10.1f %10.3f %19.3f %9d %9d %10.1f %8.1f %10.3f"
                         % (prec, n, g_ms, rate / 1e6, rate / ref_rate, x_ms, nv, nf, nbytes / 1e6, nbytes / (x_ms * 1e-3) / 1e9,
                            nbytes / (x_ms * 1e-3) / COPY_RATE))
            print(lines[-1], flush=True)
            del grid, verts, faces
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
