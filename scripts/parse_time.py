"""Wall time of the wireframe parsing (neat_amd.parsing), split into the eval forward and the post-processing (distil).

    python scripts/parse_time.py

1. toy scene (the runner test's 64 x 64 scene, 6 views, untrained abc-neat-a model): wireframe_recon, forward vs post-processing;
2. a DTU-sized synthetic view set (49 views, 60 000 masked rays and 400 ground-truth lines per view, J = 1024): distil alone on
   recorded-like outputs (rows near the ground-truth lines, outliers), median of 5 runs after a warm-up."""
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

import timing  # noqa: F401 (puts the repository root on sys.path)


def toy():
    from neat_amd import networks, parsing, synth
    from neat_amd.datasets import BlenderDataset
    from tests.test_runner import _toy_scene
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        _toy_scene(Path(d) / "abc" / "toy", n_views=6)
        ds = BlenderDataset("abc/toy", [64, 64], reverse_coordinate=True, distance_threshold=1.0, data_root=d)
        torch.manual_seed(0)
        model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF).to(dev)
        for it in range(3):
            res, info = parsing.wireframe_recon(model, ds, device=dev)
        rays = sum(v["l3d"].shape[0] for v in info["views"])
        print(f"toy scene: 6 views, {rays} masked rays: forward {1e3 * info['forward_s']:.1f} ms, post-processing {1e3 * info['post_s']:.2f} ms, "
              f"lines {len(res['lines3d_all'])}, junctions {len(res['junctions3d_initial'])}")


def dtu_sized(V=49, n=60000, m=400, J=1024):
    from neat_amd import parsing
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    views = []
    for v in range(V):
        gt = np.concatenate([rng.uniform(0, 1600, (m, 4)), np.full((m, 1), 0.99)], 1).astype(np.float32)
        pick = rng.integers(0, m, n)
        l2 = gt[pick, :4] + rng.normal(0, 1.0, (n, 4)).astype(np.float32)
        l3 = rng.normal(0, 0.5, (m, 2, 3)).astype(np.float32)[pick] + rng.normal(0, 0.004, (n, 2, 3)).astype(np.float32)
        K = np.array([[1500.0, 0, 800], [0, 1500.0, 600], [0, 0, 1]], np.float32)
        ang = 2 * np.pi * v / V
        pose = np.eye(4, dtype=np.float32)
        pose[:3, 3] = [3 * np.cos(ang), 3 * np.sin(ang), 1.0]
        views.append({k: torch.tensor(a).to(dev) for k, a in (("lines2d", l2), ("lines3d", l3), ("l3d", l3.mean(1)), ("gt_lines_001", gt),
                                                               ("gt_lines_005", gt), ("K", K), ("pose", pose))})
    junc = torch.tensor(rng.normal(0, 0.5, (J, 3)).astype(np.float32)).to(dev)
    times = []
    for it in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = parsing.distil(junc, views)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(f"DTU-sized synthetic set: {V} views x {n} rays, {m} GT lines, J = {J}: post-processing median {1e3 * np.median(times[1:]):.1f} ms "
          f"(min {1e3 * min(times[1:]):.1f}), lines {len(res['lines3d_all'])}, junctions {len(res['junctions3d_initial'])}")


if __name__ == "__main__":
    toy()
    dtu_sized()
