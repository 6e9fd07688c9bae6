"""Time of the 2-D line-segment detector (neat_amd.detect) -> profiles/detect_time.txt.

    timeout -k 10 1100 python scripts/detect_time.py [--out profiles/detect_time.txt] [--views 64] [--reps 5]

Workload: `--views` pictures of 1200 x 1600, seven in eight of them the views of tests/golden/scene_abc_00075213_8views.npz tiled
2 x 2 (each resized to 600 x 800, the four rotated through the fixture from picture to picture), every eighth a Gaussian noise field
(mean 128, sigma 20), in one detect.lines call at scale 1 and one at scale 0.8.  One process, one warm-up of each shape, the median of
`reps` repetitions of device-synchronised wall time; the one read-back of the offsets is included.  Beside them the same rule by
tests/detect_f64.py on this machine's CPU (16 threads allowed; numpy and scipy use what they use) for the first picture at scale 1,
with the segment counts of both.  The kernel table is from a run of its own: this script once more as a fresh process under
`rocprofv3 --kernel-trace --stats` (--kernel-run: eight pictures, both scales, twice).
"""
import argparse
import os
import sys
import time

import numpy as np

from timing import ROOT, kernel_table, timed
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz")
H, W = 1200, 1600


def pictures(views, seed=0):
    """uint8 [views,1200,1600,3]."""
    from PIL import Image
    fix = np.load(FIXTURE)["images"]
    big = [np.asarray(Image.fromarray(v).resize((W // 2, H // 2), Image.BILINEAR)) for v in fix]
    rng = np.random.default_rng(seed)
    out = np.empty((views, H, W, 3), dtype=np.uint8)
    for i in range(views):
        if i % 8 == 7:
            out[i] = np.clip(np.floor(128.0 + 20.0 * rng.standard_normal((H, W, 1)) + 0.5), 0, 255).astype(np.uint8)
        else:
            q = [big[(i + j) % len(big)] for j in range(4)]
            out[i] = np.concatenate([np.concatenate(q[:2], axis=1), np.concatenate(q[2:], axis=1)], axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_time.txt"))
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true", help="the traced workload only; writes nothing")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 reference on the CPU")
    ap.add_argument("--no-trace", action="store_true", help="skip the kernel table")
    opt = ap.parse_args()
    import torch
    from neat_amd import detect
    assert torch.cuda.is_available(), "detect_time.py measures on the device"
    dev = torch.device("cuda:0")
    if opt.kernel_run:
        images = torch.from_numpy(pictures(8)).to(dev)
        for _ in range(2):
            detect.lines(images, scale=1.0)
            detect.lines(images, scale=0.8)
        torch.cuda.synchronize()
        return 0
    host = pictures(opt.views)
    images = torch.from_numpy(host).to(dev)
    lines = ["# neat_amd.detect.lines on %d pictures of %d x %d (uint8 RGB, %.0f MB), one call; median (min .. max) of %d after one warm-up,"
             % (opt.views, H, W, host.nbytes / 1e6, opt.reps), "# device-synchronised wall time, the read-back of the offsets included"]
    for scale in (1.0, 0.8):
        med, lo, hi, r = timed(lambda: detect.lines(images, scale=scale), opt.reps)
        per = np.diff(r[5].cpu().numpy())
        lines.append("scale %.1f: %8.1f ms (%.1f .. %.1f)  = %6.2f ms a picture, %7.1f M pixels/s;  %d segments (%d .. %d a picture, noise pictures %d)"
                     % (scale, med * 1e3, lo * 1e3, hi * 1e3, med * 1e3 / opt.views, opt.views * H * W / med * 1e-6, int(per.sum()), int(per.min()),
                        int(per.max()), int(per[7::8].sum())))
    one = detect.lines(images[:1], scale=1.0)
    med1, lo1, hi1, _ = timed(lambda: detect.lines(images[:1], scale=1.0), opt.reps)
    lines.append("one picture, scale 1.0: %.2f ms (%.2f .. %.2f), %d segments" % (med1 * 1e3, lo1 * 1e3, hi1 * 1e3, one[0].shape[0]))
    if not opt.no_host:
        from tests import detect_f64 as D
        t0 = time.perf_counter()
        ref = D.detect(host[:1], 1.0)
        t1 = time.perf_counter() - t0
        same = ref["lines"].shape[0] == one[0].shape[0] and np.array_equal(ref["n"], one[3].cpu().numpy()) and \
            bool(np.abs(ref["lines"] - one[0].cpu().numpy()).max() < 1e-9) if ref["lines"].shape[0] == one[0].shape[0] else False
        lines.append("tests/detect_f64.detect on the CPU, the same picture: %.2f s (%.0f x), %d segments, %d regions judged; equal to the device's: %s"
                     % (t1, t1 / med1, ref["lines"].shape[0], int(ref["cand_judge"].sum()), same))
    if not opt.no_trace:
        lines += kernel_table(__file__, ["--kernel-run"], "8 pictures of 1200 x 1600 at scale 1 and at 0.8, twice; %d kernels, %.3f s of kernel time", 14, limit=420)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
