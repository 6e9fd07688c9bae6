"""numpy restatement of the frame side of neat_amd.render (neat_amd/csrc/kernels_frame.hpp): the yardstick of
tests/test_render_*.py.  The reference's own code for these steps (utils/plots.py, utils/rend_util.py, evaluation/eval.py) needs
torchvision, skimage, imageio and plotly; what it computes is restated here: `(x * 255).astype(np.uint8)` wherever that cast is defined
(clamped elsewhere), `(img1 - img2) ** 2` in float32, torchvision.utils.make_grid(nrow, padding=2, pad_value=0), and the PSNR
-10 log10(mean) with the mean taken in float64.  Every float32 step is one IEEE operation, so the device bytes compare exactly."""
import math

import numpy as np

F = np.float32


def byte(x):
    """clamp(trunc(255 x), 0, 255) on float32 x with the product in float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = F(255.0) * np.asarray(x, dtype=F)
        t = np.where(np.isnan(t), F(0.0), t)
        return np.trunc(np.clip(t, F(0.0), F(255.0))).astype(np.uint8)


def normal_byte(n):
    with np.errstate(invalid="ignore", over="ignore"):
        return byte((np.asarray(n, dtype=F) + F(1.0)) / F(2.0))


def sq_err(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(a, dtype=F) - np.asarray(b, dtype=F)
        return d * d


def put(frames, p0, rgb=None, normal=None, depth=None, gt=None):
    """neat_frame_put on numpy buffers: frames = dict(rgb8 [P,3], normal8 [P,3], depth [P], err [P,3]), updated in place."""
    n = len(next(t for t in (rgb, normal, depth) if t is not None))
    if rgb is not None:
        if frames.get("rgb8") is not None:
            frames["rgb8"][p0:p0 + n] = byte(rgb)
        if gt is not None:
            frames["err"][p0:p0 + n] = sq_err(rgb, gt[p0:p0 + n])
    if normal is not None:
        frames["normal8"][p0:p0 + n] = normal_byte(normal)
    if depth is not None:
        frames["depth"][p0:p0 + n] = np.asarray(depth, dtype=F)


def exact_sum(x):
    """The correctly rounded float64 sum of float32 values."""
    return math.fsum(np.asarray(x, dtype=np.float64).reshape(-1).tolist())


def finite_range(x):
    x = np.asarray(x, dtype=F).reshape(-1)
    x = x[np.isfinite(x)]
    return (F(x.min()), F(x.max())) if len(x) else (F(0.0), F(0.0))


def grey(d, lo, hi):
    """clamp(trunc((255 (d - lo)) / (hi - lo)), 0, 255) in float32; 0 where d is not finite or hi == lo."""
    d, lo, hi = np.asarray(d, dtype=F), F(lo), F(hi)
    if hi == lo:
        return np.zeros(d.shape, dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (F(255.0) * (d - lo)) / F(hi - lo)
        t = np.where(np.isfinite(d) & ~np.isnan(t), t, F(0.0))
        return np.trunc(np.clip(t, F(0.0), F(255.0))).astype(np.uint8)


def make_grid(images, nrow, padding=2):
    """torchvision.utils.make_grid(nrow=, padding=2, pad_value=0) on byte images [N,H,W,3] -> [rows, columns, 3]; one image: unpadded."""
    images = np.asarray(images)
    N, H, W = images.shape[:3]
    if N == 1:
        return images[0].copy()
    xmaps = min(nrow, N)
    ymaps = int(math.ceil(N / xmaps))
    canvas = np.zeros((ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3), dtype=np.uint8)
    for k in range(N):
        y0, x0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        canvas[y0:y0 + H, x0:x0 + W] = images[k]
    return canvas


def psnr(img1, img2):
    """-10 log10 of the float64 mean of the float32 squares (rend_util.get_psnr with its mean in float64)."""
    e = sq_err(img1, img2).astype(np.float64)
    return -10.0 * math.log10(exact_sum(e) / e.size)


def byte_inputs(rng, n):
    """[n] float32 values that sit on and around every decision of byte(): exact steps k / 255 and their float32 neighbours on both
    sides, 0, 1, -1e-3, 1.5, the infinities and NaN, then uniform filler."""
    k = np.arange(256, dtype=np.float64)
    steps = (k / 255.0).astype(F)
    special = np.array([0.0, 1.0, -1e-3, 1.5, np.inf, -np.inf, np.nan, -0.0, 0.999999, 256.0 / 255.0], dtype=F)
    pool = np.concatenate([steps, np.nextafter(steps, F(2.0)), np.nextafter(steps, F(-1.0)), special])
    out = rng.uniform(-0.1, 1.1, n).astype(F)
    m = min(n, len(pool))
    out[rng.permutation(n)[:m]] = rng.permutation(pool)[:m]
    return out
