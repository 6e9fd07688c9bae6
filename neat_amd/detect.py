"""2-D line segments of the views, detected on the device: the files `<scene>/<line_detector>/<image>.json` that BlenderDataset and
SceneDataset read, which the reference gets from HAWP or from `sslib.predict-lsd` (code/scripts/lsd-dtu.sh).

    python -m neat_amd.detect --scan <instance dir> [--name lsd] [--scale 1.0] [--views a:b] [--device cuda:0]

finds `images/` or `image/` under the instance directory, detects in every view and writes `<instance dir>/<name>/<stem>.json`; a conf
then says `dataset.line_detector = lsd`.  One summary line: views, segments, seconds.

    lines, width, nfa, n, k, offsets = detect.lines(images, scale=1.0)      # images: uint8 device tensor [V,H,W,3] or [V,H,W]
    detect.labels(codes)                                                     # uint8 [V,h,w], 255 = unused -> int32 labels, -1 = unused
    detect.to_wireframe(lines, nfa, H, W)                                    # -> WireframeGraph

The detector is an a-contrario one of the LSD family (Grompone von Gioi et al.) over the line-support regions of Burns, Hanson and
Riseman: connected components of the quantised gradient orientation in two overlapping partitions, validated by LSD's rectangle and
number of false alarms.  The rule is DESIGN 3j; csrc/kernels_detect.hpp implements it and tests/detect_f64.py restates it.  There is
no CPU path: CPU tensors are refused.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

from . import _lib, run_io
from .wireframe import WireframeGraph

DEFAULT_SCALE = 1.0          # NOTEBOOK: on the fixture views 0.8 meets no more of the stored segments than 1.0 does


def constants(Hs, Ws, q=2.0, tau_deg=22.5):
    """The constants the host hands to the kernels for grey pictures of Hs x Ws pixels."""
    tau = tau_deg * math.pi / 180.0
    p = tau_deg / 180.0
    logNT = 2.5 * (math.log10(Ws) + math.log10(Hs))
    return {"rho2": (q / math.sin(tau)) ** 2, "c1": math.sqrt(2.0) - 1.0, "cos_tau": math.cos(tau), "p": p, "logNT": logNT,
            "min_reg": int(math.floor(-logNT / math.log10(p))) + 1}


def gaussian_taps(out, scale):
    """The sampled Gaussian of sigma = 0.6 / scale, 2 ceil(3 sigma) + 1 taps for each of `out` output positions, centred on
    i / scale and normalised by their sum taken in tap order -> float64 [out, taps]."""
    sigma = 0.6 / scale
    h = int(math.ceil(3.0 * sigma))
    xc = np.arange(out, dtype=np.float64) / scale
    j = (np.floor(xc + 0.5).astype(np.int64) - h)[:, None] + np.arange(2 * h + 1)[None, :]
    d = (j.astype(np.float64) - xc[:, None]) / sigma
    wgt = np.exp(-0.5 * (d * d))
    return wgt / np.cumsum(wgt, axis=1)[:, -1:]


def _check_images(images):
    if not torch.is_tensor(images) or not images.is_cuda:
        raise RuntimeError("neat_amd.detect needs CUDA tensors (there is no CPU path)")
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
        raise RuntimeError(f"detect: images uint8 [V,H,W,3] or [V,H,W], got {images.dtype} {tuple(images.shape)}")
    return images.contiguous()


def lines(images, scale=DEFAULT_SCALE, q=2.0, tau_deg=22.5, density=0.7, grey=False):
    """images uint8 [V,H,W,3] or [V,H,W] on the device -> (lines float64 [N,4] = x1 y1 x2 y2, width [N], nfa [N] = -log10 NFA, n [N],
    k [N] int32, offsets int32 [V+1]) in (view, partition, label) order; the lines of view v are rows offsets[v]:offsets[v+1].  One
    synchronisation, at the end, to slice the outputs.  grey=True appends the float64 grey pictures [V,Hs,Ws] the detector worked on."""
    images = _check_images(images)
    if not 0.0 < scale <= 1.0:
        raise ValueError(f"detect: scale {scale} is outside (0, 1]")
    V, H, W = (int(s) for s in images.shape[:3])
    if V > 0 and (H < 2 or W < 2):
        raise ValueError(f"detect: pictures of {H} x {W} have no gradient")
    ch = 3 if images.dim() == 4 else 1
    dev = images.device
    lib = _lib.lib()
    Hs, Ws = (int(math.ceil(scale * H)), int(math.ceil(scale * W))) if V > 0 else (0, 0)
    offsets = torch.empty(V + 1, device=dev, dtype=torch.int32)
    f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        if V == 0 or Hs < 2 or Ws < 2:
            c = constants(2, 2, q, tau_deg)
            _lib.check(lib.neat_detect_lines(None, V, H, W, ch, float(scale), None, None, 0, c["rho2"], c["c1"], c["cos_tau"], float(density),
                                             c["logNT"], c["p"], c["min_reg"], None, 0, None, None, None, None, None, _lib.ptr(offsets),
                                             _lib.stream()), "neat_detect_lines")
            out = (f64(0, 4), f64(0), f64(0), i32(0), i32(0), offsets)
            return out + (f64(V, Hs, Ws),) if grey else out
        c = constants(Hs, Ws, q, tau_deg)
        nbytes = lib.neat_detect_scratch_bytes(V, H, W, float(scale), c["min_reg"])
        if nbytes == 0:
            raise RuntimeError(f"detect: {V} views of {H} x {W} are beyond what one call indexes; pass fewer views")
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        cap = 2 * V * (((Hs - 1) * (Ws - 1)) // c["min_reg"]) + 1
        tx = ty = None
        ntaps = 0
        if scale < 1.0:
            tx = torch.from_numpy(gaussian_taps(Ws, scale)).to(dev)
            ty = torch.from_numpy(gaussian_taps(Hs, scale)).to(dev)
            ntaps = int(tx.shape[1])
        out_lines, width, nfa, n, k = f64(cap, 4), f64(cap), f64(cap), i32(cap), i32(cap)
        _lib.check(lib.neat_detect_lines(_lib.ptr(images), V, H, W, ch, float(scale), _lib.ptr(tx), _lib.ptr(ty), ntaps, c["rho2"], c["c1"],
                                         c["cos_tau"], float(density), c["logNT"], c["p"], c["min_reg"], _lib.ptr(ws), cap, _lib.ptr(out_lines),
                                         _lib.ptr(width), _lib.ptr(nfa), _lib.ptr(n), _lib.ptr(k), _lib.ptr(offsets), _lib.stream()),
                   "neat_detect_lines")
        N = int(offsets[-1].item())
        out = (out_lines[:N].clone(), width[:N].clone(), nfa[:N].clone(), n[:N].clone(), k[:N].clone(), offsets)
        if grey:
            out = out + (ws[:8 * V * Hs * Ws].view(torch.float64).reshape(V, Hs, Ws).clone(),)
        return out


def labels(codes):
    """codes uint8 [V,h,w] on the device (255 = unused) -> int32 [V,h,w]: the smallest linear index y w + x of the pixel's 8-connected
    component of equal code, -1 for unused.  The detector's labelling step on its own."""
    if not torch.is_tensor(codes) or not codes.is_cuda:
        raise RuntimeError("neat_amd.detect needs CUDA tensors (there is no CPU path)")
    if codes.dtype != torch.uint8 or codes.dim() != 3:
        raise RuntimeError(f"detect.labels: codes uint8 [V,h,w], got {codes.dtype} {tuple(codes.shape)}")
    codes = codes.contiguous()
    V, h, w = (int(s) for s in codes.shape)
    out = torch.empty(V, h, w, device=codes.device, dtype=torch.int32)
    with torch.cuda.device(codes.device):
        _lib.check(_lib.lib().neat_detect_label(_lib.ptr(codes), V, h, w, _lib.ptr(out), _lib.stream()), "neat_detect_label")
    return out


def to_wireframe(lines, nfa, H, W):
    """The lines [N,4] of one view and their -log10 NFA -> a WireframeGraph of 2 N vertices and N edges.  The edge weight (and the score of
    its two vertices) is 1 - 10^(-nfa), so the datasets' `> 0.05` threshold keeps what the NFA test kept (all but NFA values above 0.95)."""
    lines = torch.as_tensor(lines).detach().cpu().to(torch.float64).reshape(-1, 4)
    nfa = torch.as_tensor(nfa).detach().cpu().to(torch.float64).reshape(-1)
    N = lines.shape[0]
    weight = (1.0 - torch.pow(10.0, -nfa)).float()
    edges = torch.arange(2 * N, dtype=torch.long).reshape(N, 2)
    return WireframeGraph(lines.reshape(2 * N, 2).float(), weight.repeat_interleave(2), edges, weight, frame_width=int(W), frame_height=int(H))


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.detect", description="detect the 2-D line segments of a scene's views on the device")
    ap.add_argument("--scan", type=str, required=True, help="the instance directory: images/ or image/ inside it, the output beside them")
    ap.add_argument("--name", type=str, default="lsd", help="output folder = the dataset's line_detector")
    ap.add_argument("--scale", type=float, default=DEFAULT_SCALE, help="Gaussian down-scaling before the gradient, in (0, 1]")
    ap.add_argument("--views", type=str, default=None, help="a:b, a slice of the sorted views")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--batch", type=int, default=16, help="views of equal size per call")
    return ap


parse_views = run_io.parse_views              # 'a:b'; its home is neat_amd.run_io


def load_image(path):
    """uint8 [H,W,3] through PIL."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    device = torch.device(opt.device)
    if device.type != "cuda":
        print(f"neat_amd.detect runs on the device only: --device {opt.device} is refused", file=sys.stderr, flush=True)
        return 2
    if not 0.0 < opt.scale <= 1.0 or opt.batch < 1:
        print(f"--scale {opt.scale} must lie in (0, 1] and --batch {opt.batch} be positive", file=sys.stderr, flush=True)
        return 2
    paths = run_io.scene_images(opt.scan)
    try:
        paths = [paths[i] for i in parse_views(opt.views, len(paths))]
    except ValueError as err:
        print(err, file=sys.stderr, flush=True)
        return 2
    t0 = time.perf_counter()
    total = 0
    group = []                                   # consecutive views of equal size go into one call

    def flush():
        nonlocal total
        if not group:
            return
        batch = torch.from_numpy(np.stack([img for _, img in group])).to(device)
        seg, _, nfa, _, _, off = lines(batch, scale=opt.scale)
        seg, nfa, off = seg.cpu(), nfa.cpu(), off.cpu().tolist()
        for j, (path, img) in enumerate(group):
            a, b = off[j], off[j + 1]
            wf = to_wireframe(seg[a:b], nfa[a:b], img.shape[0], img.shape[1])
            stem = os.path.splitext(os.path.basename(path))[0]
            run_io.write_wireframe_json(os.path.join(opt.scan, opt.name, stem + ".json"), wf, {"edges-nfa": nfa[a:b].tolist()})
            total += b - a
        group.clear()

    for path in paths:
        img = load_image(path)
        if group and (group[0][1].shape != img.shape or len(group) >= opt.batch):
            flush()
        group.append((path, img))
    flush()
    torch.cuda.synchronize(device)
    print(f"{len(paths)} views, {total} segments, {time.perf_counter() - t0:.3f} s -> {os.path.join(opt.scan, opt.name)}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
