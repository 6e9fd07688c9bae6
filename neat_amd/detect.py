"""2-D line segments of the views, detected on the device: the files `<scene>/<line_detector>/<image>.json` that BlenderDataset and
SceneDataset read, which the reference gets from HAWP or from `sslib.predict-lsd` (code/scripts/lsd-dtu.sh).

    python -m neat_amd.detect --scan <instance dir> [--name lsd] [--scale 1.0] [--views a:b] [--device cuda:0]

finds `images/` or `image/` under the instance directory, detects in every view and writes `<instance dir>/<name>/<stem>.json`; a conf
then says `dataset.line_detector = lsd`.  One summary line: views, segments, seconds.

    lines, width, nfa, n, k, offsets = detect.lines(images, scale=1.0)      # images: uint8 device tensor [V,H,W,3] or [V,H,W]
    detect.labels(codes)                                                     # uint8 [V,h,w], 255 = unused -> int32 labels, -1 = unused
    detect.to_wireframe(lines, nfa, H, W)                                    # -> WireframeGraph, two vertices of its own a segment

With `--junctions [--gap 4] [--gap-frac 0.4] [--angle 10] [--no-t]` the segments' ends are joined into shared junctions (DESIGN 3o,
csrc/kernels_wireframe2d.hpp, restated by tests/junctions2d_f64.py); `--from NAME` then reads the segments of `<scan>/<NAME>/*.json`
instead of detecting.  The summary line adds the vertices and edges built.

    res = detect.junctions(lines, weight, offsets, gap=4.0, frac=0.4, angle=10.0, t_junctions=True)      # dict of device tensors
    wfs = detect.wireframes(lines, nfa, offsets, H, W)                                                   # one WireframeGraph per view

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
    N = lines.shape[0]
    weight = nfa_weight(nfa)
    edges = torch.arange(2 * N, dtype=torch.long).reshape(N, 2)
    return WireframeGraph(lines.reshape(2 * N, 2).float(), weight.repeat_interleave(2), edges, weight, frame_width=int(W), frame_height=int(H))


def nfa_weight(nfa):
    """-log10 NFA -> the edge weight 1 - 10^(-nfa) as the files hold it: float32, formed in float64 on the host."""
    nfa = torch.as_tensor(nfa).detach().cpu().to(torch.float64).reshape(-1)
    return (1.0 - torch.pow(10.0, -nfa)).float()


# ---- shared junctions ------------------------------------------------------------------------------------------------------------
JUNCTION_DEFAULTS = {"gap": 4.0, "frac": 0.4, "angle": 10.0, "t_junctions": True}
JUNCTION_KEYS = ("vertices", "degree", "kind", "score", "spread", "t_edge", "voff", "ends", "edges", "eweight", "esrc", "eoff")


def check_junction_options(gap, frac, angle):
    if not (gap > 0.0 and math.isfinite(gap) and 0.0 < frac < 0.5 and 0.0 < angle <= 90.0):
        raise ValueError(f"detect.junctions: gap {gap} must be positive, frac {frac} lie in (0, 0.5) and angle {angle} in (0, 90]")


def junctions(lines, weight, offsets, gap=JUNCTION_DEFAULTS["gap"], frac=JUNCTION_DEFAULTS["frac"], angle=JUNCTION_DEFAULTS["angle"],
              t_junctions=JUNCTION_DEFAULTS["t_junctions"]):
    """The segments of V views -> their wireframes with shared junctions, on the device (the rule: DESIGN 3o, tests/junctions2d_f64.py).

    lines [S,4] = x1 y1 x2 y2 and weight [S] on the device, in (view, index) order; offsets [V+1]: the views' first segments, as
    detect.lines returns them (a device tensor: the launches are then sized for S segments a view) or on the host (a sequence or a CPU
    tensor: sized for the largest view).  gap in pixels, frac of a segment's length, angle in degrees.

    -> dict of device tensors, the views one after the other and every index a view's own.  Per vertex: vertices float64 [N,2], degree
    int32 [N], kind int32 [N] (0 a free end, 1 a junction, 2 a T), score float64 [N], spread float64 [N], t_edge int32 [N]; voff int32
    [V+1].  ends int32 [S,2]: the vertex of each end.  Per edge: edges int32 [E,2], eweight float64 [E], esrc int32 [E] (its segment);
    eoff int32 [V+1].  One synchronisation, at the end, to slice the outputs."""
    if not (torch.is_tensor(lines) and lines.is_cuda and torch.is_tensor(weight) and weight.is_cuda):
        raise RuntimeError("neat_amd.detect needs CUDA tensors (there is no CPU path)")
    if lines.dim() != 2 or lines.shape[1] != 4 or weight.numel() != lines.shape[0]:
        raise RuntimeError(f"detect.junctions: lines [S,4] and weight [S], got {tuple(lines.shape)} and {tuple(weight.shape)}")
    gap, frac, angle = float(gap), float(frac), float(angle)
    check_junction_options(gap, frac, angle)
    dev = lines.device
    S = int(lines.shape[0])
    with torch.cuda.device(dev):
        seg = lines.detach().to(torch.float64).contiguous()
        w = weight.detach().to(torch.float64).reshape(-1).contiguous()
        if torch.is_tensor(offsets) and offsets.is_cuda:
            if offsets.dim() != 1 or offsets.numel() < 1:
                raise RuntimeError(f"detect.junctions: offsets [V+1], got {tuple(offsets.shape)}")
            segoff, nmax = offsets.to(device=dev, dtype=torch.int32).contiguous(), S
        else:
            host = np.asarray(offsets.numpy() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
            if host.size < 1 or host[0] != 0 or host[-1] != S or (np.diff(host) < 0).any():
                raise ValueError(f"detect.junctions: offsets must ascend from 0 to the {S} segments")
            segoff, nmax = torch.from_numpy(host.astype(np.int32)).to(dev), int(np.diff(host).max()) if host.size > 1 else 0
        V = int(segoff.numel()) - 1
        lib = _lib.lib()
        nbytes = lib.neat_wf2d_scratch_bytes(V, S, nmax) if S < 2 ** 31 else 0
        if nbytes == 0 and S > 0:
            raise RuntimeError(f"detect.junctions: {V} views of {S} segments are beyond what one call indexes; pass fewer views")
        f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        out = {"vertices": f64(2 * S, 2), "degree": i32(2 * S), "kind": i32(2 * S), "score": f64(2 * S), "spread": f64(2 * S), "t_edge": i32(2 * S),
               "voff": i32(V + 1), "ends": i32(S, 2), "edges": i32(S, 2), "eweight": f64(S), "esrc": i32(S), "eoff": i32(V + 1)}
        _lib.check(lib.neat_wf2d_build(_lib.ptr(seg), _lib.ptr(segoff), _lib.ptr(w), V, S, nmax, gap, frac, math.sin(angle * math.pi / 180.0),
                                       1 if t_junctions else 0, _lib.ptr(ws), *(_lib.ptr(out[k]) for k in JUNCTION_KEYS), _lib.stream()),
                   "neat_wf2d_build")
        N, E = torch.stack([out["voff"][-1], out["eoff"][-1]]).tolist()
        for k in ("vertices", "degree", "kind", "score", "spread", "t_edge"):
            out[k] = out[k][:N].clone()
        for k in ("edges", "eweight", "esrc"):
            out[k] = out[k][:E].clone()
    return out


def wireframes(lines, nfa, offsets, H, W, **kw):
    """The detector's output (lines [S,4], nfa [S], offsets [V+1], on the device) -> one WireframeGraph per view with shared junctions.
    The builder sees the segments and weights as a file of to_wireframe holds them (float32), so building from such a file gives the
    same graphs.  Each graph carries `degree` and `kind` of its vertices as extra attributes."""
    if not (torch.is_tensor(lines) and lines.is_cuda):
        raise RuntimeError("neat_amd.detect needs CUDA tensors (there is no CPU path)")
    weight = nfa_weight(nfa).to(lines.device)
    return graphs(junctions(lines.float(), weight, offsets, **kw), H, W)


def graphs(res, H, W):
    """detect.junctions' result -> one WireframeGraph per view (float32 on the host), with `degree` and `kind` [N] beside the vertices.
    H, W: one size for all views, or a sequence of them."""
    host = {k: v.cpu() for k, v in res.items()}
    voff, eoff = host["voff"].tolist(), host["eoff"].tolist()
    out = []
    for v in range(len(voff) - 1):
        a, b, c, d = voff[v], voff[v + 1], eoff[v], eoff[v + 1]
        h, w = (H[v], W[v]) if isinstance(H, (list, tuple)) else (H, W)
        wf = WireframeGraph(host["vertices"][a:b].float(), host["score"][a:b].float(), host["edges"][c:d].long(), host["eweight"][c:d].float(),
                            frame_width=int(w), frame_height=int(h))
        wf.degree, wf.kind = host["degree"][a:b].tolist(), host["kind"][a:b].tolist()
        out.append(wf)
    return out


def write_graphs(folder, stems, wfs):
    """The graphs of detect.wireframes / detect.graphs as <folder>/<stem>.json, `vertices-degree` and `vertices-kind` beside the usual keys."""
    for stem, wf in zip(stems, wfs):
        run_io.write_wireframe_json(os.path.join(folder, stem + ".json"), wf, {"vertices-degree": wf.degree, "vertices-kind": wf.kind})


def read_soup(path):
    """A <scene>/<line_detector>/<image>.json of any detector -> (segments float32 [n,4] = its edges' end points, weights float32 [n], H, W)."""
    wf = WireframeGraph.load_json(path)
    seg = torch.cat([wf.vertices[wf.edges[:, 0]], wf.vertices[wf.edges[:, 1]]], dim=1).reshape(-1, 4)
    return seg, wf.weights.reshape(-1), int(wf.frame_height), int(wf.frame_width)


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.detect", description="detect the 2-D line segments of a scene's views on the device")
    ap.add_argument("--scan", type=str, required=True, help="the instance directory: images/ or image/ inside it, the output beside them")
    ap.add_argument("--name", type=str, default="lsd", help="output folder = the dataset's line_detector")
    ap.add_argument("--scale", type=float, default=DEFAULT_SCALE, help="Gaussian down-scaling before the gradient, in (0, 1]")
    ap.add_argument("--views", type=str, default=None, help="a:b, a slice of the sorted views")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--batch", type=int, default=16, help="views of equal size per call")
    ap.add_argument("--junctions", action="store_true", help="join the segments' ends into shared junctions (DESIGN 3o) instead of two vertices a segment")
    ap.add_argument("--gap", type=float, default=JUNCTION_DEFAULTS["gap"], help="--junctions: how far from its end a segment may meet another, pixels")
    ap.add_argument("--gap-frac", dest="gap_frac", type=float, default=JUNCTION_DEFAULTS["frac"], help="--junctions: and as a share of its length, in (0, 0.5)")
    ap.add_argument("--angle", type=float, default=JUNCTION_DEFAULTS["angle"], help="--junctions: the least angle between two segments that meet, degrees")
    ap.add_argument("--no-t", dest="no_t", action="store_true", help="--junctions: leave an end that stops at another segment's inside where it is")
    ap.add_argument("--from", dest="source", type=str, default=None, metavar="NAME",
                    help="--junctions: read the segments of <scan>/<NAME>/*.json (any detector's) instead of detecting")
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
    kw = {"gap": opt.gap, "frac": opt.gap_frac, "angle": opt.angle, "t_junctions": not opt.no_t}
    try:
        if opt.source is not None and not opt.junctions:
            raise ValueError("--from reads a detector's files to join their segments: it needs --junctions")
        if opt.source is not None and os.path.normpath(opt.source) == os.path.normpath(opt.name):
            raise ValueError(f"--from {opt.source} and --name {opt.name} are one folder")
        check_junction_options(opt.gap, opt.gap_frac, opt.angle)
        if opt.source is not None:
            folder = os.path.join(opt.scan, opt.source)
            paths = sorted(os.path.join(folder, n) for n in os.listdir(folder) if n.endswith(".json"))
        else:
            paths = run_io.scene_images(opt.scan)
        paths = [paths[i] for i in parse_views(opt.views, len(paths))]
    except (ValueError, FileNotFoundError) as err:
        print(err, file=sys.stderr, flush=True)
        return 2
    t0 = time.perf_counter()
    total = built_v = built_e = 0
    stem_of = lambda path: os.path.splitext(os.path.basename(path))[0]

    def summary():
        built = f"{built_v} vertices, {built_e} edges, " if opt.junctions else ""
        print(f"{len(paths)} views, {total} segments, {built}{time.perf_counter() - t0:.3f} s -> {os.path.join(opt.scan, opt.name)}", flush=True)
        return 0

    def write_built(stems, wfs):
        nonlocal built_v, built_e
        write_graphs(os.path.join(opt.scan, opt.name), stems, wfs)
        built_v += sum(wf.vertices.shape[0] for wf in wfs)
        built_e += sum(wf.edges.shape[0] for wf in wfs)

    if opt.source is not None:                   # the segments of files: --batch views a call, of any sizes
        for b0 in range(0, len(paths), opt.batch):
            soups = [read_soup(p) for p in paths[b0:b0 + opt.batch]]
            off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in soups])])
            res = junctions(torch.cat([s[0] for s in soups]).to(device), torch.cat([s[1] for s in soups]).to(device), off, **kw)
            write_built([stem_of(p) for p in paths[b0:b0 + opt.batch]], graphs(res, [s[2] for s in soups], [s[3] for s in soups]))
            total += int(off[-1])
        torch.cuda.synchronize(device)
        return summary()
    group = []                                   # consecutive views of equal size go into one call

    def flush():
        nonlocal total
        if not group:
            return
        batch = torch.from_numpy(np.stack([img for _, img in group])).to(device)
        seg, _, nfa, _, _, off = lines(batch, scale=opt.scale)
        if opt.junctions:
            write_built([stem_of(path) for path, _ in group], wireframes(seg, nfa, off.cpu().tolist(), batch.shape[1], batch.shape[2], **kw))
            total += int(seg.shape[0])
            group.clear()
            return
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
    return summary()


if __name__ == "__main__":
    sys.exit(main())
