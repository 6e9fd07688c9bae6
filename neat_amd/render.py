"""What the network renders, as pictures: every view of the dataset (or any camera) of a checkpoint -> rgb, normal and depth frames and the
PSNR per view (the reference's code/evaluation/eval.py --eval_rendering, which writes rendering_{epoch}/eval_%03d.png and
psnr_{epoch}.csv, and the pictures of the trainer's do_vis branch, code/training/volsdf_train.py:300-332 with utils/plots.py:362-396):

    python -m neat_amd.render --conf <run>/runconf.conf [--checkpoint latest] [--views all|0,5,10] [--chunksize N]
        [--maps rgb,normal,depth] [--surface] [--depth-range LO HI] [--save-depth] [--cam-json cam.json --width W --height H --fov 60]
        [--expdir <run>] [--data_root ../data] [--scan_id -1] [--gpu 0] [--precision P] [--json] [--overwrite]

A view is walked in chunks of `chunksize` pixels: VolSDFNetwork.render_pixels (camera rays, sampler, main pass: the eval forward without
its junction and line block) and ONE neat_frame_put launch, which writes the chunk's bytes, depths and squared errors into the frame; no
host synchronisation inside the walk.  After it: the float64 error sum (one read-back), the finite depth range (stays on the device) and
the grey depth picture.  Every P-sized step is a HIP kernel of neat_amd/csrc/kernels_frame.hpp behind neat_frame_* (include/neat_hip.h);
the byte rules are DESIGN 3e, restated in numpy by tests/render_f64.py.  The host reads files and encodes PNG (PIL).  No host fallback.

Files: <run>/rendering_{epoch}/eval_{idx:03d}.png (the reference's name), normal_{idx:03d}.png, depth_{idx:03d}.png, depth_{idx:03d}.npy
under --save-depth, and <run>/psnr_{epoch}.csv; epoch is read from the checkpoint.  Existing files are kept unless --overwrite.
--surface (or `surface` among --maps) adds surface_depth_{idx:03d}.png and surface_normal_{idx:03d}.png (surface_depth_{idx:03d}.npy under
--save-depth): depth and unit normal of the first hit of each pixel's ray with the raw SDF's zero level (neat_amd.trace.view),
NaN / zero where the ray hits nothing; --maps surface alone runs no volumetric forward.
--cam-json takes the list of 4 x 4 world-to-camera matrices that neat_amd.show writes as cam.json, with --width --height --fov
(show.intrinsics); pose = inverse(w2c); no PSNR on this route.

Divergences: bytes are clamped where numpy's cast wraps or is undefined; the PSNR is the float64 mean of the float32
squares (the reference: a float32 mean in an unspecified order); output goes under the run directory, not ../evals/.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

from . import _lib, ops, run_io
from ._lib import ptr as _p, stream as _stream

MAPS = ("rgb", "normal", "depth")
SURFACE = "surface"            # --maps surface / --surface: the sphere-traced first hit (neat_amd.trace.view), not a map of the volumetric forward
DEFAULT_CHUNK = 10000          # eval.py:80


# ------------------------------------------------------------------ device
def _f32(t, what):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("neat_amd.render: %s must be on the device" % what)
    return t.detach().to(torch.float32).contiguous()


pixel_grid, write_png = ops.pixel_grid, run_io.write_png              # their homes are neat_amd.ops and neat_amd.run_io


def frame_put(rgb, normal, depth, gt, p0, P, rgb8=None, normal8=None, depth_out=None, err=None):
    """One chunk into the frame buffers (neat_frame_put): rgb [n,3], normal [n,3], depth [n] float32 (any may be None), gt [P,3] or None."""
    n = next(int(t.shape[0]) for t in (rgb, normal, depth) if t is not None)
    _lib.check(_lib.lib().neat_frame_put(_p(rgb), _p(normal), _p(depth), _p(gt), n, int(p0), int(P), _p(rgb8), _p(normal8), _p(depth_out),
                                         _p(err), _stream()), "neat_frame_put")


def frame_sum(x, out=None):
    """The float64 sum of a float32 device tensor over the fixed tree of neat_frame_sum -> a float64 device tensor [1] (no read-back)."""
    x = _f32(x, "the summand").reshape(-1)
    lib = _lib.lib()
    ws = torch.empty(int(lib.neat_frame_sum_ws_bytes(x.numel())) // 8, device=x.device, dtype=torch.float64)
    out = torch.empty(1, device=x.device, dtype=torch.float64) if out is None else out
    _lib.check(lib.neat_frame_sum(_p(x), x.numel(), _p(ws), _p(out), _stream()), "neat_frame_sum")
    return out


def frame_range(x):
    """(min, max) of the finite values of a float32 device tensor, (0, 0) if there is none -> float32 device tensor [2] (no read-back)."""
    x = _f32(x, "the plane").reshape(-1)
    lib = _lib.lib()
    ws = torch.empty(int(lib.neat_frame_range_ws_bytes()) // 4, device=x.device, dtype=torch.float32)
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(lib.neat_frame_range(_p(x), x.numel(), _p(ws), _p(out), _stream()), "neat_frame_range")
    return out


def frame_grey(x, rng):
    """A float32 plane -> bytes of the same shape over the device range rng = (lo, hi) (neat_frame_grey)."""
    xc = _f32(x, "the plane")
    rng = _f32(rng, "the range").reshape(2)
    out = torch.empty(xc.shape, device=xc.device, dtype=torch.uint8)
    _lib.check(_lib.lib().neat_frame_grey(_p(xc), xc.numel(), _p(rng), _p(out), _stream()), "neat_frame_grey")
    return out


def grid_shape(N, H, W, nrow):
    """The canvas of torchvision.utils.make_grid(nrow=, padding=2) for N images of H x W -> (rows, columns); one image is unpadded."""
    if N == 1:
        return H, W
    xmaps = min(int(nrow), N)
    ymaps = -(-N // xmaps)
    return ymaps * (H + 2) + 2, xmaps * (W + 2) + 2


def grid(images, nrow):
    """Byte images [N,H,W,3] (a device tensor or a list of [H,W,3]) -> the make_grid(nrow, padding=2, pad_value=0) canvas, uint8 on the device."""
    if not torch.is_tensor(images):
        images = torch.stack(list(images))
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise RuntimeError("render.grid: uint8 images [N,H,W,3] on the device")
    images = images.contiguous()
    N, H, W = (int(v) for v in images.shape[:3])
    if N < 1 or int(nrow) < 1:
        raise ValueError("render.grid: at least one image and nrow >= 1")
    ch, cw = grid_shape(N, H, W, nrow)
    canvas = torch.empty(ch, cw, 3, device=images.device, dtype=torch.uint8)
    with torch.cuda.device(images.device):
        _lib.check(_lib.lib().neat_frame_grid(_p(images), N, H, W, int(nrow), _p(canvas), _stream()), "neat_frame_grid")
    return canvas


def psnr_of(sq_sum, count):
    """-10 log10(sum / count) in float64 (rend_util.get_psnr on the mean of the squares)."""
    mse = float(sq_sum) / count
    return float("inf") if mse == 0.0 else -10.0 * math.log10(mse)


@torch.no_grad()
def view(model, uv, pose, intrinsics, H, W, gt=None, chunksize=DEFAULT_CHUNK, maps=MAPS, depth_range=None, timings=None):
    """One view of H x W pixels: uv [P,2] or [1,P,2] (pixel_grid order), pose [4,4] or [1,4,4] camera-to-world, intrinsics [4,4] or
    [3,3] (a leading 1 allowed), gt [P,3] in [0,1] or None, all on the device -> dict of device tensors: "rgb" uint8 [H,W,3], "normal" uint8 [H,W,3], "depth"
    float32 [H,W], "depth8" uint8 [H,W] (those that `maps` names), "range" float32 [2] the depth picture's (lo, hi), and with gt "psnr" a Python
    float (None without gt) and "sq_sum", the float64 sum of the squared errors it is the logarithm of.  depth_range = (lo, hi) fixes the grey scale; default the finite range of the depth plane.
    timings = a dict receives render_s / frame_s: the walk's wall time (device-synchronised) and the frame kernels' share (HIP events)."""
    unknown = set(maps) - set(MAPS)
    if unknown:
        raise ValueError("render.view: unknown map %s" % ", ".join(sorted(unknown)))
    if model.training:
        raise RuntimeError("render.view: the model must be in eval() mode")
    P = int(H) * int(W)
    chunksize = int(chunksize)
    if chunksize < 1:
        raise ValueError("render.view: chunksize >= 1")
    uv = _f32(uv, "uv").reshape(1, -1, 2)
    if uv.shape[1] != P:
        raise ValueError("render.view: uv has %d pixels, H x W = %d" % (uv.shape[1], P))
    dev = uv.device
    pose, intrinsics = _f32(pose, "pose").reshape(1, 4, 4), _f32(intrinsics, "intrinsics")
    intrinsics = intrinsics.reshape(1, *intrinsics.shape[-2:])
    gt = _f32(gt, "gt")
    if gt is not None and gt.numel() != 3 * P:
        raise ValueError("render.view: gt must be [P,3]")
    want = {m: m in maps for m in MAPS}
    lib = _lib.lib()
    with torch.cuda.device(dev):
        rgb8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8) if want["rgb"] else None
        normal8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8) if want["normal"] else None
        depth = torch.empty(H, W, device=dev, dtype=torch.float32) if want["depth"] else None
        err = torch.empty(P, 3, device=dev, dtype=torch.float32) if gt is not None else None
        events = []
        if timings is not None:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()

        def frame_side(call):
            if timings is None:
                return call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = call()
            e1.record()
            events.append((e0, e1))
            return res
        s = _stream()
        for p0 in range(0, P, chunksize):
            n = min(chunksize, P - p0)
            rgb, nmap, dep = model.render_pixels(uv[:, p0:p0 + n], pose, intrinsics)
            rgb = _f32(rgb, "rgb") if (want["rgb"] or gt is not None) else None
            nmap = _f32(nmap, "normal_map") if want["normal"] else None
            dep = _f32(dep, "depth") if want["depth"] else None
            frame_side(lambda: _lib.check(lib.neat_frame_put(_p(rgb), _p(nmap), _p(dep), _p(gt), n, p0, P, _p(rgb8), _p(normal8), _p(depth),
                                                             _p(err), s), "neat_frame_put"))
        out = {"psnr": None}
        total = frame_side(lambda: frame_sum(err)) if gt is not None else None
        if want["depth"]:
            if depth_range is not None:
                lo, hi = float(depth_range[0]), float(depth_range[1])
                if not (math.isfinite(lo) and math.isfinite(hi)):
                    raise ValueError("render.view: depth_range must be finite")
                rng = torch.tensor([lo, hi], dtype=torch.float32).to(dev)
            else:
                rng = frame_side(lambda: frame_range(depth))
            out["depth"], out["range"] = depth, rng
            out["depth8"] = frame_side(lambda: frame_grey(depth, rng))
        if want["rgb"]:
            out["rgb"] = rgb8
        if want["normal"]:
            out["normal"] = normal8
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["render_s"] = time.perf_counter() - t0
            timings["frame_s"] = sum(e0.elapsed_time(e1) for e0, e1 in events) * 1e-3
        if total is not None:
            out["sq_sum"] = total.item()                       # the one read-back
            out["psnr"] = psnr_of(out["sq_sum"], 3 * P)
    return out


def dataset_view(dataset, idx, device):
    """View idx of a neat_amd dataset, whole, without touching the dataset's sampling state or any random stream
    -> (uv [1,P,2], pose [1,4,4], intrinsics [1,4,4] or [1,3,3] as the dataset holds them, gt [P,3], H, W) on the device."""
    H, W = (int(v) for v in dataset.img_res)
    return (pixel_grid(H, W, device)[None], dataset.pose_all[idx].to(device)[None], dataset.intrinsics_all[idx].to(device)[None],
            dataset.rgb_images[idx].to(device), H, W)


def camera_view(w2c, width, height, fov, device):
    """A world-to-camera matrix [4,4] with show.intrinsics(width, height, fov) -> (uv, pose = inverse(w2c), intrinsics [1,4,4]) on the device."""
    K = np.eye(4)
    K[:3, :3] = run_io.fov_intrinsics(width, height, fov)
    pose = np.linalg.inv(np.asarray(w2c, dtype=np.float64).reshape(4, 4))
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)[None]
    return pixel_grid(height, width, device)[None], as_dev(pose), as_dev(K)


# ------------------------------------------------------------------ files
def psnr_rows(psnrs):
    """The per-view values, then their mean and their standard deviation (ddof 0), float64 (eval.py:129-131)."""
    p = np.asarray(psnrs, dtype=np.float64).reshape(-1)
    return np.concatenate([p, [p.mean()], [p.std()]])


def write_psnr_csv(path, psnrs):
    """The text pandas.DataFrame(psnr_rows(psnrs)).to_csv(path) writes: header `,0`, rows `i,repr(value)` (a NaN as an empty field)."""
    cell = lambda v: "" if math.isnan(v) else repr(float(v))
    with open(path, "w", newline="") as fh:
        fh.write(",0\n" + "".join("%d,%s\n" % (i, cell(v)) for i, v in enumerate(psnr_rows(psnrs))))


def out_dir(run_dir, epoch):
    return os.path.join(run_dir, "rendering_{}".format(epoch))


def out_paths(run_dir, epoch, idx, maps=MAPS, save_depth=False):
    """-> {"rgb": .../rendering_{epoch}/eval_{idx:03d}.png (eval.py:121), "normal": normal_..., "depth": depth_..., "depth_npy": ....npy}."""
    d = out_dir(run_dir, epoch)
    names = {"rgb": "eval_%03d.png", "normal": "normal_%03d.png", "depth": "depth_%03d.png"}
    paths = {m: os.path.join(d, names[m] % idx) for m in MAPS if m in maps}
    if save_depth and "depth" in maps:
        paths["depth_npy"] = os.path.join(d, "depth_%03d.npy" % idx)
    return paths


def surface_paths(run_dir, epoch, idx, save_depth=False):
    """-> {"surface_depth": .../surface_depth_{idx:03d}.png, "surface_normal": ..., "surface_depth_npy": ... under save_depth}."""
    d = out_dir(run_dir, epoch)
    paths = {"surface_depth": os.path.join(d, "surface_depth_%03d.png" % idx), "surface_normal": os.path.join(d, "surface_normal_%03d.png" % idx)}
    if save_depth:
        paths["surface_depth_npy"] = os.path.join(d, "surface_depth_%03d.npy" % idx)
    return paths


def surface_view(model, pose, intrinsics, H, W, depth_range=None, timings=None):
    """The first hit of every pixel's ray (trace.view) as frames -> dict: "depth" float32 [H,W] (NaN off the surface), "depth8" uint8 [H,W]
    (grey over depth_range, default the finite range of the plane: depth_*.png's rule), "normal" uint8 [H,W,3] (byte((n + 1) / 2), a zero
    normal off the surface), "state" uint8 [H,W]."""
    from . import trace
    depth, normal, state = trace.view(model, pose, intrinsics, H, W, timings=timings)
    dev = depth.device
    with torch.cuda.device(dev):
        rng = torch.tensor([float(depth_range[0]), float(depth_range[1])], dtype=torch.float32).to(dev) if depth_range is not None else frame_range(depth)
        normal8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
        frame_put(None, normal.reshape(-1, 3), None, None, 0, H * W, normal8=normal8)
        return {"depth": depth, "depth8": frame_grey(depth, rng), "normal": normal8, "state": state}


def csv_path(run_dir, epoch):
    return os.path.join(run_dir, "psnr_{}.csv".format(epoch))


def plot_paths(run_dir, epoch):
    """The trainer's pictures: <run>/plots/rendering_{epoch}.png and normal_{epoch}.png (plots.py:374, :394)."""
    return (os.path.join(run_dir, "plots", "rendering_{}.png".format(epoch)), os.path.join(run_dir, "plots", "normal_{}.png".format(epoch)))


def plot_view(model, dataset, idx, run_dir, epoch, nrow=1, chunksize=DEFAULT_CHUNK):
    """The do_vis pictures of view idx: the rendered frame and the ground truth through grid(nrow) (nrow = 1: output above ground truth),
    and the normal frame on its own (a single image: unpadded).  The model must be in eval mode.  -> the two paths."""
    dev = next(model.parameters()).device
    uv, pose, K, gt, H, W = dataset_view(dataset, idx, dev)
    res = view(model, uv, pose, K, H, W, chunksize=chunksize, maps=("rgb", "normal"))
    gt8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    frame_put(_f32(gt, "gt").reshape(-1, 3), None, None, None, 0, H * W, rgb8=gt8)
    rendering, normal = plot_paths(run_dir, epoch)
    write_png(rendering, grid(torch.stack([res["rgb"], gt8]), nrow))
    write_png(normal, grid(res["normal"][None], nrow))
    return rendering, normal


# ------------------------------------------------------------------ command line
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("--conf", type=str, required=True)
    ap.add_argument("--checkpoint", default="latest", type=str, help="the trained model checkpoint to render")
    ap.add_argument("--views", default="all", type=str, help="`all` or comma-separated view indices of the dataset")
    ap.add_argument("--chunksize", default=None, type=int, help="pixels per chunk (default: the conf's train.split_n_pixels, else 10000)")
    ap.add_argument("--maps", default=",".join(MAPS), type=str, help="comma-separated subset of rgb,normal,depth (and surface: see --surface)")
    ap.add_argument("--surface", default=False, action="store_true", help="also write the sphere-traced surface depth and normal frames")
    ap.add_argument("--depth-range", default=None, type=float, nargs=2, metavar=("LO", "HI"), help="grey scale of the depth picture (default: its finite range)")
    ap.add_argument("--save-depth", default=False, action="store_true", help="write the float32 depth plane as depth_{idx:03d}.npy too")
    ap.add_argument("--cam-json", default=None, type=str, help="a JSON list of 4x4 world-to-camera matrices (neat_amd.show's cam.json), one frame each")
    ap.add_argument("--width", default=None, type=int)
    ap.add_argument("--height", default=None, type=int)
    ap.add_argument("--fov", default=60.0, type=float, help="vertical field of view, degrees")
    ap.add_argument("--expdir", default=None, help="run directory holding checkpoints/ (default: the conf's directory)")
    ap.add_argument("--data_root", default="../data", help="root of the dataset's data_dir")
    ap.add_argument("--scan_id", default=-1, type=int)
    ap.add_argument("--gpu", default=0, type=int, help="device index")
    ap.add_argument("--precision", choices=list(_lib.PRECISIONS), default=None)
    ap.add_argument("--json", default=False, action="store_true", help="print one JSON object with the PSNRs and the timings")
    ap.add_argument("--overwrite", default=False, action="store_true", help="rewrite files that are already on disk")
    return ap


def parse_args(argv=None):
    """The parsed options with `maps` a tuple and `views` None (all) or a list; bad combinations exit."""
    ap = build_parser()
    opt = ap.parse_args(argv)
    opt.maps = tuple(m for m in opt.maps.split(",") if m)
    if not opt.maps or set(opt.maps) - set(MAPS) - {SURFACE}:
        ap.error("--maps: a comma-separated subset of " + ",".join(MAPS + (SURFACE,)))
    opt.surface = opt.surface or SURFACE in opt.maps
    opt.maps = tuple(m for m in opt.maps if m != SURFACE)
    if opt.cam_json is not None and (opt.width is None or opt.height is None):
        ap.error("--cam-json needs --width and --height")
    if opt.chunksize is not None and opt.chunksize < 1:
        ap.error("--chunksize must be positive")
    if opt.views != "all":
        try:
            opt.views = [int(v) for v in opt.views.split(",")]
        except ValueError:
            ap.error("--views: `all` or comma-separated integers")
    else:
        opt.views = None
    return opt


def main(argv=None):
    opt = parse_args(argv)
    _lib.lib()                      # a missing library is an error before any file is read
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    model, epoch, root, conf = run_io.load_model(opt.conf, opt.checkpoint, device, opt.expdir, opt.precision)
    chunksize = opt.chunksize if opt.chunksize is not None else conf.get_int("train.split_n_pixels", default=DEFAULT_CHUNK)
    if opt.cam_json is not None:
        cams = run_io.load_cam_json(opt.cam_json)
        dataset, views = None, list(range(len(cams)))
    else:
        dataset = run_io.build_dataset(conf, opt.data_root, opt.scan_id)
        views = list(range(len(dataset))) if opt.views is None else opt.views
        bad = [v for v in views if not 0 <= v < len(dataset)]
        if bad:
            raise SystemExit("--views: %s out of range (the dataset has %d views)" % (bad, len(dataset)))
    scan_id = opt.scan_id if opt.scan_id != -1 else conf.get_int("dataset.scan_id", default=-1)
    targets = [out_paths(root, epoch, idx, opt.maps, opt.save_depth) for idx in views]
    surf = [surface_paths(root, epoch, idx, opt.save_depth) if opt.surface else {} for idx in views]
    with_csv = dataset is not None and bool(opt.maps)             # --maps surface alone: no forward, hence no PSNR
    every = [p for t in targets + surf for p in t.values()] + ([csv_path(root, epoch)] if with_csv else [])
    if not opt.overwrite and all(os.path.exists(p) for p in every):
        print("exists: all {} files under {} (--overwrite to replace them)".format(len(every), out_dir(root, epoch)), flush=True)
        if opt.json:
            print(json.dumps({"epoch": int(epoch), "views": views, "written": 0, "dir": out_dir(root, epoch)}))
        return 0
    os.makedirs(out_dir(root, epoch), exist_ok=True)
    psnrs, render_s, encode_s, written = [], 0.0, 0.0, 0
    trace_s, trace_evals = 0.0, 0
    for idx, paths, spaths in zip(views, targets, surf):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        if dataset is not None:
            uv, pose, K, gt, H, W = dataset_view(dataset, idx, device)
        else:
            (uv, pose, K), gt, H, W = camera_view(cams[idx], opt.width, opt.height, opt.fov, device), None, opt.height, opt.width
        res = view(model, uv, pose, K, H, W, gt=gt, chunksize=chunksize, maps=opt.maps, depth_range=opt.depth_range) if opt.maps else {"psnr": None}
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        for m, key in (("rgb", "rgb"), ("normal", "normal"), ("depth", "depth8")):
            if m in paths:
                written += write_png(paths[m], res[key], opt.overwrite)
        if "depth_npy" in paths and (opt.overwrite or not os.path.exists(paths["depth_npy"])):
            np.save(paths["depth_npy"], res["depth"].cpu().numpy())
            written += 1
        render_s, encode_s = render_s + (t1 - t0), encode_s + (time.perf_counter() - t1)
        if opt.surface:
            tm = {}
            sres = surface_view(model, pose, K, H, W, depth_range=opt.depth_range, timings=tm)
            trace_s, trace_evals = trace_s + tm["trace_s"], trace_evals + tm["evals"]
            t2 = time.perf_counter()
            written += write_png(spaths["surface_depth"], sres["depth8"], opt.overwrite) + write_png(spaths["surface_normal"], sres["normal"], opt.overwrite)
            if "surface_depth_npy" in spaths and (opt.overwrite or not os.path.exists(spaths["surface_depth_npy"])):
                np.save(spaths["surface_depth_npy"], sres["depth"].cpu().numpy())
                written += 1
            encode_s += time.perf_counter() - t2
        if res["psnr"] is not None:
            psnrs.append(res["psnr"])
    report = {"epoch": int(epoch), "views": views, "chunksize": int(chunksize), "render_s": render_s, "encode_s": encode_s, "written": written,
              "dir": out_dir(root, epoch)}
    if psnrs:
        rows = psnr_rows(psnrs)
        if opt.overwrite or not os.path.exists(csv_path(root, epoch)):
            write_psnr_csv(csv_path(root, epoch), psnrs)
        print("RENDERING EVALUATION {}: psnr mean = {} ; psnr std = {}".format(scan_id, "%.2f" % rows[-2], "%.2f" % rows[-1]), flush=True)
        report.update(psnr=[float(v) for v in psnrs], mean=float(rows[-2]), std=float(rows[-1]))
    print("{} views of the checkpoint of epoch {} -> {}: rendering {:.3f} s, encoding {:.3f} s".format(len(views), epoch, out_dir(root, epoch),
                                                                                                      render_s, encode_s), flush=True)
    if opt.surface:
        report.update(trace_s=trace_s, trace_evals=int(trace_evals))
        print("surface frames: tracing {:.3f} s, {} SDF evaluations".format(trace_s, trace_evals), flush=True)
    if opt.json:
        print(json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
