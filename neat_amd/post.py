"""Fuse, refine and snap a parsed 3-D line soup against the views' 2-D detections, on the device: the reference's
code/evaluation/fusion.py (:79-141), refinement.py (:95-198) and nms.py (:156-204).

    python -m neat_amd.post fuse   --conf <run>/runconf.conf --data X.npz [--dis 10] [--keep 0.5] [--score-by-label]
    python -m neat_amd.post refine --conf <run>/runconf.conf --data X.npz [--checkpoint latest] [--sdf-max 0.01] [--score-max 0.01] [--no-filter]
    python -m neat_amd.post snap   --data X.npz [--grid 512] [--max-snap D] [--unique]

Files (basename = the data file's name without .npz; run = the conf's directory, or --expdir):
    <run>/wireframes/{basename}-fused.npz   lines3d, score, count, keep
    <run>/wireframes/{basename}-ref.npz     lines3d
    {basename}-snap.npz                     junctions, edges, lines3d = junctions[edges], count   (beside the data file, or under
                                            <expdir>/wireframes with --expdir)
An existing output file is kept unless --overwrite is given.  `neat_amd.show` and `neat_amd.evaluate dtu-lines` read `lines3d`.

    views = views_of(dataset, device)                 # detections line_segments(0.05) packed with offsets, K3 / w2c per view, img_res
    fuse(lines, views) / refine(lines, views, model=None) / snap(lines, grid=512)

Every entry point walks the views without a host synchronisation (sizes that depend on the data stay on the device, buffers are sized by
their bounds) and synchronises once, at the end, to slice its outputs.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from . import conf as conf_mod, ops, run_io
from .parsing import _cameras, _dev


def pack_views(dets, Ks, poses, img_res, device):
    """Per-view detections [m_v, 5] (x1 y1 x2 y2 score), intrinsics [>= 3, >= 3] and cam-to-world poses [4,4] -> the packed view inputs."""
    offs = [0]
    for d in dets:
        offs.append(offs[-1] + int(d.shape[0]))
    rows = [_dev(d, device)[:, :5] for d in dets if d.shape[0] > 0]
    det = torch.cat(rows).contiguous() if rows else torch.zeros(0, 5, device=device)
    K3, w2c = _cameras(Ks, poses, device)
    return {"det": det, "det_off": _dev(torch.tensor(offs, dtype=torch.int32), device, torch.int32), "m": [b - a for a, b in zip(offs, offs[1:])],
            "K3": K3, "w2c": w2c, "height": float(img_res[0]), "width": float(img_res[1])}


def views_of(dataset, device):
    """The per-view inputs of a dataset: detections wireframe.line_segments(0.05), intrinsics, pose, img_res = (height, width)."""
    return pack_views(*run_io.dataset_views(dataset), dataset.img_res, device)


def as_lines(lines3d, device):
    """lines3d [N,2,3], or an object array of per-view arrays (concatenated) -> float32 device tensor [N,2,3]."""
    if isinstance(lines3d, np.ndarray) and lines3d.dtype == object:
        lines3d = run_io.stack_lines(lines3d, np.float32)
    return _dev(lines3d, device).reshape(-1, 2, 3).contiguous()


def fuse(lines, views, dis=10.0, keep=0.5, score_by_label=False):
    """fusion.py :79-141.  -> dict of device tensors: lines3d [K,2,3] (score > keep, in order), score [N], count [N] int32, keep [N] bool.
    score_by_label: the matched detection's own score instead of the score at the detection's rank among the view's matched ones."""
    lines = as_lines(lines, views["det"].device)
    score, count, flag, kept, n_kept = ops.post_fuse(lines, views["det"], views["det_off"], views["K3"], views["w2c"], dis, keep, score_by_label)
    return {"lines3d": kept[:int(n_kept.item())], "score": score, "count": count, "keep": flag}


def sdf_filter(lines, model, sdf_max=0.01, scores=None, score_max=0.01):
    """refinement.py :95-104: max |sdf| over 16 points of the line < sdf_max (and scores < score_max) -> keep [N] uint8 (device)."""
    t = torch.linspace(0, 1, 16, device=lines.device).reshape(1, -1, 1)
    pts = lines[:, :1] + t * (lines[:, 1:] - lines[:, :1])
    with torch.no_grad():
        sdf = model.implicit_network.get_sdf_vals(pts.reshape(-1, 3).contiguous()).reshape(lines.shape[0], 16).abs()
    ok = sdf.max(dim=-1)[0] < sdf_max
    if scores is not None:
        ok = ok & (_dev(scores, lines.device).reshape(-1) < score_max)
    return ok.to(torch.uint8)


def refine_device(lines, views, dis=10.0, model=None, sdf_max=0.01, scores=None, score_max=0.01):
    """The sequential walk of refinement.py :116-181 without any host synchronisation: -> (buffer [N,2,3], count int32 [1]) on the device."""
    dev = views["det"].device
    lines = as_lines(lines, dev)
    N = lines.shape[0]
    bufs = [torch.empty(max(N, 1), 2, 3, device=dev), torch.empty(max(N, 1), 2, 3, device=dev)]
    counts = [torch.empty(1, device=dev, dtype=torch.int32), torch.empty(1, device=dev, dtype=torch.int32)]
    if N == 0:
        counts[0].zero_()
        return bufs[0], counts[0]
    if model is not None and N > 0:
        ops.post_select(lines, sdf_filter(lines, model, sdf_max, scores, score_max), bufs[0], counts[0])
    else:
        bufs[0][:N].copy_(lines)
        counts[0].fill_(N)
    mmax = max(views["m"] + [1])
    ws = ops.post_refine_workspace(N, mmax, dev)
    cur = 0
    for v, m in enumerate(views["m"]):
        ops.post_refine_view(bufs[cur], counts[cur], views["det"], views["det_off"], m, mmax, views["K3"], views["w2c"], v, dis,
                             views["width"], views["height"], bufs[1 - cur], counts[1 - cur], ws)
        cur = 1 - cur
    return bufs[cur], counts[cur]


def refine(lines, views, dis=10.0, model=None, sdf_max=0.01, scores=None, score_max=0.01):
    """refinement.py :95-198: view after view, the lines that land on the same detection are merged into their mean.  -> lines3d [K,2,3]."""
    buf, count = refine_device(lines, views, dis, model, sdf_max, scores, score_max)
    return buf[:int(count.item())]


def snap(lines, grid=512, max_snap=None, unique=False, device=None):
    """nms.py :156-204: end points -> peaks of a grid^3 occupancy -> dict of device tensors junctions [P,3], count [P] int32, edges [E,2] int32,
    lines3d [E,2,3] = junctions[edges]."""
    if int(grid) > ops.POST_MAX_GRID or int(grid) < 2:            # before any launch, and before anything is moved to the device
        raise ValueError(f"snap: --grid {int(grid)} is refused (2 <= G <= {ops.POST_MAX_GRID}: cell keys (ix G + iy) G + iz are 32-bit)")
    lines = as_lines(lines, device or (lines.device if torch.is_tensor(lines) else torch.device("cuda", torch.cuda.current_device())))
    junc, pcount, edges, out, counts = ops.post_snap(lines, grid, max_snap, unique)
    P, E = counts.cpu().tolist() if lines.shape[0] > 0 else (0, 0)
    return {"junctions": junc[:P], "count": pcount[:P], "edges": edges[:E], "lines3d": out[:E]}


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.post", description="fuse, refine and snap 3-D wireframe lines on the device")
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p, need_conf):
        p.add_argument("--data", type=str, required=True, help="npz with key lines3d ([N,2,3], or an object array of per-view arrays)")
        p.add_argument("--conf", type=str, required=need_conf, default=None)
        p.add_argument("--checkpoint", default="latest", type=str)
        p.add_argument("--expdir", default=None, help="run directory (default: the conf's directory)")
        p.add_argument("--data_root", default="../data", help="root of the dataset's data_dir")
        p.add_argument("--gpu", type=int, default=0, help="device index")
        p.add_argument("--overwrite", default=False, action="store_true", help="replace an existing output file")

    f = sub.add_parser("fuse", help="score every line by the detections it lands on in each view (fusion.py)")
    common(f, True)
    f.add_argument("--dis", type=float, default=10.0, help="squared 4-vector distance below which a line matches a detection")
    f.add_argument("--keep", type=float, default=0.5, help="lines with a mean score above this stay")
    f.add_argument("--score-by-label", default=False, action="store_true",
                   help="take the matched detection's own score (default: the reference's enumerate rank)")
    r = sub.add_parser("refine", help="merge the lines that land on the same detection, view after view (refinement.py)")
    common(r, True)
    r.add_argument("--dis", type=float, default=10.0)
    r.add_argument("--sdf-max", type=float, default=0.01, help="pre-filter: max |sdf| over 16 points of the line")
    r.add_argument("--score-max", type=float, default=0.01, help="pre-filter: the data file's per-line scores, if it has them")
    r.add_argument("--no-filter", default=False, action="store_true", help="skip the SDF pre-filter (no checkpoint is read)")
    s = sub.add_parser("snap", help="junctions and edges by non-maximum suppression of end points on a grid (nms.py)")
    common(s, False)
    s.add_argument("--grid", type=int, default=512, help="grid nodes per axis (2..1024)")
    s.add_argument("--max-snap", type=float, default=None, help="keep a line only if both end points moved less than this")
    s.add_argument("--unique", default=False, action="store_true", help="drop i == j and repeated pairs; pairs (min, max) ascending")
    return ap


def out_path(opt):
    """The output file of a parsed command line."""
    base = os.path.basename(opt.data)[:-4]
    suffix = {"fuse": "fused", "refine": "ref", "snap": "snap"}[opt.cmd]
    if opt.cmd == "snap" and not opt.expdir:
        return os.path.join(os.path.dirname(os.path.abspath(opt.data)), f"{base}-snap.npz")
    root = run_io.run_dir(opt.conf, opt.expdir)
    return os.path.join(root, "wireframes", f"{base}-{suffix}.npz")


def main(argv=None):
    opt = build_parser().parse_args(argv)
    path = out_path(opt)
    if os.path.exists(path) and not opt.overwrite:
        print(f"keeping {path} (--overwrite replaces it)", flush=True)
        return 0
    if opt.cmd == "snap" and not 2 <= opt.grid <= ops.POST_MAX_GRID:
        print(f"snap: --grid {opt.grid} is refused (2 <= G <= {ops.POST_MAX_GRID})", file=sys.stderr, flush=True)
        return 2
    data = np.load(opt.data, allow_pickle=True)
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    sync = lambda: torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    lines = as_lines(data["lines3d"], device)
    out = {}
    if opt.cmd == "snap":
        sync()
        t1 = time.perf_counter()
        res = snap(lines, opt.grid, opt.max_snap, opt.unique)
        sync()
        t2 = time.perf_counter()
        out = {"junctions": res["junctions"], "edges": res["edges"], "lines3d": res["lines3d"], "count": res["count"]}
        print(f"load {t1 - t0:.3f} s, snap {t2 - t1:.3f} s: {lines.shape[0]} lines -> {res['junctions'].shape[0]} junctions, "
              f"{res['edges'].shape[0]} edges", flush=True)
    else:
        views = views_of(run_io.build_dataset(conf_mod.parse_file(opt.conf), opt.data_root, distance_threshold=1.0), device)      # the eval dataset, as neat_amd.parse builds it
        sync()
        t1 = time.perf_counter()
        if opt.cmd == "fuse":
            res = fuse(lines, views, opt.dis, opt.keep, opt.score_by_label)
            sync()
            t2 = time.perf_counter()
            out = res
            print(f"load {t1 - t0:.3f} s, fuse {t2 - t1:.3f} s ({'label' if opt.score_by_label else 'rank'} scores): {lines.shape[0]} lines -> "
                  f"{res['lines3d'].shape[0]}", flush=True)
        else:
            model, scores = None, None
            ckpt = run_io.checkpoint_path(run_io.run_dir(opt.conf, opt.expdir), opt.checkpoint)
            if opt.no_filter or not os.path.exists(ckpt):
                print("SDF pre-filter skipped" + ("" if opt.no_filter else f": no checkpoint at {ckpt}"), flush=True)
            else:
                model = run_io.load_model(opt.conf, opt.checkpoint, device, opt.expdir)[0]
                scores = np.asarray(data["scores"], np.float32) if "scores" in data.files else None
            sync()
            t1 = time.perf_counter()
            res = refine(lines, views, opt.dis, model, opt.sdf_max, scores, opt.score_max)
            sync()
            t2 = time.perf_counter()
            out = {"lines3d": res}
            print(f"load {t1 - t0:.3f} s, refine {t2 - t1:.3f} s: {lines.shape[0]} lines -> {res.shape[0]}", flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **{k: v.cpu().numpy() for k, v in out.items()})
    print(path, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
