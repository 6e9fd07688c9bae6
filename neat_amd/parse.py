"""Command line of the wireframe parsing (the reference's code/neat-final-parsing.py, same flags, defaults and output files):

    python -m neat_amd.parse --conf <run>/runconf.conf [--checkpoint latest] [--gpu 0] [--data_root ../data]

The checkpoint is read from `<dir of conf>/checkpoints/ModelParameters/<checkpoint>.pth` (or `<expdir>/checkpoints/...` with --expdir)
and loaded strictly; class paths of the conf that name the reference's classes are mapped through run_io.CLASS_MAP.  Files written under
`<run>/wireframes/` (run = the conf's directory, or --expdir):
    {checkpoint}-{h}-all.npz, -wfi.npz, -wfi_checked.npz   key `lines3d`
    {checkpoint}-{h}-neat.pth                              the result dict and `kwargs`
h = the first 8 characters of base64(sha256(repr(kwargs))) with '/' -> 'n', kwargs = conf, checkpoint, distance, sdf_junction_refine.
An existing .pth is reused (only the visibility check runs again) unless --overwrite is given.
"""
import argparse
import base64
import hashlib
import os
import sys

import numpy as np
import torch


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.parse")
    ap.add_argument("--conf", type=str, required=True)
    ap.add_argument("--gpu", type=int, default=0, help="device index")
    ap.add_argument("--checkpoint", default="latest", type=str, help="the trained model checkpoint to parse")
    ap.add_argument("--chunksize", default=2048, type=int, help="rays per eval-forward chunk")
    ap.add_argument("--reproj-dis", default=10, type=int, help="squared-distance threshold of the 2-D line matching")
    ap.add_argument("--ckdist", default=100, type=float, help="squared-distance threshold of the visibility check")
    ap.add_argument("--ckview", default=5, type=int, help="views a line must be visible in")
    ap.add_argument("--overwrite", default=False, action="store_true", help="recompute even if the .pth exists")
    ap.add_argument("--disable-junction-refine", default=False, action="store_true")
    ap.add_argument("--junc_match_threshold", default=0.02, type=float, help="3-D junction / end point matching threshold")
    ap.add_argument("--expdir", default=None, help="run directory holding checkpoints/ (default: the conf's directory)")
    ap.add_argument("--data_root", default="../data", help="root of the dataset's data_dir (neat_amd datasets)")
    return ap


def _hashable(o):
    if isinstance(o, (tuple, list)):
        return tuple(_hashable(e) for e in o)
    if isinstance(o, dict):
        return tuple(sorted((k, _hashable(v)) for k, v in o.items()))
    if isinstance(o, (set, frozenset)):
        return tuple(sorted(_hashable(e) for e in o))
    return o


def out_basename(conf, checkpoint, distance, sdf_junction_refine):
    """`{checkpoint}-{h}`: the reference's output name for these arguments."""
    key = {"conf": conf, "checkpoint": checkpoint, "distance": distance, "sdf_junction_refine": sdf_junction_refine}
    digest = base64.b64encode(hashlib.sha256(repr(_hashable(key)).encode()).digest()).decode()
    return "{}-{}".format(checkpoint, digest[:8].replace("/", "n"))


def main(argv=None):
    opt = build_parser().parse_args(argv)
    kwargs = dict(conf=opt.conf, checkpoint=opt.checkpoint, chunksize=opt.chunksize, distance=opt.reproj_dis, overwrite=opt.overwrite,
                  ckdist=opt.ckdist, ckview=opt.ckview, sdf_junction_refine=not opt.disable_junction_refine,
                  junc_match_threshold=opt.junc_match_threshold)
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    from . import parsing, run_io
    model, _, root, conf = run_io.load_model(opt.conf, opt.checkpoint, device, opt.expdir)
    dataset = run_io.build_dataset(conf, opt.data_root, distance_threshold=1.0)          # the eval dataset
    wireframe_dir = os.path.join(root, "wireframes")
    os.makedirs(wireframe_dir, exist_ok=True)
    base = out_basename(opt.conf, opt.checkpoint, opt.reproj_dis, kwargs["sdf_junction_refine"])
    pth_path = os.path.join(wireframe_dir, base + "-neat.pth")
    if os.path.exists(pth_path) and not opt.overwrite:
        print("reusing {}".format(pth_path), flush=True)
        results = torch.load(pth_path, map_location="cpu")
        # a reused result gets its visibility check again, with this call's --ckdist / --ckview (as the reference does)
        gts, Ks, poses = run_io.dataset_views(dataset)
        wfi = results["lines3d_wfi"].to(device).float().contiguous()
        _, checked, n_checked = parsing.visibility(wfi, gts, Ks, poses, opt.ckdist, opt.ckview)
        results["lines3d_wfi_checked"] = checked[:int(n_checked.item())].cpu()
    else:
        results, info = parsing.wireframe_recon(model, dataset, chunksize=opt.chunksize, line_dis_threshold=opt.reproj_dis,
                                                junc_match_threshold=opt.junc_match_threshold, ckdist=opt.ckdist, ckview=opt.ckview,
                                                sdf_junction_refine=kwargs["sdf_junction_refine"], device=device)
        print("forward {:.3f} s, post-processing {:.3f} s".format(info["forward_s"], info["post_s"]), flush=True)
        results = {k: v.cpu() for k, v in results.items()}
        results["kwargs"] = kwargs
    for key in ("all", "wfi", "wfi_checked"):
        path = os.path.join(wireframe_dir, "{}-{}.npz".format(base, key))
        np.savez(path, lines3d=results["lines3d_" + key].cpu().numpy())
        print(path, flush=True)
    torch.save(results, pth_path)
    print("done", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
