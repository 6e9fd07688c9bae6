"""What a tool reads from a run directory: the conf's classes, its dataset, the model of a checkpoint, wireframe files and cam.json.

    <run>/runconf.conf                                       run = the conf's directory, or --expdir
    <run>/checkpoints/ModelParameters/<checkpoint>.pth       {"epoch", "model_state_dict"}, written by neat_amd.runner
    <run>/wireframes/{checkpoint}-{h}-{all,wfi,wfi_checked}.npz, -neat.pth      written by neat_amd.parse

The trainer and every tool (parse, mesh, render, trace, raycast, post, show, evaluate) stand on this module and on neat_amd.ply; none of
them reaches into another tool for its files.
"""
import json
import os

import numpy as np
import torch

from . import conf as conf_mod
from .general import get_class

CLASS_MAP = {
    "datasets.blender_hawp_dataset.BlenderDataset": "neat_amd.datasets.BlenderDataset",
    "datasets.scene_hawp_dataset.SceneDataset": "neat_amd.datasets.SceneDataset",
    "model.networks.neat_wfr_rend_a.VolSDFNetwork": "neat_amd.networks.VolSDFNetwork",
    "model.networks.loss_wfr.VolSDFLoss": "neat_amd.loss.VolSDFLoss",
}


def run_dir(conf_path, expdir=None):
    """The run directory of a conf: --expdir, or the directory the conf lies in."""
    return expdir or os.path.dirname(os.path.abspath(conf_path))


def checkpoint_path(root, checkpoint):
    """`<run>/checkpoints/ModelParameters/<checkpoint>.pth`."""
    return os.path.join(root, "checkpoints", "ModelParameters", str(checkpoint) + ".pth")


def conf_class(conf, key):
    """The class a conf key names; the reference's class paths are mapped to their neat_amd counterparts."""
    name = conf.get_string(key)
    return get_class(CLASS_MAP.get(name, name))


def parse_conf(conf_path):
    """The parsed conf of a run (neat_amd.conf.parse_file)."""
    return conf_mod.parse_file(conf_path)


def build_dataset(conf, data_root, scan_id=-1, **overrides):
    """The conf's dataset (train.dataset_class over the `dataset` block).  scan_id != -1 and `overrides` replace keys of the block; a
    neat_amd dataset also gets data_root."""
    dataset_conf = dict(conf.get_config("dataset").items())
    if scan_id != -1:
        dataset_conf["scan_id"] = scan_id
    dataset_conf.update(overrides)
    ds_cls = conf_class(conf, "train.dataset_class")
    if ds_cls.__module__.startswith("neat_amd"):
        dataset_conf["data_root"] = data_root
    return ds_cls(**dataset_conf)


def load_model(conf_path, checkpoint, device, expdir=None, precision=None):
    """-> (model with the checkpoint loaded strictly, in eval mode; its epoch; the run directory; the parsed conf)."""
    conf = conf_mod.parse_file(conf_path)
    root = run_dir(conf_path, expdir)
    model = conf_class(conf, "train.model_class")(conf=conf.get_config("model")).to(device)
    if precision is not None:
        model.set_precision(precision)
    path = checkpoint_path(root, checkpoint)
    print("Checkpoint: {}".format(path), flush=True)
    state = torch.load(path, map_location=device)
    model.load_state_dict(state["model_state_dict"], strict=True)
    model.eval()
    return model, state["epoch"], root, conf


def implicit_network_of(model):
    """The SDF network of a model, or the object itself if it is one."""
    return getattr(model, "implicit_network", model)


def stack_lines(lines3d, dtype=np.float64):
    """lines3d [n,2,3] (array or tensor), or an object array of per-view blocks (concatenated in order; none: no lines) -> `dtype` [n,2,3]."""
    if torch.is_tensor(lines3d):
        lines3d = lines3d.detach().cpu().numpy()
    lines3d = np.asarray(lines3d)
    if lines3d.dtype == object:
        parts = [np.asarray(p, dtype).reshape(-1, 2, 3) for p in lines3d]
        return np.concatenate(parts) if parts else np.zeros((0, 2, 3), dtype)
    return np.asarray(lines3d, dtype).reshape(-1, 2, 3)


def load_lines(path, pth_key="lines3d_wfi_checked"):
    """A wireframe file -> (lines3d float64 [n,2,3], scores or None): `lines3d` (and `scores`, if it has them) of a -all.npz / -wfi.npz /
    -wfi_checked.npz or of any tool's .npz, or `pth_key` of the -neat.pth that neat_amd.parse writes (no scores)."""
    if path.endswith(".pth"):
        return stack_lines(torch.load(path, map_location="cpu")[pth_key]), None
    with np.load(path, allow_pickle=True) as data:
        return stack_lines(data["lines3d"]), (data["scores"] if "scores" in data.files else None)


def dataset_views(dataset):
    """Every view of a dataset -> (segments wireframe.line_segments(0.05), intrinsics [3,3], camera-to-world poses [4,4]): three lists."""
    segments, Ks, poses = [], [], []
    for i in range(len(dataset)):
        _, sample, _ = dataset[i]
        segments.append(sample["wireframe"].line_segments(0.05))
        Ks.append(sample["intrinsics"][:3, :3])
        poses.append(sample["pose"])
    return segments, Ks, poses


def scene_images(instance_dir):
    """The views of a scene directory as the dataset classes list them: `images/` (BlenderDataset) or `image/` (SceneDataset), the
    sorted *.png / *.jpg / *.JPEG / *.JPG files without "mask" in their path."""
    for sub in ("images", "image"):
        folder = os.path.join(instance_dir, sub)
        if os.path.isdir(folder):
            names = [n for n in sorted(os.listdir(folder)) if os.path.splitext(n)[1] in (".png", ".jpg", ".JPEG", ".JPG")]
            return [p for p in (os.path.join(folder, n) for n in names) if "mask" not in p]
    raise FileNotFoundError(f"{instance_dir}: neither images/ nor image/")


def write_wireframe_json(path, wireframe, extra=None):
    """A WireframeGraph as the <scene>/<line_detector>/<image>.json the dataset classes read (`extra`: further keys, which load_json ignores)."""
    d = wireframe.jsonize()
    d.update(extra or {})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "w") as fh:
        json.dump(d, fh)
    os.replace(tmp, path)


def load_cam_json(path):
    """The cam.json neat_amd.show writes, a JSON list of 4 x 4 world-to-camera matrices -> float64 [F,4,4]."""
    with open(path) as fh:
        return np.asarray(json.load(fh), dtype=np.float64).reshape(-1, 4, 4)


def keep_rule(frac, min_views=5, min_frac=0.5):
    """The keep rule of the occlusion checks (neat_amd.trace check, neat_amd.raycast check): frac [F,N], the visible fraction of line n from
    view f -> (views int32 [N], the views that see at least min_frac of the line; kept bool [N]: at least min_views of them)."""
    frac = np.asarray(frac, dtype=np.float64)
    views = (frac >= float(min_frac)).sum(axis=0).astype(np.int32)
    return views, views >= int(min_views)


def write_occl(path, lines3d, views, kept):
    """The file of an occlusion check: lines3d (the kept lines, as neat_amd.show and evaluate dtu-lines read them), views int32 [N] (the
    seeing views per input line), kept bool [N]."""
    lines3d = np.asarray(lines3d).reshape(-1, 2, 3)
    kept = np.asarray(kept, dtype=bool)
    tmp = path + ".tmp.npz"
    np.savez(tmp, lines3d=lines3d[kept], views=np.asarray(views, dtype=np.int32), kept=kept)
    os.replace(tmp, path)
