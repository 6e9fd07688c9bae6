"""What a tool reads from a run directory: the conf's classes, its dataset, the model of a checkpoint, wireframe files and cam.json.

    <run>/runconf.conf                                       run = the conf's directory, or --expdir
    <run>/checkpoints/ModelParameters/<checkpoint>.pth       {"epoch", "model_state_dict"}, written by neat_amd.runner
    <run>/wireframes/{checkpoint}-{h}-{all,wfi,wfi_checked}.npz, -neat.pth      written by neat_amd.parse

A scan directory's ground truth (lines.json, offset_scale.txt), the dataset's cameras, --views, and how every tool writes a file
(replace_file, write_png, skip_existing) are here too.  The trainer and the twelve tools (parse, mesh, render, trace, raycast, post, show,
evaluate, detect, triangulate, scenegen, creases) stand on this module and on neat_amd.ply; none of them reaches into another tool for
its files, cameras or command line (neat_amd.visibility holds what trace check and raycast check share).
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


def dataset_graphs(dataset):
    """Every view of a dataset as a graph -> (vertices [n,2], edges [e,2] into them, intrinsics [3,3], camera-to-world poses [4,4]): four
    lists.  The edges are those scoring above 0.05, in order, so vertices[edges] are the rows of dataset_views' segments."""
    vertices, edges, Ks, poses = [], [], [], []
    for i in range(len(dataset)):
        _, sample, _ = dataset[i]
        wf = sample["wireframe"]
        vertices.append(wf.vertices)
        edges.append(wf.edges[wf.weights > 0.05])
        Ks.append(sample["intrinsics"][:3, :3])
        poses.append(sample["pose"])
    return vertices, edges, Ks, poses


def scene_images(instance_dir):
    """The views of a scene directory as the dataset classes list them: `images/` (BlenderDataset) or `image/` (SceneDataset), the
    sorted *.png / *.jpg / *.JPEG / *.JPG files without "mask" in their path."""
    for sub in ("images", "image"):
        folder = os.path.join(instance_dir, sub)
        if os.path.isdir(folder):
            names = [n for n in sorted(os.listdir(folder)) if os.path.splitext(n)[1] in (".png", ".jpg", ".JPEG", ".JPG")]
            return [p for p in (os.path.join(folder, n) for n in names) if "mask" not in p]
    raise FileNotFoundError(f"{instance_dir}: neither images/ nor image/")


def replace_file(path, write):
    """Every tool's way to write a file: the parent directory is made, write(tmp) fills a temporary file beside `path` (its name ends as
    `path` does, so np.savez adds nothing to it), and the finished file is moved into place.  If `write` raises, `path` is as it was and
    the temporary file is gone."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp" + os.path.splitext(path)[1]
    try:
        write(tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write_json(path, doc):
    """`doc` as JSON through replace_file (json writes a float with float.__repr__, so it reads back to the same float64)."""
    def write(tmp):
        with open(tmp, "w") as fh:
            json.dump(doc, fh)
    replace_file(path, write)


def skip_existing(path, overwrite):
    """True, and the line that says so, when `path` is on disk and --overwrite was not given."""
    skip = os.path.exists(path) and not overwrite
    if skip:
        print("exists: {} (--overwrite to replace it)".format(path), flush=True)
    return skip


def write_png(path, image, overwrite=True):
    """uint8 [H,W,3] or [H,W] (tensor or array) -> a PNG; an existing file is kept unless `overwrite`.  -> True if written."""
    if os.path.exists(path) and not overwrite:
        return False
    from PIL import Image
    arr = image.cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    replace_file(path, lambda tmp: Image.fromarray(np.ascontiguousarray(arr)).save(tmp, format="PNG"))
    return True


def write_wireframe_json(path, wireframe, extra=None):
    """A WireframeGraph as the <scene>/<line_detector>/<image>.json the dataset classes read (`extra`: further keys, which load_json ignores)."""
    d = wireframe.jsonize()
    d.update(extra or {})
    write_json(path, d)


def read_lines_json(path):
    """A scan's lines.json -> (junctions float64 [J,3], edges int64 [E,2]: the junctions each straight edge joins)."""
    with open(path) as fh:
        gt = json.load(fh)
    return np.asarray(gt["junctions"], dtype=np.float64).reshape(-1, 3), np.asarray(gt["lines"], dtype=np.int64).reshape(-1, 2)


def read_offset_scale(path):
    """A scan's offset_scale.txt -> its four numbers, float64: the offset, then the scale (model frame = (mesh frame + offset) * scale)."""
    with open(path) as fh:
        return np.array([float(v) for v in fh.read().split()], dtype=np.float64)


def dataset_cams(dataset):
    """The world-to-camera matrices float64 [F,4,4] of a dataset (the datasets hold camera-to-world)."""
    return np.linalg.inv(np.stack([np.asarray(torch.as_tensor(dataset.pose_all[i]).numpy(), dtype=np.float64) for i in range(len(dataset))]))


def read_cams(path):
    """World-to-camera matrices float64 [F,4,4] of a cameras.npz (`extrinsics`: camera-to-world poses, as the datasets') or of the
    cam.json neat_amd.show writes (world-to-camera)."""
    if path.lower().endswith(".json"):
        return load_cam_json(path)
    with np.load(path) as z:
        return np.linalg.inv(np.asarray(z["extrinsics"], dtype=np.float64).reshape(-1, 4, 4))


def fov_intrinsics(width, height, fov=60.0):
    """-> K [3,3]: vertical field of view `fov` degrees, square pixels, principal point ((W - 1) / 2, (H - 1) / 2)."""
    f = 0.5 * height / np.tan(0.5 * fov / 180.0 * np.pi)
    return np.array([[f, 0.0, 0.5 * (width - 1)], [0.0, f, 0.5 * (height - 1)], [0.0, 0.0, 1.0]])


def camera_centres(cams):
    """4 x 4 world-to-camera matrices [F,4,4] (any array) -> the camera centres -R^T t, float64 [F,3] on the host."""
    cams = np.asarray(torch.as_tensor(cams).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4, 4)
    return -np.einsum("fji,fj->fi", cams[:, :3, :3], cams[:, :3, 3])


def parse_views(text, n, step=False):
    """--views: 'a:b', with `step` also 'a:b:step' (any part may be empty) -> the range of views."""
    if text is None:
        return range(n)
    parts = text.split(":")
    if len(parts) not in ((2, 3) if step else (2,)):
        raise ValueError(f"--views {text}: expected a:b" + (" or a:b:step" if step else ""))
    a, b, c = ([int(p) if p.strip() else None for p in parts] + [None])[:3]
    if c is not None and c < 1:
        raise ValueError(f"--views {text}: the step must be positive")
    return range(n)[slice(a, b, c)]


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
    replace_file(path, lambda tmp: np.savez(tmp, lines3d=lines3d[kept], views=np.asarray(views, dtype=np.int32), kept=kept))
