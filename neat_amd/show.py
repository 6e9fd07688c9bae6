"""Headless pictures of a parsed wireframe, optionally in front of the surface mesh: the third step of the reference's README
(code/visualization/show.py, which opens an open3d window, waits for keys and draws each frame through matplotlib; code/evaluation/
show-mesh.py for the mesh).  Turntable or fixed cameras -> PNG frames, a GIF and the cameras used.

    python -m neat_amd.show --data X-wfi_checked.npz [--mesh surface_2000.ply] --pose dtu --save-path out

The host builds cameras, reads files and encodes PNG / GIF (PIL); every pixel is written by the HIP kernels of
neat_amd/csrc/kernels_show.hpp behind neat_show_* (include/neat_hip.h), all frames of a turntable in one launch per pass.  The picture is
defined exactly in DESIGN 3d and restated in numpy by tests/show_f64.py.  There is no host fallback.

Divergences from show.py: --hide-lines is off by default and, given, draws the points only (the reference's flag is a
no-op); --line-width is in pixels (the reference's 0.03 is a matplotlib point size at dpi = width); --save-path is not needed to write
(the default directory is dirname(data)/../name); --cams takes the dataset's cameras.npz with --views, and --cam-json the list of 4 x 4
world-to-camera matrices that show.py writes as cam.json, one frame each.  Not built: the window and its key bindings, slerp between two
saved views, PDF / MP4 output.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

from . import _lib, ply, run_io
from ._lib import ptr as _p, stream as _stream

POSES = {"dtu": (-155.0, 0.0, -25.0, 3.0), "scan": (0.0, 170.0, -45.0, 3.0), None: (0.0, 0.0, 0.0, 3.0)}      # show.py:459-471
STYLE = dict(line_width=1.5, point_radius=2.5, near=0.05, depth_bias=0.01, hidden_alpha=0.0, bg=(1.0, 1.0, 1.0), line_color=(0.0, 0.0, 0.0),
             point_color=(0.0, 0.0, 1.0), mesh_color=(0.8, 0.8, 0.8), show_lines=True)


# ------------------------------------------------------------------ cameras (host)
def _axis_turn(axis, degrees):
    """The reference's three elementary matrices, entries rounded to float32 as it stores them: `x` turns y into z, `y` turns z into x
    (note the sign: its rot_theta is the transpose of the usual one), `z` turns x into y."""
    a = degrees / 180.0 * np.pi
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4, dtype=np.float32)
    if axis == "x":
        m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    elif axis == "y":
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, -s, s, c
    else:
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def camera_to_world(psi, theta, phi, radius):
    """show.py:26-66 (pose_spherical): a camera `radius` down its own z axis, turned by phi about x, theta about y, psi about z, then
    the axes relabelled (x, y, z) -> (-z, x, -y).  The reference multiplies in float32 and relabels in float64; so does this."""
    m = np.eye(4, dtype=np.float32)
    m[2, 3] = radius
    m = _axis_turn("z", psi) @ (_axis_turn("y", theta) @ (_axis_turn("x", phi) @ m))
    relabel = np.array([[0, 0, -1, 0], [1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
    return relabel @ m.astype(np.float64)


CAMERA_AXES = np.diag([1.0, -1.0, -1.0, 1.0])      # the reference's camera looks down its -z with y up; this project's down +z with y (rows) down


def orbit(rx=0.0, ry=0.0, rz=0.0, t=3.0, frames=72, step=5.0):
    """-> [frames,4,4] float64 world-to-camera matrices: frame k is CAMERA_AXES @ inverse(camera_to_world(rx, (ry + k step) mod 360, rz, t))
    (show.py:292-298).  The reference hands the bare inverse to open3d, whose view control re-derives a camera that looks at the origin;
    read as a pinhole extrinsic the bare inverse has the scene behind the camera (the origin at z = -t), so the axes are changed here."""
    if not frames:
        return np.zeros((0, 4, 4))
    return np.stack([CAMERA_AXES @ np.linalg.inv(camera_to_world(rx, (ry + k * step) % 360, rz, t)) for k in range(int(frames))])


intrinsics = run_io.fov_intrinsics              # its home is neat_amd.run_io


def pack_cameras(cameras, K):
    """cameras [F,4,4] (or [F,3,4]) world-to-camera, K [3,3] or [F,3,3] -> [F,21] float64: K then [R|T] per frame."""
    w2c = np.asarray(cameras, dtype=np.float64)
    if w2c.ndim == 2:
        w2c = w2c[None]
    F = w2c.shape[0]
    K = np.broadcast_to(np.asarray(K, dtype=np.float64)[..., :3, :3], (F, 3, 3))
    return np.concatenate([K.reshape(F, 9), w2c[:, :3, :4].reshape(F, 12)], axis=1)


def dataset_cameras(path, views):
    """cameras.npz (world_mat_i, scale_mat_i) -> (w2c [F,4,4], K [F,3,3]) through the decomposition of neat_amd.datasets."""
    from .datasets import load_K_Rt_from_P
    cams = np.load(path)
    w2c, Ks = [], []
    for i in views:
        P = (cams["world_mat_%d" % i].astype(np.float32) @ cams["scale_mat_%d" % i].astype(np.float32))[:3, :4]
        K, pose = load_K_Rt_from_P(P)
        w2c.append(np.linalg.inv(np.asarray(pose, dtype=np.float64)))
        Ks.append(K[:3, :3])
    return np.stack(w2c), np.stack(Ks)


# ------------------------------------------------------------------ device
def _dev(x, dtype, cols, device):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(np.asarray(x)))
    t = t.detach().to(device=device, dtype=dtype).reshape(-1, cols).contiguous()
    if not t.is_cuda:
        raise RuntimeError("neat_amd.show renders on the device only")
    return t


def endpoints(lines3d):
    """The distinct endpoints of lines [n,2,3] -> [m,3] float64 (sorted rows)."""
    p = np.asarray(lines3d, dtype=np.float64).reshape(-1, 3)
    return np.unique(p, axis=0) if len(p) else p


class Buffers:
    """The workspace of one render: views of its parts, for tests and timing (depth float32, index int64 with -1 for no triangle)."""

    def __init__(self, F, H, W, device):
        lib = _lib.lib()
        self.F, self.H, self.W = F, H, W
        nbytes = int(lib.neat_show_ws_bytes(F, H, W))
        if nbytes == 0:
            raise RuntimeError("neat_show_ws_bytes: a frame stack of %d x %d x %d is not rendered" % (F, H, W))
        offs = (ctypes.c_size_t * 4)()
        _lib.check(lib.neat_show_ws_layout(F, H, W, offs), "neat_show_ws_layout")
        self.ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        n = F * H * W
        self.key = self.ws[offs[0]:offs[0] + 8 * n].view(torch.int64).view(F, H, W)
        self.cov = self.ws[offs[1]:offs[1] + 4 * n].view(torch.float32).view(F, H, W)
        self.covp = self.ws[offs[2]:offs[2] + 4 * n].view(torch.float32).view(F, H, W)
        self.status = self.ws[offs[3]:offs[3] + 4].view(torch.int32)

    @property
    def depth(self):
        return (self.key >> 32).to(torch.int32).view(torch.float32)

    @property
    def index(self):
        k = self.key & 0xffffffff
        return torch.where(k == 0xffffffff, torch.full_like(k, -1), k)


def render(lines3d, cameras, K, width, height, mesh=None, points=None, return_buffers=False, timings=None, **style):
    """lines3d [n,2,3] (or None), cameras [F,4,4] world-to-camera, K [3,3] or [F,3,3], mesh = (verts [nv,3], faces [nf,3]) or None,
    points [m,3] or None -> uint8 [F,H,W,3] on the device (and the Buffers, if asked).  style: the keys of STYLE.  timings = a dict
    receives the milliseconds of every pass (HIP events on the stream; this synchronises)."""
    unknown = set(style) - set(STYLE)
    if unknown:
        raise TypeError("render: unknown style %s" % ", ".join(sorted(unknown)))
    st = dict(STYLE)
    st.update(style)
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    for x in (lines3d, points) + (tuple(mesh) if mesh is not None else ()):
        if torch.is_tensor(x) and x.is_cuda:
            dev = x.device
    cams_h = pack_cameras(cameras, K)
    F, H, W = cams_h.shape[0], int(height), int(width)
    cams = _dev(cams_h, torch.float64, 21, dev)
    lines = _dev(lines3d, torch.float64, 6, dev) if lines3d is not None and st["show_lines"] else None
    pts = _dev(points, torch.float64, 3, dev) if points is not None else None
    verts = faces = None
    if mesh is not None:
        verts, faces = _dev(mesh[0], torch.float64, 3, dev), _dev(mesh[1], torch.int32, 3, dev)
    nv, nf = (verts.shape[0], faces.shape[0]) if mesh is not None else (0, 0)
    with torch.cuda.device(dev):
        buf = Buffers(F, H, W, dev)
        out = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
        s = _stream()
        near, bias, alpha = float(st["near"]), float(st["depth_bias"]), float(st["hidden_alpha"])
        events = []

        def run(name, code):
            if timings is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            _lib.check(code(), "neat_show_" + name)
            if timings is not None:
                e1.record()
                events.append((name, e0, e1))
        run("clear", lambda: lib.neat_show_clear(_p(buf.ws), F, H, W, s))
        if nf:
            run("mesh", lambda: lib.neat_show_mesh(_p(verts), nv, _p(faces), nf, _p(cams), F, H, W, near, _p(buf.ws), s))
        if lines is not None and lines.shape[0]:
            run("lines", lambda: lib.neat_show_lines(_p(lines), lines.shape[0], _p(cams), F, H, W, near, float(st["line_width"]), bias, alpha,
                                                     _p(buf.ws), s))
        if pts is not None and pts.shape[0]:
            run("points", lambda: lib.neat_show_points(_p(pts), pts.shape[0], _p(cams), F, H, W, near, float(st["point_radius"]), bias, alpha,
                                                       _p(buf.ws), s))
        colors = (ctypes.c_double * 12)(*[float(v) for k in ("bg", "line_color", "point_color", "mesh_color") for v in st[k]])
        run("resolve", lambda: lib.neat_show_resolve(_p(verts), nv, _p(faces), nf, _p(cams), F, H, W, colors, _p(buf.ws), _p(out), s))
        if timings is not None:
            torch.cuda.synchronize()
            timings.update({name: e0.elapsed_time(e1) for name, e0, e1 in events})
        if nf and int(buf.status.item()) != 0:          # the one read-back
            raise RuntimeError("render: a face index out of range (the picture was not written)")
    return (out, buf) if return_buffers else out


# ------------------------------------------------------------------ files
def write_frames(directory, frames, gif=None, overwrite=False, first=0):
    """frames uint8 [F,H,W,3] (tensor or array) -> directory/{k:04d}.png, kept if present unless `overwrite`; gif = a path writes the
    frames as they are on disk after this call (30 per second, as show.py).  -> the PNG paths."""
    from PIL import Image
    arr = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, im in enumerate(arr):
        path = os.path.join(directory, "%04d.png" % (first + k))
        if overwrite or not os.path.exists(path):
            Image.fromarray(np.ascontiguousarray(im)).save(path)
        paths.append(path)
    if gif and paths:
        ims = [Image.open(p).convert("RGB") for p in paths]
        ims[0].save(gif, save_all=True, append_images=ims[1:], duration=1000 // 30, loop=0)
    return paths


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.show", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", type=str, required=True, help="the reconstructed wireframe: an .npz with `lines3d`, or a -neat.pth")
    ap.add_argument("--mesh", type=str, default=None, help="a triangle mesh (.ply) drawn shaded behind the wireframe; it hides what lies behind it")
    ap.add_argument("--save-path", type=str, default=None, help="output directory (default dirname(data)/..)")
    ap.add_argument("--name", type=str, default="video")
    ap.add_argument("--pose", type=str, default=None, choices=["dtu", "scan"])
    for k in ("rx", "ry", "rz", "t"):
        ap.add_argument("--" + k, type=float, default=None, help="overrides the preset's value")
    ap.add_argument("--frames", type=int, default=72)
    ap.add_argument("--step", type=float, default=5.0, help="degrees of theta per frame")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--fov", type=float, default=60.0, help="vertical field of view, degrees")
    ap.add_argument("--line-width", type=float, default=1.5, help="pixels")
    ap.add_argument("--show-points", default=False, action="store_true")
    ap.add_argument("--point-radius", type=float, default=2.5, help="pixels")
    ap.add_argument("--hide-lines", default=False, action="store_true", help="draw the endpoints only (implies --show-points)")
    ap.add_argument("--cams", type=str, default=None, help="the dataset's cameras.npz; with --views")
    ap.add_argument("--views", type=str, default=None, help="comma-separated view indices of --cams")
    ap.add_argument("--cam-json", type=str, default=None, help="a JSON list of 4x4 world-to-camera matrices, one frame each")
    ap.add_argument("--hidden-alpha", type=float, default=0.0, help="opacity of the wireframe where the mesh hides it")
    ap.add_argument("--depth-bias", type=float, default=0.01)
    ap.add_argument("--near", type=float, default=0.05)
    ap.add_argument("--bg", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    ap.add_argument("--line-color", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    ap.add_argument("--point-color", type=float, nargs=3, default=[0.0, 0.0, 1.0])
    ap.add_argument("--mesh-color", type=float, nargs=3, default=[0.8, 0.8, 0.8])
    ap.add_argument("--no-gif", default=False, action="store_true")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--overwrite", default=False, action="store_true", help="rewrite frames that are already on disk")
    return ap


def pose_of(opt):
    """-> (rx, ry, rz, t): the preset, with any of --rx --ry --rz --t over it."""
    preset = POSES[opt.pose]
    return tuple(preset[i] if getattr(opt, k) is None else getattr(opt, k) for i, k in enumerate(("rx", "ry", "rz", "t")))


def output_dir(opt):
    """DIR/name: DIR = --save-path, or dirname(data)/.. (show.py:452)."""
    return os.path.join(opt.save_path if opt.save_path is not None else os.path.join(os.path.dirname(opt.data), ".."), opt.name)


def cameras_of(opt):
    """-> (w2c [F,4,4], K [3,3] or [F,3,3]) from --cam-json, --cams / --views or the orbit."""
    K = intrinsics(opt.width, opt.height, opt.fov)
    if opt.cam_json is not None:
        return run_io.load_cam_json(opt.cam_json), K
    if opt.cams is not None:
        if not opt.views:
            raise SystemExit("--cams needs --views")
        return dataset_cameras(opt.cams, [int(v) for v in opt.views.split(",")])
    return orbit(*pose_of(opt), frames=opt.frames, step=opt.step), K


def style_of(opt):
    return dict(line_width=opt.line_width, point_radius=opt.point_radius, near=opt.near, depth_bias=opt.depth_bias, hidden_alpha=opt.hidden_alpha,
                bg=tuple(opt.bg), line_color=tuple(opt.line_color), point_color=tuple(opt.point_color), mesh_color=tuple(opt.mesh_color),
                show_lines=not opt.hide_lines)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    _lib.lib()                      # a missing library is an error before any file is read
    lines3d = run_io.load_lines(opt.data)[0]          # an object array of per-view blocks is concatenated (show.py:478-479)
    mesh = None
    if opt.mesh is not None:
        m = ply.read_ply(opt.mesh)
        if m["faces"] is None:
            raise SystemExit("%s has no faces" % opt.mesh)
        mesh = (m["points"], m["faces"])
    w2c, K = cameras_of(opt)
    points = endpoints(lines3d) if (opt.show_points or opt.hide_lines) else None
    torch.cuda.set_device(opt.gpu)
    t0 = time.perf_counter()
    frames = render(lines3d, w2c, K, opt.width, opt.height, mesh=mesh, points=points, **style_of(opt))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = output_dir(opt)
    write_frames(out, frames, gif=None if opt.no_gif else out + ".gif", overwrite=opt.overwrite)
    with open(os.path.join(out, "cam.json"), "w") as fh:
        json.dump([m.tolist() for m in np.asarray(w2c, dtype=np.float64)], fh)
    t2 = time.perf_counter()
    print("%d segments, %d triangles, %d frames of %d x %d -> %s" % (len(lines3d), 0 if mesh is None else len(mesh[1]), len(w2c), opt.width,
                                                                    opt.height, out))
    print("device rendering %.3f s, encoding %.3f s" % (t1 - t0, t2 - t1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
