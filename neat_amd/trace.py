"""Where the surface a checkpoint learnt lies along a ray: sphere tracing of the raw SDF on the device.

    from neat_amd import trace
    depth, state, steps, points, evals = trace.rays(model, origins, dirs, radius=3.0)
    depth, normal, state = trace.view(model, pose, intrinsics, H, W)
    seen = trace.visible_points(model, points, cams)            # bool [F, N]
    frac = trace.visible_lines(model, lines3d, cams)            # float [F, N]

    python -m neat_amd.trace check --conf <run>/runconf.conf --data X-wfi.npz|X-neat.pth [--min-views 5] [--min-frac 0.5] [--bias 0.01]
        [--samples 16] [--checkpoint latest] [--expdir <run>] [--data_root ../data] [--gpu 0] [--precision P] [--json] [--overwrite]

The per-ray state machine and the ordered compaction of the rays that still need a query are the kernels of csrc/kernels_trace.hpp behind
neat_trace_* (include/neat_hip.h; tests/trace_f64.py restates them in float64); the SDF between them is ops.sdf_values with
radius 0, the network without its clamp to the bounding sphere (the clamped SDF reaches zero at the sphere and would "hit" it on the
way out).  A ray that has finished is in no later query; the host reads the active count once per iteration to size the next query and
stops at zero.  There is no host fallback.

`check` is the occlusion-aware visibility test the reference runs against the ground-truth mesh (evaluation/abc-analysis.py:44-56,
open3d ray casts), asked of the learnt SDF instead (against a triangle mesh it is `python -m neat_amd.raycast check`, which shares the
keep rule and the file layout): a line is kept when at least --min-views of the dataset's cameras see at least --min-frac of its
--samples points.  It writes `<data stem>_occl.npz` beside the input: lines3d (the kept lines, as neat_amd.show and
evaluate dtu-lines read them), views int32 [N] (the seeing views per input line), kept bool [N].  The view frustum is not tested: that
stays the 2-D check of neat_amd.parse (--ckdist --ckview).  A -neat.pth contributes its `lines3d_wfi`.
"""
import argparse
import os
import sys
import time

import torch

from . import _lib, run_io, visibility

MISS, HIT, INSIDE, UNCONVERGED = 0, 1, 2, 3
DEFAULTS = dict(eps=1e-4, relax=1.0, max_steps=64, refine_steps=8, near=0.0)
DEFAULT_CHUNK = 1 << 20


def _sdf_network(sdf):
    """The SDF network of a model, or None for anything else (a bare callable field)."""
    net = run_io.implicit_network_of(sdf)
    return net if hasattr(net, "handle") and hasattr(net, "sphere_scale") else None


def field_of(sdf):
    """A model (its implicit_network, unclamped, at the model's build) or any callable points [n,3] -> values [n] on the device."""
    net = _sdf_network(sdf)
    if net is None:
        if not callable(sdf):
            raise TypeError("trace: sdf is a model or a callable points [n,3] -> values [n]")
        return sdf
    from . import ops
    return lambda pts: ops.sdf_values(net.handle(), pts, 0.0, net.sphere_scale).view(-1)


@torch.no_grad()
def rays(sdf, origins, dirs, *, radius, t_end=None, eps=DEFAULTS["eps"], relax=DEFAULTS["relax"], max_steps=DEFAULTS["max_steps"],
         refine_steps=DEFAULTS["refine_steps"], near=DEFAULTS["near"], chunk=DEFAULT_CHUNK, record=None):
    """origins, dirs [R,3] (|dir| = 1) float32 on the device, t_end [R] or None -> (depth [R] float32, NaN unless HIT or INSIDE;
    state [R] uint8; steps [R] int32, the queries made per ray; points [R,3], the hit points, NaN rows likewise; evals, the number of
    SDF evaluations = steps.sum()).  `chunk` rays are traced at a time.  record = a list receives, per iteration, (first ray of the chunk,
    the active ray ids of that iteration as an int32 device tensor): what the field was asked."""
    from . import ops
    field = field_of(sdf)
    origins, dirs = ops._f32c(origins.detach()), ops._f32c(dirs.detach())
    R = int(origins.shape[0])
    if origins.shape != (R, 3) or dirs.shape != (R, 3):
        raise ValueError("trace.rays: origins and dirs [R, 3]")
    if not (eps > 0 and relax > 0 and max_steps >= 0 and 0 <= refine_steps <= 64 and radius > 0 and int(chunk) >= 1):
        raise ValueError("trace.rays: eps, relax, radius > 0; max_steps >= 0; 0 <= refine_steps <= 64; chunk >= 1")
    chunk = min(int(chunk), ops.TRACE_MAX_RAYS)
    dev = origins.device
    depth, state = torch.empty(R, device=dev), torch.empty(R, device=dev, dtype=torch.uint8)
    steps, points = torch.empty(R, device=dev, dtype=torch.int32), torch.empty(R, 3, device=dev)
    evals = 0
    with torch.cuda.device(dev):
        for r0 in range(0, R, int(chunk)):
            r1 = min(R, r0 + int(chunk))
            run = ops.TraceRun(origins[r0:r1], dirs[r0:r1], None if t_end is None else t_end[r0:r1], radius, near)
            n = run.count()
            while n > 0:
                if record is not None:
                    record.append((r0, run.active(n).clone()))
                run.step(field(run.points[:n]), n, eps, relax, max_steps, refine_steps)
                n = run.count()
            run.finish(depth[r0:r1], state[r0:r1], steps[r0:r1], points[r0:r1])
            evals += run.evals()
    return depth, state, steps, points, evals


def _radius_of(model, radius):
    if radius is not None:
        return float(radius)
    r = float(getattr(_sdf_network(model), "sdf_bounding_sphere", 0.0) or 0.0)
    if not r > 0:
        raise ValueError("trace: the model has no bounding sphere; give radius=")
    return r


@torch.no_grad()
def view(model, pose, intrinsics, H, W, *, radius=None, timings=None, **march):
    """One view of H x W pixels: pose [4,4] camera-to-world, intrinsics [4,4] or [3,3] (a leading 1 allowed) on the device -> (depth [H,W]
    float32, the distance along the ray as in neat_amd.render's depth plane, NaN unless HIT or INSIDE; normal [H,W,3], the normalised
    SDF gradient at the HIT points, zero elsewhere; state [H,W] uint8).  Rays are neat_camera_rays', as render_pixels makes them.
    radius defaults to the model's bounding sphere; **march: eps, relax, max_steps, refine_steps, near, chunk.
    timings = a dict receives trace_s (device-synchronised wall time), evals and rays."""
    from . import ops
    net = _sdf_network(model)
    if net is None:
        raise TypeError("trace.view: a model")
    dev = next(net.parameters()).device
    pose = pose.detach().to(dev, torch.float32).reshape(1, 4, 4).contiguous()
    K = intrinsics.detach().to(dev, torch.float32)
    K = K.reshape(1, *K.shape[-2:]).contiguous()
    if timings is not None:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    with torch.cuda.device(dev):
        dirs, _, origins = ops.camera_rays(ops.pixel_grid(H, W, dev)[None], pose, K, with_origins=True)
        depth, state, _, points, evals = rays(model, origins, dirs.reshape(-1, 3), radius=_radius_of(model, radius), **march)
        normal = torch.zeros(H * W, 3, device=dev)
        hit = torch.nonzero(state == HIT).flatten()
        chunk = 1 << 18
        for i0 in range(0, hit.shape[0], chunk):
            idx = hit[i0:i0 + chunk]
            _, g = ops.sdf_point_normals(net.handle(), points[idx].contiguous(), 0.0, net.sphere_scale)
            normal[idx] = ops.unit_rows3_(g.detach().contiguous())
    if timings is not None:
        torch.cuda.synchronize(dev)
        timings.update(trace_s=time.perf_counter() - t0, evals=evals, rays=H * W)
    return depth.view(H, W), normal.view(H, W, 3), state.view(H, W)


camera_centres, keep_rule, write_occl = run_io.camera_centres, run_io.keep_rule, run_io.write_occl      # their home is neat_amd.run_io


def _visible(model, rows, cams, samples, bias, radius, march):
    net = _sdf_network(model)
    dev = next(net.parameters()).device if net is not None else rows.device
    radius = _radius_of(model, radius)
    return visibility.visible(dev, rows, cams, samples, bias, radius, march.get("near", DEFAULTS["near"]),
                              lambda o, d, t_end: rays(model, o, d, radius=radius, t_end=t_end, **march)[1] == MISS)


@torch.no_grad()
def visible_points(model, points, cams, *, bias=0.01, radius=None, **march):
    """points [N,3], cams [F,4,4] world-to-camera -> bool [F,N] on the device: point p is visible from the camera centre c iff the ray
    from c towards p, clipped to t_end = |p - c| - bias, ends as MISS.  A point outside the bounding sphere, or nearer to c than
    near + bias, is not visible.  The view frustum is not tested."""
    return _visible(model, points, cams, 1, bias, radius, march)[..., 0]


@torch.no_grad()
def visible_lines(model, lines3d, cams, *, samples=16, bias=0.01, radius=None, **march):
    """lines3d [N,2,3], cams [F,4,4] -> float32 [F,N]: the visible fraction of the `samples` points linspace(0, 1, samples) of each segment."""
    if samples < 2:
        raise ValueError("trace.visible_lines: samples >= 2")
    return _visible(model, lines3d, cams, int(samples), bias, radius, march).float().mean(dim=-1)


# ------------------------------------------------------------------ command line
def out_path(data):
    """`<data stem>_occl.npz` beside the input."""
    return os.path.splitext(data)[0] + "_occl.npz"


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m neat_amd.trace", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    ck = sub.add_parser("check", help="keep the lines of a wireframe that enough cameras see past the learnt surface")
    ck.add_argument("--conf", type=str, required=True)
    visibility.add_check_flags(ck, "--data", "--min-views", "--min-frac", "--bias", "--samples")
    ck.add_argument("--checkpoint", default="latest", type=str)
    ck.add_argument("--expdir", default=None, help="run directory holding checkpoints/ (default: the conf's directory)")
    visibility.add_check_flags(ck, "--data_root", "--gpu")
    ck.add_argument("--precision", choices=list(_lib.PRECISIONS), default=None)
    visibility.add_check_flags(ck, "--json")
    ck.add_argument("--overwrite", default=False, action="store_true", help="rewrite an _occl.npz that is already on disk")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    visibility.validate_check(ap, opt)
    return opt


def main_check(opt):
    _lib.lib()
    path = out_path(opt.data)
    if run_io.skip_existing(path, opt.overwrite):
        return 0
    torch.cuda.set_device(opt.gpu)
    device = torch.device("cuda", opt.gpu)
    model, epoch, _, conf = run_io.load_model(opt.conf, opt.checkpoint, device, opt.expdir, opt.precision)
    cams = run_io.dataset_cams(run_io.build_dataset(conf, opt.data_root))
    return visibility.run_check(opt, path, device, cams, lambda lines3d: (
        visible_lines(model, lines3d, cams, samples=opt.samples, bias=opt.bias).cpu().numpy(), {}), "tracing", "trace_s", {"epoch": int(epoch)})


def main(argv=None):
    opt = parse_args(argv)
    return main_check(opt)


if __name__ == "__main__":
    sys.exit(main())
