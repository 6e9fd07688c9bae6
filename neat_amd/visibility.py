"""The occlusion check that `python -m neat_amd.trace check` asks of a learnt SDF and `python -m neat_amd.raycast check` of a triangle
mesh: the rays from the camera centres to the targets (neat_trace_target_rays), the flags and their validation, and the body of the
sub-command.  A tool brings its occluder, its cameras, its own flags, the verb of its message and the keys of its JSON object."""
import json
import time

import numpy as np
import torch

from . import ops, run_io


@torch.no_grad()
def visible(device, rows, cams, samples, bias, radius, near, unblocked):
    """rows [N,3] (samples = 1: points) or [N,2,3] (segments, `samples` points linspace(0, 1, samples) of each), cams [F,4,4]
    world-to-camera -> bool [F,N,samples] on the device: the target lies inside the sphere of `radius`, further from the camera centre
    than near + bias, and unblocked(origins, dirs, t_end) -> bool [F N samples] says that nothing stops its ray before
    t_end = distance - bias.  radius: a number, or a callable (centres float64 [F,3] on the host, rows float32 on the device) -> a number
    that is asked only when there are targets."""
    centres = run_io.camera_centres(cams)
    rows = torch.as_tensor(rows).detach().to(device, torch.float32).reshape(-1, 3 if samples == 1 else 6).contiguous()
    F, N = centres.shape[0], int(rows.shape[0])
    if F * N == 0:
        return torch.zeros(F, N, samples, device=device, dtype=torch.bool)
    if callable(radius):
        radius = radius(centres, rows)
    centres = torch.from_numpy(centres.astype(np.float32)).to(device)
    with torch.cuda.device(device):
        o, d, t_end, ok = ops.trace_target_rays(centres, rows, samples, radius, near, bias)
        return (unblocked(o, d, t_end) & (ok != 0)).view(F, N, samples)


# ------------------------------------------------------------------ the check sub-command
CHECK_FLAGS = {
    "--data": dict(type=str, required=True, help="the wireframe: an .npz with `lines3d`, or a -neat.pth (its lines3d_wfi)"),
    "--min-views": dict(default=5, type=int, help="views that must see a line"),
    "--min-frac": dict(default=0.5, type=float, help="fraction of a line's samples a view must see"),
    "--bias": dict(default=0.01, type=float, help="a ray stops this far in front of its target"),
    "--samples": dict(default=16, type=int, help="points per line"),
    "--data_root": dict(default="../data", help="root of the dataset's data_dir"),
    "--gpu": dict(default=0, type=int, help="device index"),
    "--json": dict(default=False, action="store_true", help="print one JSON object with the counts and the seconds"),
}


def add_check_flags(ck, *flags):
    """The named flags of CHECK_FLAGS, in the order given: a tool puts its own between them, so --help lists them as it always did."""
    for flag in flags:
        ck.add_argument(flag, **CHECK_FLAGS[flag])


def validate_check(ap, opt):
    if opt.samples < 2 or opt.min_views < 0 or not 0.0 <= opt.min_frac <= 1.0 or not opt.bias >= 0.0:
        ap.error("--samples >= 2, --min-views >= 0, 0 <= --min-frac <= 1, --bias >= 0")


def run_check(opt, path, device, cams, fraction, verb, seconds_key, head=()):
    """The lines of --data (of a -neat.pth: those before the 2-D visibility check) -> run_io.keep_rule -> run_io.write_occl(path), the
    message and the --json object.  fraction(lines3d tensor [N,2,3]) -> (the visible fractions [F,N] on the host, a dict of counts that
    the message and the JSON object name after the samples); it is what the seconds measure.  head: the first items of the object."""
    lines3d = run_io.load_lines(opt.data, pth_key="lines3d_wfi")[0]
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    frac, counts = fraction(torch.from_numpy(lines3d))
    seconds = time.perf_counter() - t0
    views, kept = run_io.keep_rule(frac, opt.min_views, opt.min_frac)
    run_io.write_occl(path, lines3d, views, kept)
    print("{}: kept {} / {} lines ({} views, {} samples per line{}), {} {:.3f} s".format(
        path, int(kept.sum()), len(kept), len(cams), opt.samples, "".join(", {} {}".format(v, k) for k, v in counts.items()), verb, seconds), flush=True)
    if opt.json:
        print(json.dumps({**dict(head), "path": path, "kept": int(kept.sum()), "total": int(len(kept)), "views": int(len(cams)), **counts,
                          seconds_key: seconds}), flush=True)
    return 0
