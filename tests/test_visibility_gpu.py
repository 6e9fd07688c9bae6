"""neat_amd.visibility.visible at its edges, through both tools that stand on it: no camera, no target, one sample (visible_points), and
two samples of one segment from one camera.  raycast against tests/raycast_f64.py on the icosphere of level 1, trace against
tests/trace_f64.py on the analytic sphere of radius 0.5 inside the bounding sphere of radius 1; the boolean arrays are equal.  Every
target is chosen so that its ray passes the surface's silhouette, and ends before or behind the surface, by at least 0.05."""
import numpy as np
import pytest
import torch

from tests import raycast_f64 as RC
from tests import trace_f64 as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIAS = 0.01
RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
CENTRES = np.array([[0.0, 0.0, -2.0], [1.5, 0.5, -1.0]])
# per occluder: a target in front of it, behind it, inside it, and one that neat_trace_target_rays refuses for the first camera or for
# both (raycast: nearer to the first centre than the bias; trace: outside the bounding sphere), with what each camera sees of them
TARGETS = {"raycast": np.array([[0.0, 0.0, -1.5], [0.0, 0.0, 1.5], [0.0, 0.0, 0.0], [0.005, 0.0, -2.0]], dtype=np.float32),
           "trace": np.array([[0.0, 0.0, -0.8], [-0.5, -0.25, 0.75], [0.0, 0.0, 0.0], [0.9, 0.9, 0.0]], dtype=np.float32)}
SEEN = {"raycast": [[True, False, False, False], [True, False, False, True]], "trace": [[True, False, False, False]] * 2}


def _cams():
    cams = np.stack([np.eye(4)] * 2)
    cams[0, :3, 3] = -CENTRES[0]
    cams[1, :3, :3], cams[1, :3, 3] = RZ, -RZ @ CENTRES[1]
    return cams


def _rays(points):
    """Every camera to every point [N,3] -> (origins, dirs [F N,3], length [F N]) in float64, from the float32 values the device is given."""
    c = CENTRES.astype(np.float32).astype(np.float64)
    v = (points.astype(np.float64)[None] - c[:, None]).reshape(-1, 3)
    L = np.linalg.norm(v, axis=1)
    return np.repeat(c, len(points), 0), v / L[:, None], L


def _clear(o, d, t_end, r_in, r_out):
    """The segment o + t d, 0 <= t <= t_end, stays 0.05 outside the sphere of r_out or reaches 0.05 inside that of r_in."""
    t = np.clip(-(o * d).sum(-1), 0.0, np.maximum(t_end, 0.0))
    m = np.linalg.norm(o + t[:, None] * d, axis=1)
    return (m > r_out + 0.05) | (m < r_in - 0.05)


@pytest.fixture(scope="module")
def mesh():
    verts, faces = RC.icosphere(1)
    tv = verts[faces]
    n = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    r_in = float(np.abs((n * tv[:, 0]).sum(-1) / np.linalg.norm(n, axis=1)).min())            # the nearest face plane
    return verts, faces, r_in


def _reference(tool, points, mesh):
    """bool [F, N]: the float64 rule of the tool's occluder, and what neat_trace_target_rays refuses."""
    o, d, L = _rays(points)
    t_end = L - BIAS
    if tool == "raycast":
        assert _clear(o, d, t_end, mesh[2], 1.0)[L > 0.1].all()
        free = np.isinf(RC.cast_all(mesh[0], mesh[1], o, d, t_max=np.maximum(t_end, 0.0))[0])
        ok = L > BIAS
    else:
        inside = np.tile(np.linalg.norm(points.astype(np.float64), axis=1) <= 1.0, len(CENTRES))
        ok = inside & (L > BIAS)
        assert _clear(o, d, t_end, 0.5, 0.5)[ok].all()
        free = T.trace(T.np_field("sphere"), o, d, radius=1.0, t_end=t_end)["state"] == T.MISS
    return (free & ok).reshape(len(CENTRES), len(points))


def _tool(tool, mesh):
    """-> (module, occluder, the keywords of its visible_* calls)."""
    if tool == "raycast":
        from neat_amd import raycast
        return raycast, raycast.build(mesh[0], mesh[1], DEV), {}
    from neat_amd import trace
    return trace, T.torch_field("sphere"), {"radius": 1.0}


@pytest.mark.parametrize("tool", ["raycast", "trace"])
def test_edges_of_the_shared_visibility(tool, mesh):
    mod, occluder, kw = _tool(tool, mesh)
    cams, pts = _cams(), TARGETS[tool]
    dev_pts = torch.from_numpy(pts).to(DEV)
    want = _reference(tool, pts, mesh)
    print("  %s: reference\n%s" % (tool, want.astype(int)))
    assert want.tolist() == SEEN[tool]                                    # the cases are what they are named
    # samples = 1: visible_points
    seen = mod.visible_points(occluder, dev_pts, cams, bias=BIAS, **kw)
    assert seen.dtype == torch.bool and np.array_equal(seen.cpu().numpy(), want)
    # F = 0 and N = 0, points and segments
    none = np.zeros((0, 4, 4))
    for got, shape, dtype in ((mod.visible_points(occluder, dev_pts, none, bias=BIAS, **kw), (0, len(pts)), torch.bool),
                              (mod.visible_points(occluder, dev_pts[:0], cams, bias=BIAS, **kw), (2, 0), torch.bool),
                              (mod.visible_lines(occluder, dev_pts[:2][None], none, samples=2, bias=BIAS, **kw), (0, 1), torch.float32),
                              (mod.visible_lines(occluder, dev_pts[:0].reshape(0, 2, 3), cams, samples=2, bias=BIAS, **kw), (2, 0), torch.float32)):
        assert tuple(got.shape) == shape and got.dtype == dtype and got.device.type == "cuda"
    # samples = 2, N = 1, F = 1: the segment from the target in front to the one behind, its two ends
    march = (BIAS,) if tool == "raycast" else (BIAS, kw["radius"], {})
    both = mod._visible(occluder, dev_pts[:2][None], cams[:1], 2, *march)
    assert both.shape == (1, 1, 2) and both.dtype == torch.bool and np.array_equal(both.cpu().numpy(), want[:1, :2][:, None])
    frac = mod.visible_lines(occluder, dev_pts[:2][None], cams[:1], samples=2, bias=BIAS, **kw)
    assert frac.cpu().tolist() == [[0.5]]
