"""neat_amd.trace on the device: the stepping kernels with analytic fields (evaluated in float32 torch on the device) against the
float64 model and the closed forms of tests/trace_f64.py, and the network routes (view, visible_points, visible_lines) on the synthetic
model at its geometric initialisation."""
import numpy as np
import pytest
import torch

from neat_amd import trace
from tests import trace_f64 as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, REFINE, MAX_STEPS = 1e-4, 8, 64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(name, o, d, **kw):
    rec = []
    kw.setdefault("radius", T.RADIUS)
    if "t_end" in kw and kw["t_end"] is not None:
        kw["t_end"] = _t(np.asarray(kw["t_end"], dtype=np.float32))
    field = T.torch_field(name) if isinstance(name, str) else name
    depth, state, steps, points, evals = trace.rays(field, _t(o), _t(d), record=rec, **kw)
    return dict(depth=depth.cpu().numpy(), state=state.cpu().numpy(), steps=steps.cpu().numpy(), points=points.cpu().numpy(), evals=evals,
                lists=[(r0, ids.cpu().numpy()) for r0, ids in rec])


_scenes = {}


def _scene(name):
    """The scene's fan, its float64 model and judgement (computed once, shared, never changed)."""
    if name not in _scenes:
        o, d = T.scene(name)
        m = T.trace(T.np_field(name), o, d, eps=EPS, refine_steps=REFINE, max_steps=MAX_STEPS)
        _scenes[name] = (o, d, m, T.judge(name, o, d, m, EPS, REFINE))
    return _scenes[name]


def _accounting(g, max_steps=MAX_STEPS, refine_steps=REFINE):
    # evals = the sum of the active counts the host saw = steps.sum(): no fixed extra
    assert g["evals"] == sum(len(ids) for _, ids in g["lists"]) == int(g["steps"].sum())
    assert (g["steps"] <= 1 + max_steps + refine_steps).all() and (g["steps"] >= 0).all()
    for _, ids in g["lists"]:
        assert (np.diff(ids) > 0).all()                                   # ray order, no ray twice
    for (_, a), (_, b) in zip(g["lists"], g["lists"][1:]):
        assert np.isin(b, a).all()                                        # a finished ray is in no later query
    has = (g["state"] == T.HIT) | (g["state"] == T.INSIDE)
    assert np.isnan(g["depth"][~has]).all() and np.isfinite(g["depth"][has]).all()
    assert np.isnan(g["points"][~has]).all() and np.isfinite(g["points"][has]).all()


@pytest.mark.parametrize("name", sorted(T.FIELDS))
def test_states_and_depths_against_the_model_and_the_closed_forms(name):
    o, d, m, j = _scene(name)                                            # 1025 rays: hit and miss mixed, five workgroups
    g = _run(name, o, d)
    _accounting(g)
    keep = ~j["excluded"]
    assert j["excluded"].mean() <= 0.02
    differ = g["state"] != m["state"]
    print("%s: %d rays, %d excluded, states %s, evaluations %d (model %d), states differing from the model: %d (%d not excluded)" % (
        name, len(o), j["excluded"].sum(), np.bincount(g["state"], minlength=4).tolist(), g["evals"], m["evals"], differ.sum(), (differ & keep).sum()))
    assert np.array_equal(g["state"][keep], m["state"][keep])
    h = keep & j["hit"]
    err = np.abs(g["depth"][h].astype(np.float64) - j["tstar"][h])
    print("  worst depth error / bound: %.3g; worst error %.3g" % ((err / j["bound"][h]).max(), err.max()))
    assert (err <= j["bound"][h]).all()
    # the hit points are o + depth d
    p = o[h].astype(np.float64) + g["depth"][h, None].astype(np.float64) * d[h].astype(np.float64)
    assert np.abs(g["points"][h] - p).max() <= 4 * T.ulp32(2.0)
    assert (g["steps"][~j["alive"]] == 0).all()
    # the first list is the set-up's alone (float64 in both): the same rays; later ones may part where fp32 crosses eps a step apart
    assert np.array_equal(g["lists"][0][1], m["lists"][0])


@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 257, 1025])
def test_ray_counts_and_determinism(R):
    o, d = T.fan(max(R, 1), 5, ((0.0, 0.4),))
    o2, d2 = T.fan(max(R, 1), 6, ((0.6, 1.2),))
    o, d = o[:R].copy(), d[:R].copy()
    o[1::2], d[1::2] = o2[:R][1::2], d2[:R][1::2]                         # hit and miss rays alternate: the compaction crosses workgroups
    g = _run("sphere_x2", o, d)
    _accounting(g)
    assert g["state"].shape == (R,) and g["points"].shape == (R, 3)
    assert (g["state"][0::2] == T.HIT).all() and (g["state"][1::2] == T.MISS).all()
    if R:
        m = T.trace(T.np_field("sphere_x2"), o, d)
        assert np.array_equal(g["state"], m["state"])
    again = _run("sphere_x2", o, d)
    for k in ("depth", "state", "steps", "points"):
        assert g[k].tobytes() == again[k].tobytes(), k
    assert g["evals"] == again["evals"] and len(g["lists"]) == len(again["lists"])
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(g["lists"], again["lists"]))
    # in chunks: the same per-ray results, the same number of evaluations
    if R > 64:
        parts = _run("sphere_x2", o, d, chunk=100)
        for k in ("depth", "state", "steps", "points"):
            assert g[k].tobytes() == parts[k].tobytes(), k
        assert parts["evals"] == g["evals"] and {r0 for r0, _ in parts["lists"]} == set(range(0, R, 100))


def test_scan_carry_past_1024_tiles_equals_two_single_round_halves():
    """262 145 rays are 1025 workgroups of 256, so the one workgroup of 1024 that turns their counts into offsets (trace_scan_kernel) takes
    a second round with a carry, which no other test here reaches.  Traced as two halves (513 and 512 workgroups: one round each, the path
    judged against float64 above) every ray must come out with the same bits."""
    R = 1024 * 256 + 1
    o, d = T.scene("sphere", n=R, seed=3)
    o[-1], d[-1] = (0.0, 0.0, -2.0), (0.0, 0.0, 1.0)                      # the one ray of the last workgroup is alive: it hits head-on
    g = _run("sphere", o, d)
    parts = _run("sphere", o, d, chunk=R // 2 + 1)
    assert {r0 for r0, _ in parts["lists"]} == {0, R // 2 + 1} and {r0 for r0, _ in g["lists"]} == {0}
    for k in ("depth", "state", "steps", "points"):
        assert g[k].tobytes() == parts[k].tobytes(), k
    assert g["evals"] == parts["evals"] == int(g["steps"].sum())
    assert g["lists"][0][1][-1] == R - 1 and g["state"][-1] == T.HIT and abs(float(g["depth"][-1]) - 1.5) < 1e-3
    assert (g["state"] == T.HIT).sum() > R // 4 and (g["state"] == T.MISS).sum() > R // 4
    for _, ids in g["lists"]:
        assert (np.diff(ids) > 0).all()                                   # ray order across the carry, no ray twice


def test_state_cases():
    n = 300
    o, d = T.fan(n, 3, ((0.0, 0.3),))
    tstar, _ = T.first_hit("sphere", o.astype(np.float64), d.astype(np.float64), 0.0, np.inf)
    # every ray misses the bounding sphere: no evaluation at all
    o2, d2 = T.fan(n, 4, ((1.05, 1.5),))
    calls = []
    g = _run(lambda p: calls.append(len(p)) or T.torch_field("sphere")(p), o2, d2)
    assert (g["state"] == T.MISS).all() and g["evals"] == 0 and calls == [] and (g["steps"] == 0).all()
    # every ray starts inside: INSIDE at the start of the chord, one evaluation each
    g = _run("sphere", 0.1 * o, d)
    assert (g["state"] == T.INSIDE).all() and (g["depth"] == 0).all() and g["evals"] == n and (g["steps"] == 1).all()
    # t_end in front of the surface / behind it / at the fp32 value next above it
    g = _run("sphere", o, d, t_end=tstar - 0.05)
    _accounting(g)
    assert (g["state"] == T.MISS).all()
    g = _run("sphere", o, d, t_end=tstar + 0.05)
    assert (g["state"] == T.HIT).all() and np.abs(g["depth"] - tstar).max() < 2e-4
    g = _run("sphere", o, d, t_end=np.nextafter(tstar.astype(np.float32), np.float32(np.inf)))
    assert (g["state"] == T.HIT).all() and np.abs(g["depth"] - tstar).max() < 2e-4
    # near beyond the end of the chord: an empty interval is a MISS without a query
    g = _run("sphere", o, d, near=10.0)
    assert (g["state"] == T.MISS).all() and g["evals"] == 0
    # the under-stepping field at a small max_steps
    g = _run("sphere_half", o, d, max_steps=4)
    _accounting(g, max_steps=4)
    assert (g["state"] == T.UNCONVERGED).all() and (g["steps"] == 5).all()
    # a NaN from the field
    g = _run(lambda p: torch.full((len(p),), float("nan"), device=p.device), o, d)
    assert (g["state"] == T.UNCONVERGED).all() and (g["steps"] == 1).all()
    # refine_steps = 0, and a relaxed march
    g = _run("sphere_x2", o, d, refine_steps=0)
    assert (g["state"] == T.HIT).all() and (g["depth"] < tstar).all()
    g = _run("sphere", o, d, relax=0.5)
    m = T.trace(T.np_field("sphere"), o, d, relax=0.5)
    assert np.array_equal(g["state"], m["state"]) and (g["state"] == T.HIT).all() and np.abs(g["depth"] - tstar).max() < 2e-4


def test_target_rays_and_visibility_with_an_analytic_field():
    from neat_amd import ops
    rng = np.random.default_rng(2)
    pts = rng.uniform(-0.9, 0.9, (37, 3)).astype(np.float32)
    pts[0] = [0.99, 0.99, 0.0]                                            # outside the bounding sphere
    cams = np.stack([np.eye(4)] * 3)
    cams[0, :3, 3], cams[1, :3, 3] = [0.0, 0.0, 2.0], [0.3, -0.2, 1.8]    # centres -t for R = 1
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cams[2, :3, :3], cams[2, :3, 3] = Rz, -Rz @ np.array([1.5, 0.5, -1.0])
    c = trace.camera_centres(cams)
    assert np.allclose(c, [[0, 0, -2.0], [-0.3, 0.2, -1.8], [1.5, 0.5, -1.0]])
    o, d, t_end, ok = ops.trace_target_rays(_t(c.astype(np.float32)), _t(pts), 1, 1.0, 0.0, 0.01)
    v = pts[None].astype(np.float64) - c.astype(np.float32).astype(np.float64)[:, None]
    L = np.linalg.norm(v, axis=-1)
    assert np.array_equal(o.cpu().numpy().reshape(3, 37, 3), np.broadcast_to(c.astype(np.float32)[:, None], (3, 37, 3)))
    assert np.abs(d.cpu().numpy().reshape(3, 37, 3) - v / L[..., None]).max() <= 2.0 ** -24
    assert np.abs(t_end.cpu().numpy().reshape(3, 37).astype(np.float64) - (L - 0.01)).max() <= T.ulp32(4.0)      # one fp32 rounding of a length under 4
    inside = np.linalg.norm(pts.astype(np.float64), axis=1) <= 1.0
    assert not inside[0] and np.array_equal(ok.cpu().numpy().reshape(3, 37) != 0, np.broadcast_to(inside, (3, 37)))
    # visibility past the sphere of radius 0.5: the closed form decides, away from the silhouette
    seen = trace.visible_points(T.torch_field("sphere"), _t(pts), cams, radius=1.0).cpu().numpy()
    o64, d64 = np.repeat(c.astype(np.float32).astype(np.float64), 37, 0), (v / L[..., None]).reshape(-1, 3)
    tstar, _ = T.first_hit("sphere", o64, d64, 0.0, np.inf)
    blocked = (tstar < (L.reshape(-1) - 0.01)).reshape(3, 37)
    oc = np.linalg.norm(np.cross(o64, d64), axis=1).reshape(3, 37)        # the line's distance to the centre
    with np.errstate(invalid="ignore"):
        clear = (np.abs(oc - 0.5) > 0.01) & ~(np.abs(tstar.reshape(3, 37) - (L - 0.01)) < 1e-3)      # and away from a target at the surface
    expect = ~blocked & inside[None] & (np.linalg.norm(pts, axis=1) > 0.5)[None]
    assert clear.mean() > 0.9 and np.array_equal(seen[clear], expect[clear]) and seen.any() and not seen.all()
    # segments: 16 samples, the fraction of them seen
    lines = np.stack([pts[1:19], pts[19:37]], 1)
    frac = trace.visible_lines(T.torch_field("sphere"), _t(lines), cams, radius=1.0).cpu().numpy()
    s = np.linspace(0.0, 1.0, 16)
    samples = lines[:, None, 0].astype(np.float64) + s[None, :, None] * (lines[:, None, 1].astype(np.float64) - lines[:, None, 0])
    per = trace.visible_points(T.torch_field("sphere"), _t(samples.reshape(-1, 3).astype(np.float32)), cams, radius=1.0).cpu().numpy()
    assert frac.shape == (3, 18) and np.abs(frac - per.reshape(3, 18, 16).mean(-1)).max() <= 1.0 / 16 + 1e-6
    assert trace.visible_points(T.torch_field("sphere"), _t(pts[:0]), cams, radius=1.0).shape == (3, 0)


# ------------------------------------------------------------------ the network
@pytest.fixture(scope="module", params=["fp32", None])
def net_view(request):
    """The synthetic-conf model at its geometric initialisation (a sphere-like surface), a 48 x 64 view from outside."""
    from neat_amd import synth
    from tests.util_run import synth_init_model
    model = synth_init_model().to(DEV).eval()
    if request.param is not None:
        model.set_precision(request.param)
    H, W = 48, 64
    sc = synth.synth_scene(seed=1, n_rays=4, res=64, view=1)
    pose = torch.tensor(sc["pose"][0]).to(DEV)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 70.0
    K[0, 2], K[1, 2] = W / 2, H / 2
    timings = {}
    depth, normal, state = trace.view(model, pose, K.to(DEV), H, W, timings=timings)
    return dict(model=model, pose=pose, K=K.to(DEV), H=H, W=W, depth=depth, normal=normal, state=state, timings=timings, prec=request.param)


def _raw_sdf(model, pts):
    from neat_amd import ops
    net = model.implicit_network
    return ops.sdf_values(net.handle(), pts.contiguous(), 0.0, net.sphere_scale).view(-1)


def _view_rays(v):
    from neat_amd import ops
    from neat_amd.render import pixel_grid
    dirs, _, origins = ops.camera_rays(pixel_grid(v["H"], v["W"], torch.device(DEV))[None], v["pose"][None], v["K"][None], with_origins=True)
    return origins, dirs.reshape(-1, 3)


def test_view_hits_lie_on_the_raw_zero_level_and_misses_see_no_surface(net_view):
    v = net_view
    net = v["model"].implicit_network
    state, depth = v["state"].reshape(-1), v["depth"].reshape(-1)
    hit, miss = state == trace.HIT, state == trace.MISS
    counts = torch.bincount(state.long(), minlength=4).tolist()
    print("%s: states %s, %d evaluations for %d rays (%.1f per ray), %.3f s" % (v["prec"] or "default", counts, v["timings"]["evals"],
                                                                              v["timings"]["rays"], v["timings"]["evals"] / v["timings"]["rays"],
                                                                              v["timings"]["trace_s"]))
    assert hit.sum() > 200 and miss.sum() > 200 and counts[trace.UNCONVERGED] <= 0.02 * state.numel()
    origins, dirs = _view_rays(v)
    pts = origins[hit] + depth[hit, None] * dirs[hit]
    f = _raw_sdf(v["model"], pts)
    print("  |raw sdf| at the hits: max %.3g" % f.abs().max().item())
    assert (f.abs() < EPS).all()
    # the unclamped field is what was traced: radius 0 differs from the clamped query outside the sphere's shell
    from neat_amd import ops
    far = origins[:1] * 0 + torch.tensor([[0.0, 0.0, net.sdf_bounding_sphere - 1e-3]], device=DEV)
    assert ops.sdf_values(net.handle(), far, net.sdf_bounding_sphere, net.sphere_scale).item() < _raw_sdf(v["model"], far).item()
    # a MISS: the raw SDF is positive at 256 even samples of the clipped chord
    r = float(net.sdf_bounding_sphere)
    o64, d64 = origins[miss].double(), dirs[miss].double()
    b = (o64 * d64).sum(-1)
    disc = b * b - ((o64 * o64).sum(-1) - r * r)
    inside = disc > 0
    sq = disc.clamp(min=0).sqrt()
    t0, t1 = (-b - sq).clamp(min=0.0), -b + sq
    s = torch.linspace(0.0, 1.0, 256, device=DEV, dtype=torch.float64)
    tt = (t0[inside, None] + s[None] * (t1 - t0)[inside, None]).float()
    p = origins[miss][inside][:, None] + tt[..., None] * dirs[miss][inside][:, None]
    assert inside.sum() > 100 and (_raw_sdf(v["model"], p.reshape(-1, 3)) > 0).all()
    # normals: unit at the hits, zero elsewhere; depth NaN exactly off the hits
    n = v["normal"].reshape(-1, 3)
    assert (n[hit].norm(dim=1) - 1).abs().max() < 1e-5 and (n[~hit] == 0).all()
    assert torch.isfinite(depth[hit]).all() and torch.isnan(depth[miss]).all()
    # towards the camera: the surface faces the ray
    assert ((n[hit] * dirs[hit]).sum(-1) < 0).float().mean() > 0.99


def test_visibility_on_both_sides_of_the_traced_surface(net_view):
    """Every HIT pixel of the view, without exclusion (on the initial surface even the silhouette pixels pass: 2 bias along the ray
    in front of a hit leaves f far above eps, and the ray towards the point behind it meets the same first hit before its end)."""
    v = net_view
    bias = 0.01
    state, depth = v["state"].reshape(-1), v["depth"].reshape(-1)
    origins, dirs = _view_rays(v)
    idx = torch.nonzero(state == trace.HIT).flatten()
    front = origins[idx] + (depth[idx] - 2 * bias)[:, None] * dirs[idx]
    back = origins[idx] + (depth[idx] + 2 * bias)[:, None] * dirs[idx]
    cam = torch.linalg.inv(v["pose"].double())[None].cpu().numpy()
    seen_front = trace.visible_points(v["model"], front, cam, bias=bias)[0]
    seen_back = trace.visible_points(v["model"], back, cam, bias=bias)[0]
    frac = trace.visible_lines(v["model"], torch.stack([front, back], 1), cam, bias=bias)[0]
    between = (frac > 0) & (frac < 1)
    print("%s: %d hits: front not seen %d, back seen %d, fraction not strictly between 0 and 1: %d"
          % (v["prec"] or "default", idx.numel(), (~seen_front).sum(), seen_back.sum(), (~between).sum()))
    assert idx.numel() > 200
    assert seen_front.all()
    assert not seen_back.any()
    assert frac.shape == (idx.numel(),) and between.all()
