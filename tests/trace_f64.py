"""Float64 restatement of the sphere tracing of neat_amd/csrc/kernels_trace.hpp, analytic fields with the closed forms of
their first intersections, and the ray fans the tests trace.  Not a test file: tests/test_trace_math.py checks the model against the
closed forms on the CPU, tests/test_trace_gpu.py the kernels against the model.

The bound on a HIT's depth against the closed-form first intersection t* (derived, evaluated per ray by depth_bound):
  * a run stops with 0 <= f(t) < eps at a point before the surface, or, its refinement rounds used up, at the `a` end of its last
    bracket [a, b], which contains t*: then 0 <= t* - a <= b - a = wfin, the width the float64 model itself ends with (0 for a ray
    that stopped on f < eps).  No round of the method is guaranteed to halve a bracket (only bisection is), so the term is the width
    that was reached, not w0 / 2^refine_steps; tests/test_trace_math.py asserts that at the default 8 rounds it is never above that
    figure on any scene (there it is 0: every refined ray stops on f < eps), and checks the bound on brackets left open at 2 rounds;
  * every field here is convex along a ray up to its first hit (a distance to a convex set, scaled; for the union, the hit sphere's own
    field bounds the minimum from above and is convex), so f(t) >= c (t* - t) with c = |grad f . d| at the hit, the slope of the tangent
    there: f(t) < eps gives t* - t < eps / c.  For a field with |grad f| = 1 this c is |n . d|;
  * the fp32 run evaluates the field and the points in fp32: 8 ulp32(t_out) covers the rounding of t, of o + t d and of the clamp.
  |t - t*| <= eps / c + wfin + 8 ulp32(t_out)
"""
import numpy as np

MISS, HIT, INSIDE, UNCONVERGED = 0, 1, 2, 3
RADIUS = 1.0
BOX = np.array([0.3, 0.4, 0.25])
TWO = np.array([[-0.3, 0.0, 0.0], [0.3, 0.0, 0.0]])


# ------------------------------------------------------------------ fields: numpy float64 and float32 torch, the same formulas
def _norm(xp, p):
    return xp.sqrt((p * p).sum(-1))


def sphere(xp, p, scale=1.0):
    return scale * (_norm(xp, p) - 0.5)


def two_spheres(xp, p):
    ca, cb = (xp.asarray(c, dtype=p.dtype) if xp is np else xp.tensor(c, dtype=p.dtype, device=p.device) for c in TWO)
    return xp.minimum(_norm(xp, p - ca), _norm(xp, p - cb)) - 0.25


def box(xp, p):
    h = xp.asarray(BOX, dtype=p.dtype) if xp is np else xp.tensor(BOX, dtype=p.dtype, device=p.device)
    q = xp.abs(p) - h
    if xp is np:
        return _norm(xp, np.maximum(q, 0.0)) + np.minimum(q.max(-1), 0.0)
    return _norm(xp, xp.clamp(q, min=0.0)) + xp.clamp(q.max(-1).values, max=0.0)


FIELDS = {
    # near-grazing rays take more than 64 steps of an exact SDF (the step is the clearance): the sphere's fan leaves them out, the box's
    # fan keeps them and relies on the exclusions
    "sphere": dict(f=lambda xp, p: sphere(xp, p), grad=1.0, bands=((0.0, 0.45), (0.55, 1.2))),
    # ... and the two spheres' fan leaves out the rays that pass either sphere's surface within 0.02 (fan's `clear`): one that grazes the
    # first sphere and then hits the second runs out of steps in front of the first
    "two_spheres": dict(f=two_spheres, grad=1.0, bands=((0.0, 1.2),), clear=tuple((tuple(c), 0.25, 0.02) for c in TWO.tolist())),
    "box": dict(f=box, grad=1.0, bands=((0.0, 1.2),)),
    # 2 x the sphere: not an SDF, the march overshoots into a bracket.  Its fan keeps clear of impact parameters 0.4 .. 0.6, where an
    # overshoot can cross the whole sphere (what an inexact field does to any sphere tracer, not a matter of precision)
    "sphere_x2": dict(f=lambda xp, p: sphere(xp, p, 2.0), grad=2.0, bands=((0.0, 0.4), (0.6, 1.2))),
    # 0.5 x the sphere: under-steps; the same fan keeps a ray's number of steps clear of max_steps
    "sphere_half": dict(f=lambda xp, p: sphere(xp, p, 0.5), grad=0.5, bands=((0.0, 0.4), (0.6, 1.2))),
}


def np_field(name):
    f = FIELDS[name]["f"]
    return lambda p: f(np, np.asarray(p, dtype=np.float64))


def torch_field(name):
    """The field in float32 torch on the points' device (what the stepping kernels are tested with)."""
    import torch
    f = FIELDS[name]["f"]
    return lambda p: f(torch, p.float())


# ------------------------------------------------------------------ closed forms
def _sphere_hit(o, d, centre, r, t0, t1):
    oc = o - centre
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - r * r)
    sq = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(-b - sq >= t0, -b - sq, -b + sq)            # the first root on [t0, t1] (the start is outside the surface)
    ok = (disc > 0) & (t >= t0) & (t <= t1)
    n = (oc + t[:, None] * d) / r
    return np.where(ok, t, np.nan), np.abs((n * d).sum(-1))


def _box_hit(o, d, t0, t1):
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-BOX - o) / d, (BOX - o) / d
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    lo, hi = np.where(np.isnan(lo), -np.inf, lo), np.where(np.isnan(hi), np.inf, hi)
    tin, tout = lo.max(-1), hi.min(-1)
    ok = (tin <= tout) & (tin >= t0) & (tin <= t1)
    c = np.abs(d[np.arange(len(d)), lo.argmax(-1)])
    return np.where(ok, tin, np.nan), c


def first_hit(name, o, d, t0, t1):
    """-> (t* float64 [R], NaN where the ray does not meet the surface on [t0, t1]; c = |grad f . d| at the hit)."""
    if name == "two_spheres":
        hits = [_sphere_hit(o, d, c, 0.25, t0, t1) for c in TWO]
        ts = np.stack([np.where(np.isnan(h[0]), np.inf, h[0]) for h in hits])
        k = ts.argmin(0)
        t = ts.min(0)
        return np.where(np.isfinite(t), t, np.nan), np.where(k == 0, hits[0][1], hits[1][1])
    if name == "box":
        return _box_hit(o, d, t0, t1)
    t, c = _sphere_hit(o, d, np.zeros(3), 0.5, t0, t1)
    return t, FIELDS[name]["grad"] * c


def chord(o, d, radius=RADIUS, near=0.0, t_end=None):
    """The kernel's set-up: float64 arithmetic, both ends rounded to fp32 -> (t0, t1, alive)."""
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - radius * radius)
    sq = np.sqrt(np.maximum(disc, 0.0))
    lo, hi = np.maximum(-b - sq, near), -b + sq
    if t_end is not None:
        e = np.asarray(t_end, dtype=np.float64)
        hi = np.where((e < hi) | np.isnan(e), e, hi)
    t0, t1 = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return t0, t1, (disc > 0) & (t0 < t1)


# ------------------------------------------------------------------ the state machine
def _refine_point(ta, fa, tb, fb):
    w = tb - ta
    s = ta + w * (fa / (fa - fb))
    return np.minimum(np.maximum(s, ta + 0.05 * w), tb - 0.05 * w)


def trace(field, o, d, radius=RADIUS, t_end=None, eps=1e-4, relax=1.0, max_steps=64, refine_steps=8, near=0.0):
    """field: points float64 [n,3] -> values [n].  -> dict(state, depth (NaN unless HIT or INSIDE), steps, evals, lists = the active ray
    ids of every iteration (ascending), w0 = the first width of a ray's bracket (0: it never bracketed), t0, t1)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    R = len(o)
    t0, t1, alive = chord(o, d, radius, near, t_end)
    START, MARCH, REFINE = 4, 5, 6
    phase = np.where(alive, START, MISS)
    t, ta, fa, tb, fb, w0 = t0.copy(), t0.copy(), np.zeros(R), t0.copy(), np.zeros(R), np.zeros(R)
    steps, march, refine, side = np.zeros(R, int), np.zeros(R, int), np.zeros(R, int), np.zeros(R, int)
    wfin = np.zeros(R)
    lists = []
    while True:
        ids = np.nonzero(phase >= START)[0]
        if len(ids) == 0:
            break
        lists.append(ids)
        vals = field(o[ids] + t[ids, None] * d[ids])
        for r, f in zip(ids, vals):
            steps[r] += 1
            if f != f:
                phase[r] = UNCONVERGED
                continue
            if phase[r] == START:
                if f < 0:
                    phase[r] = INSIDE
                    continue
                phase[r] = MARCH
            if phase[r] == MARCH:
                if 0 <= f < eps:
                    phase[r] = HIT
                elif f < 0:
                    w0[r] = t[r] - ta[r]
                    if refine_steps <= 0:
                        t[r], phase[r] = ta[r], HIT
                        continue
                    tb[r], fb[r], refine[r], side[r], phase[r] = t[r], f, 0, 0, REFINE
                    t[r] = _refine_point(ta[r], fa[r], tb[r], fb[r])
                elif t[r] >= t1[r]:
                    phase[r] = MISS
                elif march[r] >= max_steps:
                    phase[r] = UNCONVERGED
                else:
                    march[r] += 1
                    ta[r], fa[r] = t[r], f
                    t[r] = min(t[r] + relax * f, t1[r])
                continue
            if f >= 0:
                if f < eps:
                    phase[r] = HIT
                    continue
                ta[r], fa[r] = t[r], f
                if side[r] == 1:
                    fb[r] *= 0.5
                side[r] = 1
            else:
                tb[r], fb[r] = t[r], f
                if side[r] == 2:
                    fa[r] *= 0.5
                side[r] = 2
            refine[r] += 1
            if refine[r] >= refine_steps:
                t[r], phase[r], wfin[r] = ta[r], HIT, tb[r] - ta[r]
                continue
            t[r] = _refine_point(ta[r], fa[r], tb[r], fb[r])
    has = (phase == HIT) | (phase == INSIDE)
    return dict(state=phase.astype(np.uint8), depth=np.where(has, t, np.nan), steps=steps, evals=int(steps.sum()), lists=lists, w0=w0,
                wfin=wfin, t0=t0, t1=t1)


# ------------------------------------------------------------------ fans, exclusions, the bound
def fan(n, seed, bands=((0.0, 1.2),), dist=2.0, clear=()):
    """n rays as float32 (origins [n,3], unit dirs [n,3]) from origins at distance `dist` of the centre, with impact parameters drawn
    evenly from `bands` (above RADIUS: the ray misses the bounding sphere).  clear = ((centre, radius, margin), ...): candidates whose
    line passes one of these spheres' surfaces within `margin` are left out (decided by the geometry alone, before any tracing)."""
    if clear:
        o, d = fan(3 * n, seed, bands, dist)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        ok = np.ones(len(o), bool)
        for centre, radius, margin in clear:
            oc = o64 - np.asarray(centre)
            impact = np.linalg.norm(oc - (oc * d64).sum(-1, keepdims=True) * d64, axis=1)
            ok &= np.abs(impact - radius) >= margin
        assert ok.sum() >= n
        return o[ok][:n], d[ok][:n]
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.standard_normal((n, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    which = rng.integers(len(bands), size=n)
    lo, hi = np.asarray(bands)[which].T
    s = rng.uniform(lo, hi) / dist                              # the sine of the angle off the line to the centre
    d = -np.sqrt(1.0 - s * s)[:, None] * u + s[:, None] * v
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (dist * u).astype(np.float32), d.astype(np.float32)


def scene(name, n=1025, seed=11):
    """The fan of a field's scene."""
    return fan(n, seed, FIELDS[name]["bands"], clear=FIELDS[name].get("clear", ()))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def judge(name, o, d, model, eps=1e-4, refine_steps=8, samples=2049):
    """The float64 side of a scene: the closed-form first hits, the exclusions (decided here alone) and the depth bound per ray.
    excluded: a hit with c < 0.1 where c = |n . d|, the cosine at the hit (|grad f . d| / |grad f|); a closed-form miss whose float64
    field goes below 10 eps somewhere on the clipped chord."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    t0, t1 = model["t0"], model["t1"]
    _, _, alive = chord(o, d)
    alive = alive & (t0 < t1)
    tstar, c = first_hit(name, o, d, t0, t1)
    tstar = np.where(alive, tstar, np.nan)
    hit = ~np.isnan(tstar)
    f = np_field(name)
    excluded = hit & (c / FIELDS[name]["grad"] < 0.1)
    miss = np.nonzero(alive & ~hit)[0]
    if len(miss):
        s = np.linspace(0.0, 1.0, samples)
        tt = t0[miss, None] + s[None] * (t1[miss] - t0[miss])[:, None]
        fmin = f(o[miss, None] + tt[..., None] * d[miss, None]).min(-1)
        excluded[miss] = fmin < 10 * eps
    tout = np.where(np.isfinite(t1), t1, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = eps / c + model["wfin"] + 8 * np.array([ulp32(x) for x in tout])
    return dict(tstar=tstar, c=c, hit=hit, alive=alive, excluded=excluded, bound=bound)
