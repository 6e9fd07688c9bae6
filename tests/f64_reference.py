"""Float64 reference for the kernel tests: the CPU oracle's own functions (oracle/neat_oracle.py) run on float64 parameters and
float64 copies of the float32 inputs the kernels see.  Nothing here restates the math; a float64 run only removes the oracle's own
rounding from what a test measures (a float32 oracle's sums over 10^4 points are wrong by ~1e-6 of their scale themselves).

References are cached at module scope by key, so that every build is compared with the same float64 tensors and the CPU work is
done once per pytest process."""
import torch

from neat_amd import synth
from oracle import neat_oracle as O

F64 = torch.float64
RADIUS, SCALE = 3.0, 20.0          # scene_bounding_sphere, implicit_network.sphere_scale of synth.ABC_NEAT_A_MODEL_CONF
BETA_MIN = synth.ABC_NEAT_A_MODEL_CONF["density"]["beta_min"]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def params(seed, variant, requires_grad=False, dtype=F64):
    """synth.synth_state_dict(seed, variant) as float64 oracle parameters (a fresh dict: gradients do not leak between references)."""
    return O.params_from_numpy(synth.synth_state_dict(seed, variant), requires_grad=requires_grad, dtype=dtype)


def f64(t, dtype=F64):
    return t.detach().cpu().to(dtype)


def sdf_forward(p, x):
    """Every forward of the SDF network at the points x (float32, any device), float64, no autograd graph kept:
    forward [P,257], get_sdf_vals [P,1], get_outputs (sdf, feature, clamped gradient), gradient (raw)."""
    x = f64(x)
    with torch.no_grad():
        out = O.sdf_forward(p, x)
        vals = O.sdf_values(p, x, RADIUS, SCALE)
    sdf, feat, grad = O.sdf_outputs(p, x, RADIUS, SCALE, create_graph=False)
    raw = O.sdf_gradient(p, x, create_graph=False)
    return {"forward": out, "sdf_vals": vals, "sdf": sdf.detach(), "feat": feat.detach(), "grad": grad.detach(), "grad_raw": raw.detach()}


def heads(p, x, normals, view, feat):
    """rendering_network and attraction_network on float64 inputs -> rgb [P,3], lines [P,2,3]."""
    with torch.no_grad():
        return O.render_head(p, f64(x), f64(normals), f64(view), f64(feat)), O.attraction_head(p, f64(x), f64(normals), f64(view), f64(feat))


def sdf_param_grads(seed, variant, x, cot_sdf, cot_feat, cot_grad):
    """Gradients of  sum(a sdf) + sum(b feat) + sum(c grad)  over get_outputs (the clamped gradient through the double backward, as
    the oracle builds it with create_graph=True) wrt every SDF-network parameter -> {name: float64 tensor}."""
    p = params(seed, variant, requires_grad=True)
    sdf, feat, grad = O.sdf_outputs(p, f64(x), RADIUS, SCALE, create_graph=True)
    loss = (sdf * f64(cot_sdf)).sum() + (feat * f64(cot_feat)).sum() + (grad * f64(cot_grad)).sum()
    loss.backward()
    return {k: v.grad.detach().clone() for k, v in p.items() if v.grad is not None}


def render(seed, variant, origins, dirs, z, eik=None, cot=None, dtype=F64):
    """oracle.render_rays in float64 (+ the raw gradient at the E extra points, as the main pass returns it for the eikonal term).
    cot = dict of float32 cotangents for rgb_values, lines3d, depth, xyz (and eik_grad): also every parameter's gradient of
    sum(cot * output), density.beta included -> (outputs, grads or None).  dtype=torch.float32: the oracle as it is (what the
    reference computes), to tell where float32 arithmetic of the reference's own formulas is what a comparison measures."""
    p = params(seed, variant, requires_grad=cot is not None, dtype=dtype)
    with torch.set_grad_enabled(cot is not None):
        out = O.render_rays(p, f64(origins, dtype), f64(dirs, dtype), f64(z, dtype), RADIUS, SCALE)
        if eik is not None:
            out["eik_grad"] = O.sdf_gradient(p, f64(eik, dtype), create_graph=cot is not None)
        grads = None
        if cot is not None:
            loss = sum((out[k] * f64(c, dtype)).sum() for k, c in cot.items())
            loss.backward()
            grads = {k: v.grad.detach().clone() for k, v in p.items() if v.grad is not None}
    return {k: v.detach() for k, v in out.items()}, grads
