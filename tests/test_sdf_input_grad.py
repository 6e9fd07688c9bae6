"""Gradients with respect to the query points through the SDF network (neat_sdf_backward_x): ImplicitNetwork.get_outputs, gradient,
forward and get_sdf_vals are autograd in x in the reference (rend_a :78-137).  Every build against float64 autograd over the oracle at
the tile-edge sizes of test_f64_edges.py, with points in the shell |x| in [2.9, 3.1] where the sphere clamp is the output; the
parameter gradients unchanged by asking for d_x; a frozen network (no weight-gradient work); zero-cotangent padding; and 20 steps of
gradient descent on the points against the same loop in float64.  The math of the kernels is pinned on the CPU by
test_sdf_input_grad_math.py.  NEAT_XGRAD_TABLE=<path> writes every measured error as JSON lines."""
import json
import os

import pytest
import torch

from oracle import neat_oracle as O
from tests import f64_reference as ref
from tests.test_f64_edges import BUILDS, GRAD_SIZES, PAD_BAR, SEED, VARIANT, model

pytestmark = pytest.mark.gpu
RADIUS, SCALE = ref.RADIUS, ref.SCALE
SIZES = sorted(set(GRAD_SIZES) | {1, 127, 128, 129})
P_POOL = max(SIZES)
ENTRIES = ("get_outputs", "gradient", "forward", "get_sdf_vals")

# fp32-grade builds: max |d_x - ref| / max |ref| per entry point; 16-bit builds: relative L2.  Measured on MI355X (worst over the
# sizes and the four entry points, frozen network included): fp32 2.5e-6, fp16x3 6.2e-4, fp16 4.4e-3, bf16 1.7e-2 (relative L2).  Bars
# ~4x the measurement; fp16x3 keeps 2e-3 (its parameter-gradient bar, test_gpu_parity.py); bf16x3 (not measured by default) 2e-2, and
# fp16 / bf16 start from GRAD_REL_L2 of test_f64_edges.py (0.06 / 0.12) brought down to the measurement
X_MAX_BAR = {"fp32": 1e-5, "fp16x3": 2e-3, "bf16x3": 2e-2}
X_REL_L2 = {"fp16": 2e-2, "bf16": 7e-2}

_TABLE = []


def record(build, entry, P, err):
    _TABLE.append({"build": build, "entry": entry, "P": P, "err": float(err)})
    return err


@pytest.fixture(scope="module", autouse=True)
def _write_table():
    yield
    path = os.environ.get("NEAT_XGRAD_TABLE")
    if path and _TABLE:
        with open(path, "a") as f:
            for row in _TABLE:
                f.write(json.dumps(row) + "\n")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neat_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _pool():
    """Seeded points in [-1.5, 1.5]^3; every 5th in the shell |x| in [2.9, 3.1] (RADIUS 3, SCALE 20: the clamp is the output there);
    per-point cotangents of the three outputs of get_outputs and of forward()."""
    def make():
        g = torch.Generator().manual_seed(5)
        x = torch.rand(P_POOL, 3, generator=g) * 3 - 1.5
        shell = torch.nn.functional.normalize(torch.randn(P_POOL, 3, generator=g), dim=1) * (2.9 + 0.2 * torch.rand(P_POOL, 1, generator=g))
        pick = torch.arange(P_POOL) % 5 == 2
        x[pick] = shell[pick]
        cot = {"sdf": torch.randn(P_POOL, 1, generator=g), "feat": torch.randn(P_POOL, 256, generator=g) * 0.1,
               "grad": torch.randn(P_POOL, 3, generator=g), "out": torch.randn(P_POOL, 257, generator=g) * 0.1}
        return x, cot
    return ref.cached("xgrad_pool", make)


def _loss(entry, outs, cot):
    """The scalar each entry point is differentiated through: the same on the GPU and in float64."""
    if entry == "get_outputs":
        sdf, feat, grad = outs
        return (sdf * cot["sdf"]).sum() + (feat * cot["feat"]).sum() + (grad * cot["grad"]).sum()
    if entry == "gradient":
        return (outs * cot["grad"]).sum()
    if entry == "forward":
        return (outs * cot["out"]).sum()
    return (outs * cot["sdf"]).sum()


def _ref_dx(entry):
    """float64 autograd d loss / dx at every pool point (per-point cotangents: the reference of x[:P] is the first P rows)."""
    def make():
        x, cot = _pool()
        p = ref.params(SEED, VARIANT)
        xr = ref.f64(x).requires_grad_(True)
        c = {k: ref.f64(v) for k, v in cot.items()}
        out = O.sdf_forward(p, xr)
        if entry == "forward":
            outs = out
        elif entry == "gradient":
            (outs,) = torch.autograd.grad(out[:, :1], xr, torch.ones_like(out[:, :1]), create_graph=True)
        else:
            sdf = O.sphere_clamp(out[:, :1], xr, RADIUS, SCALE)
            if entry == "get_sdf_vals":
                outs = sdf
            else:
                (grad,) = torch.autograd.grad(sdf, xr, torch.ones_like(sdf), create_graph=True)
                outs = (sdf, out[:, 1:], grad)
        (dx,) = torch.autograd.grad(_loss(entry, outs, c), xr)
        return dx.detach()
    return ref.cached("xgrad_ref_" + entry, make)


def _gpu_dx(net, entry, x, cot):
    x = x.clone().requires_grad_(True)
    outs = {"get_outputs": net.get_outputs, "gradient": net.gradient, "forward": net.forward, "get_sdf_vals": net.get_sdf_vals}[entry](x)
    _loss(entry, outs, cot).backward()
    return x.grad


def _err(build, entry, P, got, want):
    assert got is not None, f"{build} {entry}: x.grad is None (no gradient through the query points)"
    got = got.detach().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    if build in X_MAX_BAR:
        err = float((got - want).abs().max()) / float(want.abs().max())
        bar = X_MAX_BAR[build]
    else:
        err = float((got - want).norm()) / float(want.norm())
        bar = X_REL_L2[build]
    record(build, entry, P, err)
    return err, bar


def _dev_cot(P, dev):
    _, cot = _pool()
    return {k: v[:P].to(dev) for k, v in cot.items()}


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("P", SIZES)
def test_x_gradient_vs_float64(dev, build, P):
    x, _ = _pool()
    m = model(dev, build).train()
    net = m.implicit_network
    try:
        for entry in ENTRIES:
            m.zero_grad(set_to_none=True)
            got = _gpu_dx(net, entry, x[:P].to(dev), _dev_cot(P, dev))
            err, bar = _err(build, entry, P, got, _ref_dx(entry)[:P])
            assert err <= bar, f"{build} {entry} P={P}: d_x err {err:.3e} > {bar:.1e}"
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("P", [129, 16385])
def test_parameter_gradients_unchanged_by_x_gradient(dev, build, P):
    """With x requiring grad the backward keeps a^_4 in its own buffer (no two-buffer alternation) and adds launches after the chains:
    the parameter gradients stay bit for bit those of the x-constant backward."""
    x, _ = _pool()
    m = model(dev, build).train()
    net = m.implicit_network
    cot = _dev_cot(P, dev)
    try:
        grads = []
        for need_x in (False, True):
            m.zero_grad(set_to_none=True)
            xx = x[:P].to(dev).requires_grad_(need_x)
            _loss("get_outputs", net.get_outputs(xx), cot).backward()
            assert (xx.grad is not None) == need_x
            grads.append({k: v.grad.clone() for k, v in net.named_parameters()})
        for k in grads[0]:
            assert torch.equal(grads[0][k], grads[1][k]), f"{build} P={P}: {k} changed when x requires grad"
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()


# the 16-bit builds' tangent / reverse launches with in-kernel weight gradients (kernels_dw.hpp) run from DW_MIN_POINTS = 49152 points
# by default; tuning key 16 = 2 turns them on at every size (test_gpu_parity.py::test_chain_variables_in_two_buffers_change_nothing does
# the same).  That chain alternates its chain variables between two buffers (tuning key 24), where a^_2 overwrites a^_4: with x
# requiring grad the alternation is off and a^_4 / a^_0 stay in m[4] / m[0] for the x-gradient.  These tests run that path.
HALF_BUILDS = [b for b in BUILDS if b in ("fp16x3", "fp16", "bf16")]


@pytest.fixture
def fused_dw(dev):
    from neat_amd import _lib
    lib = _lib.lib()
    _lib.check(lib.neat_set_tuning(16, 2), "neat_set_tuning")
    try:
        yield
    finally:
        lib.neat_set_tuning(16, 1)


@pytest.mark.parametrize("build", HALF_BUILDS)
@pytest.mark.parametrize("P", [129, 16385, P_POOL])
def test_x_gradient_with_in_kernel_weight_gradients(dev, fused_dw, build, P):
    """Trainable 16-bit network on the fused weight-gradient chain: d_x of every entry point against float64 (same bars as above), and
    the parameter gradients of the x-constant run (two-buffer alternation on) bit for bit those of the x-gradient run (off)."""
    x, _ = _pool()
    m = model(dev, build).train()
    net = m.implicit_network
    cot = _dev_cot(P, dev)
    try:
        for entry in ENTRIES:
            m.zero_grad(set_to_none=True)
            got = _gpu_dx(net, entry, x[:P].to(dev), cot)
            err, bar = _err(build, entry + "_dw", P, got, _ref_dx(entry)[:P])
            assert err <= bar, f"{build} {entry} P={P} (in-kernel weight gradients): d_x err {err:.3e} > {bar:.1e}"
        grads = []
        for need_x in (False, True):
            m.zero_grad(set_to_none=True)
            xx = x[:P].to(dev).requires_grad_(need_x)
            _loss("get_outputs", net.get_outputs(xx), cot).backward()
            assert (xx.grad is not None) == need_x
            grads.append({k: v.grad.clone() for k, v in net.named_parameters()})
        for k in grads[0]:
            assert torch.isfinite(grads[1][k]).all(), k
            assert torch.equal(grads[0][k], grads[1][k]), f"{build} P={P}: {k} changed when x requires grad (in-kernel weight gradients)"
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()


def test_gated_query_refuses_x_gradient(dev):
    """get_sdf_vals with a device gate is the sampler's query (under no_grad); differentiating it in x would have to ignore the gate."""
    m = model(dev, "fp32").eval()
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    x = torch.zeros(8, 3, device=dev, requires_grad=True)
    with pytest.raises(ValueError):
        m.implicit_network.get_sdf_vals(x, gate=(ctl, 0, 1))
    with torch.no_grad():
        assert m.implicit_network.get_sdf_vals(x, gate=(ctl, 1, 0)).shape == (8, 1)


@pytest.mark.parametrize("build", BUILDS)
def test_frozen_network_x_gradient(dev, build):
    """requires_grad_(False) on the network (a trained model whose query points are optimised): d_x alone, no parameter gradient."""
    x, _ = _pool()
    m = model(dev, build).eval()
    net = m.implicit_network
    net.requires_grad_(False)
    try:
        for P in (129, 16385):
            for entry in ENTRIES:
                got = _gpu_dx(net, entry, x[:P].to(dev), _dev_cot(P, dev))
                err, bar = _err(build, entry + "_frozen", P, got, _ref_dx(entry)[:P])
                assert err <= bar, f"{build} frozen {entry} P={P}: d_x err {err:.3e} > {bar:.1e}"
                assert all(p.grad is None for p in net.parameters())
    finally:
        net.requires_grad_(True)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("P", [33, 129, 16385])
def test_x_gradient_zero_cotangent_padding(dev, build, P):
    x, _ = _pool()
    Pp = P + 128 if P + 128 <= P_POOL else P_POOL
    m = model(dev, build).train()
    net = m.implicit_network
    try:
        cot = _dev_cot(P, dev)
        got = _gpu_dx(net, "get_outputs", x[:P].to(dev), cot)
        cpad = {k: torch.cat([v, torch.zeros(Pp - P, v.shape[1], device=dev)]) for k, v in cot.items()}
        m.zero_grad(set_to_none=True)
        padded = _gpu_dx(net, "get_outputs", x[:Pp].to(dev), cpad)
        err = float((padded[:P] - got).abs().max()) / max(float(got.abs().max()), 1e-30)
        record(build, "zero_pad", P, err)
        assert err <= PAD_BAR, f"{build} P={P}: zero-cotangent points past P change d_x by {err:.3e}"
        assert torch.equal(padded[P:], torch.zeros_like(padded[P:])), f"{build}: d_x of zero-cotangent points is not 0"
    finally:
        m.zero_grad(set_to_none=True)
        m.eval()


# 20 steps of x <- x - LR d/dx sum sdf(x)^2 (get_sdf_vals) on 4096 points, frozen network, against the same loop in float64.  The
# "rough" network's |d sdf / dx| reaches ~18: the step must keep 2 LR |d sdf / dx|^2 < 2, or the iteration oscillates across the surface
# and amplifies every rounding (LR 0.01 moves points 0.24 away from float64 in fp32; 0.05 diverges in float64 as well).  At LR 0.002
# the loss falls by 25% and the float32 oracle's own loop ends 8.4e-6 from float64
GD_STEPS, GD_LR, GD_POINTS = 20, 0.002, 4096
# measured on MI355X (max |x - x64| over the points): fp32 6.8e-6, fp16x3 1.0e-2 (its backward pass is the f16 one: ~6e-4 of max |d_x|
# per step, summed over 20 steps at the worst point).  Bars ~4x
GD_BAR = {"fp32": 3e-5, "fp16x3": 4e-2}


def _gd_ref():
    def make():
        p = ref.params(SEED, VARIANT)
        x = ref.f64(_gd_start())
        losses = []
        for _ in range(GD_STEPS):
            x = x.detach().requires_grad_(True)
            loss = (O.sdf_values(p, x, RADIUS, SCALE) ** 2).sum()
            (g,) = torch.autograd.grad(loss, x)
            losses.append(float(loss.detach()))
            x = x - GD_LR * g
        return x.detach(), losses
    return ref.cached("xgrad_gd", make)


def _gd_start():
    return torch.rand(GD_POINTS, 3, generator=torch.Generator().manual_seed(9)) * 3 - 1.5


@pytest.mark.parametrize("build", ["fp32", "fp16x3"])
def test_gradient_descent_on_points(dev, build):
    m = model(dev, build).eval()
    net = m.implicit_network
    net.requires_grad_(False)
    try:
        x = _gd_start().to(dev)
        losses = []
        for _ in range(GD_STEPS):
            x = x.detach().requires_grad_(True)
            loss = (net.get_sdf_vals(x) ** 2).sum()
            loss.backward()
            losses.append(float(loss.detach()))
            x = x - GD_LR * x.grad
        want, ref_losses = _gd_ref()
        err = float((x.detach().cpu().double() - want).abs().max())
        record(build, "gradient_descent", GD_POINTS, err)
        assert losses[-1] < 0.9 * losses[0] and ref_losses[-1] < 0.9 * ref_losses[0], (losses[0], losses[-1])
        assert err <= GD_BAR[build], f"{build}: points after {GD_STEPS} steps off float64 by {err:.3e} > {GD_BAR[build]:.0e}"
    finally:
        net.requires_grad_(True)


@pytest.mark.parametrize("build", ["fp32", "fp16x3"])
@pytest.mark.parametrize("frozen", [False, True])
def test_torch_op_x_gradient_equals_module(dev, build, frozen):
    """torch.ops.neat_hip.sdf_outputs carries the same x-gradient (and parameter gradients) as the module API: same launches, same bits."""
    from neat_amd import _lib, torch_ops
    P = 129
    x, _ = _pool()
    m = model(dev, build).train()
    net = m.implicit_network
    cot = _dev_cot(P, dev)
    net.requires_grad_(not frozen)
    try:
        m.zero_grad(set_to_none=True)
        xa = x[:P].to(dev).requires_grad_(True)
        _, sdf, feat, grad = net._outputs(xa, RADIUS)
        _loss("get_outputs", (sdf, feat, grad), cot).backward()
        want_p = {k: None if v.grad is None else v.grad.clone() for k, v in net.named_parameters()}
        m.zero_grad(set_to_none=True)
        prm = torch_ops.net_params(m)[:27]
        xb = x[:P].to(dev).requires_grad_(True)
        _, sdf, feat, grad, _ws = torch.ops.neat_hip.sdf_outputs(xb, prm, RADIUS, SCALE, _lib.PRECISIONS[build])
        _loss("get_outputs", (sdf, feat, grad), cot).backward()
        assert torch.equal(xa.grad, xb.grad)
        for k, v in net.named_parameters():
            if frozen:
                assert v.grad is None and want_p[k] is None
            else:
                assert torch.equal(v.grad, want_p[k]), k
    finally:
        net.requires_grad_(True)
        m.zero_grad(set_to_none=True)
        m.eval()
