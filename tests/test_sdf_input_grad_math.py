"""The x-gradient of the SDF network as the HIP backward forms it (neat_sdf_backward_x), restated in float64 from explicit per-layer
passes and checked against torch.autograd over the oracle (rend_a :78-137).

For  L = <d_out, out> + <d_sdf, sdf> + <d_feat, feat> + <c, grad>  with e = PE6(x), J = de/dx:

    dL/dx = J^T abar_e + sum_j u_e[j] (d^2 e_j / dx^2) c~ + clamp terms
    abar_e = W0^T a^_0 + W4skip^T a^_4        (total PE-level cotangent of the reverse chain, the normal's tangent terms included)
    u_e    = W0^T u_0  + W4skip^T u_4         (what the adjoint chain contracts into the normal: grad_raw = J^T u_e)

c~ = c where the sphere clamp is off and 0 where it is on; there the clamped outputs sdf = s (r - |x|), grad = -s x / |x| add
-s x^ d_sdf - s (I - x^ x^T) c / |x|.  This is the math the kernels implement; the GPU test (test_sdf_input_grad.py) checks the kernels."""
import math

import pytest
import torch

from oracle import neat_oracle as O
from tests import f64_reference as ref

F64 = torch.float64
RADIUS, SCALE = ref.RADIUS, ref.SCALE
SQRT2 = math.sqrt(2.0)


def _sp_derivs(a):
    """softplus(beta = 100, threshold = 20) -> (phi', phi'') as torch's softplus differentiates it (linear past the threshold)."""
    lin = 100.0 * a > 20.0
    s = torch.sigmoid(100.0 * a)
    d1 = torch.where(lin, torch.ones_like(a), s)
    d2 = torch.where(lin, torch.zeros_like(a), 100.0 * s * (1.0 - s))
    return d1, d2


def _pe_jacobian_hessian(x):
    """J [P,39,3] and the diagonal Hessian H [P,39,3] (d^2 e_j / dx_i^2; PE-6 is separable per coordinate) in posenc's row order."""
    P = x.shape[0]
    J = torch.zeros(P, 39, 3, dtype=F64)
    H = torch.zeros(P, 39, 3, dtype=F64)
    for i in range(3):
        J[:, i, i] = 1.0
        for k in range(6):
            f = 2.0 ** k
            xs, xc = torch.sin(f * x[:, i]), torch.cos(f * x[:, i])
            J[:, 3 + 6 * k + i, i] = f * xc
            J[:, 6 + 6 * k + i, i] = -f * xs
            H[:, 3 + 6 * k + i, i] = -f * f * xs
            H[:, 6 + 6 * k + i, i] = -f * f * xc
    return J, H


def decomposed_dx(p, x, d_out, d_sdf, d_feat, c, radius, inside_out=False):
    """dL/dx from the decomposition: primal, adjoint (u), tangent (a-dot) and reverse (a^) chains written out layer by layer."""
    W = [O.wn_weight(p, f"implicit_network.lin{l}") for l in range(9)]
    b = [p[f"implicit_network.lin{l}.bias"] for l in range(9)]
    W4h, W4s = W[4][:, :217] / SQRT2, W[4][:, 217:] / SQRT2       # the skip concat's 1/sqrt2, folded as the packs do
    w8, b8 = W[8].clone(), b[8].clone()
    if inside_out:                                                 # the sign of the sdf row (networks.ImplicitNetwork.triples)
        w8[0], b8[0] = -w8[0], -b8[0]
    e = O.posenc(x, 6)
    J, H = _pe_jacobian_hessian(x)
    # primal: a_l = W_l in_l + b_l, h_{l+1} = softplus(a_l)
    a, h = [], [None]
    inp = e
    for l in range(8):
        z = inp @ (W4h.T if l == 4 else W[l].T) + b[l] + ((e @ W4s.T) if l == 4 else 0.0)
        a.append(z)
        h_next = torch.nn.functional.softplus(z, beta=100.0)
        inp = h_next
        h.append(h_next)
    out = h[8] @ w8.T + b8
    d1, d2 = zip(*[_sp_derivs(z) for z in a])
    Wh = [W4h if l == 4 else W[l] for l in range(8)]
    # adjoint: u_l = d sdf_raw / d a_l
    u = [None] * 8
    u[7] = w8[0] * d1[7]
    for l in range(7, 0, -1):
        u[l - 1] = (u[l] @ Wh[l]) * d1[l - 1]
    u_e = u[0] @ W[0] + u[4] @ W4s
    grad_raw = torch.einsum("pj,pji->pi", u_e, J)
    # the sphere clamp
    nr = x.norm(dim=1, keepdim=True)
    mask = torch.zeros_like(nr, dtype=torch.bool) if radius <= 0 else (SCALE * (radius - nr) < out[:, :1])
    keep = (~mask).to(F64)
    ct = c * keep                                                  # c~: the normal cotangent where the network's normal is the output
    # tangent along e^ = J c~: a-dot_l; m_l = the normal's extra cotangent of a_l
    eh = torch.einsum("pji,pi->pj", J, ct)
    ad = []
    hd = None
    for l in range(8):
        z = eh @ W[0].T if l == 0 else hd @ Wh[l].T + ((eh @ W4s.T) if l == 4 else 0.0)
        ad.append(z)
        hd = d1[l] * z
    m = [None] * 8
    m[7] = w8[0] * d2[7] * ad[7]
    for l in range(7, 0, -1):
        m[l - 1] = (u[l] @ Wh[l]) * d2[l - 1] * ad[l - 1]
    # reverse: a^_8 = cotangent of lin8's output; a^_{l-1} = (W_l^T a^_l) phi'(a_{l-1}) + m_{l-1}
    abar8 = d_out.clone()
    abar8[:, :1] += d_sdf * keep
    abar8[:, 1:] += d_feat
    ah = [None] * 8
    ah[7] = (abar8 @ w8) * d1[7] + m[7]
    for l in range(7, 0, -1):
        ah[l - 1] = (ah[l] @ Wh[l]) * d1[l - 1] + m[l - 1]
    abar_e = ah[0] @ W[0] + ah[4] @ W4s
    dx = torch.einsum("pj,pji->pi", abar_e, J) + torch.einsum("pj,pji->pi", u_e, H) * ct
    xh = x / nr
    clamp = -SCALE * xh * d_sdf - SCALE * (c - xh * (xh * c).sum(1, keepdim=True)) / nr
    dx = dx + mask.to(F64) * clamp
    return dx, out, grad_raw, mask


def autograd_dx(p, x, d_out, d_sdf, d_feat, c, radius):
    """The reference: rend_a's get_outputs in x (sphere clamp, create_graph normal) + forward(), differentiated by autograd."""
    x = x.detach().clone().requires_grad_(True)
    out = O.sdf_forward(p, x)
    sdf = O.sphere_clamp(out[:, :1], x, radius, SCALE)
    (grad,) = torch.autograd.grad(sdf, x, torch.ones_like(sdf), create_graph=True)
    L = (d_out * out).sum() + (d_sdf * sdf).sum() + (d_feat * out[:, 1:]).sum() + (c * grad).sum()
    (dx,) = torch.autograd.grad(L, x)
    return dx, out.detach(), grad.detach()


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    inner = (torch.rand(n, 3, generator=g, dtype=F64) * 2 - 1) * 1.5
    d = torch.randn(n, 3, generator=g, dtype=F64)
    shell = d / d.norm(dim=1, keepdim=True) * (2.9 + 0.2 * torch.rand(n, 1, generator=g, dtype=F64))
    return torch.cat([inner, shell])


def _cot(P, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(P, 257, generator=g, dtype=F64), torch.randn(P, 1, generator=g, dtype=F64),
            torch.randn(P, 256, generator=g, dtype=F64), torch.randn(P, 3, generator=g, dtype=F64))


@pytest.mark.parametrize("inside_out", [False, True])
@pytest.mark.parametrize("radius", [RADIUS, 0.0])
@pytest.mark.parametrize("which", ["all", "sdf", "feat", "out", "grad"])
def test_decomposition_equals_autograd(which, radius, inside_out):
    p = ref.params(42, "rough")
    x = _points(48, 7)
    d_out, d_sdf, d_feat, c = _cot(x.shape[0], 11)
    zero = {"sdf": (d_out, d_feat, c), "feat": (d_out, d_sdf, c), "out": (d_sdf, d_feat, c), "grad": (d_out, d_sdf, d_feat)}.get(which, ())
    for t in zero:
        t.zero_()
    old = O.OPTS["inside_out"]
    O.OPTS["inside_out"] = inside_out
    try:
        want, out_ref, grad_ref = autograd_dx(p, x, d_out, d_sdf, d_feat, c, radius)
    finally:
        O.OPTS["inside_out"] = old
    got, out, grad_raw, mask = decomposed_dx(p, x, d_out, d_sdf, d_feat, c, radius, inside_out)
    # the explicit primal / adjoint chains are the oracle's
    assert torch.allclose(out, out_ref, rtol=0, atol=1e-12)
    if radius <= 0:
        assert torch.allclose(grad_raw, grad_ref, rtol=0, atol=1e-10)
    else:
        # the shell points straddle the clamp: both branches are exercised
        assert 0 < int(mask.sum()) < x.shape[0]
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err < 1e-10, (which, radius, inside_out, err)
