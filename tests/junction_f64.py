"""Float64 references and seeded CPU inputs for tests/test_f64_junction_edges.py (the kernels of neat_amd/csrc/kernels_junction.hpp).

References are the oracle's own functions (oracle/neat_oracle.py: project2d, camera_rays, _line_loss, neat_loss, ffn_junctions) run on
float64 copies of the float32 inputs the kernel sees; `dtype=torch.float32` runs the same formulation in float32 on the CPU (the yardstick
for what float32 arithmetic of the formula costs).  Where the oracle has no function (Adam, the junction gate, l3d, the small inverse)
the reference is a few lines of plain torch here.  Nothing in this module imports the code under test, and nothing needs a GPU: the
inputs are built with margins from every decision boundary (relu masks, the gate, straight-or-flipped, sign(d), the matching) and the
`*_margin*` functions measure those margins from the float64 reference alone."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import neat_oracle as O
from tests.f64_reference import F64, cached, f64  # noqa: F401

K_SKEW = [[560.0, 0.3, 256.0], [0.0, 555.0, 250.0], [0.0, 0.0, 1.0]]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _signs(shape, g):
    return torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def leaf(t, dtype):
    """A fresh leaf of `dtype` holding t's values (never t itself: `t.to(t.dtype)` is t)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def rel_max(a, b):
    """max |a - b| relative to max |b| (gradients: their scale is far below 1, where tests.f64_table.rel_err would measure nothing);
    never smaller than rel_err of the same pair."""
    a = a.detach().cpu().to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all(), "non-finite values"
    if a.numel() == 0:
        return 0.0
    d, s = float((a - b).abs().max()), float(b.abs().max())
    return 0.0 if d == 0.0 else d / max(s, 1e-30)


def world_to_camera(seed=5):
    """[R | T] with a random rotation; T_z = 4 keeps every point of [-1.2, 1.2]^3 at cam_z >= 1.9."""
    q = torch.linalg.qr(torch.randn(3, 3, generator=gen(seed)))[0]
    return torch.cat([q, torch.tensor([[0.1], [-0.2], [4.0]])], 1).contiguous()


# ---- junction MLP ------------------------------------------------------------------------------------------------------------
FFN_KEYS = ("latents", "ffn.0.weight", "ffn.0.bias", "ffn.2.weight", "ffn.2.bias", "ffn.4.weight", "ffn.4.bias")


def ffn_inputs(J, seed):
    """Latents [J,256] ~ N(0,1), the three layers with nn.Linear's initial range (+-1/16), a cotangent [J,3]."""
    g = gen(seed)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) / 16
    p = {"latents": torch.randn(J, 256, generator=g), "ffn.0.weight": u(256, 256), "ffn.0.bias": u(256), "ffn.2.weight": u(256, 256),
         "ffn.2.bias": u(256), "ffn.4.weight": u(3, 256), "ffn.4.bias": u(3)}
    return p, torch.randn(J, 3, generator=g)


def ffn_reference(p32, cot, dtype=F64):
    """oracle.ffn_junctions and its gradients of sum(cot * y); the two hidden pre-activations (for the relu margin and the saved
    activations handed to the backward kernels) are the oracle's first two lines once more."""
    p = {k: leaf(v, dtype) for k, v in p32.items()}
    y = O.ffn_junctions(p)
    (y * cot.to(dtype)).sum().backward()
    with torch.no_grad():
        a1 = F.linear(p["latents"], p["ffn.0.weight"], p["ffn.0.bias"])
        a2 = F.linear(torch.relu(a1), p["ffn.2.weight"], p["ffn.2.bias"])
    return {"y": y.detach(), "a1": a1, "a2": a2, "h1": torch.relu(a1), "h2": torch.relu(a2),
            "grads": {k: p[k].grad.detach() for k in FFN_KEYS}}


def ffn_relu_margin(r64):
    return min(float(r64["a1"].abs().min()), float(r64["a2"].abs().min()))


# ---- line losses -------------------------------------------------------------------------------------------------------------
def line_inputs(L, seed):
    """Pixel segments >= 60 px long; predictions = the target (odd rows: end points swapped) +- [0.5, 3] px per coordinate; rows
    i % 7 == 5 lie 400 px off (beyond the 100 px gate), rows i % 11 == 3 equal their target exactly, rows i % 5 == 2 have weight 0."""
    g = gen(seed)
    i = torch.arange(L)
    p1 = torch.rand(L, 2, generator=g) * 400 + 56
    ang, ln = torch.rand(L, generator=g) * 2 * math.pi, 60 + 140 * torch.rand(L, generator=g)
    gt = torch.cat([p1, p1 + ln[:, None] * torch.stack([ang.cos(), ang.sin()], 1)], 1)
    tgt = torch.where((i % 2 == 1)[:, None], gt[:, [2, 3, 0, 1]], gt)
    pred = tgt + _signs((L, 4), g) * (0.5 + 2.5 * torch.rand(L, 4, generator=g))
    pred[i % 7 == 5] += 400.0
    pred[i % 11 == 3] = tgt[i % 11 == 3]
    w = torch.rand(L, generator=g)
    w[i % 5 == 2] = 0.0
    return pred.contiguous(), gt.contiguous(), w


def line_margins(pred, gt, thr):
    """From float64 values alone: (min |ds - df| of the straight-or-flipped choice, min |per_line - thr|, smallest non-zero
    |pred - target|, number of exact zeros of pred - target)."""
    pred, gt = f64(pred), f64(gt)
    sw = gt[:, [2, 3, 0, 1]]
    ds, df = ((pred - gt) ** 2).sum(-1), ((pred - sw) ** 2).sum(-1)
    d = pred - torch.where((ds < df)[:, None], gt, sw)
    per = d.abs().mean(-1)
    nz = d[d != 0].abs()
    return float((ds - df).abs().min()), float((per - thr).abs().min()), float(nz.min()) if nz.numel() else math.inf, int((d == 0).sum())


def line_loss_reference(pred, gt, w, thr, dtype=F64):
    p = leaf(pred, dtype)
    loss, per = O._line_loss(p, gt.to(dtype), w.to(dtype), thr)
    loss.backward()
    return {"loss": loss.detach(), "per_line": per, "count": int((per < thr).sum()), "d_pred": p.grad.detach()}


def calibrate64(K, gt4):
    """K^-1 (x, y, 1) divided by its third component, float64 (input construction and margins only)."""
    g2 = f64(gt4).reshape(-1, 2)
    gh = (torch.linalg.inv(f64(K)) @ torch.cat([g2, torch.ones_like(g2[:, :1])], -1).t()).t()
    return (gh[:, :2] / gh[:, 2:]).reshape(-1, 4)


def tail_inputs(L, R, E, K, J, good_mode, seed):
    """Everything ops.loss_tail reads, float32 on the CPU.  The calibrated predictions sit 1e-3 .. 5e-3 from their (straight or swapped)
    calibrated target; `lines3d` are 3-D end points whose projection by `w2c` is `pred_calib` (up to float32 rounding: 1e-7).  Global
    junctions on a jittered lattice (pairwise L1 distance >= 0.06), matched local ones within 0.015 of their partner, surplus local
    ones ~12 away; one pair 12 apart in z (beyond the jcount gate of 10) where K <= J."""
    g = gen(seed)
    pred_px, gt4, w = line_inputs(L, seed + 1)
    Km = torch.tensor(K_SKEW)
    w2c = world_to_camera()
    i = torch.arange(L)
    gc = calibrate64(Km, gt4)
    tgt = torch.where((i % 3 == 0)[:, None], gc[:, [2, 3, 0, 1]], gc)
    uv = (tgt + (_signs((L, 4), g) * (1e-3 + 4e-3 * torch.rand(L, 4, generator=g))).to(F64)).reshape(L, 2, 2)
    z = (2.0 + 2.0 * torch.rand(L, 2, 1, generator=g)).to(F64)
    cam = torch.cat([uv * z, z], -1)
    Rm, T = f64(w2c[:, :3]), f64(w2c[:, 3])
    lines3d = ((cam - T) @ Rm).float().contiguous()                     # rows: R^T (c - T)
    inp = {"pred_px": pred_px, "gt5": torch.cat([gt4, w[:, None]], 1).contiguous(), "K": Km, "w2c": w2c, "lines3d": lines3d,
           "pred_calib": uv.reshape(L, 4).float().contiguous()}
    rgb = torch.rand(R, 3, generator=g)
    rgb_gt = rgb - _signs((R, 3), g) * (0.01 + 0.5 * torch.rand(R, 3, generator=g))
    r = torch.arange(R)
    rgb_gt[r % 6 == 1] = rgb[r % 6 == 1]
    inp["rgb"], inp["rgb_gt"] = rgb, rgb_gt
    if E:
        gth = F.normalize(torch.randn(E, 3, generator=g), dim=1) * (0.5 + torch.rand(E, 1, generator=g))
        if E > 1:
            gth[E // 2] = 0.0
        inp["gtheta"] = gth.contiguous()
    if J:
        cells = torch.randperm(11 ** 3, generator=g)[:J]
        lat = torch.stack([cells // 121, (cells // 11) % 11, cells % 11], 1).float()
        glo3 = (lat - 5.0) * 0.18 + (torch.rand(J, 3, generator=g) - 0.5) * 0.06
        glo2c = O.project2d(torch.eye(3, dtype=F64), Rm, T[:, None], f64(glo3))
        glo2 = torch.rand(J, 2, generator=g) * 512
        n = min(K, J)
        perm = torch.randperm(J, generator=g)[:n]
        far = None
        if 5 <= K <= J:
            top = int(glo3[:, 2].argmax())
            hit = (perm == top).nonzero()
            if hit.numel():
                perm[int(hit[0])] = perm[1]
            perm[1] = top
            far = 1
        loc3 = torch.rand(K, 3, generator=g) + 5.0
        loc2c = torch.rand(K, 2, generator=g)
        loc2 = torch.rand(K, 2, generator=g) * 512
        loc3[:n] = glo3[perm] + _signs((n, 3), g) * (1e-3 + 4e-3 * torch.rand(n, 3, generator=g))
        loc2c[:n] = (glo2c[perm] + (_signs((n, 2), g) * (1e-3 + 4e-3 * torch.rand(n, 2, generator=g))).to(F64)).float()
        loc2[:n] = glo2[perm] + torch.randn(n, 2, generator=g) * 2
        if far is not None:
            loc3[far, 2] += 12.0
        k = torch.arange(K)
        good = {"all": k >= 0, "some": k % 9 != 4, "none": k < 0}[good_mode]
        inp.update(glo3=glo3.contiguous(), glo2c=glo2c.float().contiguous(), glo2=glo2, loc3=loc3.contiguous(), loc2c=loc2c.contiguous(),
                   loc2=loc2, good=good)
    return inp


def pair_cost64(inp):
    """The oracle's junction pair cost (neat_loss: cdist_1 + 0.1 cdist_1) of ALL local rows, float64, for the matching margins; the
    calibrated global junctions are the float64 projection when `fold` else the given tensor -- they differ by 1e-7."""
    return torch.cdist(f64(inp["loc3"]), f64(inp["glo3"]), p=1) + 0.1 * torch.cdist(f64(inp["loc2c"]), f64(inp["glo2c"]), p=1)


def matching_margin(cost, good):
    """scipy's assignment of the good rows of `cost` and the gap by which it is the only optimum: every matched entry is the strict
    minimum of its row (rows <= columns) or of its column (more rows) by the returned gap, so the sum of those minima is a lower bound
    that only this assignment reaches.  -> (rows, cols, gap, largest matched cost)."""
    keep = good.nonzero().flatten()
    c = cost[keep]
    if c.numel() == 0:
        return keep[:0], keep[:0], math.inf, 0.0
    ri, ci = O.hungarian(c)
    m = c[ri, ci]
    other = c.clone()
    other[ri, ci] = math.inf
    if c.shape[0] <= c.shape[1]:
        gap = (other[ri].min(1)[0] - m).min() if c.shape[1] > 1 else torch.tensor(math.inf)
    else:
        gap = (other[:, ci].min(0)[0] - m).min()
    return keep[ri], ci, float(gap), float(m.max())


def tail_reference(inp, fold, dtype=F64, weights=(0.1, 0.01, 0.1, 0.01)):
    """oracle.neat_loss on the inputs of ops.loss_tail -> (scalars, gradients of the total loss wrt every differentiable input).
    fold: the calibrated lines and global junctions are oracle.project2d(I, w2c, .) of lines3d / glo3 (gradients reach those)."""
    c = lambda k: inp[k].to(dtype)
    Rm, T, eye = c("w2c")[:, :3], c("w2c")[:, 3:], torch.eye(3, dtype=dtype)
    leaves = {"rgb": leaf(inp["rgb"], dtype)}
    res = {"rgb_values": leaves["rgb"], "lines2d": c("pred_px"), "K": c("K")}
    if fold:
        leaves["lines3d"] = leaf(inp["lines3d"], dtype)
        res["lines2d_calib"] = O.project2d(eye, Rm, T, leaves["lines3d"]).reshape(-1, 4)
    else:
        leaves["pred_calib"] = leaf(inp["pred_calib"], dtype)
        res["lines2d_calib"] = leaves["pred_calib"]
    if "gtheta" in inp:
        leaves["gtheta"] = leaf(inp["gtheta"], dtype)
        res["grad_theta"] = leaves["gtheta"]
    res["j3d_local"] = torch.zeros(0, 3, dtype=dtype)
    if "glo3" in inp:
        good = inp["good"]
        leaves["glo3"] = leaf(inp["glo3"], dtype)
        if fold:
            glo2c = O.project2d(eye, Rm, T, leaves["glo3"])
        else:
            glo2c = leaves["glo2c"] = leaf(inp["glo2c"], dtype)
        res.update(j3d_local=c("loc3")[good], j2d_local_calib=c("loc2c")[good], j2d_local=c("loc2")[good], j3d_global=leaves["glo3"],
                   j2d_global_calib=glo2c, j2d_global=c("glo2"))
    out = O.neat_loss(res, c("rgb_gt"), c("gt5")[None], *weights)
    names = list(leaves)
    grads = torch.autograd.grad(out["loss"], [leaves[k] for k in names], allow_unused=True)
    scal = {k: (v.detach().to(dtype) if torch.is_tensor(v) else torch.tensor(float(v), dtype=dtype)) for k, v in out.items()}
    return scal, {k: (torch.zeros_like(leaves[k]) if gr is None else gr.detach()) for k, gr in zip(names, grads)}


# ---- projections, l3d, camera glue, the small inverse ----------------------------------------------------------------------------
def proj_inputs(N, seed):
    """Points whose camera depth is +-[0.1, 5] (both signs), a K with skew, a random [R | T], a cotangent per output."""
    g = gen(seed)
    w2c = world_to_camera(seed + 50)
    z = _signs((N, 1), g) * (0.1 + 4.9 * torch.rand(N, 1, generator=g))
    cam = torch.cat([torch.randn(N, 2, generator=g) * z.abs(), z], 1).to(F64)
    X = ((cam - f64(w2c[:, 3])) @ f64(w2c[:, :3])).float().contiguous()
    return torch.tensor(K_SKEW), w2c, X, torch.randn(N, 2, generator=g), torch.randn(N, 2, generator=g)


def project_reference(K, w2c, X, cot, dtype=F64):
    """oracle.project2d, its camera depth (for the margin) and d sum(cot * uv) / dX."""
    x = leaf(X, dtype)
    Kd, Rm, T = K.to(dtype), w2c[:, :3].to(dtype), w2c[:, 3:].to(dtype)
    uv = O.project2d(Kd, Rm, T, x)
    (uv * cot.to(dtype)).sum().backward()
    with torch.no_grad():
        depth = (Kd @ (Rm @ x.t() + T))[2]
    return uv.detach(), x.grad.detach(), depth


def l3d_inputs(R, seed):
    """Rays and normals with |<d, n>| >= 0.05: n = s (c d + sqrt(1 - c^2) e) with |c| in [0.05, 1) and e a unit vector normal to d."""
    g = gen(seed)
    d = F.normalize(torch.randn(R, 3, generator=g), dim=1)
    e = F.normalize(torch.cross(d, torch.randn(R, 3, generator=g), dim=1), dim=1)
    c = _signs((R, 1), g) * (0.06 + 0.9 * torch.rand(R, 1, generator=g))
    n = c * d + (1 - c * c).sqrt() * e
    return torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g), d.contiguous(), n.contiguous()


def l3d_reference(x, o, d, n, dtype=F64):
    """rend_a :441-447: t = <x - o, n> / (<d, n> +- 1e-6), l3d = o + t d -> (l3d, <d, n>)."""
    x, o, d, n = (t.to(dtype) for t in (x, o, d, n))
    den = (d * n).sum(-1)
    t = ((x - o) * n).sum(-1) / (den + torch.where(den >= 0, torch.full_like(den, 1e-6), torch.full_like(den, -1e-6)))
    return o + d * t[:, None], den


CYCLE3 = [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]          # a rotation (det +1) with a zero diagonal


def pivot_pose(seed, tilt=0.0):
    """Camera-to-world pose whose rotation is the cyclic permutation (times a small rotation of `tilt` radians about z): the leading
    entry of every elimination step is zero or tiny, so Gauss-Jordan must exchange rows at every step."""
    cz, sz = math.cos(tilt), math.sin(tilt)
    rot = torch.tensor(CYCLE3) @ torch.tensor([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    pose = torch.eye(4)
    pose[:3, :3] = rot
    pose[:3, 3] = torch.randn(3, generator=gen(seed))
    return pose


def random_pose(seed):
    g = gen(seed)
    pose = torch.eye(4)
    pose[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    pose[:3, 3] = torch.randn(3, generator=g) * 2
    return pose


def inv_matrices():
    """name -> square matrix (n = 1 .. 4): well-ordered ones, and ones that need a row exchange at every elimination step."""
    g = gen(77)
    K = torch.tensor(K_SKEW)
    m = {"n1": torch.tensor([[4.0]]), "n1_neg": torch.tensor([[-0.03125]]),
         "n2_dominant": torch.tensor([[3.0, 1.0], [-1.0, 2.0]]), "n2_swap": torch.tensor([[0.0, 2.0], [3.0, 1.0]]),
         "n3_K": K, "n3_K_rows_exchanged": K[[1, 0, 2]].contiguous(), "n3_cycle": torch.tensor(CYCLE3) * torch.tensor([2.0, 0.5, 3.0]),
         "n3_random": torch.randn(3, 3, generator=g) + 3 * torch.eye(3),
         "n4_pose_random": random_pose(3), "n4_pose_cycle": pivot_pose(4), "n4_pose_cycle_tilted": pivot_pose(5, 0.01),
         "n4_shift": torch.roll(torch.diag(torch.tensor([2.0, -3.0, 0.5, 4.0])), 1, 1) + 0.01 * torch.randn(4, 4, generator=g)}
    return m


def swaps_needed(A):
    """Number of elimination steps of float64 Gauss-Jordan with partial pivoting at which the pivot is NOT the row in place."""
    a = f64(A).clone()
    n, swaps = a.shape[0], 0
    for c in range(n):
        r = c + int(a[c:, c].abs().argmax())
        if r != c:
            a[[c, r]] = a[[r, c]]
            swaps += 1
        a[c] = a[c] / a[c, c]
        for q in range(n):
            if q != c:
                a[q] = a[q] - a[q, c] * a[c]
    return swaps


def camera_reference(uv, pose, Kin, dtype=F64):
    """oracle.camera_rays of uv [1,R,2], and [R | T] = the first three rows of pose^-1."""
    dirs, origin = O.camera_rays(uv.to(dtype), pose.to(dtype)[None], Kin.to(dtype)[None])
    return dirs[0], origin[0], torch.linalg.inv(pose.to(dtype))[:3]


# ---- junction cost and gate ------------------------------------------------------------------------------------------------------
def junction_cost_reference(cand2d, gt2d, dtype=F64):
    return ((cand2d.to(dtype)[None] - gt2d.to(dtype)[:, None]) ** 2).sum(-1).sqrt()


def gate_reference(rows, cols, cost, cand3d, cand2d, cand2dc, use_median):
    """Exact (comparisons and gathers of the same float32 numbers): rend_a :474-489 on padded pairs.  With no valid pair nanmedian is
    NaN; the gate then falls back to 10, as neat_amd.networks' torch path does (`torch.where(isnan(median), 10, median)`)."""
    ok = (rows >= 0) & (cols >= 0)
    r, c = rows.clamp_min(0), cols.clamp_min(0)
    m = torch.where(ok, cost[r, c], torch.full((rows.shape[0],), float("nan")))
    med = None
    if use_median:
        med = torch.nanmedian(m)
        if torch.isnan(med):
            med = torch.tensor(10.0)
    good = (m < (med if use_median else 10.0)) & ok
    z = lambda t: torch.where(ok[:, None], t[c], torch.zeros_like(t[c]))
    return med, good, z(cand3d), z(cand2d), z(cand2dc)


# ---- DBSCAN --------------------------------------------------------------------------------------------------------------------------
def dbscan_points(n, seed):
    """The construction of tests/test_lsap.py::test_dbscan_means_vs_sklearn: blobs of sigma 0.002, n/8 isolated points, one long chain (its length n/4 - n/8, so that odd n fit)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (max(n // 16, 2), 3))
    pts = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.002, (n, 3))
    pts[: n // 8] = rng.uniform(-1, 1, (n // 8, 3))
    t = np.linspace(0, 1, n // 4 - n // 8)[:, None]
    pts[n // 8: n // 4] = np.array([0.5, -0.5, 0.2]) + t * np.array([0.6, 0.1, -0.3])
    return pts.astype(np.float32)


def dbscan_reference(pts, eps=0.01):
    """sklearn's clusters and float64 means -> (centres [k,3] float64, the number of point pairs whose float64 distance lies within
    1e-5 eps of eps: the decision boundary of the eps-graph, which must be empty)."""
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN
    labels = DBSCAN(eps=eps, min_samples=2).fit(pts).labels_
    p64 = pts.astype(np.float64)
    ref = np.array([p64[labels == i].mean(axis=0) for i in range(labels.max() + 1)]).reshape(-1, 3)
    tree = cKDTree(p64)
    near = int(tree.count_neighbors(tree, eps * (1 + 1e-5))) - int(tree.count_neighbors(tree, eps * (1 - 1e-5)))
    return torch.tensor(ref, dtype=F64), near


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------
def f32(x):
    """The float32 rounding of a Python number, as a Python float: what a C `float` argument of the ABI holds."""
    return float(torch.tensor(x, dtype=torch.float32))


def adam_inputs(sizes, steps, seed):
    """Parameters ~ N(0,1) and per-step gradients, tensor k scaled by 10^(-6 + 9 k / (n - 1)) (1e-6 .. 1e3; a single tensor: 1), every 13th element 0."""
    g = gen(seed)
    n = len(sizes)
    p0 = [torch.randn(s, generator=g) for s in sizes]
    grads = []
    for _ in range(steps):
        row = []
        for k, s in enumerate(sizes):
            t = torch.randn(s, generator=g) * (10.0 ** (-6 + 9 * k / (n - 1)) if n > 1 else 1.0)
            t[torch.arange(s) % 13 == 5] = 0.0
            row.append(t)
        grads.append(row)
    return p0, grads


def adam_reference(p0, grads, lr, betas, eps, keep, dtype=F64):
    """torch.optim.Adam's formula (amsgrad=False, weight_decay=0), per-tensor step counts; grads[t][k] None = no gradient: the tensor
    does not step.  -> {step: (params, exp_avg, exp_avg_sq, step counts)} for the steps in `keep` (1-based)."""
    b1, b2 = betas
    p = [t.to(dtype).clone() for t in p0]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    count = [0] * len(p)
    out = {}
    for t, row in enumerate(grads, 1):
        for k, gk in enumerate(row):
            if gk is None:
                continue
            gk = gk.to(dtype)
            count[k] += 1
            m[k] = b1 * m[k] + (1 - b1) * gk
            v[k] = b2 * v[k] + (1 - b2) * gk * gk
            bc1, bc2 = 1 - b1 ** count[k], 1 - b2 ** count[k]
            p[k] = p[k] - (lr / bc1) * (m[k] / (v[k].sqrt() / math.sqrt(bc2) + eps))
        if t in keep:
            out[t] = ([x.clone() for x in p], [x.clone() for x in m], [x.clone() for x in v], list(count))
    return out
