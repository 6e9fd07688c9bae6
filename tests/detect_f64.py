"""The 2-D line-segment detector of neat_amd.detect (csrc/kernels_detect.hpp), restated in numpy float64: this file is the definition
(DESIGN 3j).  An a-contrario detector of the LSD family whose line-support regions are those of Burns, Hanson and Riseman: connected
components of the quantised gradient orientation in two overlapping partitions, so nothing depends on an order of visits.

Every float64 value is formed by the same IEEE operations, in the same order, as on the device: no fused multiply-add (numpy has
none), sums of a region taken one pixel after the other in ascending pixel index (np.cumsum is sequential; np.sum is pairwise and is
not used for them), and no transcendental function before the NFA.  The only values that may differ from the device's in the last
bits are therefore the NFA's (lgamma, exp, log).

    labels(codes)                     uint8 [V,h,w], 255 = unused -> int32 [V,h,w]: smallest linear index of the 8-connected component
    detect(images, scale, ...)        uint8 [V,H,W,3] or [V,H,W] -> dict (lines, width, nfa, n, k, view, part, label, offsets, judge ...)
    two_polygons(), rectangles(), noise()        the pictures of the tests
"""
import math

import numpy as np
from scipy import ndimage

JUDGE_EPS = 1e-9


def constants(Hs, Ws, q=2.0, tau_deg=22.5):
    """The host-side constants of an image of Hs x Ws grey pixels (after scaling)."""
    tau = tau_deg * math.pi / 180.0
    p = tau_deg / 180.0
    logNT = 2.5 * (math.log10(Ws) + math.log10(Hs))
    return {"rho2": (q / math.sin(tau)) ** 2, "c1": math.sqrt(2.0) - 1.0, "cos_tau": math.cos(tau), "p": p, "logNT": logNT,
            "min_reg": int(math.floor(-logNT / math.log10(p))) + 1}


def scaled_size(size, scale):
    return int(math.ceil(scale * size))


def gaussian_taps(out, scale):
    """The sampled Gaussian of sigma = 0.6 / scale for each of `out` output positions: taps [out, 2 h + 1] (normalised by their
    sequential sum) and the source index of the first tap (before clamping to the image)."""
    sigma = 0.6 / scale
    h = int(math.ceil(3.0 * sigma))
    xc = np.arange(out, dtype=np.float64) / scale
    first = np.floor(xc + 0.5).astype(np.int64) - h
    j = first[:, None] + np.arange(2 * h + 1)[None, :]
    d = (j.astype(np.float64) - xc[:, None]) / sigma
    wgt = np.exp(-0.5 * (d * d))
    return wgt / np.cumsum(wgt, axis=1)[:, -1:], first


def grey(images, scale=1.0):
    """uint8 [V,H,W,3] or [V,H,W] -> float64 [V,Hs,Ws]."""
    images = np.asarray(images)
    assert images.dtype == np.uint8
    if images.ndim == 4:
        c = images.astype(np.int64)
        g = (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
    else:
        g = images.astype(np.int64)
    g = g.astype(np.float64)
    if scale == 1.0:
        return g
    V, H, W = g.shape
    Hs, Ws = scaled_size(H, scale), scaled_size(W, scale)
    tx, fx = gaussian_taps(Ws, scale)
    ty, fy = gaussian_taps(Hs, scale)
    tmp = np.zeros((V, H, Ws))
    for t in range(tx.shape[1]):                       # fixed tap order, acc = acc + w * g
        tmp = tmp + tx[None, None, :, t] * g[:, :, np.clip(fx + t, 0, W - 1)]
    out = np.zeros((V, Hs, Ws))
    for t in range(ty.shape[1]):
        out = out + ty[None, :, t, None] * tmp[:, np.clip(fy + t, 0, H - 1), :]
    return out


def gradient(g):
    """float64 [Hs,Ws] -> gx, gy, m2 on the (Hs-1) x (Ws-1) grid of 2 x 2 blocks a b / c d."""
    a, b, c, d = g[:-1, :-1], g[:-1, 1:], g[1:, :-1], g[1:, 1:]
    gx = ((b + d) - (a + c)) * 0.5
    gy = ((c + d) - (a + b)) * 0.5
    return gx, gy, gx * gx + gy * gy


def orientation_codes(gx, gy, m2, rho2, c1):
    """-> uint8 [2,h,w]: the octant in partition 0 (boundaries at k 45 deg) and 1 (at 22.5 + k 45 deg); 255 = unused."""
    used = m2 >= rho2
    ax, ay = np.abs(gx), np.abs(gy)
    sx, sy = gx < 0, gy < 0
    code0 = sy * 4 + sx * 2 + (ay > ax)
    not_h, not_v = ay > c1 * ax, ax > c1 * ay
    quad = np.where(sx, np.where(sy, 5, 3), np.where(sy, 7, 1))
    code1 = np.where(~not_h, np.where(sx, 4, 0), np.where(~not_v, np.where(sy, 6, 2), quad))
    return np.stack([np.where(used, code0, 255), np.where(used, code1, 255)]).astype(np.uint8)


def label_map(code):
    """uint8 [h,w] -> int32 [h,w]: per pixel the smallest linear index of its 8-connected component of equal code; -1 for code 255."""
    h, w = code.shape
    out = np.full((h, w), -1, dtype=np.int32)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    for c in np.unique(code):
        if c == 255:
            continue
        lab, n = ndimage.label(code == c, structure=np.ones((3, 3), dtype=bool))
        mins = np.asarray(ndimage.minimum(idx, lab, index=np.arange(1, n + 1)), dtype=np.int64).reshape(-1)
        sel = lab > 0
        out[sel] = mins[lab[sel] - 1]
    return out


def labels(codes):
    codes = np.asarray(codes, dtype=np.uint8)
    return np.stack([label_map(c) for c in codes]) if codes.shape[0] else np.zeros(codes.shape, np.int32)


def log10_binomial_tail(n, k, p):
    """log10 of sum_{i=k..n} C(n,i) p^i (1-p)^(n-i), through lgamma and a log-sum-exp."""
    i = np.arange(k, n + 1, dtype=np.float64)
    lg = np.vectorize(math.lgamma, otypes=[np.float64])
    t = math.lgamma(n + 1.0) - lg(i + 1.0) - lg(n - i + 1.0) + i * math.log(p) + (n - i) * math.log(1.0 - p)
    m = t.max()
    return (m + math.log(np.exp(t - m).sum())) / math.log(10.0)


def _seq(x):
    return np.cumsum(x)[-1]


def _region(idx, gx, gy, m2, used, c, density):
    """One kept line-support region (idx: its pixels' linear indices, ascending) -> its rectangle, counts, score and judge flag."""
    h, w = gx.shape
    x, y = (idx % w).astype(np.float64), (idx // w).astype(np.float64)
    fgx, fgy, fm2 = gx.reshape(-1)[idx], gy.reshape(-1)[idx], m2.reshape(-1)[idx]
    wt = np.sqrt(fm2)
    sumw = _seq(wt)
    cx, cy = _seq(wt * x) / sumw, _seq(wt * y) / sumw
    dx, dy = x - cx, y - cy
    Ixx, Iyy, Ixy = _seq((wt * dy) * dy) / sumw, _seq((wt * dx) * dx) / sumw, -_seq((wt * dx) * dy) / sumw
    d = Ixx - Iyy
    lam = 0.5 * ((Ixx + Iyy) - math.sqrt(d * d + 4.0 * (Ixy * Ixy)))
    ux, uy = (Ixy, lam - Ixx) if abs(Ixx) > abs(Iyy) else (lam - Iyy, Ixy)
    nrm = math.sqrt(ux * ux + uy * uy)
    if nrm > 0.0:
        ux, uy = ux / nrm, uy / nrm
    else:
        ux, uy = 1.0, 0.0
    l, t = dx * ux + dy * uy, dy * ux - dx * uy
    l0, l1, t0, t1 = l.min(), l.max(), t.min(), t.max()
    S = _seq(fgy * ux - fgx * uy)
    s = float(S > 0) - float(S < 0)
    wd = t1 - t0
    pad = (1.0 - wd) * 0.5 if wd < 1.0 else 0.0
    t0p, t1p = t0 - pad, t1 + pad
    # the rectangle's bounding box (any superset of the rectangle gives the same counts)
    px = [cx + ll * ux - tt * uy for ll in (l0, l1) for tt in (t0p, t1p)]
    py = [cy + ll * uy + tt * ux for ll in (l0, l1) for tt in (t0p, t1p)]
    bx0, bx1 = max(int(math.floor(min(px))) - 1, 0), min(int(math.ceil(max(px))) + 1, w - 1)
    by0, by1 = max(int(math.floor(min(py))) - 1, 0), min(int(math.ceil(max(py))) + 1, h - 1)
    Y, X = np.meshgrid(np.arange(by0, by1 + 1), np.arange(bx0, bx1 + 1), indexing="ij")
    bdx, bdy = X.astype(np.float64) - cx, Y.astype(np.float64) - cy
    bl, bt = bdx * ux + bdy * uy, bdy * ux - bdx * uy
    inrect = (bl >= l0) & (bl <= l1) & (bt >= t0p) & (bt <= t1p)
    bgx, bgy, bm2, bused = (a[by0:by1 + 1, bx0:bx1 + 1] for a in (gx, gy, m2, used))
    gn = bgy * ux - bgx * uy
    thr = np.sqrt(bm2) * c["cos_tau"]
    aligned = inrect & bused & (gn * s > 0) & (np.abs(gn) >= thr)
    n, k = int(inrect.sum()), int(aligned.sum())
    dense = not (k < density * n)
    nfa = -(c["logNT"] + log10_binomial_tail(n, k, c["p"])) if dense else -math.inf
    # judge: a decision within JUDGE_EPS of its boundary (the region's own extremal pixels, which sit on it exactly, apart)
    own = np.zeros((h, w), dtype=bool)
    own.reshape(-1)[idx] = True
    bown = own[by0:by1 + 1, bx0:bx1 + 1]
    inside_other = (bl >= l0 - JUDGE_EPS) & (bl <= l1 + JUDGE_EPS) & (bt >= t0p - JUDGE_EPS) & (bt <= t1p + JUDGE_EPS)
    edge = np.zeros_like(inrect)
    for v, b in ((bl, l0), (bl, l1), (bt, t0p), (bt, t1p)):
        edge |= (np.abs(v - b) < JUDGE_EPS) & ~((v == b) & bown)
    judge = bool((edge & inside_other).any())
    judge |= abs(k - density * n) < JUDGE_EPS or abs(S) < JUDGE_EPS
    judge |= bool((inrect & bused & (np.abs(np.abs(gn) - thr) < JUDGE_EPS)).any())
    judge |= dense and abs(nfa) < JUDGE_EPS
    return {"line": ((cx + l0 * ux) + 0.5, (cy + l0 * uy) + 0.5, (cx + l1 * ux) + 0.5, (cy + l1 * uy) + 0.5), "width": wd, "nfa": nfa,
            "n": n, "k": k, "keep": dense and nfa > 0.0, "judge": judge}


def detect_view(g, scale=1.0, q=2.0, tau_deg=22.5, density=0.7):
    """One grey picture float64 [Hs,Ws] -> the candidate regions (size and votes passed) in (partition, label) order, each a dict."""
    Hs, Ws = g.shape
    if Hs < 2 or Ws < 2:
        return []
    c = constants(Hs, Ws, q, tau_deg)
    gx, gy, m2 = gradient(g)
    codes = orientation_codes(gx, gy, m2, c["rho2"], c["c1"])
    used = codes[0] != 255
    hw = gx.size
    lab = [label_map(codes[p]).reshape(-1) for p in (0, 1)]
    u = used.reshape(-1)
    size = [np.bincount(lab[p][u], minlength=hw) for p in (0, 1)]
    s0, s1 = size[0][np.maximum(lab[0], 0)], size[1][np.maximum(lab[1], 0)]
    vote0 = u & (s0 >= s1)
    votes = [np.bincount(lab[0][vote0], minlength=hw), np.bincount(lab[1][u & ~vote0], minlength=hw)]
    out = []
    for p in (0, 1):
        order = np.argsort(lab[p], kind="stable")            # pixels grouped by label, ascending index within a label
        sorted_lab = lab[p][order]
        for root in np.flatnonzero((size[p] >= c["min_reg"]) & (2 * votes[p] >= size[p]) & (size[p] > 0)):
            a, b = np.searchsorted(sorted_lab, root, "left"), np.searchsorted(sorted_lab, root, "right")
            r = _region(order[a:b], gx, gy, m2, used, c, density)
            r["line"] = tuple(v / scale for v in r["line"])
            r.update(part=p, label=int(root), size=int(size[p][root]))
            out.append(r)
    return out


def detect(images, scale=1.0, q=2.0, tau_deg=22.5, density=0.7):
    """-> dict of arrays over the KEPT regions in (view, partition, label) order: lines [N,4], width, nfa, n, k, view, part, label;
    offsets [V+1]; and over ALL candidate regions: cand [M,3] = (view, partition, label), cand_keep, cand_judge; grey [V,Hs,Ws]."""
    g = grey(images, scale)
    rows, cand = [], []
    offsets = [0]
    for v in range(g.shape[0]):
        for r in detect_view(g[v], scale, q, tau_deg, density):
            cand.append((v, r["part"], r["label"], r["keep"], r["judge"]))
            if r["keep"]:
                rows.append((v, r))
        offsets.append(len(rows))
    f = lambda key, dt: np.array([r[key] for _, r in rows], dtype=dt)
    cand = np.array(cand, dtype=np.int64).reshape(-1, 5)
    return {"lines": f("line", np.float64).reshape(-1, 4), "width": f("width", np.float64), "nfa": f("nfa", np.float64),
            "n": f("n", np.int32), "k": f("k", np.int32), "view": np.array([v for v, _ in rows], dtype=np.int32),
            "part": f("part", np.int32), "label": f("label", np.int32), "offsets": np.array(offsets, dtype=np.int32),
            "cand": cand[:, :3], "cand_keep": cand[:, 3].astype(bool), "cand_judge": cand[:, 4].astype(bool), "grey": g}


# ---- pictures -----------------------------------------------------------------------------------------------------------------------------------
def _inside(poly, X, Y):
    """Points inside a convex polygon (vertices in order, either orientation)."""
    poly = np.asarray(poly, dtype=np.float64)
    sign = None
    ok = np.ones(X.shape, dtype=bool)
    for (x0, y0), (x1, y1) in zip(poly, np.roll(poly, -1, axis=0)):
        cr = (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0)
        if sign is None:
            c = poly.mean(axis=0)
            sign = 1.0 if (x1 - x0) * (c[1] - y0) - (y1 - y0) * (c[0] - x0) > 0 else -1.0
        ok &= cr * sign >= 0
    return ok


def render_polygons(H, W, polys, background=40, ss=8):
    """Anti-aliased (ss x ss point samples a pixel) convex polygons [(vertices, grey)] painted in order -> uint8 [H,W].  Pixel (x, y)
    covers [x - 0.5, x + 0.5] x [y - 0.5, y + 0.5]: integer coordinates are pixel centres, as in the datasets."""
    o = (np.arange(ss) + 0.5) / ss - 0.5
    Y = (np.arange(H)[:, None, None, None] + o[None, None, :, None]) + np.zeros((1, W, 1, ss))
    X = (np.arange(W)[None, :, None, None] + o[None, None, None, :]) + np.zeros((H, 1, ss, 1))
    img = np.full((H, W, ss, ss), float(background))
    for verts, value in polys:
        img[_inside(verts, X, Y)] = float(value)
    return np.clip(np.floor(img.mean(axis=(2, 3)) + 0.5), 0, 255).astype(np.uint8)


# A segment ends where the turning gradient of a corner leaves the region's 45-degree sector, so it falls short of the corner by about a
# pixel; by more when the edge's normal lies near a sector boundary of the partition that holds it, or when the corner is sharp.  The
# picture's edges therefore keep their normals well inside a sector of one partition (a rectangle turned by 30 degrees with one corner
# pulled out, a triangle without a corner under 50 degrees).
QUAD = [(21.4, 5.0), (59.6, 27.0), (47.6, 55.0), (6.4, 31.0)]
TRIANGLE = [(56.4, 60.2), (86.7, 54.3), (82.1, 88.9)]


def two_polygons():
    """96 x 96: a quadrilateral (grey 200) and a triangle (120) on 40 -> (uint8 [96,96], the seven edges [7,4])."""
    img = render_polygons(96, 96, [(QUAD, 200), (TRIANGLE, 120)])
    edges = [a + b for poly in (QUAD, TRIANGLE) for a, b in zip(poly, poly[1:] + poly[:1])]
    return img, np.array(edges, dtype=np.float64)


def noise(H=96, W=96, sigma=20.0, seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(np.floor(128.0 + sigma * rng.standard_normal((H, W)) + 0.5), 0, 255).astype(np.uint8)


def rectangles(V=3, H=97, W=131, seed=5):
    """V colour pictures of four rotated rectangles each (12 in all), at angles away from the axes -> uint8 [V,H,W,3]."""
    rng = np.random.default_rng(seed)
    out = np.zeros((V, H, W, 3), dtype=np.uint8)
    for v in range(V):
        polys = []
        for q, (qx, qy) in enumerate(((0.27, 0.27), (0.75, 0.27), (0.27, 0.75), (0.75, 0.75))):
            ang = math.radians(rng.uniform(8.0, 82.0) + 90.0 * rng.integers(0, 4))
            a, b = rng.uniform(14.0, 20.0), rng.uniform(7.0, 11.0)
            cx, cy = qx * W + rng.uniform(-2, 2), qy * H + rng.uniform(-2, 2)
            ca, sa = math.cos(ang), math.sin(ang)
            polys.append(([(cx + sx * a * ca - sy * b * sa, cy + sx * a * sa + sy * b * ca) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))],
                          q))
        for ch in range(3):
            vals = rng.integers(110, 250, size=4)
            out[v, :, :, ch] = render_polygons(H, W, [(p, vals[i]) for p, i in polys], background=int(rng.integers(10, 60)), ss=4)
    return out


def endpoint_distance(a, b):
    """Sum of the two end-point distances between segments a and b [4], the better of the two directions."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = lambda p, q: math.hypot(p[0] - q[0], p[1] - q[1])
    return min(d(a[:2], b[:2]) + d(a[2:], b[2:]), d(a[:2], b[2:]) + d(a[2:], b[:2]))
