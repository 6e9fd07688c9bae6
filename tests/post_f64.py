"""Restatement of the reference's post-processing rules, written from reading code/evaluation/fusion.py (:79-141), refinement.py
(:95-198) and nms.py (:156-204).  fuse and refine are float64; snap's cell arithmetic is literal numpy float32 (the reference's
arithmetic) and its distances are float64.  Each function also returns the margin of its decisions: the smallest relative distance of a
compared quantity from the value at which the decision flips (cost against threshold, score against keep, coordinate against the image
border, best against runner-up).  `torch_*` are the float32 torch siblings of the same rules (scripts/post_time.py times them).
"""
import numpy as np

from tests.parse_f64 import project


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def view_costs(lines3d, view):
    """-> uv [n,4], dis1 [n,m], dis2 [n,m] (dis2: the detection against the reversed line; fusion.py :107-108, refinement.py :140-141)."""
    uv = project(view["K"], view["pose"], np.asarray(lines3d, np.float64).reshape(-1, 3))
    g = np.asarray(view["det"], np.float64)[:, :4]
    d1 = ((uv[:, None, :] - g[None]) ** 2).sum(-1)
    d2 = ((uv[:, None, [2, 3, 0, 1]] - g[None]) ** 2).sum(-1)
    return uv, d1, d2


def _best(d1, d2, thr):
    """-> idx [n] (lowest index of min(dis1, dis2)), cost [n], nan rows, margin of cost against thr and of best against runner-up."""
    d = np.minimum(d1, d2)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(d).any(1)
    dd = np.where(np.isnan(d), np.inf, d)
    idx = dd.argmin(1)
    cost = dd[np.arange(len(dd)), idx]
    margin = np.inf
    for i in range(len(dd)):
        if bad[i] or not np.isfinite(cost[i]):
            continue
        margin = min(margin, _rel(cost[i], thr))
        if cost[i] < thr and dd.shape[1] > 1:
            ru = np.partition(dd[i], 1)[1]
            if ru != cost[i] or (dd[i] == cost[i]).sum() == 1:       # an exact duplicate is decided by the index rule, not by arithmetic
                margin = min(margin, _rel(ru, cost[i]))
    return idx, cost, bad, margin


def fuse(lines3d, views, dis=10.0, keep=0.5, by_label=False):
    """fusion.py :85-133.  views: dicts with K, pose (cam-to-world), det [m,5].  -> dict(score, count, keep, lines3d, margin)."""
    L = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    n = len(L)
    scores, counts, margin = np.zeros(n), np.zeros(n), np.inf
    for view in views:
        det = np.asarray(view["det"], np.float64)
        if len(det) == 0 or n == 0:
            continue                                                     # the reference raises on an empty view; here it sees nothing
        _, d1, d2 = view_costs(L, view)
        idx, cost, bad, mg = _best(d1, d2, dis)
        margin = min(margin, mg)
        avail = ~bad & (cost < dis)                                      # :114
        label_set = np.unique(idx[avail])                                # :116
        for i, label in enumerate(label_set):                            # :119: i = rank of the label among the matched labels
            cur = avail & (idx == label)
            scores[cur] += det[label if by_label else i, 4]              # :121
            counts[cur] += 1
    score = scores / np.maximum(counts, 1)                               # :131
    for s in score:
        margin = min(margin, _rel(s, keep))
    kept = score > keep                                                  # :133
    return {"score": score, "count": counts.astype(np.int64), "keep": kept, "lines3d": L[kept], "margin": margin}


def refine(lines3d, views, width, height, dis=10.0):
    """refinement.py :114-181, without the unused points3d_all.  -> dict(lines3d, sizes (set size after each view), groups (largest
    group), margin)."""
    L = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    margin, sizes, largest = np.inf, [], 0
    for view in views:
        det = np.asarray(view["det"], np.float64)
        if len(det) == 0 or len(L) == 0:
            sizes.append(len(L))
            continue
        uv, d1, d2 = view_costs(L, view)
        with np.errstate(invalid="ignore"):
            inside = ((uv[:, [0, 2]] >= 0).all(1) & (uv[:, [1, 3]] >= 0).all(1) & (uv[:, [0, 2]] <= width).all(1)
                      & (uv[:, [1, 3]] <= height).all(1))                # :135
        idx, cost, bad, mg = _best(d1, d2, dis)
        margin = min(margin, mg)
        for i in range(len(L)):
            if not bad[i] and cost[i] < dis:
                for c, hi in zip(uv[i], (width, height, width, height)):
                    for b in (0.0, float(hi)):
                        if c != b:                                       # exactly on the border is inside by the comparison itself
                            margin = min(margin, abs(c - b) / max(hi, 1.0))
        possible = inside & ~bad & (cost < dis)                          # :147
        if not possible.any():                                           # :148
            sizes.append(len(L))
            continue
        ar = np.arange(len(L))
        reverse = possible & (d2[ar, idx] < d1[ar, idx])                 # :150: mindis != mindis1
        for i in np.nonzero(possible)[0]:
            a, b = d1[i, idx[i]], d2[i, idx[i]]
            if a != b:
                margin = min(margin, _rel(a, b))
        wait = L.copy()
        wait[reverse] = wait[reverse][:, [1, 0]]                         # :159
        means = []
        for it in np.unique(idx[possible]):                              # :162-175
            sel = possible & (idx == it)
            largest = max(largest, int(sel.sum()))
            means.append(wait[sel].mean(0))
        L = np.concatenate([L[~possible], np.stack(means)])              # :179-181
        sizes.append(len(L))
    return {"lines3d": L, "sizes": sizes, "groups": largest, "margin": margin}


# ---- snap ------------------------------------------------------------------------------------------------------------------------------
def linspace_f32(lo, hi, G):
    """torch.linspace(lo, hi, G) in float32 on the CPU: lo + step i below the middle, hi - step (G - 1 - i) from it on, each one fused
    multiply-add (the product of two float32 is exact in float64, so one rounding to float32 is the fused result)."""
    lo, hi = np.float32(lo), np.float32(hi)
    step = np.float32(np.float32(hi - lo) / np.float32(G - 1))
    i = np.arange(G)
    a = (np.float64(lo) + np.float64(step) * i).astype(np.float32)
    b = (np.float64(hi) - np.float64(step) * (G - 1 - i)).astype(np.float32)
    return np.where(i < G // 2, a, b)


def cells_f32(points, G):
    """nms.py :162-175 in literal numpy float32: -> cells [M,3] int64, bbox_min, bbox_max, delta.  A zero-extent axis (the reference
    divides by zero there) has cell 0."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    delta = (hi - lo) / np.float32(G - 1)
    assert delta.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (p - lo[None]) / delta
    q = np.where(delta[None] > 0, q, np.float32(0))
    return np.array(q.round(), dtype=np.int64), lo, hi, delta


def snap(lines3d, G=512, max_snap=None, unique=False):
    """nms.py :158-200.  -> dict(junctions [P,3] float32, count [P], edges [E,2], lines3d, cells [M,3], nearest [M], margin)."""
    L32 = np.asarray(lines3d, np.float32).reshape(-1, 2, 3)
    cells, lo, hi, _ = cells_f32(L32, G)
    occ, cnt = np.unique(cells, axis=0, return_counts=True)               # :179 (sorted rows = row-major order)
    table = {tuple(c): int(k) for c, k in zip(occ, cnt)}
    peaks = []
    for c, k in zip(occ, cnt):                                            # :182-184: max_pool3d(3, padding 1) == grid and > 0
        best = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    best = max(best, table.get((c[0] + dx, c[1] + dy, c[2] + dz), 0))
        if k >= best:
            peaks.append((tuple(c), int(k)))
    axes = [linspace_f32(lo[a], hi[a], G) for a in range(3)]
    junc = np.array([[axes[a][c[a]] for a in range(3)] for c, _ in peaks], np.float32).reshape(-1, 3)
    pts = L32.reshape(-1, 3).astype(np.float64)
    d = ((pts[:, None] - junc.astype(np.float64)[None]) ** 2).sum(-1)    # :191-194
    near = d.argmin(1)
    dmin = d[np.arange(len(pts)), near]
    margin = np.inf
    if d.shape[1] > 1:
        ru = np.partition(d, 1, axis=1)[:, 1]
        for a, b in zip(dmin, ru):
            if b != a:
                margin = min(margin, abs(b - a) / max(b, 1e-30))
    pair = near.reshape(-1, 2)
    keep = np.ones(len(pair), bool)
    if max_snap is not None:
        moved = np.sqrt(dmin).reshape(-1, 2)
        keep = (moved < max_snap).all(1)
        for m in moved.reshape(-1):
            margin = min(margin, _rel(m, max_snap))
    edges = pair[keep]
    if unique:
        e = np.sort(edges[edges[:, 0] != edges[:, 1]], axis=1)
        edges = np.unique(e, axis=0) if len(e) else e.reshape(0, 2)
    return {"junctions": junc, "count": np.array([k for _, k in peaks], np.int64), "edges": edges.astype(np.int64).reshape(-1, 2),
            "lines3d": junc[edges.reshape(-1, 2)].reshape(-1, 2, 3), "cells": cells, "nearest": near, "margin": margin}


# ---- float32 torch siblings (any device) --------------------------------------------------------------------------------------------------
def _torch_project(view, L):
    import torch
    K, pose = view["K"], view["pose"]
    w2c = torch.linalg.inv(pose)[:3]
    cam = (K[:3, :3] @ (w2c[:, :3] @ L.reshape(-1, 3).T + w2c[:, 3:])).T
    return (cam[:, :2] / cam[:, 2:]).reshape(-1, 4)


def _torch_best(uv, g, chunk=4096):
    import torch
    cost, idx, d1b = [], [], []
    for s in range(0, len(uv), chunk):
        u = uv[s:s + chunk]
        d1 = ((u[:, None] - g[None]) ** 2).sum(-1)
        d2 = ((u[:, None, [2, 3, 0, 1]] - g[None]) ** 2).sum(-1)
        c, i = torch.minimum(d1, d2).min(1)
        cost.append(c), idx.append(i), d1b.append(d1.gather(1, i[:, None])[:, 0])
    return torch.cat(cost), torch.cat(idx), torch.cat(d1b)


def torch_fuse(L, views, dis=10.0, keep=0.5):
    import torch
    scores, counts = torch.zeros(len(L), device=L.device), torch.zeros(len(L), device=L.device)
    for view in views:
        det = view["det"]
        cost, idx, _ = _torch_best(_torch_project(view, L), det[:, :4])
        avail = cost < dis
        present = torch.zeros(len(det), device=L.device, dtype=torch.long)
        present[idx[avail]] = 1
        rank = torch.cumsum(present, 0) - present
        scores += torch.where(avail, det[rank[idx], 4], torch.zeros_like(scores))
        counts += avail
    return L[scores / counts.clamp(min=1) > keep]


def torch_refine(L, views, width, height, dis=10.0):
    import torch
    for view in views:
        det = view["det"]
        uv = _torch_project(view, L)
        cost, idx, d1 = _torch_best(uv, det[:, :4])
        possible = ((uv >= 0).all(1) & (uv[:, [0, 2]] <= width).all(1) & (uv[:, [1, 3]] <= height).all(1) & (cost < dis))
        if not bool(possible.any()):
            continue
        rev = possible & (cost != d1)
        W = torch.where(rev[:, None, None], L[:, [1, 0]], L)[possible]
        lab, inv = torch.unique(idx[possible], return_inverse=True)
        s = torch.zeros(len(lab), 2, 3, device=L.device).index_add_(0, inv, W)
        c = torch.zeros(len(lab), device=L.device).index_add_(0, inv, torch.ones(len(inv), device=L.device))
        L = torch.cat([L[~possible], s / c[:, None, None]])
    return L


def torch_snap(L, G=512, chunk=2048):
    import torch
    p = L.reshape(-1, 3)
    lo, hi = p.min(0)[0], p.max(0)[0]
    cells = ((p - lo) / ((hi - lo) / (G - 1))).round().long()
    occ, cnt = torch.unique(cells, dim=0, return_counts=True)
    grid = torch.zeros(G, G, G, device=L.device)
    grid[occ[:, 0], occ[:, 1], occ[:, 2]] = cnt.float()
    pool = torch.nn.functional.max_pool3d(grid[None], 3, padding=1, stride=1)
    idx = ((pool == grid) & (pool > 0))[0].nonzero()
    axes = [torch.linspace(float(lo[a]), float(hi[a]), G, device=L.device) for a in range(3)]
    junc = torch.stack([axes[a][idx[:, a]] for a in range(3)], -1)
    near = torch.cat([((p[s:s + chunk, None] - junc[None]) ** 2).sum(-1).argmin(1) for s in range(0, len(p), chunk)])
    return junc, near.reshape(-1, 2)
