"""The four evaluation scripts of the reference (code/evaluation/eval-dtu.py, eval-lsr-dtu.py, eval-wfr-dtu.py, eval-abc.py) restated in
numpy / scipy on arrays: the oracle of neat_amd.evaluate on the box.  Squared distances are ((dx dx) + dy dy) + dz dz, the order of
sklearn's kd-tree; the thinning is the sequential loop; nearest points come from brute force (exact, small clouds) or from
scipy.spatial.cKDTree (large clouds, tree=True).  thin_rounds emulates the device's round rule."""
import warnings

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial import cKDTree


def d2_rows(p, cloud):
    """squared distances of one point (or [m,1,3] points) to the cloud, in the kd-tree's order"""
    d = p - cloud
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def sample_mesh(verts, faces, density):
    """eval-dtu.py:48-71 -> the vertices followed by the lattice samples, triangle-major, then i, then j."""
    verts = np.asarray(verts, dtype=np.float64)
    tri = verts[np.asarray(faces)]
    v1, v2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    out = [verts]
    for t in np.nonzero((area2 > 0)[:, 0])[0]:
        thr = density * np.sqrt(l1[t] * l2[t] / area2[t])
        n1, n2 = float(np.floor(l1[t] / thr)[0]), float(np.floor(l2[t] / thr)[0])
        k0 = (np.arange(int(n1) + 1, dtype=np.float64) + 0.5) / max(n1, 1e-7)
        k1 = (np.arange(int(n2) + 1, dtype=np.float64) + 0.5) / max(n2, 1e-7)
        inside = (k0[:, None] + k1[None, :]) < 1
        i, j = np.nonzero(inside)
        out.append(v1[t:t + 1] * k0[i, None] + v2[t:t + 1] * k1[j, None] + tri[t:t + 1, 0])
    return np.concatenate(out, axis=0)


def thin_sequential(points, radius):
    """-> bool mask: point c stays iff no earlier staying point lies within radius (<=)."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    r2 = radius * radius
    gone = np.zeros(n, dtype=bool)
    for c in range(n):
        if gone[c]:
            continue
        gone[c + 1:] |= d2_rows(points[c], points[c + 1:]) <= r2
    return ~gone


def neighbours(points, radius):
    """lists of the earlier points within radius of every point (brute force, exact)"""
    points = np.asarray(points, dtype=np.float64)
    r2 = radius * radius
    return [np.nonzero(d2_rows(points[c], points[:c]) <= r2)[0] for c in range(points.shape[0])]


def thin_rounds(points, radius):
    """The device's rule, a round at a time on a snapshot of the states -> (bool mask, rounds)."""
    nb = neighbours(points, radius)
    n = len(nb)
    state = np.zeros(n, dtype=np.int8)          # 0 undecided, 1 kept, 2 removed
    rounds = 0
    while (state == 0).any():
        rounds += 1
        if rounds > n:
            raise RuntimeError("the rounds do not converge")
        new = state.copy()
        for c in np.nonzero(state == 0)[0]:
            s = state[nb[c]]
            if (s == 1).any():
                new[c] = 2
            elif (s == 2).all():
                new[c] = 1
        state = new
    return state == 1, rounds


def nearest_brute(cloud, queries, chunk=256):
    """-> (distance, index of the nearest cloud point; ties: the lowest index), float64, exact order of operations."""
    cloud, queries = np.asarray(cloud, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    m = queries.shape[0]
    dist, idx = np.full(m, np.inf), np.full(m, -1, dtype=np.int64)
    if cloud.shape[0] == 0:
        return dist, idx
    for i0 in range(0, m, chunk):
        d2 = d2_rows(queries[i0:i0 + chunk, None, :], cloud[None])
        k = d2.argmin(1)
        idx[i0:i0 + chunk] = k
        dist[i0:i0 + chunk] = np.sqrt(d2[np.arange(len(k)), k])
    return dist, idx


def nearest_tree(cloud, queries, workers=16):
    d, i = cKDTree(cloud).query(queries, k=1, workers=workers)
    return d, i


def obs_flags(points, obs_mask, bb, res, patch=60.0, f32_quotient=False):
    """eval-dtu.py:98-110 -> uint8: bit 0 inside the padded box, bit 1 also in an observed voxel."""
    points = np.asarray(points, dtype=np.float64)
    bb = np.asarray(bb).astype(np.float32)
    inbound = ((points >= bb[:1] - patch) & (points < bb[1:] + patch * 2)).sum(axis=-1) == 3
    q = (points - bb[:1]) / np.float64(res)
    g = np.around(q.astype(np.float32)).astype(np.int64) if f32_quotient else np.around(q).astype(np.int64)
    shape = np.array(np.asarray(obs_mask).shape)[None]
    gin = ((g >= 0) & (g < shape)).sum(axis=-1) == 3
    gc = np.where(gin[:, None], g, 0)
    obs = np.asarray(obs_mask)[gc[:, 0], gc[:, 1], gc[:, 2]].astype(bool)
    return inbound.astype(np.uint8) | ((inbound & gin & obs).astype(np.uint8) << 1)


def mean_below(d, max_dist):
    return d[d < max_dist].mean()


def dtu_scores(points, stl, obs_mask, bb, res, plane, density=0.2, patch=60.0, max_dist=20.0, order=None, f32_quotient=False,
               thinning=True, tree=False, details=None):
    """steps 2-4 -> (mean data->stl, mean stl->data)"""
    points, stl = np.asarray(points, dtype=np.float64), np.asarray(stl, dtype=np.float64)
    seq = points[order] if order is not None else points
    if thinning:
        if tree:
            nb = cKDTree(seq).query_ball_point(seq, density, workers=16)
            mask = np.ones(len(seq), dtype=bool)
            for c, idxs in enumerate(nb):
                if mask[c]:
                    mask[idxs] = False
                    mask[c] = True
        else:
            mask = thin_sequential(seq, density)
        data_down = seq[mask]
    else:
        data_down = seq
    flags = obs_flags(data_down, obs_mask, bb, res, patch, f32_quotient)
    data_in, data_in_obs = data_down[(flags & 1) != 0], data_down[(flags & 2) != 0]
    hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (np.asarray(plane, dtype=np.float64).reshape((1, 4)) * hom).sum(-1) > 0
    near = nearest_tree if tree else nearest_brute
    d2s = near(stl, data_in_obs)[0]
    s2d = near(data_in, stl[above])[0]
    if details is not None:
        details.update(data_down=data_down, flags=flags, above=above, dist_d2s=d2s, dist_s2d=s2d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return mean_below(d2s, max_dist), mean_below(s2d, max_dist)


def scale_points(scale_mat, x):
    h = scale_mat @ np.concatenate([x, np.ones([x.shape[0], 1])], axis=-1).T
    return h[:3].transpose(1, 0)


def line_cloud(lines3d, scale_mat):
    """eval-lsr-dtu.py:64-81 -> (32 points per line through the scale matrix, mean length)"""
    lines3d = np.asarray(lines3d)
    e = np.concatenate((lines3d.reshape(-1, 3), np.ones((2 * lines3d.shape[0], 1))), axis=1)
    e = scale_mat @ e.T
    e = (e[:3] / e[3:]).T.reshape(-1, 2, 3)
    mean_length = np.mean(np.linalg.norm(e[:, 0] - e[:, 1], axis=1))
    t = np.linspace(0, 1, 32).reshape(1, -1, 1)
    pts = ((lines3d[:, :1] * t) + (lines3d[:, 1:] * (1 - t))).reshape(-1, 3)
    return scale_points(scale_mat, pts), mean_length


def junction_cloud(lines3d, scale_mat):
    """eval-wfr-dtu.py:111, :31-32: unique end points (lexicographic rows) through the scale matrix"""
    j = np.unique(np.asarray(lines3d).reshape(-1, 3), axis=0)
    return scale_points(scale_mat, j), j.shape[0]


def abc_costs(junctions_pred, lines_pred, junctions_gt, edges_gt, offset_scale):
    off = [float(v) for v in offset_scale]
    s = 1.0 / off[-1]
    m = np.array([[s, 0, 0, -off[0]], [0, s, 0, -off[1]], [0, 0, s, -off[2]], [0, 0, 0, 1.0]])
    jg = np.asarray(junctions_gt, dtype=np.float64)
    jp = (np.asarray(junctions_pred) @ m[:3, :3].T) + m[:3, 3]
    lp = ((np.asarray(lines_pred).reshape(-1, 3) @ m[:3, :3].T) + m[:3, 3]).reshape(-1, 2, 3)
    lg = jg[np.asarray(edges_gt)]
    cj = np.linalg.norm(jp[:, None] - jg[None], axis=-1)
    c1 = np.linalg.norm(lp[:, None, :] - lg[None, :, :], axis=-1).mean(axis=-1)
    c2 = np.linalg.norm(lp[:, None, :] - lg[None, :, [1, 0]], axis=-1).mean(axis=-1)
    return cj, np.minimum(c1, c2), m[0, 0]


def abc_scores(junctions_pred, lines_pred, junctions_gt, edges_gt, offset_scale, thresholds=(0.01, 0.02, 0.05)):
    cj, cl, scale = abc_costs(junctions_pred, lines_pred, junctions_gt, edges_gt, offset_scale)
    res = {}
    for name, c in (("junctions", cj), ("lines", cl)):
        cost = c[linear_sum_assignment(c)]
        correct = [int((cost < th * scale).sum()) for th in thresholds]
        res[name + "_correct"] = correct
        res[name + "_precision"] = [k / c.shape[0] for k in correct]
        res[name + "_recall"] = [k / c.shape[1] for k in correct]
    return res
