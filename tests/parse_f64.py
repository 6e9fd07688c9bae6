"""Float64 numpy restatement of the wireframe parsing (code/neat-final-parsing.py :191-336, steps 2b-7 of neat_amd/parsing.py), with
the distance of every thresholded decision and every argmin from flipping.  Used by tests/test_parse_math.py (against the reference's
recorded outputs), tests/test_parse_gpu.py (discrete intermediates) and tests/golden/make_parse_golden.py (margins of a draw)."""
import numpy as np
from scipy.optimize import linear_sum_assignment


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def match(lines2d, gt, thr):
    """-> label [2n] (-1 = none), mindis [2n], margin (smallest relative distance of a decision from flipping)."""
    l = np.asarray(lines2d, np.float64).reshape(-1, 4)
    rows = np.concatenate([l, l[:, [2, 3, 0, 1]]])
    g = np.asarray(gt, np.float64)[:, :4]
    if g.shape[0] == 0:
        return np.full(len(rows), -1), np.full(len(rows), np.inf), np.inf
    d = ((rows[:, None, :] - g[None]) ** 2).sum(-1)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(d).any(1)
        dd = np.where(np.isnan(d), np.inf, d)
        idx = dd.argmin(1)
        mind = dd[np.arange(len(rows)), idx]
    label = np.where(~bad & (mind < thr), idx, -1)
    margin = np.inf
    for r in np.nonzero(~bad)[0]:
        margin = min(margin, _rel(mind[r], thr))
        if label[r] >= 0 and g.shape[0] > 1:
            second = np.partition(dd[r], 1)[1]
            margin = min(margin, (second - mind[r]) / max(second, 1e-30))
    return label, np.where(bad, np.nan, mind), margin


def group(label, lines3d, l3d):
    """-> labels present (ascending), lines [L,2,3], scores [L]."""
    L3 = np.asarray(lines3d, np.float64).reshape(-1, 2, 3)
    rows3 = np.concatenate([L3, L3[:, [1, 0]]])
    p = np.asarray(l3d, np.float64).reshape(-1, 3)
    pts = np.concatenate([p, p])
    labs = np.unique(label[label >= 0])
    lines, scores = [], []
    for lab in labs:
        idx = np.nonzero(label == lab)[0]
        v = rows3[idx].mean(0)
        s = pts[idx]
        dist = np.linalg.norm(np.cross(s - v[0], s - v[1]), axis=-1) / max(np.linalg.norm(v[1] - v[0]), 1e-6)
        lines.append(v)
        scores.append(dist.mean())
    return labs, np.array(lines).reshape(-1, 2, 3), np.array(scores)


def cdist(a, b):
    return np.sqrt(((np.asarray(a, np.float64)[:, None] - np.asarray(b, np.float64)[None]) ** 2).sum(-1))


def vote(junctions, lines, thr):
    """-> [(junction, pair index)] of the pairs with cost < thr (rows ascending), the pairs, margin."""
    ep = lines.reshape(-1, 3)
    if len(ep) == 0 or len(junctions) == 0:
        return [], (np.zeros(0, int), np.zeros(0, int)), np.inf
    cost = cdist(junctions, ep)
    r, c = linear_sum_assignment(cost)
    out, margin = [], np.inf
    for k, (i, j) in enumerate(zip(r, c)):
        margin = min(margin, _rel(cost[i, j], thr))
        if cost[i, j] < thr:
            out.append((int(i), k))
    return out, (r, c), margin


def wireframe(lines, junctions):
    """get_wireframe_from_lines_and_junctions with rel_matching_distance_threshold = 0 -> graph [K,K], edges [(i, j)], margin."""
    K = len(junctions)
    graph = np.zeros((K, K))
    margin = np.inf
    if K == 0:
        return graph, [], margin
    ep1, ep2 = lines[:, 0], lines[:, 1]
    c1, c2 = cdist(ep1, junctions), cdist(ep2, junctions)
    i1, i2 = c1.argmin(1), c2.argmin(1)
    m1, m2 = c1.min(1), c2.min(1)
    length = np.linalg.norm(ep1 - ep2, axis=-1)
    for t in range(len(lines)):
        margin = min(margin, _rel(max(m1[t], m2[t]), length[t]))
        if K > 1:
            for c in (c1[t], c2[t]):
                s = np.sort(c)
                margin = min(margin, (s[1] - s[0]) / max(s[1], 1e-30))
        if max(m1[t], m2[t]) < length[t]:
            a, b = min(i1[t], i2[t]), max(i1[t], i2[t])
            graph[a, b] = graph[b, a] = 1
    edges = [(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(graph)))]
    return graph, edges, margin


def project(K, pose, X):
    w2c = np.linalg.inv(np.asarray(pose, np.float64))[:3]
    cam = (np.asarray(K, np.float64)[:3, :3] @ (w2c[:, :3] @ X.reshape(-1, 3).T + w2c[:, 3:])).T
    w = cam[:, 2:]
    w = w + np.where(np.abs(w) < 1e-8, 1e-8, 0.0) * np.where(w >= 0, 1.0, -1.0)
    return (cam / w)[:, :2].reshape(-1, 4)


def visibility(lines, views, ckdist):
    """-> per-line visible-view counts, margin."""
    cnt = np.zeros(len(lines), int)
    margin = np.inf
    for v in views:
        g = np.asarray(v["gt_lines_005"], np.float64)[:, :4]
        if len(lines) == 0 or len(g) == 0:
            continue
        u = project(v["K"], v["pose"], lines)
        d1 = ((u[:, None] - g[None]) ** 2).sum(-1)
        d2 = ((u[:, None] - g[None][:, :, [2, 3, 0, 1]]) ** 2).sum(-1)
        m = np.minimum(d1, d2).min(1)
        cnt += m < ckdist
        margin = min(margin, min(_rel(x, ckdist) for x in m))
    return cnt, margin


def distil(junctions, views, line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0, ckview=5):
    """-> dict with the reference's keys, the discrete intermediates (labels, votes, first-vote order, pairs, visibility counts) and
    `margin`, the smallest relative distance of any decision from flipping."""
    junctions = np.asarray(junctions, np.float64)
    first, votes = {}, np.zeros(len(junctions), int)
    margin = np.inf
    all_lines, all_scores, labels, pairs = [], [], [], []
    for vi, v in enumerate(views):
        lab, _, m = match(v["lines2d"], v["gt_lines_001"], line_dis_threshold)
        margin = min(margin, m)
        labels.append(lab)
        labs, lines, scores = group(lab, v["lines3d"], v["l3d"])
        if len(labs) == 0:
            pairs.append(None)
            continue
        for s in scores:
            margin = min(margin, _rel(s, line_score_threshold))
        got, pr, m = vote(junctions, lines, junc_match_threshold)
        pairs.append(pr)
        margin = min(margin, m)
        for j, k in got:
            votes[j] += 1
            first.setdefault(j, (vi, k))
        all_lines.append(lines)
        all_scores.append(scores)
    lines_all = np.concatenate(all_lines) if all_lines else np.zeros((0, 2, 3))
    scores_all = np.concatenate(all_scores) if all_scores else np.zeros(0)
    lines_all = lines_all[scores_all < line_score_threshold]
    order = [j for j in first if votes[j] > 1]          # dict insertion order = order of the first votes
    junc = junctions[order].reshape(-1, 3)
    graph, edges, m = wireframe(lines_all, junc)
    margin = min(margin, m)
    wfi = np.array([[junc[i], junc[j]] for i, j in edges]).reshape(-1, 2, 3)
    cnt, m = visibility(wfi, views, ckdist)
    margin = min(margin, m)
    return {"junctions3d_initial": junc, "lines3d_all": lines_all, "graph_initial": graph, "lines3d_wfi": wfi,
            "lines3d_wfi_checked": wfi[cnt >= ckview], "labels": labels, "votes": votes, "order": order, "edges": edges,
            "vis_count": cnt, "pairs": pairs, "margin": margin}
