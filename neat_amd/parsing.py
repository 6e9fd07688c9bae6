"""Wireframe parsing of a trained model: the reference's code/neat-final-parsing.py (initial_recon :159-302,
get_wireframe_from_lines_and_junctions :134-157, visibility_checking :305-336) on the device.

    junctions = refined_junctions(model)                  # step 1: ffn(latents), one SDF projection, sorted by SDF value
    result = distil(junctions, views)                     # steps 2b-7 from per-view model outputs (ABI v15 kernels)
    result, timing = wireframe_recon(model, dataset)      # step 2's chunked eval forward + distil

`distil` issues no host synchronisation while it walks the views (every data-dependent size stays on the device, buffers are sized by
their bounds); it synchronises once, at the end, to slice the outputs.  Divergence from the reference: if no junction receives two
votes the reference fails in `torch.stack([])`; here the results are empty and a warning goes to stderr.
"""
import sys
import time

import torch

from . import ops
from .general import split_input

RESULT_KEYS = ("junctions3d_initial", "lines3d_all", "graph_initial", "lines3d_wfi", "lines3d_wfi_checked")


def refined_junctions(model, refine=True):
    """Step 1 (:173-185): g = ffn(latents); with refine, g - sdf * grad, then sorted by the SDF value at the refined points."""
    with torch.no_grad():
        g = model._global_junctions() if hasattr(model, "_global_junctions") else model.ffn(model.latents)
        g = g.detach()
        if not refine:
            return g
        net = model.implicit_network
        sdf, _, grad = net.get_outputs(g)
        g = (g - sdf * grad).detach()
        s = net.get_sdf_vals(g).flatten()
        return g[torch.argsort(s)]


def _dev(t, device, dtype=torch.float32):
    return torch.as_tensor(t).to(device=device, dtype=dtype, non_blocking=True)


def _pack_gt(gts, device):
    """Ground-truth lines of every view [m_v, >= 4] -> packed [sum m_v, 4] and offsets int32 [V+1] (both on the device)."""
    offs = [0]
    for g in gts:
        offs.append(offs[-1] + int(g.shape[0]))
    rows = [_dev(g, device)[:, :4] for g in gts if g.shape[0] > 0]
    packed = torch.cat(rows).contiguous() if rows else torch.zeros(0, 4, device=device)
    return packed, _dev(torch.tensor(offs, dtype=torch.int32), device, torch.int32)


def _cameras(Ks, poses, device):
    """K3 [V,3,3] and w2c [V,3,4] = the first three rows of pose^-1 (neat_camera_mats per view)."""
    K3, w2c = [], []
    for K, pose in zip(Ks, poses):
        w, k = ops.camera_mats(_dev(pose, device).reshape(4, 4).contiguous(), _dev(K, device))
        K3.append(k)
        w2c.append(w)
    if not K3:
        return torch.zeros(0, 3, 3, device=device), torch.zeros(0, 3, 4, device=device)
    return torch.stack(K3), torch.stack(w2c)


def visibility(lines, gts, Ks, poses, ckdist=100.0, ckview=5, n_lines=None):
    """Step 7 (:305-336): -> (vis_count [E] int32, checked [E,2,3], n_checked int32 [1]) on the device, no synchronisation.
    gts: per view ground-truth lines [m_v, >= 4] (line_segments(0.05)); Ks: intrinsics [>= 3, >= 3]; poses [4,4] cam-to-world."""
    device = lines.device
    gt, off = _pack_gt(gts, device)
    K3, w2c = _cameras(Ks, poses, device)
    return ops.parse_visibility(lines, n_lines, gt, off, K3, w2c, ckdist, ckview)


def distil_device(junctions, views, *, line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0,
                  ckview=5):
    """Steps 2b-7 without any host synchronisation: -> the padded device state (see distil)."""
    device = junctions.device
    junctions = junctions.detach().float().contiguous()
    J, V = junctions.shape[0], len(views)
    mcap = max([int(v["gt_lines_001"].shape[0]) for v in views] + [1])
    vlines = torch.empty(max(V, 1), mcap, 2, 3, device=device)
    vscores = torch.empty(max(V, 1), mcap, device=device)
    vcount = torch.zeros(max(V, 1), device=device, dtype=torch.int32)
    votes = torch.zeros(max(J, 1), device=device, dtype=torch.int32)
    first = torch.zeros(max(J, 1), 2, device=device, dtype=torch.int32)
    for v, view in enumerate(views):
        gt = _dev(view["gt_lines_001"], device)
        lines2d = _dev(view["lines2d"], device).reshape(-1, 4)
        label, _ = ops.parse_match(lines2d, gt, line_dis_threshold)
        ops.parse_group(label, _dev(view["lines3d"], device), _dev(view["l3d"], device), int(gt.shape[0]),
                        out=(vlines[v], vscores[v], vcount[v:v + 1]))
        if J > 0:
            ops.parse_vote(junctions, vlines[v], vcount[v:v + 1], junc_match_threshold, v, votes, first)
    g = ops.parse_graph(vlines[:V], vscores[:V], vcount[:V], line_score_threshold, junctions, votes[:J], first[:J])
    vis_count, checked, n_checked = visibility(g["wfi"], [v["gt_lines_005"] for v in views], [v["K"] for v in views],
                                               [v["pose"] for v in views], ckdist, ckview, n_lines=g["counts"][2:3])
    return {"graph": g, "vis_count": vis_count, "checked": checked, "n_checked": n_checked, "votes": votes[:J], "first": first[:J],
            "vcount": vcount[:V], "J": J}


def distil(junctions, views, *, line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0, ckview=5):
    """Steps 2b-7 of the reference from per-view model outputs.

    junctions [J,3] as refined_junctions returns them; views: a list of dicts with `lines3d` [n,2,3], `lines2d` [n,4], `l3d` [n,3] (the
    eval forward over the view's masked pixels), `gt_lines_001` / `gt_lines_005` (wireframe.line_segments(0.01) / (0.05)), `K` and
    `pose`.  -> the reference's keys: junctions3d_initial [K,3], lines3d_all [N,2,3], graph_initial [K,K] (0/1 float), lines3d_wfi
    [E,2,3], lines3d_wfi_checked [E2,2,3], all on the junctions' device."""
    st = distil_device(junctions, views, line_dis_threshold=line_dis_threshold, line_score_threshold=line_score_threshold,
                       junc_match_threshold=junc_match_threshold, ckdist=ckdist, ckview=ckview)
    return finish(st)


def finish(st):
    """The one synchronisation: read the counts and slice the padded outputs."""
    g, J = st["graph"], st["J"]
    N, K, E, E2 = torch.cat([g["counts"], st["n_checked"]]).cpu().tolist()
    if K == 0:
        print("[neat_amd.parsing] no junction received two votes: the wireframe is empty (the reference fails here in torch.stack([]))",
              file=sys.stderr, flush=True)
    return {"junctions3d_initial": g["junctions"][:K], "lines3d_all": g["lines"][:N],
            "graph_initial": g["graph"][:J * J].view(J, J)[:K, :K].float() if J > 0 else g["junctions"].new_zeros(0, 0),
            "lines3d_wfi": g["wfi"][:E], "lines3d_wfi_checked": st["checked"][:E2]}


def view_inputs(dataset, idx, device):
    """One view of a dataset as the eval forward reads it, restricted to its masked pixels (:191-201)."""
    _, sample, _ = dataset[idx]
    mask = sample["mask"].to(device).reshape(-1).bool()
    keep = mask.nonzero().flatten()
    wf = sample["wireframe"]
    inp = {"uv": sample["uv"].to(device)[keep][None], "uv_proj": sample["uv_proj"].to(device)[keep][None],
           "intrinsics": sample["intrinsics"].to(device)[None], "pose": sample["pose"].to(device)[None], "wireframe": [wf]}
    return inp, int(keep.numel())


def wireframe_recon(model, dataset, *, chunksize=2048, line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02,
                    ckdist=100.0, ckview=5, sdf_junction_refine=True, device=None):
    """Step 2's chunked eval forward (model(s) under eval / no_grad on `chunksize` rays) over every view, then distil.
    -> (result dict, {"forward_s", "post_s", "views"}): the forward time includes the junction refinement; "views" = what distil read."""
    device = device or next(model.parameters()).device
    model.eval()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    junctions = refined_junctions(model, sdf_junction_refine)
    views = []
    with torch.no_grad():
        for i in range(len(dataset)):
            inp, n = view_inputs(dataset, i, device)
            outs = [model(s) for s in split_input(inp, n, n_pixels=chunksize)] if n > 0 else []
            cat = lambda k, w: torch.cat([o[k].detach().reshape(-1, *w) for o in outs]) if outs else torch.zeros(0, *w, device=device)
            wf = inp["wireframe"][0]
            views.append({"lines3d": cat("lines3d", (2, 3)), "lines2d": cat("lines2d", (4,)), "l3d": cat("l3d", (3,)),
                          "gt_lines_001": wf.line_segments(0.01), "gt_lines_005": wf.line_segments(0.05),
                          "K": inp["intrinsics"][0, :3, :3], "pose": inp["pose"][0]})
    torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    result = distil(junctions, views, line_dis_threshold=line_dis_threshold, line_score_threshold=line_score_threshold,
                    junc_match_threshold=junc_match_threshold, ckdist=ckdist, ckview=ckview)
    torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    return result, {"forward_s": t1 - t0, "post_s": t2 - t1, "views": views}
