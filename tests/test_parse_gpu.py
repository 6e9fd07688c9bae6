"""GPU: the wireframe parsing kernels (ABI v15) and neat_amd.parsing / python -m neat_amd.parse against the reference's recorded
outputs (golden G19), a float64 restatement (tests/parse_f64.py) and torch, at tile and LDS-chunk edges."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import parse_f64 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = dict(line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0, ckview=5)
GT_CHUNK = 1024          # kernels_parse.hpp PARSE_GT_CHUNK


def golden_views(g, device):
    keys = ("lines3d", "lines2d", "l3d", "gt_lines_001", "gt_lines_005", "K", "pose")
    return [{k: torch.tensor(g[f"v{v}_{k}"]).to(device) for k in keys} for v in range(int(g["n_views"]))]


def close(a, ref, what, rel=1e-6):
    a = a.detach().cpu().double().numpy()
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if ref.size:
        assert np.all(np.abs(a - ref) <= rel * np.maximum(1.0, np.abs(ref))), (what, float(np.abs(a - ref).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [1, 0])
def test_distil_reproduces_reference(golden, refine):
    from neat_amd import ops, parsing
    dev = torch.device("cuda:0")
    g = golden("g19_final_parsing")
    views = golden_views(g, dev)
    junc = torch.tensor(g[f"junctions_refine{refine}"]).to(dev)
    res = parsing.distil(junc, views, **THR)
    for k in parsing.RESULT_KEYS:
        close(res[k], g[f"r{refine}_{k}"], k)
    assert torch.equal(res["graph_initial"].cpu(), torch.tensor(g[f"r{refine}_graph_initial"]))
    # the discrete intermediates against the float64 restatement (which reproduces the reference: tests/test_parse_math.py)
    f = F.distil(g[f"junctions_refine{refine}"], [{k: v.cpu().numpy() for k, v in vw.items()} for vw in views], **THR)
    st = parsing.distil_device(junc, views, **THR)
    for v, vw in enumerate(views):
        label, mindis = ops.parse_match(vw["lines2d"], vw["gt_lines_001"], THR["line_dis_threshold"])
        assert np.array_equal(label.cpu().numpy(), f["labels"][v]), v
        assert int(st["vcount"][v]) == len(np.unique(f["labels"][v][f["labels"][v] >= 0]))
    assert np.array_equal(st["votes"].cpu().numpy(), f["votes"])
    assert np.array_equal(st["vis_count"][:len(f["vis_count"])].cpu().numpy(), f["vis_count"])
    E = int(st["graph"]["counts"][2])
    assert [tuple(p) for p in st["graph"]["pairs"][:E].cpu().tolist()] == f["edges"]
    assert any(i == j for i, j in f["edges"])          # the diagonal edge is there


def _match_case(n, m, seed, device):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0, 64, (max(m, 1), 5)).astype(np.float32)[:m]
    if m >= 6:
        gt[5] = gt[2]                                   # a duplicate: the lowest index must win
    rows = rng.uniform(0, 64, (n, 4)).astype(np.float32)
    if m > 0:
        pick = rng.integers(0, m, n)
        near = gt[pick, :4] + rng.normal(0, 1.0, (n, 4)).astype(np.float32)
        flip = rng.random(n) < 0.5
        near[flip] = near[flip][:, [2, 3, 0, 1]]
        use = rng.random(n) < 0.7
        rows[use] = near[use]
    if m >= 6:
        rows[0] = gt[2, :4] + 0.1                       # nearest to the duplicated pair 2 / 5
    if n > 3:
        rows[1 + rng.choice(n - 1, 3, replace=False), rng.integers(0, 4)] = np.nan
    return torch.tensor(rows).to(device), torch.tensor(gt.reshape(m, 5)).to(device)


def _torch_match(rows, gt):
    """float32 torch: dis [2n, m] in row chunks -> min, argmin, runner-up."""
    l = torch.cat([rows, rows[:, [2, 3, 0, 1]]])
    mins, args, seconds = [], [], []
    for c in torch.split(l, 4096):
        d = ((c[:, None] - gt[None, :, :4]) ** 2).sum(-1)
        top = torch.topk(torch.nan_to_num(d, nan=float("inf")), min(2, d.shape[1]), dim=1, largest=False)
        mn, am = d.min(dim=1)
        mins.append(mn)
        args.append(am)
        seconds.append(top.values[:, 1] if d.shape[1] > 1 else torch.full_like(mn, float("inf")))
    return torch.cat(mins), torch.cat(args), torch.cat(seconds)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(n, m) for n in (1, 63, 64, 65, 257, 4097) for m in (0, 1, 63, 64, 65, GT_CHUNK - 1, GT_CHUNK + 1, 5000)]
                         + [(200000, 5000), (200000, 65)])
def test_line_match_vs_torch(n, m):
    from neat_amd import ops
    dev = torch.device("cuda:0")
    rows, gt = _match_case(n, m, n * 7 + m, dev)
    thr = 10.0
    label, mindis = ops.parse_match(rows, gt, thr)
    assert label.shape == (2 * n,) and mindis.shape == (2 * n,)
    if m == 0:
        assert (label == -1).all() and torch.isinf(mindis).all()
        return
    mn, am, sec = _torch_match(rows, gt)
    nan = torch.isnan(mn)
    assert torch.equal(torch.isnan(mindis), nan) and (label[nan] == -1).all()
    ok = ~nan
    assert torch.all((mindis[ok] - mn[ok]).abs() <= 1e-6 * mn[ok].abs().clamp_min(1.0))
    safe = ok & ((mn - thr).abs() > 1e-5 * thr) & (torch.isinf(sec) | ((sec - mn) > 1e-5 * sec.clamp_min(1e-30)))
    ref = torch.where(mn < thr, am, torch.full_like(am, -1)).to(torch.int32)
    assert torch.equal(label[safe], ref[safe])
    tie = ((am == 2) | (am == 5)) if m >= 6 else torch.zeros_like(ok)     # rows nearest the duplicated pair: an exact tie
    assert safe[ok & ~tie].float().mean() > 0.99
    if m >= 6:                                          # on the tie the lower index wins
        assert int(label[0]) == 2 and not (label == 5).any()
        assert (label[ok & tie & (mn < thr * (1 - 1e-5))] == 2).all()
    # nothing matched
    label0, _ = ops.parse_match(rows, gt, 0.0)
    assert (label0 == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,seed", [(1, 1, 0), (300, 7, 1), (5000, 40, 2), (70000, 300, 3),
                                      (6000, 1500, 4)])      # 1500 labels: the scan over the labels (one workgroup of 1024) carries into a second round
def test_group_deterministic_and_vs_float64(n, m, seed):
    from neat_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    lines3d = rng.normal(0, 1, (n, 2, 3)).astype(np.float32)
    l3d = rng.normal(0, 1, (n, 3)).astype(np.float32)
    used = rng.choice(m, max(1, m // 3), replace=False)        # sparse labels
    label = np.where(rng.random(2 * n) < 0.6, rng.choice(used, 2 * n), -1).astype(np.int32)
    if n > 1:
        single = sorted(set(range(m)) - set(used))[:1]         # a label with a single row
        if single:
            label[n // 2] = single[0]
    lab_t = torch.tensor(label).to(dev)
    a = ops.parse_group(lab_t, torch.tensor(lines3d).to(dev), torch.tensor(l3d).to(dev), m)
    b = ops.parse_group(lab_t, torch.tensor(lines3d).to(dev), torch.tensor(l3d).to(dev), m)
    L = int(a[2])
    assert L == int(b[2]) and torch.equal(a[0][:L], b[0][:L]) and torch.equal(a[1][:L], b[1][:L])
    labs, lines, scores = F.group(label, lines3d, l3d)
    assert L == len(labs)
    close(a[0][:L], lines, "lines")
    close(a[1][:L], scores, "scores")


def _vis_case(seed, ms, device):
    rng = np.random.default_rng(seed)
    E = 300
    lines = rng.uniform(-0.5, 0.5, (E, 2, 3))
    views = []
    for v, m in enumerate(ms):
        ang = 2 * np.pi * v / len(ms)
        c = np.array([3 * np.cos(ang), 3 * np.sin(ang), 1.0])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, -R @ c
        K = np.array([[300.0, 0, 256], [0, 300.0, 256], [0, 0, 1]])
        pose = np.linalg.inv(w2c)
        proj = F.project(K, pose, lines)
        gt = rng.uniform(0, 512, (m, 5))
        take = rng.choice(E, min(m // 2, E), replace=False)
        gt[:len(take), :4] = proj[take] + rng.normal(0, 2.0, (len(take), 4))
        views.append({"gt_lines_005": gt.astype(np.float32), "K": K.astype(np.float32), "pose": pose.astype(np.float32)})
    return lines.astype(np.float32), views


@pytest.mark.gpu
def test_visibility_ragged_views_and_empty_cases():
    from neat_amd import parsing
    dev = torch.device("cuda:0")
    ms = [0, 1, 70, GT_CHUNK + 5, 1500, 3]
    lines, views = _vis_case(0, ms, dev)
    lt = torch.tensor(lines).to(dev)
    cnt, checked, n_checked = parsing.visibility(lt, [torch.tensor(v["gt_lines_005"]).to(dev) for v in views],
                                                 [torch.tensor(v["K"]).to(dev) for v in views],
                                                 [torch.tensor(v["pose"]).to(dev) for v in views], 100.0, 2)
    ref, _ = F.visibility(lines.astype(np.float64), views, 100.0)
    # per (line, view) float64 distance from the threshold: compare the counts of the lines without a near-threshold decision
    safe = np.ones(len(lines), bool)
    for v in views:
        g = np.asarray(v["gt_lines_005"], np.float64)[:, :4]
        if len(g) == 0:
            continue
        u = F.project(v["K"], v["pose"], lines.astype(np.float64))
        d = np.minimum(((u[:, None] - g[None]) ** 2).sum(-1), ((u[:, None] - g[None][:, :, [2, 3, 0, 1]]) ** 2).sum(-1)).min(1)
        safe &= np.abs(d - 100.0) > 1e-4 * 100.0
    assert safe.mean() > 0.95
    assert np.array_equal(cnt.cpu().numpy()[safe], ref[safe])
    assert (cnt.cpu().numpy() <= len(ms) - 1).all()              # the view without ground-truth lines sees nothing
    keep = cnt.cpu().numpy() >= 2
    n = int(n_checked)
    assert n == keep.sum() and torch.equal(checked[:n].cpu(), lt.cpu()[torch.tensor(keep)])
    # no lines at all
    cnt0, _, n0 = parsing.visibility(lt[:0], [torch.tensor(v["gt_lines_005"]).to(dev) for v in views],
                                     [torch.tensor(v["K"]).to(dev) for v in views], [torch.tensor(v["pose"]).to(dev) for v in views])
    assert cnt0.numel() == 0 and int(n0) == 0


@pytest.mark.gpu
def test_no_junctions_gives_empty_results(golden, capsys):
    from neat_amd import parsing
    dev = torch.device("cuda:0")
    g = golden("g19_final_parsing")
    views = golden_views(g, dev)
    for junc in (torch.zeros(0, 3, device=dev), torch.full((8, 3), 50.0, device=dev)):     # none / none near the lines: no votes
        res = parsing.distil(junc, views, **THR)
        assert res["junctions3d_initial"].shape == (0, 3) and res["graph_initial"].shape == (0, 0)
        assert res["lines3d_wfi"].shape == (0, 2, 3) and res["lines3d_wfi_checked"].shape == (0, 2, 3)
        assert res["lines3d_all"].shape[0] > 0
    assert "no junction received two votes" in capsys.readouterr().err


@pytest.mark.gpu
def test_distil_does_not_synchronise_per_view(golden):
    from neat_amd import parsing
    dev = torch.device("cuda:0")
    g = golden("g19_final_parsing")
    views = golden_views(g, dev)
    junc = torch.tensor(g["junctions_refine1"]).to(dev)
    parsing.finish(parsing.distil_device(junc, views, **THR))          # warm-up: library load, first launches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        st = parsing.distil_device(junc, views, **THR)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    res = parsing.finish(st)
    close(res["lines3d_wfi"], g["r1_lines3d_wfi"], "wfi")


def _f64_restatement(junc, views, thr):
    """The reference's steps 3-7 in float64 (tests/parse_f64.py) over the same model outputs, with each decision's margin."""
    dv = [{k: (v.detach().cpu().double() if torch.is_tensor(v) else v) for k, v in vw.items()} for vw in views]
    f = F.distil(junc.detach().cpu().double().numpy(), [{k: v.numpy() for k, v in vw.items()} for vw in dv], **thr)
    return f


@pytest.mark.gpu
def test_cli_end_to_end_on_a_runner_checkpoint(tmp_path):
    from neat_amd import parsing, run_io, synth
    from neat_amd.parse import out_basename
    from neat_amd.runner import TrainRunner
    from tests.test_runner import _toy_scene, _hocon
    _toy_scene(tmp_path / "data" / "abc" / "toy", n_views=6)
    conf = {"train": {"expname": "toy_parse", "dataset_class": "datasets.blender_hawp_dataset.BlenderDataset",
                      "model_class": "model.networks.neat_wfr_rend_a.VolSDFNetwork", "loss_class": "model.networks.loss_wfr.VolSDFLoss",
                      "learning_rate": 5.0e-4, "num_pixels": 128, "checkpoint_freq": 1},
            "loss": dict(synth.ABC_NEAT_A_LOSS_CONF),
            "dataset": {"data_dir": "abc/toy", "img_res": [64, 64], "reverse_coordinate": True},
            "model": synth.ABC_NEAT_A_MODEL_CONF}
    path = tmp_path / "toy.conf"
    path.write_text(_hocon(conf))
    runner = TrainRunner(str(path), nepochs=1, exps_folder=str(tmp_path / "exps"), data_root=str(tmp_path / "data"), log_freq=100)
    runner.run()
    run_dir = os.path.dirname(runner.checkpoints_path)
    # the runner replays captured graphs: release them now, not in a garbage collection during some later test's capture
    del runner
    torch.cuda.synchronize()
    gc.collect()
    conf_path = os.path.join(run_dir, "runconf.conf")
    with open(conf_path, "w") as fh:
        fh.write(_hocon(conf))
    # --ckview 1: a one-epoch model on a 64 x 64 toy scene sees few lines in five views
    args = [sys.executable, "-m", "neat_amd.parse", "--conf", conf_path, "--data_root", str(tmp_path / "data"), "--ckview", "1",
            "--reproj-dis", "50", "--junc_match_threshold", "0.2"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "post-processing" in p.stdout
    base = out_basename(conf_path, "latest", 50, True)
    wdir = os.path.join(run_dir, "wireframes")
    for key in ("all", "wfi", "wfi_checked"):
        assert os.path.exists(os.path.join(wdir, f"{base}-{key}.npz")), os.listdir(wdir)
    saved = torch.load(os.path.join(wdir, f"{base}-neat.pth"), map_location="cpu")
    assert saved["kwargs"]["distance"] == 50 and saved["kwargs"]["sdf_junction_refine"] is True
    # the same model outputs through the test-side float64 restatement
    dev = torch.device("cuda:0")
    model, _, _, conf_read = run_io.load_model(conf_path, "latest", dev)
    dataset = run_io.build_dataset(conf_read, str(tmp_path / "data"), distance_threshold=1.0)
    thr = dict(line_dis_threshold=50, line_score_threshold=0.01, junc_match_threshold=0.2, ckdist=100.0, ckview=1)
    res, info = parsing.wireframe_recon(model, dataset, device=dev, **{k: v for k, v in thr.items() if k != "line_score_threshold"})
    junc = parsing.refined_junctions(model)
    f = _f64_restatement(junc, info["views"], thr)
    for k in parsing.RESULT_KEYS:          # the CLI's files hold what the library computes on the same model
        got = np.load(os.path.join(wdir, f"{base}-{k.replace('lines3d_', '')}.npz"))["lines3d"] if k.startswith("lines3d") else None
        if got is not None:
            assert np.array_equal(got, res[k].cpu().numpy()), k
    if f["margin"] > 1e-5:
        for k in parsing.RESULT_KEYS:
            close(res[k], f[k], k, rel=1e-5)
    else:
        print(f"end-to-end: a decision within {f['margin']:.1e} of flipping; counts only: "
              f"N {len(res['lines3d_all'])}/{len(f['lines3d_all'])}, K {len(res['junctions3d_initial'])}/{len(f['junctions3d_initial'])}")
    # a second run without --overwrite reuses the .pth
    p2 = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p2.returncode == 0, p2.stdout[-3000:] + p2.stderr[-3000:]
    assert "reusing" in p2.stdout and "post-processing" not in p2.stdout
    again = torch.load(os.path.join(wdir, f"{base}-neat.pth"), map_location="cpu")
    assert torch.equal(again["lines3d_wfi_checked"], saved["lines3d_wfi_checked"])
