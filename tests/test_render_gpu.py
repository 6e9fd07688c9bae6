"""neat_amd.render on the device: the neat_frame_* kernels against tests/render_f64.py (exact: every step is one IEEE float32 operation),
and end to end on a checkpoint the runner wrote on the toy scene with vis_images=True."""
import ctypes
import gc
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from neat_amd import render
from tests import render_f64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ kernels
def _frame_case(H, W, seed):
    rng = np.random.default_rng(seed)
    P = H * W
    rgb = R.byte_inputs(rng, 3 * P).reshape(P, 3)
    nrm = rng.standard_normal((P, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * rng.uniform(0.999, 1.002, (P, 1))).astype(np.float32)      # length slightly above 1 too
    nrm.reshape(-1)[::7] = (R.byte_inputs(rng, len(nrm.reshape(-1)[::7])) * np.float32(2.0) - np.float32(1.0))
    depth = rng.uniform(0.5, 4.0, P).astype(np.float32)
    depth[rng.permutation(P)[:max(P // 10, 1)]] = rng.choice(np.array([np.inf, -np.inf, np.nan, 0.0], np.float32), max(P // 10, 1))
    gt = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    gt.reshape(-1)[::5] = R.byte_inputs(rng, len(gt.reshape(-1)[::5]))
    return rgb, nrm, depth, gt


def _sentinels(P):
    host = {"rgb8": np.full((P, 3), 77, np.uint8), "normal8": np.full((P, 3), 78, np.uint8), "depth": np.full(P, -7.0, np.float32),
            "err": np.full((P, 3), -9.0, np.float32)}
    return host, {k: _t(v) for k, v in host.items()}


def _same(dev, host):
    for k in host:
        assert np.array_equal(dev[k].cpu().numpy(), host[k], equal_nan=host[k].dtype.kind == "f"), k


@pytest.mark.parametrize("H,W", [(17, 19), (1, 1), (1, 70)])
def test_frame_put_writes_its_chunk_exactly_and_nothing_else(H, W):
    P, chunk = H * W, 100
    rgb, nrm, depth, gt = _frame_case(H, W, 10 * H + W)
    d_rgb, d_nrm, d_depth, d_gt = _t(rgb), _t(nrm), _t(depth), _t(gt)
    chunks = [(p0, min(chunk, P - p0)) for p0 in range(0, P, chunk)]
    assert (H, W) != (17, 19) or chunks[-1] == (300, 23)                                      # a ragged last chunk; p0 no multiple of 64
    put = lambda bufs, p0, n, with_gt=True: render.frame_put(d_rgb[p0:p0 + n], d_nrm[p0:p0 + n], d_depth[p0:p0 + n], d_gt if with_gt else None,
                                                             p0, P, bufs["rgb8"], bufs["normal8"], bufs["depth"], bufs["err"] if with_gt else None)
    # one chunk from the middle (the last of a short frame): every pixel outside it keeps its sentinel
    host, dev = _sentinels(P)
    p0, n = chunks[len(chunks) // 2]
    put(dev, p0, n)
    R.put(host, p0, rgb[p0:p0 + n], nrm[p0:p0 + n], depth[p0:p0 + n], gt)
    _same(dev, host)
    # all chunks: the whole frame, exactly; without gt the error plane is not touched
    host, dev = _sentinels(P)
    for p0, n in chunks:
        put(dev, p0, n, with_gt=False)
        R.put(host, p0, rgb[p0:p0 + n], nrm[p0:p0 + n], depth[p0:p0 + n], None)
    _same(dev, host)
    assert (host["err"] == -9.0).all() and np.array_equal(host["rgb8"], R.byte(rgb)) and np.array_equal(host["normal8"], R.normal_byte(nrm))
    for p0, n in chunks:
        put(dev, p0, n)
        R.put(host, p0, rgb[p0:p0 + n], nrm[p0:p0 + n], depth[p0:p0 + n], gt)
    _same(dev, host)
    assert np.array_equal(host["err"], R.sq_err(rgb, gt), equal_nan=True)
    # any subset of the inputs
    host, dev = _sentinels(P)
    render.frame_put(None, None, d_depth, None, 0, P, depth_out=dev["depth"])
    render.frame_put(d_rgb, None, None, d_gt, 0, P, err=dev["err"])
    host["depth"], host["err"] = depth.copy(), R.sq_err(rgb, gt)
    _same(dev, host)


def test_frame_put_refuses_a_chunk_outside_the_frame():
    """Return codes only: the entry point validates on the host and launches nothing, so the buffers keep their sentinels."""
    from neat_amd import _lib
    lib, P = _lib.lib(), 323
    host, dev = _sentinels(P)
    src = _t(np.zeros((100, 3), np.float32))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda n, p0, total=P: lib.neat_frame_put(ptr(src), None, None, None, n, p0, total, ptr(dev["rgb8"]), None, None, None, None)
    for n, p0 in ((100, -1), (-1, 0), (100, 224), (1, P), (100, 2 ** 40)):
        assert call(n, p0) != 0, (n, p0)
    assert call(10, 0, -5) != 0
    assert lib.neat_frame_put(None, ptr(src), None, None, 100, 0, P, None, None, None, None, None) != 0      # normals without their output
    assert lib.neat_frame_put(ptr(src), None, None, ptr(src), 100, 0, P, ptr(dev["rgb8"]), None, None, None, None) != 0      # gt without err
    torch.cuda.synchronize()
    _same(dev, host)
    assert call(100, 223) == 0 and call(0, P) == 0
    with pytest.raises(RuntimeError):
        render.frame_put(src, None, None, None, 300, P, rgb8=dev["rgb8"])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 969, 65537])
def test_frame_sum_is_a_float64_sum_and_repeats_bit_for_bit(n):
    rng = np.random.default_rng(n)
    x = (10.0 ** rng.uniform(-8.0, 0.0, n)).astype(np.float32)
    d = _t(x)
    a, b = render.frame_sum(d).item(), render.frame_sum(d).item()
    ref = R.exact_sum(x)
    print("n = %d: device %.17g, fsum %.17g, relative error %.3g (bound %.3g)" % (n, a, ref, abs(a - ref) / ref, n * 2.0 ** -53))
    assert abs(a - ref) <= n * 2.0 ** -53 * ref            # no float64 sum of n non-negative terms is further off
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    assert render.frame_sum(torch.empty(0, device=DEV)).item() == 0.0


def test_frame_range_and_grey_over_non_finite_values():
    rng = np.random.default_rng(5)
    mixed = rng.uniform(-3.0, 9.0, 70001).astype(np.float32)
    mixed[rng.permutation(mixed.size)[:3000]] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 3000)
    planes = {"mixed": mixed, "tiny": np.array([np.nan, 2.5, np.inf], np.float32), "none": np.array([np.nan, np.inf, -np.inf] * 100, np.float32),
              "constant": np.full(300, 1.25, np.float32), "one": np.array([-4.0], np.float32)}
    for name, x in planes.items():
        d = _t(x)
        rng_d = render.frame_range(d)
        lo, hi = R.finite_range(x)
        assert rng_d.cpu().numpy().tolist() == [float(lo), float(hi)], name
        assert np.array_equal(render.frame_grey(d, rng_d).cpu().numpy(), R.grey(x, lo, hi)), name
    assert R.finite_range(planes["none"]) == (0.0, 0.0) and not R.grey(planes["constant"], 1.25, 1.25).any()
    # a given scale: values below lo and above hi clamp; steps of the scale and their neighbours land on their bytes
    steps = (np.arange(256) / 255.0 * 3.0 + 1.0).astype(np.float32)
    x = np.concatenate([steps, np.nextafter(steps, np.float32(9)), np.nextafter(steps, np.float32(-9)), mixed[:5000]])
    got = render.frame_grey(_t(x), _t(np.array([1.0, 4.0], np.float32))).cpu().numpy()
    assert np.array_equal(got, R.grey(x, 1.0, 4.0)) and got.min() == 0 and got.max() == 255


@pytest.mark.parametrize("N,nrow,shape", [(1, 8, (5, 7)), (2, 1, (16, 11)), (3, 2, (16, 20)), (4, 8, (9, 38))])
def test_frame_grid_is_make_grid(N, nrow, shape):
    images = np.random.default_rng(N).integers(1, 256, (N, 5, 7, 3), dtype=np.uint8)
    got = render.grid(_t(images), nrow).cpu().numpy()
    assert got.shape == shape + (3,) and np.array_equal(got, R.make_grid(images, nrow))
    assert np.array_equal(render.grid([_t(im) for im in images], nrow).cpu().numpy(), got)


# ------------------------------------------------------------------ end to end
CONF_TRAIN = {"expname": "toy_render", "dataset_class": "datasets.blender_hawp_dataset.BlenderDataset",
              "model_class": "model.networks.neat_wfr_rend_a.VolSDFNetwork", "loss_class": "model.networks.loss_wfr.VolSDFLoss",
              "learning_rate": 5.0e-4, "num_pixels": 128, "checkpoint_freq": 1, "plot_freq": 1, "split_n_pixels": 1000}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Two epochs of the runner on the toy scene (64 x 64, 3 views) with vis_images=True, then the checkpoint loaded once."""
    from neat_amd import run_io, synth
    from neat_amd.runner import TrainRunner
    from tests.test_runner import _toy_scene, _hocon
    tmp = tmp_path_factory.mktemp("render")
    _toy_scene(tmp / "data" / "abc" / "toy", n_views=3)
    conf = {"train": dict(CONF_TRAIN), "plot": {"plot_nimgs": 1, "resolution": 40, "grid_boundary": [-1.5, 1.5]},
            "loss": dict(synth.ABC_NEAT_A_LOSS_CONF), "dataset": {"data_dir": "abc/toy", "img_res": [64, 64], "reverse_coordinate": True},
            "model": synth.ABC_NEAT_A_MODEL_CONF}
    path = tmp / "toy.conf"
    path.write_text(_hocon(conf))
    runner = TrainRunner(str(path), nepochs=2, exps_folder=str(tmp / "exps"), data_root=str(tmp / "data"), log_freq=100, vis_images=True)
    runner.run()
    run_dir = os.path.dirname(runner.checkpoints_path)
    stats = {"training": runner.model.training, "replays": runner.trainer.replays, "eager": runner.trainer.eager_steps,
             "capture_error": runner.trainer.capture_error}
    del runner
    torch.cuda.synchronize()
    gc.collect()
    conf_path = os.path.join(run_dir, "runconf.conf")
    with open(conf_path, "w") as fh:
        fh.write(_hocon(conf))
    model, epoch, root, conf_read = run_io.load_model(conf_path, "latest", torch.device(DEV))
    dataset = run_io.build_dataset(conf_read, str(tmp / "data"))
    assert epoch == 2 and root == run_dir and len(dataset) == 3
    return {"dir": run_dir, "conf": conf_path, "data": str(tmp / "data"), "model": model, "dataset": dataset, "stats": stats, "tmp": tmp}


def _forward_chunks(run, idx, chunk):
    """model(s) on the chunks of the whole view idx -> (rgb [P,3], normal [P,3], depth [P]) float32 numpy, and the per-chunk device outputs."""
    from neat_amd.general import split_input
    _, sample, _ = run["dataset"][idx]
    inp = {"uv": sample["uv"].to(DEV)[None], "uv_proj": sample["uv_proj"].to(DEV)[None], "intrinsics": sample["intrinsics"].to(DEV)[None],
           "pose": sample["pose"].to(DEV)[None], "wireframe": [sample["wireframe"]]}
    outs = []
    with torch.no_grad():
        for s in split_input(inp, inp["uv"].shape[1], n_pixels=chunk):
            o = run["model"](s)
            outs.append((s, o["rgb_values"], o["normal_map"], o["depth"]))
    cat = lambda k: torch.cat([o[k].reshape(-1, 3) if k < 3 else o[k].reshape(-1) for o in outs]).cpu().numpy()
    return (cat(1), cat(2), cat(3)), outs


_cache = {}


def _reference(run, idx=1, chunk=1000):
    if (idx, chunk) not in _cache:
        _cache[(idx, chunk)] = _forward_chunks(run, idx, chunk)
    return _cache[(idx, chunk)]


@pytest.mark.parametrize("chunk", [1000, 4096])
def test_render_pixels_is_the_forward_bit_for_bit(run, chunk):
    _, outs = _reference(run, 1, chunk)
    assert len(outs) == -(-4096 // chunk)
    for s, rgb, nmap, depth in outs:
        got = run["model"].render_pixels(s["uv"], s["pose"], s["intrinsics"])
        for name, a, b in zip(("rgb_values", "normal_map", "depth"), got, (rgb, nmap, depth)):
            assert a.shape == b.shape and torch.equal(a, b), (name, (a - b).abs().max().item())


def test_view_is_the_restatement_of_the_forward_chunks(run):
    (rgb, nmap, depth), _ = _reference(run, 1, 1000)
    uv, pose, K, gt, H, W = render.dataset_view(run["dataset"], 1, torch.device(DEV))
    res = render.view(run["model"], uv, pose, K, H, W, gt=gt, chunksize=1000)
    P = H * W
    assert np.array_equal(res["rgb"].cpu().numpy(), R.byte(rgb).reshape(H, W, 3))
    assert np.array_equal(res["normal"].cpu().numpy(), R.normal_byte(nmap).reshape(H, W, 3))
    assert np.array_equal(res["depth"].cpu().numpy(), depth.reshape(H, W), equal_nan=True)
    lo, hi = R.finite_range(depth)
    assert res["range"].cpu().numpy().tolist() == [float(lo), float(hi)] and hi > lo
    assert np.array_equal(res["depth8"].cpu().numpy(), R.grey(depth, lo, hi).reshape(H, W))
    e = R.sq_err(rgb, gt.cpu().numpy())
    mean_ref = R.exact_sum(e) / (3 * P)
    mean = res["sq_sum"] / (3 * P)
    print("mean of squares: device %.17g, float64 %.17g, relative error %.3g (bound %.3g); psnr %.6f" % (
        mean, mean_ref, abs(mean - mean_ref) / mean_ref, 3 * P * 2.0 ** -53, res["psnr"]))
    assert abs(mean - mean_ref) <= 3 * P * 2.0 ** -53 * mean_ref
    assert res["psnr"] == -10.0 * math.log10(mean) and abs(res["psnr"] - R.psnr(rgb, gt.cpu().numpy())) <= 1e-9
    # two calls: the same bytes; a subset of the maps and a given depth scale
    again = render.view(run["model"], uv, pose, K, H, W, gt=gt, chunksize=1000)
    for k in ("rgb", "normal", "depth", "depth8", "range"):
        assert again[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    assert again["psnr"] == res["psnr"] and again["sq_sum"] == res["sq_sum"]
    part = render.view(run["model"], uv[0], pose[0], K[0], H, W, chunksize=4096, maps=("depth",), depth_range=(1.0, 3.0))
    assert set(part) == {"psnr", "depth", "depth8", "range"} and part["psnr"] is None
    assert np.array_equal(part["depth8"].cpu().numpy(), R.grey(_reference(run, 1, 4096)[0][2], 1.0, 3.0).reshape(H, W))


def test_cam_json_pose_gives_the_dataset_frame(run, tmp_path):
    """A dataset view's inverse(pose) written as cam.json and read back the way the CLI reads it.  The toy scene's principal point is
    (W / 2, H / 2) and show.intrinsics (what --fov builds) puts it at ((W - 1) / 2, (H - 1) / 2), so --fov cannot reproduce the dataset's
    intrinsics: the comparison goes through render.view with the dataset's K and the pose of the --cam-json route."""
    dev = torch.device(DEV)
    uv, pose, K, gt, H, W = render.dataset_view(run["dataset"], 1, dev)
    with open(tmp_path / "cam.json", "w") as fh:
        json.dump([np.linalg.inv(pose[0].cpu().numpy().astype(np.float64)).tolist()], fh)
    with open(tmp_path / "cam.json") as fh:
        cams = np.asarray(json.load(fh), dtype=np.float64).reshape(-1, 4, 4)
    uv2, pose2, K2 = render.camera_view(cams[0], W, H, 60.0, dev)
    assert torch.equal(uv2, uv) and torch.allclose(pose2, pose, rtol=0.0, atol=1e-12) and K2.shape == (1, 4, 4)
    assert abs(K2[0, 1, 1].item() - 0.5 * H / math.tan(math.radians(30.0))) < 1e-4 and K2[0, 0, 2].item() == 0.5 * (W - 1)
    a = render.view(run["model"], uv, pose, K, H, W, chunksize=1000, maps=("rgb",))
    b = render.view(run["model"], uv2, pose2, K, H, W, chunksize=1000, maps=("rgb",))
    assert torch.equal(a["rgb"], b["rgb"])


def test_runner_pictures_and_replays(run):
    from PIL import Image
    st = run["stats"]
    # epoch 0 steps the three views eagerly; epochs 1 and 2 run from the captured graphs -- after the pictures of epochs 1 and 2
    assert st["capture_error"] is None and st["eager"] == 3 and st["replays"] == 6 and st["training"] is True
    ds = run["dataset"]
    for epoch in (0, 1, 2):
        rendering, normal = render.plot_paths(run["dir"], epoch)
        im = np.asarray(Image.open(rendering))
        assert im.shape == (134, 68, 3)                                       # output above ground truth, make_grid's padding of 2
        gt8 = R.byte(ds.rgb_images[epoch % 3].numpy()).reshape(64, 64, 3)     # the view is (epoch // plot_freq) % len(dataset)
        assert np.array_equal(im[68:132, 2:66], gt8)
        border = np.ones((134, 68), bool)
        border[2:66, 2:66] = border[68:132, 2:66] = False
        assert not im[border].any()
        assert np.asarray(Image.open(normal)).shape == (64, 64, 3)            # a single image: unpadded


def test_cli_writes_every_file_and_keeps_them(run):
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = [sys.executable, "-m", "neat_amd.render", "--conf", run["conf"], "--data_root", run["data"], "--json", "--save-depth"]
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    assert report["epoch"] == 2 and report["views"] == [0, 1, 2] and report["chunksize"] == 1000 and len(report["psnr"]) == 3      # train.split_n_pixels
    assert report["render_s"] > 0 and report["encode_s"] > 0 and report["written"] == 12
    m = re.search(r"^RENDERING EVALUATION -1: psnr mean = (-?\d+\.\d\d) ; psnr std = (\d+\.\d\d)$", p.stdout, flags=re.M)
    assert m and m.group(1) == "%.2f" % report["mean"] and m.group(2) == "%.2f" % report["std"]
    # the CSV: pandas' layout; its rows are the JSON's values, then their mean and standard deviation
    lines = open(render.csv_path(run["dir"], 2)).read().splitlines()
    assert lines[0] == ",0" and [l.split(",")[0] for l in lines[1:]] == ["0", "1", "2", "3", "4"]
    vals = [float(l.split(",")[1]) for l in lines[1:]]
    assert vals[:3] == report["psnr"] and vals[3] == np.mean(report["psnr"]) == report["mean"] and vals[4] == np.std(report["psnr"]) == report["std"]
    # the pictures re-read equal render.view's bytes in this process
    dev = torch.device(DEV)
    files = []
    for idx in range(3):
        uv, pose, K, gt, H, W = render.dataset_view(run["dataset"], idx, dev)
        res = render.view(run["model"], uv, pose, K, H, W, gt=gt, chunksize=1000)
        paths = render.out_paths(run["dir"], 2, idx, save_depth=True)
        assert os.path.basename(paths["rgb"]) == "eval_%03d.png" % idx
        for key, name in (("rgb", "rgb"), ("normal", "normal"), ("depth", "depth8")):
            assert np.array_equal(np.asarray(Image.open(paths[key])), res[name].cpu().numpy()), (idx, key)
        assert np.array_equal(np.load(paths["depth_npy"]), res["depth"].cpu().numpy(), equal_nan=True)
        assert res["psnr"] == report["psnr"][idx]
        files += list(paths.values())
    files.append(render.csv_path(run["dir"], 2))
    # a second call without --overwrite rewrites nothing
    stamps = [os.stat(f).st_mtime_ns for f in files]
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "exists" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert [os.stat(f).st_mtime_ns for f in files] == stamps
    # the --cam-json route: any camera, no PSNR, no CSV
    other = run["tmp"] / "free"
    (other / "checkpoints").mkdir(parents=True)
    os.symlink(os.path.join(run["dir"], "checkpoints", "ModelParameters"), other / "checkpoints" / "ModelParameters")
    w2c = np.linalg.inv(run["dataset"].pose_all[0].numpy().astype(np.float64))
    with open(other / "cam.json", "w") as fh:
        json.dump([w2c.tolist(), w2c.tolist()], fh)
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "neat_amd.render", "--conf", run["conf"], "--expdir", str(other),
                        "--cam-json", str(other / "cam.json"), "--width", "20", "--height", "12", "--maps", "rgb,depth", "--chunksize", "100"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "RENDERING EVALUATION" not in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(other / "rendering_2")) == ["depth_000.png", "depth_001.png", "eval_000.png", "eval_001.png"]
    assert not os.path.exists(render.csv_path(str(other), 2))
    a, b = (np.asarray(Image.open(other / "rendering_2" / ("eval_%03d.png" % k))) for k in (0, 1))
    assert a.shape == (12, 20, 3) and np.array_equal(a, b)
