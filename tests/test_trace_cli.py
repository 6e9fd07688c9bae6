"""python -m neat_amd.trace check and python -m neat_amd.render --surface end to end on a tiny saved run: the synthetic model at its
geometric initialisation as the checkpoint, the toy scene of tests/test_runner.py as the dataset (three 64 x 64 views)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import render_f64 as R

pytestmark = pytest.mark.gpu
EPOCH = 7


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tests.util_run import write_synth_run
    run = write_synth_run(tmp_path_factory.mktemp("trace_cli"), epoch=EPOCH, n_views=3, train_extra={"split_n_pixels": 1024})
    run_dir = run["dir"]
    # a wireframe: short segments well outside the initial surface (a sphere of about 0.6) and segments inside it
    rng = np.random.default_rng(1)
    u = rng.standard_normal((12, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lines = np.concatenate([np.stack([1.2 * u[:6], 1.2 * u[:6] + 0.1 * u[6:]], 1), np.stack([0.2 * u[:6], 0.2 * u[6:]], 1)])
    (run_dir / "wireframes").mkdir()
    data = run_dir / "wireframes" / "latest-abcdefgh-wfi.npz"
    np.savez(data, lines3d=lines)
    return {**run, "lines": lines, "data": str(data)}


def test_check_writes_the_occlusion_file_and_keeps_it(run, capsys):
    from neat_amd import run_io, trace
    args = ["check", "--conf", run["conf"], "--data", run["data"], "--data_root", run["data_root"], "--min-views", "1", "--precision", "fp32", "--json"]
    assert trace.main(args) == 0
    out = capsys.readouterr().out
    path = trace.out_path(run["data"])
    assert path == str(run["dir"] / "wireframes" / "latest-abcdefgh-wfi_occl.npz") and os.path.exists(path)
    report = json.loads(out.strip().splitlines()[-1])
    assert report["total"] == 12 and report["views"] == 3 and report["epoch"] == EPOCH and report["trace_s"] > 0 and report["path"] == path
    assert "kept %d / 12 lines" % report["kept"] in out and "tracing" in out
    with np.load(path) as z:
        assert sorted(z.files) == ["kept", "lines3d", "views"]
        views, kept, lines = z["views"], z["kept"], z["lines3d"]
    assert views.dtype == np.int32 and views.shape == (12,) and kept.dtype == bool and kept.shape == (12,)
    assert np.array_equal(kept, views >= 1) and np.array_equal(lines, run["lines"][kept]) and int(kept.sum()) == report["kept"]
    # segments inside the surface are seen by no camera; a segment outside it by at least one of three cameras around the object
    assert not kept[6:].any() and (views[6:] == 0).all() and kept[:6].any() and views.max() <= 3
    assert np.array_equal(run_io.load_lines(path)[0], lines)
    # the library gives what the file holds
    model, _, _, conf = run_io.load_model(run["conf"], "latest", torch.device("cuda:0"), precision="fp32")
    ds = run_io.build_dataset(conf, run["data_root"])
    cams = np.linalg.inv(np.stack([ds.pose_all[i].numpy().astype(np.float64) for i in range(3)]))
    frac = trace.visible_lines(model, torch.from_numpy(run["lines"]), cams).cpu().numpy()
    assert np.array_equal(trace.keep_rule(frac, 1, 0.5)[0], views)
    # kept unless --overwrite
    stamp = os.stat(path).st_mtime_ns
    assert trace.main(args) == 0 and "exists" in capsys.readouterr().out and os.stat(path).st_mtime_ns == stamp
    assert trace.main(args + ["--overwrite", "--min-views", "4"]) == 0
    with np.load(path) as z:
        assert not z["kept"].any() and z["lines3d"].shape == (0, 2, 3) and np.array_equal(z["views"], views)


def test_render_surface_files_and_the_plain_file_set(run, capsys):
    from PIL import Image
    from neat_amd import render
    d = run["dir"] / ("rendering_%d" % EPOCH)
    base = ["--conf", run["conf"], "--data_root", run["data_root"], "--precision", "fp32", "--json"]
    # --maps surface alone: no volumetric forward, hence no eval / normal / depth picture and no PSNR
    assert render.main(base + ["--maps", "surface", "--save-depth"]) == 0
    out = capsys.readouterr().out
    report = json.loads(out.strip().splitlines()[-1])
    assert sorted(os.listdir(d)) == sorted(n % i for i in range(3) for n in ("surface_depth_%03d.png", "surface_normal_%03d.png", "surface_depth_%03d.npy"))
    assert not os.path.exists(render.csv_path(str(run["dir"]), EPOCH)) and "RENDERING EVALUATION" not in out and "psnr" not in report
    assert report["written"] == 9 and report["trace_s"] > 0 and report["trace_evals"] > 64 * 64
    for i in range(3):
        dep, nrm = Image.open(d / ("surface_depth_%03d.png" % i)), Image.open(d / ("surface_normal_%03d.png" % i))
        assert dep.mode == "L" and dep.size == (64, 64) and nrm.mode == "RGB" and nrm.size == (64, 64)
        plane = np.load(d / ("surface_depth_%03d.npy" % i))
        assert plane.shape == (64, 64) and plane.dtype == np.float32
        hit = np.isfinite(plane)
        # the grey picture is depth_*.png's rule (tests/render_f64.py) over the finite range of the plane, byte for byte
        assert 200 < hit.sum() < 64 * 64 and np.array_equal(np.asarray(dep), R.grey(plane, *R.finite_range(plane)))
        assert np.asarray(dep)[hit].max() >= 254 and np.asarray(dep)[hit].min() == 0 and (np.asarray(dep)[~hit] == 0).all()
        assert (np.asarray(nrm)[~hit] == 127).all()                      # byte((0 + 1) / 2)
    for f in os.listdir(d):
        os.remove(d / f)
    # a plain call: exactly the files it writes without the feature, and a report without the new keys
    assert render.main(base) == 0
    out = capsys.readouterr().out
    report = json.loads(out.strip().splitlines()[-1])
    assert sorted(os.listdir(d)) == sorted(n % i for i in range(3) for n in ("eval_%03d.png", "normal_%03d.png", "depth_%03d.png"))
    assert os.path.exists(render.csv_path(str(run["dir"]), EPOCH))
    assert set(report) == {"epoch", "views", "chunksize", "render_s", "encode_s", "written", "dir", "psnr", "mean", "std"} and "surface" not in out
    plain = {f: (d / f).read_bytes() for f in os.listdir(d)}
    # --surface beside the maps: the plain files byte for byte, plus the two surface pictures per view
    assert render.main(base + ["--surface", "--overwrite"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(d)) == sorted(list(plain) + [n % i for i in range(3) for n in ("surface_depth_%03d.png", "surface_normal_%03d.png")])
    assert all((d / f).read_bytes() == b for f, b in plain.items()) and report["written"] == 15 and "trace_s" in report and "trace_evals" in report
