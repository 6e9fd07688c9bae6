"""python -m neat_amd.mesh: flags, defaults and file naming on a fake run directory (CPU), and end to end on a checkpoint written by the
runner on the synthetic scene (GPU): the PLY exists, re-reads and equals mesh.surface on the same checkpoint."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_f64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_and_defaults():
    from neat_amd.mesh import build_parser
    opt = build_parser().parse_args(["--conf", "x/runconf.conf"])
    expect = {"checkpoint": "latest", "resolution": None, "grid_boundary": None, "level": 0.0, "largest_component": False, "expdir": None,
              "gpu": 0, "precision": None, "overwrite": False, "no_normals": False}
    for k, v in expect.items():
        assert getattr(opt, k) == v, k
    opt = build_parser().parse_args(["--conf", "c", "--checkpoint", "1000", "--resolution", "512", "--grid-boundary", "-1", "1.25", "--level",
                                     "0.01", "--largest-component", "--expdir", "run", "--gpu", "3", "--precision", "fp32", "--overwrite"])
    assert (opt.checkpoint, opt.resolution, opt.grid_boundary, opt.level) == ("1000", 512, [-1.0, 1.25], 0.01)
    assert opt.largest_component and opt.overwrite and opt.expdir == "run" and opt.gpu == 3 and opt.precision == "fp32"
    for bad in ([], ["--conf", "c", "--grid-boundary", "1"], ["--conf", "c", "--precision", "int8"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_file_naming_and_plot_block_on_a_fake_run_directory(tmp_path):
    from neat_amd import conf as conf_mod, mesh
    from neat_amd.synth import hocon_text
    from tests.util_run import write_synth_run
    run = write_synth_run(tmp_path, plot={"plot_nimgs": 1, "resolution": 100, "grid_boundary": [-1.5, 1.5]})["dir"]
    assert mesh.out_path(str(run), 1000) == str(run / "plots" / "surface_1000.ply")          # the reference's name (plots.py)
    conf_path = run / "runconf.conf"
    block = mesh.plot_block(conf_mod.parse_file(str(conf_path)))
    assert int(block["resolution"]) == 100 and [float(v) for v in block["grid_boundary"]] == [-1.5, 1.5]
    conf_path.write_text(hocon_text({"train": {"expname": "toy"}}))
    assert mesh.plot_block(conf_mod.parse_file(str(conf_path))) == {}
    assert mesh._bounds3((-1.5, 1.5)) == ((-1.5,) * 3, (1.5,) * 3) and mesh._shape3(7) == (7, 7, 7) and mesh._shape3([2, 3, 4]) == (2, 3, 4)
    with pytest.raises(ValueError):
        mesh._shape3((2, 3))


def test_runner_takes_vis_mesh():
    import inspect
    from neat_amd.runner import TrainRunner
    assert inspect.signature(TrainRunner.__init__).parameters["vis_mesh"].default is False      # off by default, as the reference's do_vis


@pytest.mark.gpu
def test_cli_end_to_end_on_a_runner_checkpoint(tmp_path):
    from neat_amd import mesh, run_io, synth
    from neat_amd.runner import TrainRunner
    from tests.test_runner import _toy_scene, _hocon
    _toy_scene(tmp_path / "data" / "abc" / "toy", n_views=3)
    conf = {"train": {"expname": "toy_mesh", "dataset_class": "datasets.blender_hawp_dataset.BlenderDataset",
                      "model_class": "model.networks.neat_wfr_rend_a.VolSDFNetwork", "loss_class": "model.networks.loss_wfr.VolSDFLoss",
                      "learning_rate": 5.0e-4, "num_pixels": 128, "checkpoint_freq": 1, "plot_freq": 1},
            "plot": {"plot_nimgs": 1, "resolution": 40, "grid_boundary": [-1.5, 1.5]},
            "loss": dict(synth.ABC_NEAT_A_LOSS_CONF),
            "dataset": {"data_dir": "abc/toy", "img_res": [64, 64], "reverse_coordinate": True},
            "model": synth.ABC_NEAT_A_MODEL_CONF}
    path = tmp_path / "toy.conf"
    path.write_text(_hocon(conf))
    runner = TrainRunner(str(path), nepochs=1, exps_folder=str(tmp_path / "exps"), data_root=str(tmp_path / "data"), log_freq=100, vis_mesh=True)
    runner.run()
    run_dir = os.path.dirname(runner.checkpoints_path)
    del runner
    torch.cuda.synchronize()
    gc.collect()
    # --vis_mesh: one file per plot_freq epochs, written by the training loop itself
    for epoch in (0, 1):
        v, n, f = M.read_ply(mesh.out_path(run_dir, epoch))
        assert len(v) > 0 and len(f) > 0 and n is not None and f.max() == len(v) - 1
    os.remove(mesh.out_path(run_dir, 1))
    conf_path = os.path.join(run_dir, "runconf.conf")
    with open(conf_path, "w") as fh:
        fh.write(_hocon(conf))
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = [sys.executable, "-m", "neat_amd.mesh", "--conf", conf_path]
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "grid evaluation" in p.stdout and "extraction" in p.stdout
    out = mesh.out_path(run_dir, 1)                               # `latest` is the checkpoint of epoch 1
    assert os.path.exists(out), os.listdir(os.path.dirname(out))
    v, n, f = M.read_ply(out)
    model, epoch, root, conf_read = run_io.load_model(conf_path, "latest", torch.device("cuda:0"))
    plot = mesh.plot_block(conf_read)
    assert epoch == 1 and root == run_dir and int(plot["resolution"]) == 40
    res = mesh.surface(model, plot_conf=plot)
    assert np.array_equal(v, res["verts"].cpu().numpy()) and np.array_equal(f, res["faces"].cpu().numpy())
    assert np.array_equal(n, res["normals"].cpu().numpy())
    # an existing file is kept unless --overwrite; a level nothing reaches writes nothing and says so
    stamp = os.path.getmtime(out)
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "exists" in p.stdout and os.path.getmtime(out) == stamp
    os.remove(out)
    p = subprocess.run(["timeout", "-k", "10", "600"] + args + ["--level", "50", "--resolution", "16"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "nothing written" in p.stdout and not os.path.exists(out), p.stdout[-2000:] + p.stderr[-2000:]
