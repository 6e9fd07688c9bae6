"""The synthetic run directory of the command-line tests: a runconf.conf, the checkpoint of the synthetic-conf model at its geometric
initialisation (a sphere-like surface of radius about 0.6) and, with n_views, the toy scene of tests/test_runner.py as the dataset."""
import torch


def synth_init_model():
    """networks.VolSDFNetwork of the synthetic conf with synth_state_dict(7, "init") loaded, on the host."""
    from neat_amd import networks, synth
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in synth.synth_state_dict(7, "init").items()})
    return model


def write_synth_run(tmp, *, epoch=7, n_views=0, plot=None, train_extra=None):
    """tmp/exps/toy/2024_01_01_00_00_00/{runconf.conf, checkpoints/ModelParameters/latest.pth} and, with n_views > 0, the 64 x 64 toy scene
    under tmp/data/abc/toy.  plot = the conf's plot block, train_extra = further keys of its train block.
    -> {"dir": the run directory (a Path), "conf", "checkpoint", "data_root": strings}."""
    from neat_amd import synth
    run_dir = tmp / "exps" / "toy" / "2024_01_01_00_00_00"
    (run_dir / "checkpoints" / "ModelParameters").mkdir(parents=True)
    conf = {"train": {"expname": "toy", "model_class": "model.networks.neat_wfr_rend_a.VolSDFNetwork", **(train_extra or {})},
            "model": synth.ABC_NEAT_A_MODEL_CONF}
    if plot is not None:
        conf["plot"] = plot
    if n_views:
        from tests.test_runner import _toy_scene
        _toy_scene(tmp / "data" / "abc" / "toy", n_views=n_views)
        conf["train"]["dataset_class"] = "datasets.blender_hawp_dataset.BlenderDataset"
        conf["dataset"] = {"data_dir": "abc/toy", "img_res": [64, 64], "reverse_coordinate": True}
    (run_dir / "runconf.conf").write_text(synth.hocon_text(conf))
    checkpoint = run_dir / "checkpoints" / "ModelParameters" / "latest.pth"
    torch.save({"model_state_dict": synth_init_model().state_dict(), "epoch": epoch}, str(checkpoint))
    return {"dir": run_dir, "conf": str(run_dir / "runconf.conf"), "checkpoint": str(checkpoint), "data_root": str(tmp / "data")}
