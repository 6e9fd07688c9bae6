"""python -m neat_amd.render: flags, defaults, refused combinations and file naming on a fake run directory (CPU)."""
import pytest

from neat_amd import render


def test_flags_and_defaults():
    opt = render.parse_args(["--conf", "x/runconf.conf"])
    expect = {"checkpoint": "latest", "views": None, "chunksize": None, "maps": ("rgb", "normal", "depth"), "depth_range": None,
              "save_depth": False, "cam_json": None, "width": None, "height": None, "fov": 60.0, "expdir": None, "data_root": "../data",
              "scan_id": -1, "gpu": 0, "precision": None, "json": False, "overwrite": False}
    for k, v in expect.items():
        assert getattr(opt, k) == v, k
    assert render.DEFAULT_CHUNK == 10000                                  # eval.py's fall-back for train.split_n_pixels
    opt = render.parse_args(["--conf", "c", "--checkpoint", "1000", "--views", "0,5,10", "--chunksize", "2048", "--maps", "rgb,depth",
                             "--depth-range", "0.5", "4", "--save-depth", "--expdir", "run", "--data_root", "d", "--scan_id", "24", "--gpu", "3",
                             "--precision", "fp32", "--json", "--overwrite"])
    assert (opt.checkpoint, opt.views, opt.chunksize, opt.maps, opt.depth_range) == ("1000", [0, 5, 10], 2048, ("rgb", "depth"), [0.5, 4.0])
    assert opt.save_depth and opt.json and opt.overwrite and (opt.expdir, opt.data_root, opt.scan_id, opt.gpu, opt.precision) == ("run", "d", 24, 3, "fp32")
    opt = render.parse_args(["--conf", "c", "--cam-json", "cam.json", "--width", "160", "--height", "120", "--fov", "45"])
    assert (opt.cam_json, opt.width, opt.height, opt.fov) == ("cam.json", 160, 120, 45.0)


@pytest.mark.parametrize("bad", [[], ["--conf", "c", "--cam-json", "cam.json"], ["--conf", "c", "--cam-json", "cam.json", "--width", "64"],
                                 ["--conf", "c", "--cam-json", "cam.json", "--height", "64"], ["--conf", "c", "--maps", "rgb,albedo"],
                                 ["--conf", "c", "--maps", ""], ["--conf", "c", "--depth-range", "1"], ["--conf", "c", "--views", "a,b"],
                                 ["--conf", "c", "--chunksize", "0"], ["--conf", "c", "--precision", "int8"]])
def test_bad_combinations_exit(bad):
    with pytest.raises(SystemExit):
        render.parse_args(bad)


def test_file_names_on_a_fake_run_directory(tmp_path):
    from tests.util_run import write_synth_run
    run = write_synth_run(tmp_path)["dir"]
    d = run / "rendering_1000"
    assert render.out_dir(str(run), 1000) == str(d)
    assert render.out_paths(str(run), 1000, 7) == {"rgb": str(d / "eval_007.png"), "normal": str(d / "normal_007.png"),
                                                   "depth": str(d / "depth_007.png")}                         # eval_%03d.png: the reference's name
    assert render.out_paths(str(run), 1000, 123, ("rgb", "depth"), save_depth=True) == {
        "rgb": str(d / "eval_123.png"), "depth": str(d / "depth_123.png"), "depth_npy": str(d / "depth_123.npy")}
    assert render.out_paths(str(run), 5, 0, ("normal",), save_depth=True) == {"normal": str(run / "rendering_5" / "normal_000.png")}
    assert render.csv_path(str(run), 1000) == str(run / "psnr_1000.csv")
    assert render.plot_paths(str(run), 200) == (str(run / "plots" / "rendering_200.png"), str(run / "plots" / "normal_200.png"))


def test_write_png_keeps_an_existing_file(tmp_path):
    import numpy as np
    from PIL import Image
    path = tmp_path / "sub" / "a.png"
    rgb = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert render.write_png(str(path), rgb) is True and np.array_equal(np.asarray(Image.open(path)), rgb)
    assert render.write_png(str(path), rgb[::-1], overwrite=False) is False and np.array_equal(np.asarray(Image.open(path)), rgb)
    assert render.write_png(str(path), rgb[::-1]) is True and np.array_equal(np.asarray(Image.open(path)), rgb[::-1])
    grey = np.arange(35, dtype=np.uint8).reshape(5, 7)
    render.write_png(str(tmp_path / "g.png"), grey)
    im = Image.open(tmp_path / "g.png")
    assert im.mode == "L" and np.array_equal(np.asarray(im), grey)
