"""CPU checks of `python -m neat_amd.detect`: its arguments, where it looks for the views, and that nothing runs off the device."""
import os

import numpy as np
import pytest
import torch


def test_parser_defaults_and_views():
    from neat_amd import detect
    opt = detect.build_parser().parse_args(["--scan", "x"])
    assert (opt.name, opt.scale, opt.views, opt.device, opt.batch) == ("lsd", detect.DEFAULT_SCALE, None, "cuda:0", 16)
    assert detect.DEFAULT_SCALE == 1.0
    with pytest.raises(SystemExit):
        detect.build_parser().parse_args([])                            # --scan is required
    assert list(detect.parse_views(None, 5)) == [0, 1, 2, 3, 4]
    assert list(detect.parse_views("1:3", 5)) == [1, 2]
    assert list(detect.parse_views(":2", 5)) == [0, 1]
    assert list(detect.parse_views("3:", 5)) == [3, 4]
    assert list(detect.parse_views("2:99", 5)) == [2, 3, 4]
    for bad in ("3", "1:2:3", "a:b"):
        with pytest.raises(ValueError):
            detect.parse_views(bad, 5)


def test_cpu_is_refused_loudly(tmp_path, capsys):
    from neat_amd import detect
    assert detect.main(["--scan", str(tmp_path), "--device", "cpu"]) == 2          # before the directory is even looked at
    assert "refused" in capsys.readouterr().err
    assert detect.main(["--scan", str(tmp_path), "--scale", "1.5"]) == 2
    assert detect.main(["--scan", str(tmp_path), "--scale", "0"]) == 2
    with pytest.raises(RuntimeError, match="CUDA"):
        detect.lines(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        detect.labels(torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        detect.lines(np.zeros((1, 8, 8, 3), dtype=np.uint8))


def test_scene_images_finds_either_folder(tmp_path):
    from PIL import Image
    from neat_amd import run_io
    with pytest.raises(FileNotFoundError):
        run_io.scene_images(str(tmp_path))
    for sub in ("image", "images"):
        root = tmp_path / ("scene_" + sub)
        os.makedirs(root / sub)
        for name in ("b.png", "a.png", "a_mask.png", "c.jpg", "notes.txt"):
            if name.endswith(".txt"):
                open(root / sub / name, "w").write("x")
            else:
                Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(root / sub / name)
        assert [os.path.basename(p) for p in run_io.scene_images(str(root))] == ["a.png", "b.png", "c.jpg"]
