"""CPU checks of `python -m neat_amd.triangulate`: its arguments, the output path, the slicing of views, the host's camera block and
neighbour table against the reference's, and that nothing runs off the device."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import triangulate_f64 as T


def test_parser_defaults_and_output_path():
    from neat_amd import triangulate
    opt = triangulate.build_parser().parse_args(["--conf", "x.conf"])
    assert (opt.data_root, opt.scan_id, opt.views, opt.out, opt.gpu) == ("../data", -1, None, None, 0)
    assert (opt.neighbours, opt.min_views, opt.min_score, opt.sigma, opt.overlap, opt.angle) == (6, 3, 1.5, 2.5, 0.25, 5.0)
    assert triangulate.DEFAULTS == T.DEFAULTS == {"neighbours": 6, "angle_min": 5.0, "overlap_min": 0.25, "sigma_px": 2.5, "min_score": 1.5,
                                                  "min_views": 3}
    with pytest.raises(SystemExit):
        triangulate.build_parser().parse_args([])                       # --conf is required
    assert triangulate.out_path(opt, "/data/abc/7", "hawp") == os.path.join("/data/abc/7", "hawp-l3d.npz")
    assert triangulate.out_path(opt, "/data/DTU/scan24", "lsd") == os.path.join("/data/DTU/scan24", "lsd-l3d.npz")
    opt = triangulate.build_parser().parse_args(["--conf", "x.conf", "--out", "here.npz", "--neighbours", "10", "--min-views", "4"])
    assert triangulate.out_path(opt, "/data/abc/7", "hawp") == "here.npz" and (opt.neighbours, opt.min_views) == (10, 4)


def test_views_slicing():
    from neat_amd import triangulate
    assert list(triangulate.parse_views(None, 5)) == [0, 1, 2, 3, 4]
    assert list(triangulate.parse_views("1:3", 5)) == [1, 2]
    assert list(triangulate.parse_views(":2", 5)) == [0, 1]
    assert list(triangulate.parse_views("0:100:4", 100)) == list(range(0, 100, 4))
    assert list(triangulate.parse_views("::2", 5)) == [0, 2, 4]
    assert list(triangulate.parse_views("2:99:", 5)) == [2, 3, 4]
    for bad in ("3", "1:2:3:4", "a:b", "0:4:0", "0:4:-1"):
        with pytest.raises(ValueError):
            triangulate.parse_views(bad, 5)


def test_cpu_tensors_are_refused():
    from neat_amd import triangulate
    seg, Ks, poses = T.random_scene([3, 3, 3], 3, seed=1)
    with pytest.raises(RuntimeError, match="CUDA"):
        triangulate.lines([torch.from_numpy(s) for s in seg], Ks, poses)
    with pytest.raises(RuntimeError, match="CUDA"):
        triangulate.lines(seg, Ks, poses)                               # numpy arrays are no device tensors either
    with pytest.raises(RuntimeError, match="CUDA"):
        triangulate.hypotheses([torch.from_numpy(s) for s in seg], Ks, poses)
    with pytest.raises(RuntimeError, match="CUDA"):
        triangulate.lines([], Ks[:0], poses[:0], device="cpu")
    with pytest.raises(RuntimeError, match="per view"):
        triangulate.lines(torch.zeros(3, 4), Ks, poses)


def test_host_camera_block_and_neighbours_equal_the_reference():
    """The host layer and the reference each write the camera formulas out; the bits must agree, skew and unequal focal lengths included."""
    from neat_amd import triangulate
    Ks, poses = T.ring_cameras(9, seed=4)
    Ks = Ks.copy()
    Ks[:, 0, 1], Ks[:, 1, 1], Ks[:, 0, 2] = 0.37, 611.5, 250.25
    cam, ref = triangulate.camera_block(Ks, poses), T.cameras(Ks, poses)
    assert cam.shape == (9, triangulate.CAM) and cam.dtype == np.float64
    for key, lo, hi in (("Kinv", 0, 9), ("R", 9, 18), ("t", 18, 21), ("K", 21, 30), ("P", 30, 42), ("C", 42, 45)):
        assert np.array_equal(cam[:, lo:hi], ref[key].reshape(9, -1)), key
    assert np.allclose(ref["Kinv"] @ Ks, np.eye(3), atol=1e-12) and np.allclose(ref["R"] @ ref["C"][:, :, None] + ref["t"][:, :, None], 0, atol=1e-12)
    assert np.array_equal(triangulate.camera_block(torch.from_numpy(Ks).float(), [torch.from_numpy(p) for p in poses])[:, 42:45], ref["C"])
    for M in (0, 1, 6, 8, 20):
        nb = triangulate.neighbour_table(ref["C"], M)
        assert nb.dtype == np.int32 and np.array_equal(nb, T.neighbour_table(ref["C"], M)) and nb.shape == (9, min(M, 8))
    assert triangulate.neighbour_table(np.zeros((1, 3)), 6).shape == (1, 0) and triangulate.neighbour_table(np.zeros((0, 3)), 6).shape == (0, 0)
    bad = Ks.copy()
    bad[0, 2, 2] = 2.0
    with pytest.raises(ValueError, match="upper triangular"):
        triangulate.camera_block(bad, poses)


def test_output_file_is_written_through_a_temporary_one(tmp_path):
    from neat_amd import run_io, triangulate
    path = str(tmp_path / "deep" / "hawp-l3d.npz")
    lines3d = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    triangulate.write_lines(path, lines3d, [3, 4], [2.5, 1.75], np.tile(np.eye(4), (5, 1, 1)))
    assert os.listdir(os.path.dirname(path)) == ["hawp-l3d.npz"]
    with np.load(path) as data:
        assert sorted(data.files) == ["cameras", "lines3d", "support", "views"] and "scores" not in data.files
        assert data["views"].dtype == np.int32 and data["support"].tolist() == [2.5, 1.75] and data["cameras"].shape == (5, 4, 4)
    got, scores = run_io.load_lines(path)
    assert got.dtype == np.float64 and np.array_equal(got, lines3d) and scores is None
    assert isinstance(triangulate.build_parser(), argparse.ArgumentParser)
