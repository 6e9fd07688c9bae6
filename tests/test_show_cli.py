"""The command line of neat_amd.show without a device: flags and defaults, the --pose presets, the default output directory, what
--hide-lines means here, the per-view object array of `lines3d`, and frames kept on disk unless --overwrite."""
import os

import numpy as np
import pytest

from neat_amd import run_io, show


def _opt(*argv):
    return show.build_parser().parse_args(["--data", "/x/run/wireframes/a-wfi_checked.npz", *argv])


def test_flags_and_defaults():
    o = _opt()
    assert (o.mesh, o.save_path, o.name, o.pose, o.cams, o.views, o.cam_json) == (None, None, "video", None, None, None, None)
    assert (o.rx, o.ry, o.rz, o.t) == (None, None, None, None)
    assert (o.frames, o.step, o.width, o.height, o.fov) == (72, 5.0, 1024, 1024, 60.0)
    assert (o.line_width, o.point_radius, o.hidden_alpha, o.depth_bias, o.near) == (1.5, 2.5, 0.0, 0.01, 0.05)
    assert (o.show_points, o.hide_lines, o.no_gif, o.overwrite, o.gpu) == (False, False, False, False, 0)
    assert (o.bg, o.line_color, o.point_color, o.mesh_color) == ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.8, 0.8, 0.8])
    st = show.style_of(o)
    assert set(st) == set(show.STYLE) and st == {**show.STYLE, **st} and all(st[k] == show.STYLE[k] for k in show.STYLE)
    with pytest.raises(SystemExit):
        show.build_parser().parse_args([])                       # --data is required
    with pytest.raises(SystemExit):
        _opt("--pose", "elsewhere")
    o = _opt("--mesh", "s.ply", "--frames", "4", "--step", "90", "--width", "128", "--height", "96", "--line-width", "3", "--bg", "0", "0", "0",
             "--hidden-alpha", "0.3", "--no-gif", "--overwrite", "--gpu", "1", "--views", "0,5,10", "--cams", "cameras.npz")
    assert (o.mesh, o.frames, o.step, o.width, o.height, o.line_width, o.bg, o.hidden_alpha) == ("s.ply", 4, 90.0, 128, 96, 3.0, [0.0] * 3, 0.3)
    assert o.no_gif and o.overwrite and o.gpu == 1 and o.views == "0,5,10" and o.cams == "cameras.npz"


def test_pose_presets():
    assert show.pose_of(_opt("--pose", "dtu")) == (-155.0, 0.0, -25.0, 3.0)
    assert show.pose_of(_opt("--pose", "scan")) == (0.0, 170.0, -45.0, 3.0)
    assert show.pose_of(_opt()) == (0.0, 0.0, 0.0, 3.0)
    assert show.pose_of(_opt("--pose", "dtu", "--ry", "20", "--t", "2.5")) == (-155.0, 20.0, -25.0, 2.5)
    w2c, K = show.cameras_of(_opt("--pose", "scan", "--frames", "3", "--step", "10", "--width", "64", "--height", "48"))
    assert w2c.shape == (3, 4, 4) and np.array_equal(w2c, show.orbit(0.0, 170.0, -45.0, 3.0, frames=3, step=10.0))
    assert np.array_equal(K, show.intrinsics(64, 48, 60.0))
    assert not np.allclose(w2c[0], w2c[1])


def test_default_output_directory():
    assert show.output_dir(_opt()) == os.path.join("/x/run/wireframes", "..", "video")
    assert show.output_dir(_opt("--name", "turn")) == os.path.join("/x/run/wireframes", "..", "turn")
    assert show.output_dir(_opt("--save-path", "/out", "--name", "turn")) == os.path.join("/out", "turn")


def test_hide_lines_draws_points_only():
    assert show.style_of(_opt())["show_lines"] is True
    assert show.style_of(_opt("--show-points"))["show_lines"] is True
    assert show.style_of(_opt("--hide-lines"))["show_lines"] is False          # the reference's flag changes nothing; this one does


def test_lines3d_object_array_is_concatenated(tmp_path):
    rng = np.random.default_rng(0)
    blocks = [rng.normal(size=(n, 2, 3)).astype(np.float32) for n in (3, 0, 5)]
    obj = np.empty(3, dtype=object)
    for i, b in enumerate(blocks):
        obj[i] = b
    path = str(tmp_path / "a-all.npz")
    np.savez(path, lines3d=obj)
    got = run_io.load_lines(path)[0]
    assert got.shape == (8, 2, 3) and got.dtype == np.float64 and np.array_equal(got, np.concatenate(blocks).astype(np.float64))
    flat = str(tmp_path / "a-wfi_checked.npz")
    np.savez(flat, lines3d=blocks[2], scores=np.ones(5))
    assert np.array_equal(run_io.load_lines(flat)[0], blocks[2].astype(np.float64))
    import torch
    pth = str(tmp_path / "a-neat.pth")
    torch.save({"lines3d_wfi_checked": torch.tensor(blocks[0])}, pth)
    assert np.array_equal(run_io.load_lines(pth)[0], blocks[0].astype(np.float64))
    assert len(show.endpoints(np.stack([blocks[0][0], blocks[0][0][::-1]]))) == 2          # distinct endpoints


def test_frames_on_disk_are_kept_unless_overwrite(tmp_path):
    from PIL import Image
    d = str(tmp_path / "video")
    a = np.zeros((2, 6, 8, 3), dtype=np.uint8)
    b = np.full((2, 6, 8, 3), 200, dtype=np.uint8)
    paths = show.write_frames(d, a)
    assert [os.path.basename(p) for p in paths] == ["0000.png", "0001.png"]
    show.write_frames(d, b)
    assert np.array_equal(np.asarray(Image.open(paths[0])), a[0]) and np.array_equal(np.asarray(Image.open(paths[1])), a[1])          # kept
    show.write_frames(d, b, overwrite=True)
    assert np.array_equal(np.asarray(Image.open(paths[1])), b[1])
    c = np.zeros((3, 6, 8, 3), dtype=np.uint8)
    c[1, 2, 3] = (255, 0, 0)
    c[2, 4, 5] = (0, 255, 0)
    show.write_frames(d, c, gif=d + ".gif", overwrite=True)
    g = Image.open(d + ".gif")
    assert g.n_frames == 3 and g.size == (8, 6)


def test_cam_json_gives_one_frame_per_matrix(tmp_path):
    import json
    w2c = show.orbit(*show.POSES["dtu"], frames=4, step=30.0)
    path = str(tmp_path / "cam.json")
    with open(path, "w") as fh:
        json.dump([m.tolist() for m in w2c], fh)
    got, K = show.cameras_of(_opt("--cam-json", path, "--width", "128", "--height", "96"))
    assert np.array_equal(got, w2c) and np.array_equal(K, show.intrinsics(128, 96, 60.0))          # repr round-trips float64 exactly
    with pytest.raises(SystemExit):
        show.cameras_of(_opt("--cams", "cameras.npz"))              # --cams needs --views


def test_dataset_cameras_project_where_the_dataset_puts_a_point(tmp_path):
    """--cams cameras.npz --views: world_mat_i @ scale_mat_i is decomposed into K and a pose; a point then lands, by the picture's
    arithmetic (tests/show_f64.py), where P = world_mat @ scale_mat puts it.  Float32 products and a float32 pose are on this path
    (as in neat_amd.datasets), so the agreement is to float32: a pixel is f X / Z + c with f about 2900, the camera about 4 scaled units away and each entry of
    R, C and P good to 2^-24 relative, a few times 2900 x 4 x 6e-8 = 7e-4 pixels; the bound is 1e-2."""
    from tests import show_f64 as S
    rng = np.random.default_rng(3)
    mats, Ps = {}, []
    for i in range(3):
        ang = 0.7 * i + 0.2
        Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
        Rx = np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
        R = Rx @ Rz
        C = R.T @ np.array([0.1 * i, -0.2, -600.0])                   # the camera 600 units from the scene, looking at it
        K = np.array([[2890.0 + i, 0.0, 820.0], [0.0, 2880.0, 610.0 - i], [0.0, 0.0, 1.0]])
        W = np.eye(4)
        W[:3, :4] = K @ np.concatenate([R, (-R @ C)[:, None]], 1)
        Sm = np.diag([150.0, 150.0, 150.0, 1.0])
        Sm[:3, 3] = [10.0, -20.0, 5.0]
        mats["world_mat_%d" % i], mats["scale_mat_%d" % i] = W, Sm
        Ps.append(W @ Sm)
    path = str(tmp_path / "cameras.npz")
    np.savez(path, **mats)
    opt = _opt("--cams", path, "--views", "0,2", "--width", "1600", "--height", "1200")
    w2c, K = show.cameras_of(opt)
    assert w2c.shape == (2, 4, 4) and K.shape == (2, 3, 3)
    cams = show.pack_cameras(w2c, K)
    X = rng.uniform(-0.8, 0.8, (20, 3))
    for f, i in enumerate((0, 2)):
        h = (Ps[i] @ np.concatenate([X, np.ones((20, 1))], 1).T).T
        want = h[:, :2] / h[:, 2:3]
        Xc = S.to_cam(cams[f], X)
        x, y, ok = S.project(cams[f], Xc)
        assert ok.all() and (Xc[:, 2] > 0).all()
        print("view %d: worst difference %.2e px" % (i, np.abs(np.stack([x, y], -1) - want).max()))
        np.testing.assert_allclose(np.stack([x, y], -1), want, rtol=0, atol=1e-2)
