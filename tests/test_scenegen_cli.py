"""The command line of neat_amd.scenegen: its arguments, the files of a scene directory and the 2-D wireframes made of a run list (host
only), and one run on the device whose directory the dataset, the detector and the triangulation take as it is."""
import json
import os

import numpy as np
import pytest
import torch


def test_arguments():
    from neat_amd import scenegen
    opt = scenegen.parse_args(["--shape", "box", "--out", "x"])
    assert (opt.views, opt.res, opt.focal, opt.radius, opt.ss, opt.name, opt.subdivide, opt.gpu, opt.overwrite) == (100, 512, 560.0, 2.0, 3, "gt", 0, 0, False)
    assert (opt.step, opt.min_len, opt.bias) == tuple(scenegen.DEFAULTS[k] for k in ("step", "min_len", "bias"))
    opt = scenegen.parse_args(["--mesh", "m.OBJ", "--lines", "l.json", "--out", "x", "--views", "6", "--res", "64", "--ss", "1", "--min-len", "3",
                               "--bias", "0.01", "--step", "0.5", "--name", "truth", "--subdivide", "2", "--overwrite"])
    assert (opt.mesh, opt.lines, opt.shape, opt.views, opt.res, opt.ss, opt.min_len, opt.bias, opt.step, opt.name, opt.subdivide, opt.overwrite) == \
        ("m.OBJ", "l.json", None, 6, 64, 1, 3.0, 0.01, 0.5, "truth", 2, True)
    for bad in (["--out", "x"], ["--shape", "box"], ["--shape", "box", "--mesh", "m.obj", "--lines", "l.json", "--out", "x"],
                ["--mesh", "m.obj", "--out", "x"], ["--mesh", "m.stl", "--lines", "l.json", "--out", "x"], ["--shape", "ball", "--out", "x"],
                ["--shape", "box", "--out", "x", "--ss", "0"], ["--shape", "box", "--out", "x", "--ss", "17"],
                ["--shape", "box", "--out", "x", "--step", "0"], ["--shape", "box", "--out", "x", "--step", "0.001"],
                ["--shape", "box", "--out", "x", "--views", "0"], ["--shape", "box", "--out", "x", "--bias", "-1"]):
        with pytest.raises(SystemExit):
            scenegen.parse_args(bad)


def test_file_names_and_the_static_files(tmp_path):
    from neat_amd import ply, raycast, scenegen
    out = str(tmp_path / "scene")
    paths = scenegen.scene_paths(out, 3, "gt")
    rel = lambda p: os.path.relpath(p, out).replace(os.sep, "/")
    assert [rel(p) for p in paths["images"]] == ["images/image_0000.png", "images/image_0001.png", "images/image_0002.png"]
    assert [rel(p) for p in paths["masks"]] == ["mask/0000.png", "mask/0001.png", "mask/0002.png"]
    assert [rel(p) for p in paths["wireframes"]] == ["gt/image_0000.json", "gt/image_0001.json", "gt/image_0002.json"]
    assert [rel(paths[k]) for k in ("cameras", "mesh", "lines", "offset_scale")] == ["cameras.npz", "mesh.obj", "lines.json", "offset_scale.txt"]
    verts, faces, J, E = scenegen.shapes["lblock"]
    verts, J = scenegen.normalise(verts * 1.7 + 0.3, J * 1.7 + 0.3)
    K, poses = scenegen.cameras(3, 64)
    scenegen.write_static(paths, verts, faces, J, E, K, poses)
    assert open(paths["offset_scale"]).read().split() == ["0", "0", "0", "1"]
    with np.load(paths["cameras"]) as z:
        assert sorted(z.files) == ["extrinsics", "intrinsics"] and z["intrinsics"].shape == (3, 3, 3) and z["extrinsics"].shape == (3, 4, 4)
        assert np.array_equal(z["extrinsics"], poses) and np.array_equal(z["intrinsics"], K)
    v, f = ply.read_obj(paths["mesh"])
    assert np.array_equal(v, verts) and np.array_equal(f, faces)                     # the float64 values come back
    j, e = scenegen.read_lines(paths["lines"])
    assert np.array_equal(j, J) and np.array_equal(e, E)
    inv_scale, j32, e2 = raycast.scan_wireframe(out)                                 # what raycast analysis and evaluate abc read
    assert np.array_equal(inv_scale, np.eye(4)) and np.array_equal(j32, J.astype(np.float32)) and np.array_equal(e2, E)
    assert not [n for n in os.listdir(out) if ".tmp" in n]


def test_wireframes_share_true_junctions_and_keep_the_other_ends_apart():
    from neat_amd import scenegen
    E = np.array([[0, 1], [1, 2], [2, 0]], np.int32)
    idx = np.array([[0, 0, 0, 9], [0, 1, 0, 4], [0, 1, 7, 9], [0, 2, 0, 9], [2, 0, 3, 9]], np.int32)        # (view, edge, first, last)
    p2 = np.array([[1.0, 1.0, 9.0, 1.0], [9.0, 1.0 + 1e-13, 9.0, 5.0], [9.0, 7.0, 9.0, 9.0], [9.0, 9.0, 1.0, 1.0], [4.0, 1.0, 9.0, 1.0]])
    junc = np.array([[1, 1], [1, 0], [0, 1], [1, 1], [0, 1]], bool)
    g0, g1, g2 = scenegen.to_wireframes((idx, p2, np.zeros((5, 2, 3)), junc), 3, 12, 16, E)
    # view 0: junctions 0, 1, 2 once each, in the order met, and the two ends of the occlusion gap on edge 1 on their own
    assert g0.vertices.tolist() == [[1.0, 1.0], [9.0, 1.0], [9.0, 5.0], [9.0, 7.0], [9.0, 9.0]]
    assert g0.edges.tolist() == [[0, 1], [1, 2], [3, 4], [4, 0]]
    assert g0.weights.tolist() == [1.0] * 4 and g0.v_confidences.tolist() == [1.0] * 5
    assert (g0.frame_height, g0.frame_width) == (12, 16) and g0.edges.dtype == torch.long and g0.vertices.dtype == torch.float32
    assert g0.line_segments(0.05).shape == (4, 5)
    assert g1.vertices.shape == (0, 2) and g1.edges.shape == (0, 2)                     # a view without a run
    assert g2.vertices.tolist() == [[4.0, 1.0], [9.0, 1.0]] and g2.edges.tolist() == [[0, 1]]
    # without the edge list nothing names a junction: every end stays apart
    h0 = scenegen.to_wireframes((idx, p2, np.zeros((5, 2, 3)), junc), 3, 12, 16)[0]
    assert h0.vertices.shape == (8, 2) and h0.edges.tolist() == [[0, 1], [2, 3], [4, 5], [6, 7]]
    d = g0.jsonize()
    assert sorted(d) == ["edges", "edges-weights", "height", "vertices", "vertices-score", "width"] and json.dumps(d)


@pytest.mark.gpu
def test_cli_writes_a_scene_the_other_tools_take(tmp_path, capsys):
    from neat_amd import datasets, detect, run_io, scenegen, triangulate
    from tests import triangulate_f64 as T
    from tests.test_triangulate_gpu import check_lines, host
    out = str(tmp_path / "box")
    assert scenegen.main(["--shape", "box", "--views", "6", "--res", "64", "--out", out]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith(out + ": 6 views of 64 x 64, 12 triangles, 12 edges, ")
    paths = scenegen.scene_paths(out, 6)
    every = paths["images"] + paths["masks"] + paths["wireframes"] + [paths[k] for k in ("cameras", "mesh", "lines", "offset_scale")]
    assert all(os.path.isfile(p) for p in every)
    found = sorted(os.path.join(d, n) for d, _, names in os.walk(out) for n in names)
    assert found == sorted(every)                                                     # and nothing else, no temporary file
    assert scenegen.main(["--shape", "box", "--views", "6", "--res", "64", "--out", out]) == 0
    assert capsys.readouterr().out.startswith("exists: ")
    # the dataset loads it as it is
    ds = datasets.BlenderDataset("box", [64, 64], line_detector="gt", data_root=str(tmp_path))
    assert len(ds) == 6
    images = np.stack([np.rint(ds.rgb_images[i].numpy() * 255.0).astype(np.uint8).reshape(64, 64, 3) for i in range(6)])
    K, poses = scenegen.cameras(6, 64)
    assert np.array_equal(ds.pose_all.numpy(), poses.astype(np.float32)) and np.array_equal(ds.intrinsics_all.numpy(), K.astype(np.float32))
    assert [int(w.edges.shape[0]) for w in ds.wireframes] == [7, 9, 7, 9, 7, 9]       # the edges of a box seen over an edge and from a corner
    # the detector runs on its pictures
    from PIL import Image
    pics = torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths["images"]])).to("cuda:0")
    masks = np.stack([np.asarray(Image.open(p)) for p in paths["masks"]])
    assert tuple(pics.shape) == (6, 64, 64, 3) and masks.shape == (6, 64, 64) and set(np.unique(masks)) == {0, 255}
    assert np.array_equal(images, pics.cpu().numpy())                                 # the dataset's colours are the pictures'
    found_lines = detect.lines(pics)
    assert int(found_lines[-1][-1]) == found_lines[0].shape[0] and tuple(found_lines[-1].shape) == (7,)
    # triangulation from its views and its ground-truth segments equals the float64 restatement on the same input
    segments, Ks, Ts = run_io.dataset_views(ds)
    seg64 = [np.ascontiguousarray(s[:, :4].numpy(), dtype=np.float64) for s in segments]
    Ks64 = np.stack([k.numpy() for k in Ks]).astype(np.float64)
    Ts64 = np.stack([t.numpy() for t in Ts]).astype(np.float64)
    want = T.lines(seg64, Ks64, Ts64)
    got = host(triangulate.lines([torch.from_numpy(s).to("cuda:0") for s in seg64], Ks64, Ts64))
    assert want["lines3d"].shape[0] > 0
    check_lines(got, want)
