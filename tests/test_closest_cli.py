"""python -m neat_amd.raycast distance: the parser, the names and the refusal to overwrite without a GPU; --data and --points end to
end on a box mesh with its twelve edges as lines (what scenegen --shape box writes), marked gpu."""
import json
import os

import numpy as np
import pytest

from tests import closest_f64 as CP
from tests.raycast_f64 import BOX_EDGES


def test_parser_and_argument_errors(capsys):
    from neat_amd import raycast
    opt = raycast.parse_args(["distance", "--mesh", "m.obj", "--data", "x-wfi.npz"])
    assert (opt.command, opt.samples, opt.threshold, opt.max_dist, opt.scale_file, opt.gpu, opt.json, opt.overwrite, opt.points) == (
        "distance", 32, 0.05, float("inf"), None, 0, False, False, None)
    opt = raycast.parse_args(["distance", "--mesh", "m.PLY", "--points", "cloud.ply", "--threshold", "0.1", "--max-dist", "2", "--samples", "8",
                              "--scale-file", "offset_scale.txt", "--json", "--overwrite", "--gpu", "1"])
    assert (opt.points, opt.data, opt.threshold, opt.max_dist, opt.samples, opt.scale_file, opt.json, opt.overwrite, opt.gpu) == (
        "cloud.ply", None, 0.1, 2.0, 8, "offset_scale.txt", True, True, 1)
    for bad in (["distance", "--mesh", "m.ply"], ["distance", "--mesh", "m.ply", "--data", "x.npz", "--points", "p.ply"],
                ["distance", "--data", "x.npz"], ["distance", "--mesh", "m.stl", "--data", "x.npz"],
                ["distance", "--mesh", "m.ply", "--points", "p.npz"], ["distance", "--mesh", "m.ply", "--data", "x.npz", "--samples", "1"],
                ["distance", "--mesh", "m.ply", "--data", "x.npz", "--threshold", "-1"],
                ["distance", "--mesh", "m.ply", "--data", "x.npz", "--max-dist", "nan"]):
        with pytest.raises(SystemExit) as e:
            raycast.main(bad)
        assert e.value.code == 2 and "usage:" in capsys.readouterr().err, bad


def test_output_name_and_refusal_without_overwrite(tmp_path, capsys):
    from neat_amd import raycast
    assert raycast.dist_path("/a/b/latest-wfi.npz") == "/a/b/latest-wfi_dist.npz"
    assert raycast.dist_path("runs/x-neat.pth") == "runs/x-neat_dist.npz" and raycast.dist_path("surface_100.ply") == "surface_100_dist.npz"
    data = tmp_path / "lines.npz"
    np.savez(data, lines3d=np.zeros((1, 2, 3)))
    out = tmp_path / "lines_dist.npz"
    out.write_bytes(b"kept")
    # an output that is already there is left alone, before the mesh is read or a device is touched
    assert raycast.main(["distance", "--mesh", str(tmp_path / "missing.obj"), "--data", str(data)]) == 0
    assert "exists:" in capsys.readouterr().out and out.read_bytes() == b"kept"
    # the frame of --scale-file: x / scale - offset, evaluate abc's mapping
    (tmp_path / "offset_scale.txt").write_text("0.5 -0.25 1.0 2.0\n")
    x = np.array([[[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]])
    assert np.array_equal(raycast.to_mesh_frame(x, str(tmp_path / "offset_scale.txt")), [[[0.0, 1.25, 0.5], [-0.5, 0.25, -1.0]]])


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """A box mesh as mesh.obj (quads, as scenegen writes them) and as a PLY, its twelve edges as lines, line 10 lifted 0.125 off its
    face and line 11 pushed 0.125 along itself; everything dyadic, so that the files hold the numbers exactly."""
    from neat_amd import ply
    tmp = tmp_path_factory.mktemp("closest_cli")
    verts, faces = CP.box(lo=(-0.5, -0.25, -0.125), hi=(0.5, 0.25, 0.125))
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    (tmp / "mesh.obj").write_text("".join("v %.17g %.17g %.17g\n" % tuple(p) for p in verts) + "".join("f %d %d %d %d\n" % tuple(i + 1 for i in q) for q in quads))
    ply.write_ply(str(tmp / "mesh.ply"), verts, faces)
    lines = verts[np.asarray(BOX_EDGES)]
    lines[10] = lines[10] + np.array([0.0, 0.125, 0.0])           # edge (2, 6) runs along z at x = -0.5, y = 0.25: lifted off the face y = 0.25
    lines[11] = lines[11] + np.array([0.0, 0.0, 0.125])           # edge (3, 7) runs along z at x = 0.5, y = 0.25: moved along itself
    return {"tmp": tmp, "verts": verts, "faces": faces, "lines": lines}


@pytest.mark.gpu
def test_distance_of_lines(scan, capsys):
    from neat_amd import raycast, run_io
    tmp, verts, faces, lines = scan["tmp"], scan["verts"], scan["faces"], scan["lines"]
    data = str(tmp / "box-wfi.npz")
    np.savez(data, lines3d=lines)
    args = ["distance", "--mesh", str(tmp / "mesh.obj"), "--data", data, "--samples", "8", "--threshold", "0.0625", "--json"]
    assert raycast.main(args) == 0
    out = capsys.readouterr().out
    path = raycast.dist_path(data)
    assert path == str(tmp / "box-wfi_dist.npz") and os.path.exists(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["dist", "max", "mean", "on_surface", "tri"]
        got = {k: z[k] for k in z.files}
    mverts, mfaces = raycast.read_mesh(str(tmp / "mesh.obj"))
    assert np.array_equal(mverts, verts) and mfaces.shape == (12, 3)
    want = CP.closest_all(mverts, mfaces, CP.line_samples(run_io.load_lines(data)[0], 8).reshape(-1, 3))
    dist = np.sqrt(want[0]).reshape(12, 8)
    assert got["dist"].dtype == np.float64 and got["dist"].tobytes() == dist.tobytes()
    assert got["tri"].dtype == np.int32 and np.array_equal(got["tri"], want[1].reshape(12, 8))
    assert np.array_equal(got["mean"], dist.mean(1)) and np.array_equal(got["max"], dist.max(1))
    assert got["on_surface"].dtype == bool and got["on_surface"].tolist() == [True] * 10 + [False, False]
    # ten edges lie on the mesh (their samples to the rounding of the sampling formula); line 10 hangs 0.125 off its face; line 11, moved
    # along itself, leaves the mesh by exactly 0.125 at its far end
    assert dist[:10].max() <= 1e-15 and np.abs(dist[10] - 0.125).max() <= 1e-15 and dist[11].max() == 0.125 and dist[11].min() <= 1e-15
    report = json.loads(out.strip().splitlines()[-1])
    assert report["lines"] == 12 and report["on_surface"] == 10 and report["samples"] == 8 and report["triangles"] == 12 and report["path"] == path
    assert report["mean"] == float(dist.mean(1).mean()) and report["median"] == float(np.median(dist.mean(1))) and report["query_s"] > 0
    assert "10 / 12 lines on the surface" in out and "mean distance %.6g, median %.6g" % (report["mean"], report["median"]) in out
    # kept without --overwrite, replaced with it; a stricter threshold; no temporary file stays behind
    stamp = os.stat(path).st_mtime_ns
    assert raycast.main(args) == 0 and "exists:" in capsys.readouterr().out and os.stat(path).st_mtime_ns == stamp
    assert raycast.main(args[:-1] + ["--overwrite", "--threshold", "0.125", "--max-dist", "0.0625"]) == 0
    assert "10 / 12 lines" in capsys.readouterr().out
    with np.load(path) as z:
        assert np.isinf(z["dist"][10]).all() and (z["tri"][10] == -1).all() and z["on_surface"].tolist() == [True] * 10 + [False, False]
    # --scale-file: lines stored in the model frame come back to the mesh's frame
    (tmp / "offset_scale.txt").write_text("0.25 -0.5 0.125 0.5\n")
    model = (lines + np.array([0.25, -0.5, 0.125])) * 0.5
    np.savez(str(tmp / "model-wfi.npz"), lines3d=model)
    assert raycast.main(["distance", "--mesh", str(tmp / "mesh.ply"), "--data", str(tmp / "model-wfi.npz"), "--samples", "8", "--threshold", "0.0625",
                         "--scale-file", str(tmp / "offset_scale.txt")]) == 0
    with np.load(str(tmp / "model-wfi_dist.npz")) as z:
        assert z["dist"].tobytes() == dist.tobytes()
    assert not [n for n in os.listdir(tmp) if ".tmp" in n]


@pytest.mark.gpu
def test_distance_of_points_and_a_refused_mesh(scan, capsys):
    from neat_amd import ply, raycast
    tmp, verts, faces = scan["tmp"], scan["verts"], scan["faces"]
    rng = np.random.default_rng(12)
    cloud = np.concatenate([verts, rng.uniform(-0.75, 0.75, (500, 3))])
    ply.write_ply_cloud(str(tmp / "cloud.ply"), cloud)
    args = ["distance", "--mesh", str(tmp / "mesh.ply"), "--points", str(tmp / "cloud.ply"), "--threshold", "0.1", "--json"]
    assert raycast.main(args) == 0
    out = capsys.readouterr().out
    path = str(tmp / "cloud_dist.npz")
    with np.load(path) as z:
        assert sorted(z.files) == ["dist", "point", "tri"]
        dist, tri, point = z["dist"], z["tri"], z["point"]
    want = CP.closest_all(verts, faces, cloud)
    assert dist.tobytes() == np.sqrt(want[0]).tobytes() and np.array_equal(tri, want[1]) and point.tobytes() == want[2].tobytes()
    assert (dist[:8] == 0.0).all()
    report = json.loads(out.strip().splitlines()[-1])
    assert report["points"] == 508 and report["acc"] == float(dist.mean()) and report["median"] == float(np.median(dist))
    assert report["prec"] == float((dist < 0.1).mean()) and 0.0 < report["prec"] < 1.0
    assert "Acc %.6g, median %.6g, Prec %.4f" % (report["acc"], report["median"], report["prec"]) in out
    # the other way round: the vertices of the mesh against a mesh, here itself
    assert raycast.main(["distance", "--mesh", str(tmp / "mesh.obj"), "--points", str(tmp / "mesh.ply")]) == 0
    assert "8 points; Acc 0, median 0, Prec 1.0000" in capsys.readouterr().out
    # a face index outside the vertices: an error message and an exit code, no file
    (tmp / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 2 9\n")
    os.remove(path)
    assert raycast.main(["distance", "--mesh", str(tmp / "bad.obj"), "--points", str(tmp / "cloud.ply")]) == 1
    cap = capsys.readouterr()
    assert "a face index lies outside the vertices" in cap.err and not os.path.exists(path)
    assert not [n for n in os.listdir(tmp) if ".tmp" in n]
