"""The evaluation's arithmetic without a device: tests/eval_f64.py (the numpy restatement of the reference's four scripts) against
g20_evaluation.npz, which the reference's own scripts produced; the device's round rule for the thinning against the sequential loop; the
PLY reader, the .mat / .npz loaders and the CLI's parsing and output format.

Bar of the means: n 2^-53 relative, n the number of distances that the mean averages (those below max_dist), counted per mean.  Both
sides average the same n non-negative float64 distances (the thinned sets are identical) and a sum of n such terms carries under
n 2^-53 relative error in any order.  "overall" halves the sum of two means: the larger of their two counts, plus one for the addition.
The mean length averages one length per line.  n < 2^14 here, so every bar is under 1e-12.
"""
import os

import numpy as np
import pytest

from tests import eval_f64 as F


def bar(n):
    return n * 2.0 ** -53


def counts(details, max_dist=20.0):
    """the number of averaged distances of each of the two means"""
    return int((details["dist_d2s"] < max_dist).sum()), int((details["dist_s2d"] < max_dist).sum())


def close(got, ref, n, what):
    print(what, got, ref, "rel %.3g" % (abs(got - ref) / ref), "bar %.3g" % bar(n))
    assert abs(got - ref) <= bar(n) * ref, what


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_evaluation")


def kw(g, **extra):
    return dict(obs_mask=g["obs"], bb=g["bb"], res=float(g["res"]), plane=g["plane"], patch=float(g["patch"]), **extra)


def test_sampling_and_thinning_are_the_reference_s_row_for_row(g20):
    cloud = F.sample_mesh(g20["verts"], g20["faces"], 0.2)
    assert cloud.shape[0] == g20["mesh_perm"].shape[0]
    seq = cloud[g20["mesh_perm"]]
    down = seq[F.thin_sequential(seq, 0.2)]
    assert down.shape == g20["mesh_data_down"].shape and np.array_equal(down, g20["mesh_data_down"])
    seq = g20["pcd_cloud"][g20["pcd_perm"]]
    assert np.array_equal(seq[F.thin_sequential(seq, 0.2)], g20["pcd_data_down"])


def test_restatement_reproduces_every_printed_number(g20):
    g = g20
    cloud = F.sample_mesh(g["verts"], g["faces"], 0.2)
    for name, pts, perm in (("mesh", cloud, g["mesh_perm"]), ("pcd", g["pcd_cloud"], g["pcd_perm"])):
        det = {}
        acc, comp = F.dtu_scores(pts, g["stl"], order=perm, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        close((acc + comp) / 2, ref[2], max(na, nc) + 1, name + " overall")
    for name, lines in (("lines", g["lines"]), ("lines_score", g["lines"][g["scores"] < 0.6])):
        det = {}
        pts, mean_length = F.line_cloud(lines, g["scale_mat"])
        acc, comp = F.dtu_scores(pts, g["stl"], order=g[name + "_perm"], f32_quotient=True, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        close(mean_length, ref[2], lines.shape[0], name + " length")
        assert lines.shape[0] == ref[3]
    for name in ("junc_pth", "junc_npz"):
        det = {}
        pts, count = F.junction_cloud(g["lines"], g["scale_mat"])
        acc, comp = F.dtu_scores(pts, g["stl"], order=g[name + "_perm"], f32_quotient=True, thinning=False, details=det, **kw(g))
        ref, (na, nc) = g[name + "_numbers"], counts(det)
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        assert count == ref[2], name
    res = F.abc_scores(g["abc_junctions_pred"], g["lines"], g["abc_junctions_gt"], g["abc_edges_gt"], g["abc_offset_scale"])
    from neat_amd.evaluate import abc_lines
    assert list(abc_lines(res)) == [str(s) for s in g["abc_lines"]]


def test_the_scene_exercises_every_branch(g20):
    g = g20
    cloud = F.sample_mesh(g["verts"], g["faces"], 0.2)
    seq = cloud[g["mesh_perm"]]
    flags = F.obs_flags(g["mesh_data_down"], g["obs"], g["bb"], float(g["res"]), float(g["patch"]))
    box, seen = int(((flags & 1) != 0).sum()), int(((flags & 2) != 0).sum())
    assert 0 < seen < box < len(flags)
    assert len(g["mesh_data_down"]) < len(seq)
    hom = np.concatenate([g["stl"].astype(np.float64), np.ones((len(g["stl"]), 1))], 1)
    above = (g["plane"].reshape(1, 4) * hom).sum(-1) > 0
    assert 0 < above.sum() < len(above)
    f32 = F.obs_flags(seq, g["obs"], g["bb"], float(g["res"]), float(g["patch"]), f32_quotient=True)
    assert f32.shape == (len(seq),)


@pytest.mark.parametrize("case", ["random", "lattice", "duplicates", "line"])
def test_round_rule_equals_the_sequential_loop(case):
    rng = np.random.default_rng(3)
    if case == "random":
        pts = rng.uniform(0, 3, (1500, 3))
    elif case == "lattice":          # unshuffled, spacing = radius exactly: long dependency chains and ties on the radius
        a = np.arange(9) * 0.2
        pts = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    elif case == "duplicates":
        base = rng.uniform(0, 1.5, (300, 3))
        pts = np.concatenate([base, base[:150], base[:50]])[rng.permutation(500)]
    else:
        pts = np.stack([np.arange(300) * 0.15, np.zeros(300), np.zeros(300)], 1)
    seq = F.thin_sequential(pts, 0.2)
    par, rounds = F.thin_rounds(pts, 0.2)
    assert np.array_equal(seq, par) and 1 <= rounds <= len(pts)
    kept = pts[seq]
    d2 = F.d2_rows(kept[:, None, :], kept[None])
    assert (d2[~np.eye(len(kept), dtype=bool)] > 0.04).all()


def test_ply_reader_ascii_binary_and_our_own_meshes(tmp_path):
    import torch
    from neat_amd import ply
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.25, 2]], dtype=np.float64)
    f = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int32)
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\nproperty list uchar int vertex_indices\n"
                 "end_header\n" + "".join("%r %r %r 255 0 7\n" % tuple(float(x) for x in r) for r in v) + "3 0 1 2\n3 1 2 3\n")
    r = ply.read_ply(str(p))
    assert np.array_equal(r["points"], v) and np.array_equal(r["faces"], f) and r["colors"].shape == (4, 3) and r["normals"] is None
    nrm = np.tile([[0.0, 0.0, 1.0]], (4, 1))
    ply.write_ply(str(tmp_path / "b.ply"), torch.tensor(v, dtype=torch.float32), torch.tensor(f), torch.tensor(nrm, dtype=torch.float32))
    r = ply.read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(r["points"], v.astype(np.float32).astype(np.float64)) and np.array_equal(r["faces"], f)
    assert np.array_equal(r["normals"], nrm)
    ply.write_ply(str(tmp_path / "c.ply"), torch.tensor(v, dtype=torch.float32), torch.tensor(f))
    assert ply.read_ply(str(tmp_path / "c.ply"))["normals"] is None
    ply.write_ply_cloud(str(tmp_path / "d.ply"), v * 1.1, np.array([[1, 0, 0.5]] * 4))          # a double cloud, as the stl clouds are
    r = ply.read_ply(str(tmp_path / "d.ply"))
    assert np.array_equal(r["points"], v * 1.1) and r["faces"] is None and r["colors"][0].tolist() == [255, 0, 128]
    (tmp_path / "e.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError):
        ply.read_ply(str(tmp_path / "e.ply"))
    (tmp_path / "f.ply").write_bytes(b"plx\n")
    with pytest.raises(ValueError):
        ply.read_ply(str(tmp_path / "f.ply"))


def test_mat_and_npz_loaders(tmp_path, g20):
    from scipy.io import savemat
    from neat_amd import evaluate as E
    os.makedirs(tmp_path / "ObsMask")
    savemat(str(tmp_path / "ObsMask" / "ObsMask7_10.mat"), {"ObsMask": g20["obs"], "BB": g20["bb"], "Res": np.array([[0.25]])})
    savemat(str(tmp_path / "ObsMask" / "Plane7.mat"), {"P": g20["plane"]})
    a = E.load_obs(str(tmp_path), 7)
    np.savez(str(tmp_path / "obs.npz"), ObsMask=g20["obs"], BB=g20["bb"], Res=0.25, P=g20["plane"])
    b = E.load_obs(npz=str(tmp_path / "obs.npz"))
    for m in (a, b):
        assert np.array_equal(m["ObsMask"], g20["obs"]) and np.array_equal(m["BB"], g20["bb"]) and m["Res"] == 0.25
        assert np.array_equal(m["P"], g20["plane"].reshape(4))
    np.savez(str(tmp_path / "bad.npz"), ObsMask=g20["obs"])
    with pytest.raises(KeyError):
        E.load_obs(npz=str(tmp_path / "bad.npz"))


def test_cli_flags_defaults_and_output_format():
    from neat_amd import evaluate as E
    ap = E.build_parser()
    o = ap.parse_args(["dtu-mesh"])
    assert (o.data, o.scan, o.mode, o.dataset_dir, o.downsample_density, o.patch_size, o.max_dist, o.visualize_threshold) == \
        ("data_in.ply", 1, "mesh", ".", 0.2, 60, 20, 10)
    assert (o.seed, o.gpu, o.json, o.vis_out_dir) == (0, 0, False, None)
    o = ap.parse_args(["dtu-lines", "--data", "x.npz", "--score", "0.5", "--noscale", "--seed", "4", "--gpu", "2", "--json"])
    assert (o.data, o.score, o.noscale, o.seed, o.gpu, o.json, o.cam, o.threshold) == ("x.npz", 0.5, True, 4, 2, True, None, 1.0)
    assert o.dataset_dir == "/home/xn/datasets/DTU" and o.downsample_density == 0.2 and o.max_dist == 20
    o = ap.parse_args(["dtu-junctions", "--data", "x-neat.pth", "--scan", "24"])
    assert o.scan == 24 and o.score is None
    o = ap.parse_args(["abc", "--data", "x-neat.pth", "--scan", "dir"])
    assert (o.data, o.scan) == ("x-neat.pth", "dir")
    res = {"junctions_precision": [0.0666, 1 / 3, 1.0], "junctions_recall": [0.0625, 0.3125, 0.9375],
           "lines_precision": [0.0, 1 / 3, 5 / 6], "lines_recall": [0.0, 4 / 11, 10 / 11]}
    assert E.abc_lines(res) == ("0.067 & 0.333 & 1.000 & 0.062 & 0.312 & 0.938", "0.000 & 0.333 & 0.833 & 0.000 & 0.364 & 0.909")
