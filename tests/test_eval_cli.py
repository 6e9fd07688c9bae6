"""python -m neat_amd.evaluate end to end on files written from g20_evaluation.npz (GPU): each of the four sub-commands reproduces the
numbers that the reference's scripts printed for the same scene.  The golden's k-th shuffle is numpy.random.default_rng(11 + k)'s
permutation, which is what --seed 11 + k draws.  The bar on a mean is n 2^-53 relative, n the number of distances it averages
(tests/test_eval_math.py).  Then argument errors and a missing library, without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(args, env=None):
    return subprocess.run([sys.executable, "-m", "neat_amd.evaluate"] + [str(a) for a in args], cwd=ROOT, capture_output=True, text=True,
                          env=dict(os.environ, **(env or {})), timeout=600)


@pytest.fixture(scope="module")
def files(golden, tmp_path_factory):
    from scipy.io import savemat
    from neat_amd import ply
    g = golden("g20_evaluation")
    d = tmp_path_factory.mktemp("dtu")
    os.makedirs(d / "ObsMask")
    os.makedirs(d / "Points" / "stl")
    savemat(str(d / "ObsMask" / "ObsMask7_10.mat"), {"ObsMask": g["obs"], "BB": g["bb"], "Res": np.array([[float(g["res"])]])})
    savemat(str(d / "ObsMask" / "Plane7.mat"), {"P": g["plane"]})
    ply.write_ply_cloud(str(d / "Points" / "stl" / "stl007_total.ply"), g["stl"].astype(np.float64))
    write_mesh_f64(str(d / "surface_100.ply"), g["verts"], g["faces"])
    ply.write_ply_cloud(str(d / "cloud.ply"), g["pcd_cloud"])
    np.savez(str(d / "cameras.npz"), scale_mat_0=g["scale_mat"])
    np.savez(str(d / "x-wfi_checked.npz"), lines3d=g["lines"], scores=g["scores"])
    torch.save({"lines3d_wfi_checked": torch.tensor(g["lines"]), "junctions3d_initial": torch.tensor(g["abc_junctions_pred"])}, str(d / "x-neat.pth"))
    os.makedirs(d / "abc")
    with open(d / "abc" / "lines.json", "w") as f:
        json.dump({"junctions": g["abc_junctions_gt"].tolist(), "lines": g["abc_edges_gt"].tolist()}, f)
    with open(d / "abc" / "offset_scale.txt", "w") as f:
        f.write(" ".join(repr(float(v)) for v in g["abc_offset_scale"]))
    return g, d


def write_mesh_f64(path, verts, faces):
    """A binary PLY with double vertices: the reference read this mesh in float64, and a float32 file would be another mesh."""
    rec = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, faces
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                  "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode("ascii"))
        fh.write(np.ascontiguousarray(verts, dtype="<f8").tobytes())
        fh.write(rec.tobytes())


def bar(n):
    return n * 2.0 ** -53


def close(got, ref, n, what):
    print(what, got, ref, "rel %.3g" % (abs(got - ref) / ref), "bar %.3g" % bar(n))
    assert abs(got - ref) <= bar(n) * ref, what


def common(d, g):
    return ["--scan", 7, "--dataset_dir", d, "--patch_size", float(g["patch"])]


@pytest.mark.gpu
def test_dtu_mesh_and_pcd_end_to_end(files):
    from neat_amd import ply
    g, d = files
    r = run_cli(["dtu-mesh", "--data", d / "surface_100.ply", "--vis_out_dir", d / "vis", "--seed", 11] + common(d, g))
    assert r.returncode == 0, r.stderr
    vis = ply.read_ply(str(d / "vis" / "vis_007_s2d.ply"))
    assert vis["points"].shape == (len(g["stl"]), 3) and vis["colors"].shape == (len(g["stl"]), 3)
    down = ply.read_ply(str(d / "vis" / "vis_007_d2s.ply"))
    assert np.array_equal(down["points"], g["mesh_data_down"]) and down["colors"].shape == down["points"].shape
    # the averaged distances are counted from the colours: white to red is a distance below max_dist, green one beyond, blue not scored
    na = int((down["colors"][:, 0] == 255).sum())
    nc = int((vis["colors"][:, 0] == 255).sum())
    ref = g["mesh_numbers"]
    text = [float(x) for x in r.stdout.strip().split("\n")[-1].split(" ")]
    saved = [float(x) for x in open(d / "surface_100.txt").read().split("\t")]
    assert len(text) == 3 and text == saved
    close(text[0], ref[0], na, "mesh acc"), close(text[1], ref[1], nc, "mesh comp"), close(text[2], ref[2], max(na, nc) + 1, "mesh overall")
    # pcd mode; --json carries the stages and the counts
    r = run_cli(["dtu-mesh", "--data", d / "cloud.ply", "--mode", "pcd", "--json", "--seed", 12] + common(d, g))
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert set(out["seconds"]) == {"sample_s", "thin_s", "mask_s", "d2s_s", "s2d_s"} and out["points"] == len(g["pcd_cloud"])
    assert out["thinned"] == len(g["pcd_data_down"])
    ref, na, nc = g["pcd_numbers"], out["averaged"][0], out["averaged"][1]
    close(out["acc"], ref[0], na, "pcd acc"), close(out["comp"], ref[1], nc, "pcd comp")
    close(out["overall"], ref[2], max(na, nc) + 1, "pcd overall")
    saved = [float(x) for x in open(d / "cloud.txt").read().split("\t")]
    assert saved == [out["acc"], out["comp"], out["overall"]]


@pytest.mark.gpu
def test_lines_junctions_and_abc_end_to_end(files):
    from tests import eval_f64 as F
    g, d = files
    for name, seed, extra in (("lines", 13, []), ("lines_score", 14, ["--score", 0.6])):
        r = run_cli(["dtu-lines", "--data", d / "x-wfi_checked.npz", "--cam", d / "cameras.npz", "--seed", seed, "--json"] + extra + common(d, g))
        assert r.returncode == 0, r.stderr
        out = json.loads(r.stdout.strip().split("\n")[-1])
        ref, na, nc = g[name + "_numbers"], out["averaged"][0], out["averaged"][1]
        close(out["acc"], ref[0], na, name + " acc"), close(out["comp"], ref[1], nc, name + " comp")
        close(out["mean_length"], ref[2], out["num_lines"], name + " length")
        assert out["num_lines"] == ref[3]
    # junctions are not thinned, so the permutation only reorders a sum; the text output, as the reference prints it
    det = {}          # the text output carries no counts: the oracle's, on two dozen junctions
    F.dtu_scores(F.junction_cloud(g["lines"], g["scale_mat"])[0], g["stl"], g["obs"], g["bb"], float(g["res"]), g["plane"], patch=float(g["patch"]),
                 f32_quotient=True, thinning=False, details=det)
    na, nc = int((det["dist_d2s"] < 20.0).sum()), int((det["dist_s2d"] < 20.0).sum())
    for name, data in (("junc_pth", "x-neat.pth"), ("junc_npz", "x-wfi_checked.npz")):
        r = run_cli(["dtu-junctions", "--data", d / data, "--cam", d / "cameras.npz"] + common(d, g))
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().split("\n")
        ref = g[name + "_numbers"]
        acc, comp = float(lines[-2].split("ACC = ")[1].split()[0]), float(lines[-2].split("COMP = ")[1].split()[0])
        close(acc, ref[0], na, name + " acc"), close(comp, ref[1], nc, name + " comp")
        assert lines[-1] == "num junctions: %d" % ref[2]
    r = run_cli(["abc", "--data", d / "x-neat.pth", "--scan", d / "abc"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split("\n")[-2:] == [str(s) for s in g["abc_lines"]]


def test_argument_errors():
    from neat_amd.evaluate import build_parser
    ap = build_parser()
    for bad in ([], ["dtu-lines"], ["abc", "--data", "x"], ["dtu-mesh", "--mode", "voxels"], ["dtu-junctions", "--data", "x", "--scan", "a"],
                ["nothing"], ["dtu-mesh", "--gpu", "zero"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_a_missing_library_is_an_error_not_a_fallback(tmp_path):
    r = run_cli(["abc", "--data", "none.pth", "--scan", "none"], env={"NEAT_HIP_LIB": str(tmp_path / "absent.so")})
    assert r.returncode != 0 and "is missing" in r.stderr and "fallback" in r.stderr
