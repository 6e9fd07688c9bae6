"""python -m neat_amd.raycast check and analysis end to end on the tiny saved run of tests/util_run.py (three 64 x 64 views on the
radius-2 sphere about the origin); the parts that launch kernels are marked gpu."""
import json
import os

import numpy as np
import pytest
import torch

from tests import raycast_f64 as RC


def test_argument_errors_use_the_parser(capsys):
    from neat_amd import raycast
    for bad in (["check", "--mesh", "m.ply", "--data", "x.npz"], ["check", "--mesh", "m.ply", "--data", "x.npz", "--cams", "c.npz", "--min-views", "-1"],
                ["check", "--data", "x.npz", "--cams", "c.npz"], ["analysis", "--scan", "s"], ["nothing"]):
        with pytest.raises(SystemExit) as e:
            raycast.main(bad)
        assert e.value.code == 2 and "usage:" in capsys.readouterr().err


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tests.util_run import write_synth_run
    tmp = tmp_path_factory.mktemp("raycast_cli")
    run = write_synth_run(tmp, n_views=3)
    with np.load(os.path.join(run["data_root"], "abc", "toy", "cameras.npz")) as z:
        poses, intr = z["extrinsics"].astype(np.float64), z["intrinsics"].astype(np.float64)
    return {**run, "tmp": tmp, "poses": poses, "intrinsics": intr}


@pytest.mark.gpu
def test_check_writes_the_occlusion_file_and_keeps_it(run, capsys):
    from neat_amd import ply, raycast, run_io
    centres = run["poses"][:, :3, 3]
    assert (np.linalg.norm(centres, axis=1) > 1.5).all()
    verts, faces = RC.icosphere(2)
    mesh = str(run["tmp"] / "occluder.ply")
    ply.write_ply(mesh, 0.3 * verts, faces)                       # a sphere of radius 0.3 about the origin
    # six short segments between camera 0 and the sphere, six inside the sphere
    rng = np.random.default_rng(1)
    u = rng.standard_normal((12, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c0 = centres[0] / np.linalg.norm(centres[0])
    a = 0.6 * c0 + 0.05 * u[:6]
    lines = np.concatenate([np.stack([a, a + 0.05 * u[6:]], 1), np.stack([0.1 * u[:6], 0.1 * u[6:]], 1)])
    (run["dir"] / "wireframes").mkdir(exist_ok=True)
    data = str(run["dir"] / "wireframes" / "latest-abcdefgh-wfi.npz")
    np.savez(data, lines3d=lines)
    args = ["check", "--mesh", mesh, "--data", data, "--conf", run["conf"], "--data_root", run["data_root"], "--min-views", "1", "--json"]
    assert raycast.main(args) == 0
    out = capsys.readouterr().out
    path = raycast.out_path(data)
    assert path == str(run["dir"] / "wireframes" / "latest-abcdefgh-wfi_occlmesh.npz") and os.path.exists(path)
    report = json.loads(out.strip().splitlines()[-1])
    assert report["total"] == 12 and report["views"] == 3 and report["triangles"] == 320 and report["cast_s"] > 0 and report["path"] == path
    assert "kept %d / 12 lines" % report["kept"] in out
    with np.load(path) as z:
        assert sorted(z.files) == ["kept", "lines3d", "views"]
        views, kept, kept_lines = z["views"], z["kept"], z["lines3d"]
    assert views.dtype == np.int32 and views.shape == (12,) and kept.dtype == bool and kept.shape == (12,)
    assert kept.tolist() == [True] * 6 + [False] * 6 and (views[6:] == 0).all() and (views[:6] >= 1).all() and views.max() <= 3
    assert np.array_equal(kept_lines, lines[kept]) and report["kept"] == 6
    assert np.array_equal(run_io.load_lines(path)[0], kept_lines)                # what show and evaluate dtu-lines read
    # the library gives what the file holds; the float64 rule on the same targets agrees
    cams = np.linalg.inv(run["poses"])
    v32 = np.asarray(0.3 * verts, np.float32).astype(np.float64)                 # the PLY holds float32
    scene = raycast.build(v32, faces, torch.device("cuda:0"))
    frac = raycast.visible_lines(scene, torch.from_numpy(lines), cams).cpu().numpy()
    assert np.array_equal(run_io.keep_rule(frac, 1, 0.5)[0], views)
    s = np.linspace(0.0, 1.0, 16)
    lines32 = lines.astype(np.float32).astype(np.float64)
    for f in range(3):
        c = centres[f].astype(np.float32).astype(np.float64)
        p = lines32[:, :1] + s[None, :, None] * (lines32[:, 1:] - lines32[:, :1])
        vec = (p - c).reshape(-1, 3)
        L = np.linalg.norm(vec, axis=1)
        t, _, _ = RC.cast_all(v32, faces, np.broadcast_to(c, vec.shape), vec / L[:, None], t_max=L - 0.01)
        ref = np.isinf(t).reshape(12, 16).mean(1)
        assert np.abs(ref - frac[f]).max() < 1e-6, f
    # the cameras from a file instead of the conf
    cams_npz = os.path.join(run["data_root"], "abc", "toy", "cameras.npz")
    stamp = os.stat(path).st_mtime_ns
    args2 = ["check", "--mesh", mesh, "--data", data, "--cams", cams_npz, "--min-views", "1"]
    assert raycast.main(args2) == 0 and "exists:" in capsys.readouterr().out and os.stat(path).st_mtime_ns == stamp
    assert raycast.main(args2 + ["--overwrite", "--min-views", "4"]) == 0
    with np.load(path) as z:
        assert not z["kept"].any() and z["lines3d"].shape == (0, 2, 3) and np.array_equal(z["views"], views)


def _project(K, w2c, X):
    x = (K @ (w2c[:3, :3] @ X.T + w2c[:3, 3:])).T
    den = x[:, 2:]
    den = den + np.where(np.abs(den) < 1e-8, 1e-8, 0.0) * np.where(den >= 0, 1.0, -1.0)
    return (x / den)[:, :2]


@pytest.mark.gpu
def test_analysis_on_a_hand_made_scan(run, capsys):
    from scipy.optimize import linear_sum_assignment
    from neat_amd import ops, raycast
    verts, faces = RC.box(lo=(-0.25, -0.2, -0.15), hi=(0.25, 0.2, 0.15))          # small enough to project inside every 64 x 64 view
    edges = np.asarray(RC.BOX_EDGES)
    off, scale = np.array([0.1, -0.05, 0.02]), 2.0
    # raw = what inv(scale_mat) maps onto the box: x' = scale (x + off)
    raw = verts / scale - off
    scan = run["tmp"] / "scan"
    scan.mkdir()
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    (scan / "mesh.obj").write_text("".join("v %.17g %.17g %.17g\n" % tuple(p) for p in raw) + "".join("f %d %d %d %d\n" % tuple(i + 1 for i in q) for q in quads))
    json.dump({"junctions": raw.tolist(), "lines": edges.tolist()}, open(scan / "lines.json", "w"))
    (scan / "offset_scale.txt").write_text("%r %r %r %r\n" % (float(off[0]), float(off[1]), float(off[2]), scale))
    # detections: the projected corners half a pixel off, the twelve edges; a view's first corner moved far away
    hawp = os.path.join(run["data_root"], "abc", "toy", "hawp")
    Ks, w2cs = run["intrinsics"], np.linalg.inv(run["poses"])
    for v in range(3):
        p = _project(Ks[v][:3, :3], w2cs[v], verts) + 0.5
        p[v] += 40.0
        json.dump({"vertices": p.tolist(), "vertices-score": [0.9] * 8, "edges": edges.tolist(), "edges-weights": [0.99] * 12, "height": 64, "width": 64},
                  open(os.path.join(hawp, "image_%04d.json" % v), "w"))
    assert raycast.main(["analysis", "--conf", run["conf"], "--scan", str(scan), "--data_root", run["data_root"], "--json"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    report = json.loads(out[-1])
    six = [float(x) for x in out[-7:-1]]
    with np.load(scan / "wireframe_visibility.npz") as z:
        assert sorted(z.files) == ["junction_rate", "junctions_hit", "junctions_seen", "line_rate", "lines_hit", "lines_seen"]
        res = {k: z[k] for k in z.files}
    assert res["junctions_seen"].shape == (3, 8) and res["junctions_seen"].dtype == bool and res["lines_seen"].shape == (3, 12)
    assert res["junctions_hit"].dtype == np.int32 and res["lines_hit"].dtype == np.int32 and res["lines_hit"].shape == (12,)
    # the float64 restatement: the rule by brute force on the same rays, scipy's assignment
    dev = torch.device("cuda:0")
    inv_scale, J32, E = raycast.scan_wireframe(str(scan))
    assert np.abs(J32 - verts).max() < 1e-6 and np.array_equal(E, edges)
    mverts = (inv_scale[:3, :3] @ raw.T + inv_scale[:3, 3:]).T
    mfaces = np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    J = J32.astype(np.float64)
    lines = J[edges]
    j_hit, l_hit, j_rate, l_rate = np.zeros(8, int), np.zeros(12, int), 0.0, 0.0
    centres = run["poses"][:, :3, 3]
    robust = 0

    def seen(p2d, X, v, tol):
        uv = torch.from_numpy(p2d.astype(np.float32)).to(dev)
        dirs, _, origins = ops.camera_rays(uv[None], torch.from_numpy(run["poses"][v]).float().to(dev)[None],
                                           torch.from_numpy(Ks[v]).float().to(dev)[None], with_origins=True)
        o, d = origins.cpu().numpy(), dirs[0].cpu().numpy()
        t, _, _ = RC.cast_all(mverts, mfaces, o, d)
        with np.errstate(invalid="ignore"):
            return np.linalg.norm(o.astype(np.float64) + d.astype(np.float64) * t[:, None] - X, axis=1) < tol

    for v in range(3):
        K, w2c = Ks[v][:3, :3], w2cs[v]
        j2d = _project(K, w2c, J)
        valid = raycast.inside(j2d, 64, 64) & seen(j2d, J, v, 1e-4)
        assert np.array_equal(res["junctions_seen"][v], valid), v
        # a corner whose three faces all face the camera is seen, the opposite corner is hidden behind the box (a corner with a face
        # seen edge-on lies on the silhouette: the ray through it grazes the box, and only the equality above holds for it)
        c = centres[v]
        front = [k for k in range(8) if all(c[a] * J[k, a] > 0 and abs(c[a]) > abs(J[k, a]) + 0.05 for a in range(3))]
        robust += len(front)
        for k in front:
            assert valid[k] and not valid[7 - k], (v, k)
        det = json.load(open(os.path.join(hawp, "image_%04d.json" % v)))
        pred = np.asarray(det["vertices"], np.float32).astype(np.float64)
        cost = np.linalg.norm(pred[:, None] - j2d[None], axis=-1)
        r, c = linear_sum_assignment(cost)
        hit = (cost[r, c] < 20) & valid[c]
        j_hit[c[hit]] += 1
        j_rate += hit.sum() / max(valid.sum(), 1)
        l2d = _project(K, w2c, lines.reshape(-1, 3)).reshape(-1, 4)
        is_in = raycast.inside(l2d[:, :2], 64, 64) & raycast.inside(l2d[:, 2:], 64, 64) & seen(l2d[:, :2], lines[:, 0], v, 0.1) & seen(l2d[:, 2:], lines[:, 1], v, 0.1)
        assert np.array_equal(res["lines_seen"][v], is_in), v
        seg = np.concatenate([pred[edges[:, 0]], pred[edges[:, 1]]], 1)
        d1 = np.linalg.norm(seg[:, None, :2] - l2d[None, :, :2], axis=-1) + np.linalg.norm(seg[:, None, 2:] - l2d[None, :, 2:], axis=-1)
        d2 = np.linalg.norm(seg[:, None, :2] - l2d[None, :, 2:], axis=-1) + np.linalg.norm(seg[:, None, 2:] - l2d[None, :, :2], axis=-1)
        cost = np.minimum(d1, d2) * 0.5
        r, c = linear_sum_assignment(cost)
        hit = (cost[r, c] < 20) & is_in[c]
        l_hit[c[hit]] += 1
        l_rate += hit.sum() / max(is_in.sum(), 1)
    assert robust >= 1                                                           # some view looks at a corner of the box
    assert 0 < res["junctions_seen"].sum() < 24 and 0 < res["lines_seen"].sum() < 36
    assert np.array_equal(res["junctions_hit"], j_hit) and np.array_equal(res["lines_hit"], l_hit)
    assert abs(float(res["junction_rate"]) - j_rate / 3) < 1e-12 and abs(float(res["line_rate"]) - l_rate / 3) < 1e-12
    assert 0 < j_rate / 3 <= 1 and 0 < l_rate / 3 <= 1
    expect = [8, 12, int((j_hit > 0).sum()), j_rate / 3, l_rate / 3, 12]
    assert np.allclose(six, expect, rtol=0, atol=1e-12)
    assert report["junctions"] == 8 and report["lines"] == 12 and report["junctions_hit"] == expect[2] and report["views"] == 3
    assert report["lines_hit"] == int((l_hit > 0).sum()) and report["lines_kept"] == 12
