"""Generate tests/golden/g20_evaluation.npz by running the REFERENCE's four evaluation scripts themselves (authoring container only).

    python tests/golden/make_eval_golden.py        # needs /root/reference, sklearn, tqdm ; writes tests/golden/g20_evaluation.npz

code/evaluation/eval-dtu.py, eval-lsr-dtu.py, eval-wfr-dtu.py and eval-abc.py run under runpy on the CPU with sys.modules stubs: an
`open3d` whose read_triangle_mesh / read_point_cloud hand back the synthetic arrays below and whose write_point_cloud records what it is
given (data_down and the error colours come out that way), empty GPUtil and trimesh, and pdb.set_trace as a no-op.  After sklearn and
scipy are imported numpy.random.default_rng is replaced by an object whose shuffle applies a recorded permutation.  The .mat files are
written with scipy.io.savemat.  The scene: a jittered, once-subdivided octahedron of radius 5 mm (32 generic triangles) plus a zero-area
triangle and a right isosceles triangle whose lattice spacing equals the thinning radius; 12 000 noisy ground-truth points (float32
values); an ObsMask with an unobserved slab and a box the cloud leaves on every side; a ground plane that cuts the cloud; a dozen lines
and their junctions; an offset_scale.txt.  Only DATA is written: inputs, permutations, thinned clouds, the printed numbers.
"""
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/code/evaluation"
sys.path.insert(0, REPO)

import scipy.io  # noqa: E402
import scipy.optimize  # noqa: E402,F401
import sklearn.neighbors  # noqa: E402,F401

SCAN, PATCH, RES = 7, 0.5, 0.25


def scene(seed=0):
    rng = np.random.default_rng(seed)
    v = [np.array(p, dtype=np.float64) for p in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    mid, out = {}, []
    for a, b, c in faces:
        m = []
        for i, j in ((a, b), (b, c), (c, a)):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            m.append(mid[key])
        out += [(a, m[0], m[2]), (m[0], b, m[1]), (m[2], m[1], c), (m[0], m[1], m[2])]
    verts = np.array(v) * 5.0 + rng.normal(0, 0.35, (len(v), 3))
    extra = np.array([[-2.0, -2.0, 5.3], [2.0, -2.0, 5.3], [-2.0, 2.0, 5.3],          # right isosceles, legs 4: lattice spacing 0.2
                      [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]])               # collinear: zero area
    n0 = len(verts)
    verts = np.concatenate([verts, extra])
    out += [(n0, n0 + 1, n0 + 2), (n0 + 3, n0 + 4, n0 + 5)]
    faces = np.array(out, dtype=np.int32)
    d = rng.normal(size=(12000, 3))
    stl = d / np.linalg.norm(d, axis=1, keepdims=True) * 5.0 + rng.normal(0, 0.2, (12000, 3))
    stl = stl.astype(np.float32)
    bb = np.array([[-4.0, -4.0, -4.0], [3.0, 3.0, 3.0]])
    obs = np.ones((30, 30, 30), dtype=np.uint8)
    obs[:, 10:13, :] = 0
    plane = np.array([[0.02, 0.01, 1.0, 1.5]])
    scale_mat = np.array([[5.0, 0, 0, 0.3], [0, 5.0, 0, -0.2], [0, 0, 5.0, 0.1], [0, 0, 0, 1.0]])
    unit = (verts[:n0] - scale_mat[:3, 3]) / 5.0
    edges = sorted({(min(a, b), max(a, b)) for f in out[:32] for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))})
    pick = rng.choice(len(edges), 12, replace=False)
    lines = np.array([[unit[edges[k][0]], unit[edges[k][1]]] for k in pick]) + rng.normal(0, 0.01, (12, 2, 3))
    lines[3:, 0] = lines[:9, 1]                                                      # shared end points: `unique` has something to merge
    lines = lines.astype(np.float32)
    scores = rng.uniform(0, 1, 12)
    return dict(verts=verts, faces=faces, stl=stl, bb=bb, obs=obs, plane=plane, scale_mat=scale_mat, lines=lines, scores=scores)


class Shuffler:
    perms = []

    def shuffle(self, x, axis=0):
        perm = np.random.Generator(np.random.PCG64(len(Shuffler.perms) + 11)).permutation(len(x))
        Shuffler.perms.append(perm)
        x[:] = x[perm]


def install_stubs(arrays, written):
    o3d = types.ModuleType("open3d")
    o3d.io, o3d.geometry, o3d.utility = types.SimpleNamespace(), types.SimpleNamespace(), types.SimpleNamespace()
    o3d.io.read_triangle_mesh = lambda path: types.SimpleNamespace(vertices=arrays[path][0].copy(), triangles=arrays[path][1].copy())
    o3d.io.read_point_cloud = lambda path: types.SimpleNamespace(points=arrays[path].copy())
    o3d.io.write_point_cloud = lambda path, pcd: written.__setitem__(os.path.basename(path), (np.array(pcd.points), np.array(pcd.colors)))
    o3d.geometry.PointCloud = lambda *a: types.SimpleNamespace(points=a[0] if a else None, colors=None)
    o3d.utility.Vector3dVector = lambda x: np.asarray(x)
    sys.modules["open3d"] = o3d
    for name in ("GPUtil", "trimesh"):
        sys.modules[name] = types.ModuleType(name)
    import pdb
    pdb.set_trace = lambda *a, **k: None
    np.random.default_rng = lambda *a, **k: Shuffler()


def run(script, argv):
    old = sys.argv
    sys.argv = [script] + [str(a) for a in argv]
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            runpy.run_path(os.path.join(REF, script), run_name="__main__")
    finally:
        sys.argv = old
    return buf.getvalue()


def main():
    sc = scene()
    real_rng = np.random.default_rng
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "ObsMask"))
    scipy.io.savemat(os.path.join(tmp, "ObsMask", "ObsMask%d_10.mat" % SCAN), {"ObsMask": sc["obs"], "BB": sc["bb"], "Res": np.array([[RES]])})
    scipy.io.savemat(os.path.join(tmp, "ObsMask", "Plane%d.mat" % SCAN), {"P": sc["plane"]})
    stl_path = "%s/Points/stl/stl%03d_total.ply" % (tmp, SCAN)
    mesh_path = os.path.join(tmp, "surface_100.ply")
    arrays = {stl_path: sc["stl"].astype(np.float64), mesh_path: (sc["verts"], sc["faces"])}
    written = {}
    install_stubs(arrays, written)
    common = ["--scan", SCAN, "--dataset_dir", tmp, "--patch_size", PATCH]
    out = {k: sc[k] for k in ("verts", "faces", "stl", "bb", "obs", "plane", "scale_mat", "lines", "scores")}
    out.update(scan=np.array(SCAN), patch=np.array(PATCH), res=np.array(RES))

    # eval-dtu.py, mesh and pcd mode
    run("eval-dtu.py", ["--data", mesh_path, "--mode", "mesh", "--vis_out_dir", tmp] + common)
    out["mesh_numbers"] = np.array([float(x) for x in open(mesh_path[:-4] + ".txt").read().split("\t")])
    out["mesh_perm"] = Shuffler.perms[-1].astype(np.int32)
    out["mesh_data_down"] = written["vis_%03d_d2s.ply" % SCAN][0]
    out["mesh_colors_d2s"] = (written["vis_%03d_d2s.ply" % SCAN][1] * 255).round().astype(np.uint8)
    out["mesh_colors_s2d"] = (written["vis_%03d_s2d.ply" % SCAN][1] * 255).round().astype(np.uint8)
    pcd_path = os.path.join(tmp, "cloud.ply")
    cloud = sc["verts"][:18] + 0.0
    cloud = np.concatenate([cloud, real_rng(5).normal(0, 1, (3000, 3)) * [3.0, 3.0, 0.05] + [0, 0, 4.6]])
    arrays[pcd_path] = cloud
    out["pcd_cloud"] = cloud
    run("eval-dtu.py", ["--data", pcd_path, "--mode", "pcd", "--vis_out_dir", tmp] + common)
    out["pcd_numbers"] = np.array([float(x) for x in open(pcd_path[:-4] + ".txt").read().split("\t")])
    out["pcd_perm"] = Shuffler.perms[-1].astype(np.int32)
    out["pcd_data_down"] = written["vis_%03d_d2s.ply" % SCAN][0]

    # eval-lsr-dtu.py (with and without --score) and eval-wfr-dtu.py (.pth and .npz)
    cam = os.path.join(tmp, "cameras.npz")
    np.savez(cam, scale_mat_0=sc["scale_mat"])
    npz = os.path.join(tmp, "x-wfi_checked.npz")
    np.savez(npz, lines3d=sc["lines"], scores=sc["scores"])
    for tag, extra in (("lines", []), ("lines_score", ["--score", 0.6])):
        text = run("eval-lsr-dtu.py", ["--data", npz, "--cam", cam] + extra + common).split("\n")
        out[tag + "_numbers"] = np.array([float(x) for x in text[4:8]])
        out[tag + "_perm"] = Shuffler.perms[-1].astype(np.int32)
    pth = os.path.join(tmp, "x-neat.pth")
    junc_pred = torch.tensor(np.unique(sc["lines"].reshape(-1, 3), axis=0)[::-1].copy()) + 0.004
    torch.save({"lines3d_wfi_checked": torch.tensor(sc["lines"]), "junctions3d_initial": junc_pred}, pth)
    for tag, path in (("junc_pth", pth), ("junc_npz", npz)):
        text = run("eval-wfr-dtu.py", ["--data", path, "--cam", cam] + common)
        acc, comp = text.split("ACC = ")[1].split()[0], text.split("COMP = ")[1].split()[0]
        out[tag + "_numbers"] = np.array([float(acc), float(comp), float(text.split("num junctions: ")[1].split()[0])])
        out[tag + "_perm"] = Shuffler.perms[-1].astype(np.int32)

    # eval-abc.py
    scan_dir = os.path.join(tmp, "abc")
    os.makedirs(scan_dir)
    offset_scale = [0.11, -0.07, 0.05, 1.9]
    s = 1.0 / offset_scale[-1]
    gt_j = np.unique(sc["lines"].reshape(-1, 3).astype(np.float64), axis=0) * s - offset_scale[:3]
    gt_j = gt_j + real_rng(9).normal(0, 0.008, gt_j.shape)
    gt_j = np.concatenate([gt_j, [[0.9, 0.9, 0.9]]])
    scaled = sc["lines"].astype(np.float64) * s - offset_scale[:3]
    edges = []
    for l in scaled[:10]:
        a = int(np.argmin(np.linalg.norm(gt_j - l[0], axis=1)))
        b = int(np.argmin(np.linalg.norm(gt_j - l[1], axis=1)))
        edges.append([b, a])
    edges.append([0, len(gt_j) - 1])
    with open(os.path.join(scan_dir, "lines.json"), "w") as f:
        json.dump({"junctions": gt_j.tolist(), "lines": edges}, f)
    with open(os.path.join(scan_dir, "offset_scale.txt"), "w") as f:
        f.write(" ".join(str(v) for v in offset_scale))
    text = run("eval-abc.py", ["--data", pth, "--scan", scan_dir]).strip().split("\n")
    out["abc_lines"] = np.array(text[-2:])
    out["abc_junctions_pred"] = junc_pred.numpy()
    out["abc_junctions_gt"] = gt_j
    out["abc_edges_gt"] = np.array(edges, dtype=np.int32)
    out["abc_offset_scale"] = np.array(offset_scale)

    np.random.default_rng = real_rng
    path = os.path.join(HERE, "g20_evaluation.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
    for k in ("mesh_numbers", "pcd_numbers", "lines_numbers", "lines_score_numbers", "junc_pth_numbers", "junc_npz_numbers", "abc_lines"):
        print(k, out[k])
    print("mesh: thinned %d of %d" % (len(out["mesh_data_down"]), len(out["mesh_perm"])))


if __name__ == "__main__":
    main()
