"""The ray-casting rule and the model of the tree (tests/raycast_f64.py), the OBJ reader and the host side of the neat_raycast_* entry
points: everything that needs no GPU."""
import ctypes
import math

import numpy as np
import pytest

from tests import raycast_f64 as RC

RAYCAST_SYMBOLS = ("neat_raycast_bvh_bytes", "neat_raycast_ws_bytes", "neat_raycast_build", "neat_raycast_cast")
SCENES = {"ico0": lambda: RC.icosphere(0), "ico2": lambda: RC.icosphere(2), "strips": lambda: RC.strips()}
CENTRE = {"ico0": (0.0, 0.0, 0.0), "ico2": (0.0, 0.0, 0.0), "strips": (0.5, 0.5, 0.5)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_tree_equals_brute_force(name):
    verts, faces = SCENES[name]()
    o, d = RC.fan(11, 1025, centre=CENTRE[name])
    t, tri, uv = RC.cast_all(verts, faces, o, d)
    tree = RC.Tree(verts, faces)
    mt, mtri, muv, counts = tree.cast(o, d)
    hits = int((tri >= 0).sum())
    assert 100 < hits < 1025 - 100                                   # hits and misses mixed
    assert RC.judge(verts, faces, o, d).sum() == 0                   # random rays meet no tie (the 1 % cap of the GPU tests)
    assert np.array_equal(mtri, tri) and np.array_equal(mt, t) and np.array_equal(muv, uv)
    assert np.isinf(t[tri < 0]).all() and (t[tri >= 0] > 0).all()
    # the tree culls, and every ray costs at least the root
    assert counts[:, 0].min() >= 1 and counts[:, 1].mean() < max(faces.shape[0] / 4, 3)
    # any hit: blocked exactly where the closest hit lies before t_max
    rng = np.random.default_rng(5)
    t_max = rng.uniform(1.0, 5.0, 1025).astype(np.float32)
    at, _, _, _ = tree.cast(o[:257], d[:257], t_max=t_max[:257], any_hit=True)
    assert np.array_equal(np.isfinite(at), t[:257] < t_max[:257].astype(np.float64))


def test_tie_goes_to_the_lowest_face_and_limits_are_half_open():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    faces = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 2]], np.int32)                # three coincident triangles, both windings
    o, d = np.array([[0.25, 0.25, 1.0]], np.float32), np.array([[0, 0, -1.0]], np.float32)
    for f in (faces, faces[::-1]):
        t, tri, uv = RC.cast_all(verts, f, o, d)
        mt, mtri, _, _ = RC.Tree(verts, f).cast(o, d)
        assert tri[0] == 0 and mtri[0] == 0 and t[0] == 1.0 and mt[0] == 1.0
    assert np.allclose(RC.cast_all(verts, faces, o, d)[2][0], (0.25, 0.25))
    one = np.float32(1.0)
    below, above = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))
    for t_min, t_max, hit in ((None, [one], False), (None, [above], True), ([one], None, True), ([above], None, False), ([below], [above], True)):
        assert (RC.cast_all(verts, faces, o, d, t_min, t_max)[1][0] >= 0) == hit
        assert (RC.Tree(verts, faces).cast(o, d, t_min, t_max)[1][0] >= 0) == hit
    # a ray in the plane of the triangle: det == 0, a miss
    o2, d2 = np.array([[-1.0, 0.25, 0.0]], np.float32), np.array([[1.0, 0, 0]], np.float32)
    assert RC.cast_all(verts, faces, o2, d2)[1][0] == -1 and RC.Tree(verts, faces).cast(o2, d2)[1][0] == -1


def test_degenerate_and_non_finite_triangles_are_never_hit():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [np.nan, 0, 0], [1, 1, 0]], np.float64)
    faces = np.array([[0, 3, 1], [1, 3, 1], [0, 4, 2], [1, 5, 2]], np.int32)     # a sliver of zero area, a repeated vertex, a NaN, a good one
    assert RC.valid_triangles(verts, faces).tolist() == [True, False, False, True]
    faces[0] = (1, 3, 2)                                                         # collinear: zero area
    assert RC.valid_triangles(verts, faces).tolist() == [False, False, False, True]
    o, d = np.array([[0.75, 0.75, 1.0], [0.25, 0.25, 1.0]], np.float32), np.array([[0, 0, -1.0]] * 2, np.float32)
    t, tri, _ = RC.cast_all(verts, faces, o, d)
    mt, mtri, _, _ = RC.Tree(verts, faces).cast(o, d)
    assert tri.tolist() == [3, -1] and mtri.tolist() == [3, -1] and t[0] == 1.0 and mt[0] == 1.0


@pytest.mark.parametrize("level", [0, 2])
def test_icosphere_hits_lie_within_the_sagitta_of_the_unit_sphere(level):
    verts, faces = RC.icosphere(level)
    assert faces.shape[0] == 20 * 4 ** level and np.allclose(np.linalg.norm(verts, axis=1), 1.0, atol=1e-15)
    tv = verts[faces]
    # a planar triangle with corners on the unit sphere lies between its plane's distance from the centre and 1: the sagitta of the
    # chord through its circumcircle, 1 - sqrt(1 - a^2) for the circumradius a
    n = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    plane = np.abs((n * tv[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)
    a = np.sqrt(1.0 - plane ** 2)
    sagitta = float((1.0 - np.sqrt(1.0 - a ** 2)).max())
    # the icosahedron's inscribed sphere has radius 0.79465: a sagitta of 0.20535; halving the chords quarters it, and the middle
    # triangles of a subdivided face come out up to a fifth longer than the corner ones (1.2^2 / 16 of the level below twice over)
    assert sagitta < (0.2054 if level == 0 else 0.2054 / 16 * 1.5)
    o, d = RC.fan(3, 1025)
    t, tri, uv = RC.cast_all(verts, faces, o, d)
    hit = tri >= 0
    p = o[hit].astype(np.float64) + t[hit, None] * d[hit].astype(np.float64)
    r = np.linalg.norm(p, axis=1)
    assert hit.sum() > 100 and r.min() >= 1.0 - sagitta - 1e-12 and r.max() <= 1.0 + 1e-12
    # the analytic sphere: a ray that misses the unit sphere misses the mesh inside it, and a hit lies on the chord of the sphere
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    b = (o64 * d64).sum(1) / (d64 * d64).sum(1)
    disc = b * b - ((o64 * o64).sum(1) - 1.0) / (d64 * d64).sum(1)
    assert not hit[disc < 0].any()
    t_in = -b[hit] - np.sqrt(disc[hit])
    assert (t[hit] >= t_in - 1e-12).all() and (t[hit] <= -b[hit] + np.sqrt(disc[hit]) + 1e-12).all()
    # the barycentrics give the same point
    q = (1 - uv[hit, :1] - uv[hit, 1:]) * tv[tri[hit], 0] + uv[hit, :1] * tv[tri[hit], 1] + uv[hit, 1:] * tv[tri[hit], 2]
    assert np.abs(q - p).max() < 1e-12


def test_read_obj_index_forms_negative_indices_and_polygons(tmp_path):
    from neat_amd import ply
    path = tmp_path / "m.obj"
    path.write_text("\n".join([
        "# a comment", "mtllib x.mtl", "o thing", "v 0 0 0", "v 1 0 0 1.0", "v 1 1 0", "v 0 1 0", "vt 0 0", "vn 0 0 1", "",
        "f 1 2 3", "f 1/1 3/1 4/1", "f 1//1 2//1 3//1", "f 1/1/1 2/1/1 4/1/1", "g other", "s off", "usemtl m",
        "v 0.5 0.5 1.5e0", "f -1 -5 -4", "f 1 2 3 4", "v 2 2 2", "f 1 2 3 4 -1", "l 1 2", ""]))
    verts, faces = ply.read_obj(str(path))
    assert verts.dtype == np.float64 and faces.dtype == np.int32
    assert np.array_equal(verts, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.5], [2, 2, 2]])
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3], [4, 0, 1],                    # the four index forms, negative indices
                              [0, 1, 2], [0, 2, 3],                                                     # a quad: the fan about its first corner
                              [0, 1, 2], [0, 2, 3], [0, 3, 5]]                                          # a pentagon, its last corner negative
    empty = tmp_path / "e.obj"
    empty.write_text("# nothing\n")
    v, f = ply.read_obj(str(empty))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    bad = tmp_path / "b.obj"
    bad.write_text("v 0 0 0\nf 0 1 1\n")
    with pytest.raises(ValueError):
        ply.read_obj(str(bad))


def test_library_exports_the_entries_and_rejects_bad_arguments_before_any_launch():
    from neat_amd import _lib
    lib = _lib.lib()
    assert lib.neat_abi_version() == 15
    for name in RAYCAST_SYMBOLS:
        getattr(lib, name)
        assert name in _lib.exported_symbols() and not hasattr(lib, "f16_" + name)
    for size in (lib.neat_raycast_bvh_bytes, lib.neat_raycast_ws_bytes):
        assert size(-1) == 0 and size(-2 ** 31) == 0 and size(2 ** 24 + 1) == 0
        last = size(0)
        for nf in (1, 2, 3, 63, 64, 65, 255, 256, 257, 320, 1025, 5120, 327680, 2 ** 24):
            assert size(nf) >= last and size(nf) % 256 == 0, nf
            last = size(nf)
    assert lib.neat_raycast_bvh_bytes(0) > 0                                      # the empty tree
    for nf in (1, 5, 1025, 327680):
        L = 1 << max(nf - 1, 0).bit_length()
        # the status word, 2 L float32 boxes, 80 bytes a triangle; the workspace: two keys, two values, the sort's room
        assert lib.neat_raycast_bvh_bytes(nf) >= 4 + 2 * L * 24 + 80 * nf and lib.neat_raycast_ws_bytes(nf) >= 2 * 8 * nf + 2 * 4 * nf + 12 * nf
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    build, cast = lib.neat_raycast_build, lib.neat_raycast_cast
    assert build(None, 0, None, 0, None, None, None) == -1                       # no tree buffer
    assert build(None, 0, None, 0, a + 4, None, None) == -1                      # misaligned
    assert build(a, -1, a, 1, a, a, None) == -1 and build(a, 3, a, -1, a, a, None) == -1 and build(a, 3, a, 2 ** 24 + 1, a, a, None) == -1
    assert build(a, 3, None, 1, a, a, None) == -1 and build(None, 3, a, 1, a, a, None) == -1 and build(a, 3, a, 1, a, None, None) == -1
    assert build(a, 3, a, 1, a, a + 8, None) == -1
    assert cast(None, 0, a, a, None, None, 4, 0, a, a, a, None, None) == -1
    assert cast(a, -1, a, a, None, None, 4, 0, a, a, a, None, None) == -1 and cast(a, 1, a, a, None, None, -4, 0, a, a, a, None, None) == -1
    assert cast(a, 1, a, a, None, None, 4, 2, a, a, a, None, None) == -1
    for k in (2, 3, 8, 9, 10):                                                    # origins, dirs, t, tri, uv
        args = [a, 1, a, a, None, None, 4, 0, a, a, a, None, None]
        args[k] = None
        assert cast(*args) == -1
    assert cast(a, 1, None, None, None, None, 0, 0, None, None, None, None, None) == 0          # no rays: nothing to do


def test_cli_flags_and_defaults(capsys):
    from neat_amd import raycast
    opt = raycast.parse_args(["check", "--mesh", "m.ply", "--data", "x-wfi.npz", "--cams", "cameras.npz"])
    assert (opt.min_views, opt.min_frac, opt.bias, opt.samples, opt.overwrite, opt.json, opt.conf) == (5, 0.5, 0.01, 16, False, False, None)
    assert raycast.out_path("a/b/latest-abcdefgh-wfi.npz") == "a/b/latest-abcdefgh-wfi_occlmesh.npz"
    opt = raycast.parse_args(["analysis", "--conf", "c.conf", "--scan", "s"])
    assert opt.data_root == "../data" and not opt.json
    base = ["check", "--mesh", "m.obj", "--data", "x.npz"]
    for bad in (base, base + ["--cams", "c.npz", "--conf", "r.conf"], base + ["--cams", "c.npz", "--samples", "1"],
                base + ["--cams", "c.npz", "--min-frac", "1.5"], base + ["--cams", "c.npz", "--bias", "-1"],
                ["check", "--mesh", "m.stl", "--data", "x.npz", "--cams", "c.npz"], ["analysis", "--conf", "c.conf"], []):
        with pytest.raises(SystemExit):
            raycast.parse_args(bad)
        assert "usage:" in capsys.readouterr().err                                # ap.error, not a traceback


def test_keep_rule_and_writer_are_shared_with_trace(tmp_path):
    from neat_amd import raycast, run_io, trace
    assert trace.keep_rule is run_io.keep_rule and trace.write_occl is run_io.write_occl
    frac = np.array([[1.0, 0.4, 0.5], [0.5, 0.6, 0.0]])
    views, kept = run_io.keep_rule(frac, 2, 0.5)
    assert views.dtype == np.int32 and views.tolist() == [2, 1, 1] and kept.tolist() == [True, False, False]
    lines = np.arange(18.0).reshape(3, 2, 3)
    path = raycast.out_path(str(tmp_path / "w.npz"))
    run_io.write_occl(path, lines, views, kept)
    with np.load(path) as z:
        assert sorted(z.files) == ["kept", "lines3d", "views"] and np.array_equal(z["lines3d"], lines[:1])
    assert np.array_equal(run_io.load_lines(path)[0], lines[:1])


def test_project2d_is_the_guarded_division():
    from neat_amd import raycast
    K = np.array([[70.0, 0, 32], [0, 70, 32], [0, 0, 1]])
    X = np.array([[0.1, -0.2, 2.0], [0.3, 0.1, 0.0], [0.0, 0.0, -1e-9], [0.2, 0.2, -3.0]])
    p = raycast.project2d(K, np.eye(3), np.zeros(3), X)
    x = (K @ X.T).T
    den = np.array([2.0, 1e-8, -1e-9 - 1e-8, -3.0])
    assert np.allclose(p, x[:, :2] / den[:, None], rtol=1e-15, atol=0) and np.isfinite(p).all()
    assert raycast.inside(np.array([[0.0, 0.0], [64.0, 1.0], [63.99, 63.99], [-0.01, 5.0]]), 64, 64).tolist() == [True, False, True, False]
    assert math.isclose(p[0, 0], 70 * 0.05 + 32)
