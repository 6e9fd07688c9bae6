"""CPU: the evaluation-mesh definitions (csrc/kernels_evalmesh.hpp) through their float64 restatement
(tests/evalmesh_f64.py): the moments' closed form against a quadrature that is exact for quadratics, the principal frame of a rotated
cuboid, mesh.aligned_grid against the literal numpy.linspace / numpy.arange of get_grid, the welded cut against topology and an
independent per-triangle polygon clip, the constants the GPU tests size their cases by, and the argument checks of the C entry points
(no device work)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import evalmesh_f64 as E
from tests import mesh_f64 as M
from tests.test_mesh_math import sample, sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_moments_formula_is_the_edge_midpoint_quadrature():
    """A / 3 sum_i f(m_i) over the edge midpoints is exact for polynomials of degree 2, so it gives the integrals of 1, x, x x^T."""
    rng = np.random.default_rng(0)
    a, b, c = rng.normal(size=(3, 500, 3))
    area, first, second = E.triangle_moments(a, b, c)
    mids = [(a + b) / 2, (b + c) / 2, (c + a) / 2]
    q_first = (area / 3)[:, None] * sum(mids)
    q_second = (area / 3)[:, None, None] * sum(m[:, :, None] * m[:, None, :] for m in mids)
    assert np.abs(first - q_first).max() <= 1e-12 * np.abs(q_first).max()
    assert np.abs(second - q_second).max() <= 1e-12 * np.abs(q_second).max()
    # and the summed form, with the upper-triangle order of the kernel's output
    verts = np.concatenate([a, b, c])
    faces = np.arange(1500).reshape(3, 500).T
    got = E.moments(verts, faces, [0.1, -0.2, 0.3])
    o = np.array([0.1, -0.2, 0.3])
    _, f1, f2 = E.triangle_moments(a - o, b - o, c - o)
    want = np.concatenate([[area.sum()], f1.sum(0), f2.sum(0)[np.triu_indices(3)]])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def cuboid(ext, n):
    """The surface of [-ext/2, ext/2] tessellated with n x n quads per face -> (verts, faces), outward normals."""
    verts, faces = [], []
    u = np.linspace(-0.5, 0.5, n + 1)
    for axis in range(3):
        for side in (-0.5, 0.5):
            a, b = [(axis + 1) % 3, (axis + 2) % 3] if side > 0 else [(axis + 2) % 3, (axis + 1) % 3]
            base = sum(len(v) for v in verts)
            p = np.zeros((n + 1, n + 1, 3))
            p[..., axis] = side
            p[..., a], p[..., b] = u[:, None], u[None, :]
            verts.append(p.reshape(-1, 3) * ext)
            i, j = [g.reshape(-1) for g in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
            v00, v10, v01, v11 = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j, base + i * (n + 1) + j + 1, base + (i + 1) * (n + 1) + j + 1
            faces += [np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]
    return np.concatenate(verts), np.concatenate(faces)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_frame_of_a_rotated_cuboid(seed):
    from neat_amd import mesh
    ext = np.array([1.0, 2.0, 3.0])
    v, f = cuboid(ext, 6)
    assert (np.einsum("ij,ij->i", M.face_normals(v, f), v[f].mean(axis=1)) > 0).all()
    Q, shift = rotation(seed), np.array([0.3, -0.2, 0.1])
    w = v @ Q.T + shift                                         # the cuboid's axes are the columns of Q
    for R, mean in (E.principal_frame(w, f), mesh.frame_from_moments(E.moments(w, f, shift + 0.01), shift + 0.01)):
        assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
        assert np.abs(mean - shift).max() <= 1e-12
        for r in range(3):
            assert R[r, np.argmax(np.abs(R[r]))] > 0                # the sign rule
        # the surface of a 1 x 2 x 3 cuboid spreads least along its short edge: ascending eigenvalue = ascending edge length, so the
        # frame is the known rotation's axes with the sign rule, and rows 1 and 2 swapped where that makes det = +1
        want = Q.T.copy()
        for r in range(3):
            want[r] *= np.sign(want[r, np.argmax(np.abs(want[r]))])
        if np.linalg.det(want) < 0:
            want = want[[0, 2, 1]]
        assert np.abs(R - want).max() <= 1e-12


BOXES = {0: ([-0.31, -0.62, -0.93], [0.29, 0.58, 0.87]), 1: ([-0.8, -0.2, -0.5], [0.7, 0.25, 0.6]), 2: ([-0.5, -0.9, 0.1], [0.55, 0.9, 0.45])}


@pytest.mark.parametrize("eps", [0.0, 0.01, 0.1])
@pytest.mark.parametrize("short", [0, 1, 2])
@pytest.mark.parametrize("resolution", [17, 100])
def test_aligned_grid_is_get_grid(short, eps, resolution):
    from neat_amd import mesh
    lo, hi = BOXES[short]
    shape, lo3, hi3 = mesh.aligned_grid(lo, hi, resolution, eps)
    axes = E.aligned_axes_literal(lo, hi, resolution, eps)
    assert shape == tuple(len(a) for a in axes) and shape[short] == resolution
    for a in range(3):
        ours = mesh.linspace_f32(lo3[a], hi3[a], shape[a])
        theirs = axes[a].astype(np.float32)
        # one float32 ulp of the node.  Where cancellation leaves a node next to zero its own ulp is tiny and what is left is the float64
        # error of numpy.arange itself: it fills start + i * ((start + step) - start), and that difference carries the rounding of
        # start + step, up to 2^-53 |start|, i times over -- under n 2^-52 of the axis's largest magnitude, far below a float32 ulp there
        ulp = np.spacing(np.maximum(np.abs(ours), np.abs(theirs))).astype(np.float64)
        bar = np.maximum(ulp, shape[a] * 2.0 ** -52 * np.abs(axes[a]).max())
        assert (np.abs(ours.astype(np.float64) - theirs.astype(np.float64)) <= bar).all(), a


def test_aligned_grid_when_the_quotient_lands_on_an_integer():
    """Extents that make (stop - start) / h land within 1e-12 of an integer: the node count is numpy.arange's, whichever side it falls."""
    from neat_amd import mesh
    met = 0
    for k in range(1, 40):
        for eps in (0.0, 0.01, 0.1):
            lo = np.array([0.0, -0.3, 0.1])
            h = (1.0 + 2 * eps) / 16                               # the short axis: [0, 1] with 17 nodes
            hi = np.array([1.0, -0.3 + (16 + k) * h - 2 * eps, 0.1 + (20 + k) * h - 2 * eps])      # (hi + h + eps) - (lo - eps) = (17 + k) h
            shape, lo3, hi3 = mesh.aligned_grid(lo, hi, 17, eps)
            axes = E.aligned_axes_literal(lo, hi, 17, eps)
            assert shape == tuple(len(a) for a in axes), (k, eps)
            for a in (1, 2):
                q = ((hi[a] + h + eps) - (lo[a] - eps)) / h
                met += abs(q - round(q)) <= 1e-12
    assert met >= 100


def test_aligned_grid_refuses_2_to_31_nodes_and_names_the_resolution_that_fits():
    from neat_amd import mesh
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.05, 1.1]
    with pytest.raises(ValueError) as err:
        mesh.aligned_grid(lo, hi, 2048, 0.1)
    fit = int(re.search(r"fits this box is (\d+)", str(err.value)).group(1))
    assert np.prod(mesh.aligned_grid(lo, hi, fit, 0.1)[0], dtype=object) < 2 ** 31
    with pytest.raises(ValueError):
        mesh.aligned_grid(lo, hi, fit + 1, 0.1)
    with pytest.raises(ValueError):
        mesh.aligned_grid(lo, [1.0, -1.0, 1.0], 10, 0.0)


@pytest.fixture(scope="module")
def sphere_mesh():
    v, f = M.extract(sample(sphere([0.013, -0.007, 0.021], 0.5), (25, 25, 25)), -1.5, 1.5)
    return v.astype(np.float32).astype(np.float64), f


@pytest.mark.parametrize("axis,value,sign", [(0, 0.1, 1), (2, -0.2, -1), (1, 0.125, 1)])      # 0.125 = a grid plane: vertices on the plane
def test_cut_by_one_plane(sphere_mesh, axis, value, sign):
    v, f = sphere_mesh
    cv, cf = E.cut_plane(v, f, axis, value, sign, round32=False)
    assert len(cf) > 0 and cf.min() == 0 and cf.max() == len(cv) - 1 and len(np.unique(cf)) == len(cv)
    assert M.euler(len(cv), cf) == 1                               # a disc
    plane = float(np.float32(value))
    ends = cv[E.open_edges(cf)]
    assert len(ends) > 0 and (ends[..., axis] == plane).all()      # open only along the cut
    assert (sign * (cv[:, axis] - plane) >= 0).all()
    want = E.polygon_clip_area(v, f, [(axis, value, sign)])
    assert abs(E.mesh_area(cv, cf) - want) <= 1e-12 * want
    # winding kept: normals still point away from the centre
    n = M.face_normals(cv, cf)
    big = np.linalg.norm(n, axis=1) > 1e-12
    assert (np.einsum("ij,ij->i", n, cv[cf].mean(axis=1) - [0.013, -0.007, 0.021])[big] > 0).all()
    # the float32 form differs only by the rounding of the cut vertices
    rv, rf = E.cut_plane(v, f, axis, value, sign)
    assert np.array_equal(rf, cf) and np.abs(rv - cv).max() <= 2.0 ** -24


def test_cut_by_a_box(sphere_mesh):
    v, f = sphere_mesh
    lo, hi = np.array([-0.3, -0.6, -0.1]), np.array([0.35, 0.2, 0.6])
    cv, cf = E.clip_box(v, f, lo, hi, round32=False)
    lo32, hi32 = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    assert len(cf) > 0 and (cv >= lo32).all() and (cv <= hi32).all()
    ends = cv[E.open_edges(cf)]                                    # [edges, 2, 3]
    on_plane = ((ends == lo32) | (ends == hi32)).all(axis=1).any(axis=1)      # both ends on one and the same box plane
    assert len(ends) > 0 and on_plane.all()
    planes = [(axis, (lo, hi)[side][axis], sign) for axis, side, sign in E.BOX_PLANES]
    want = E.polygon_clip_area(v, f, planes)
    assert abs(E.mesh_area(cv, cf) - want) <= 1e-12 * want
    # wholly inside: the same arrays; wholly outside: empty
    iv, i_f = E.clip_box(v, f, -1.0, 1.0)
    assert np.array_equal(iv, v) and np.array_equal(i_f, f)
    ov, of = E.clip_box(v, f, 0.8, 1.2)
    assert ov.shape == (0, 3) and of.shape == (0, 3)


def test_kernel_constants():
    text = open(os.path.join(ROOT, "neat_amd", "csrc", "kernels_evalmesh.hpp")).read()
    # tests/test_evalmesh_gpu.py sizes its edge cases by these
    assert int(re.search(r"EMESH_WG\s*=\s*(\d+)", text).group(1)) == 256
    assert int(re.search(r"MOMENTS_TILE\s*=\s*(\d+)", text).group(1)) == 1024


def test_entry_points_check_their_arguments_before_any_launch():
    from neat_amd import _lib
    lib = _lib.lib()
    names = ("neat_grid_points_affine", "neat_mesh_moments_ws_bytes", "neat_mesh_moments", "neat_affine_rows3", "neat_affine_bounds3_ws_bytes",
             "neat_affine_bounds3", "neat_mesh_cut_count", "neat_mesh_cut_emit")
    for name in names:
        assert name in _lib.exported_symbols()
    d3, d9, d12 = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_double * 12)(*([0.0] * 12))
    n3, b0, b1 = (ctypes.c_int * 3)(4, 4, 4), (ctypes.c_double * 3)(-1, -1, -1), (ctypes.c_double * 3)(1, 1, 1)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    nan9 = (ctypes.c_double * 9)(*([float("nan")] * 9))
    assert lib.neat_grid_points_affine(None, 64, 0, 64, n3, b0, b1, d9, d3, None) == -1
    assert lib.neat_grid_points_affine(p, 64, 1, 64, n3, b0, b1, d9, d3, None) == -1            # runs past the last node
    assert lib.neat_grid_points_affine(p, 32, 0, 64, n3, b0, b1, d9, d3, None) == -1            # stride under the count
    assert lib.neat_grid_points_affine(p, 64, 0, 64, n3, b0, b1, nan9, d3, None) == -1
    assert lib.neat_grid_points_affine(p, 64, 0, 64, n3, b0, b1, None, d3, None) == -1
    assert lib.neat_mesh_moments_ws_bytes(-1) == 0 and lib.neat_mesh_moments_ws_bytes(1024) == lib.neat_mesh_moments_ws_bytes(1)
    assert lib.neat_mesh_moments_ws_bytes(100 * 1024) > lib.neat_mesh_moments_ws_bytes(1024) >= 8
    assert lib.neat_mesh_moments(p, 4, p, 2, d3, None, None, p, None) == -1
    assert lib.neat_mesh_moments(p, 4, None, 2, d3, None, p, p, None) == -1
    assert lib.neat_mesh_moments(p, 4, p, 2000, d3, None, p, p, None) == -1                      # more than one tile needs a workspace
    assert lib.neat_affine_rows3(None, 4, d12, None) == -1 and lib.neat_affine_rows3(p, -1, d12, None) == -1
    assert lib.neat_affine_rows3(p, 4, None, None) == -1 and lib.neat_affine_rows3(None, 0, d12, None) == 0
    assert lib.neat_affine_bounds3_ws_bytes() > 0
    assert lib.neat_affine_bounds3(p, 0, d12, p, p, None) == -1 and lib.neat_affine_bounds3(p, 4, d12, None, p, None) == -1
    assert lib.neat_mesh_cut_count(p, 4, p, 2, 3, 0.0, 1, p, p, p, None) == -1                   # no such axis
    assert lib.neat_mesh_cut_count(p, 4, p, 2, 0, 0.0, 0, p, p, p, None) == -1                   # sign is +1 or -1
    assert lib.neat_mesh_cut_count(p, 4, p, 2, 0, 0.1, 1, p, p, p, None) == -1                   # 0.1 is no float32 value
    assert lib.neat_mesh_cut_count(p, 4, None, 2, 0, 0.5, 1, p, p, p, None) == -1
    assert lib.neat_mesh_cut_emit(p, 4, p, 2, 0, 0.5, 1, p, p, p, p, 2, 3, p, 4, p, 2, None) == -1      # nkeep + ncut is not nv_out
    assert lib.neat_mesh_cut_emit(p, 4, p, 2, 0, 0.5, 1, p, p, p, None, 2, 2, p, 4, p, 2, None) == -1   # keys missing


def test_cli_flags_of_the_evaluation_mesh(tmp_path):
    from neat_amd import mesh
    opt = mesh.build_parser().parse_args(["--conf", "c"])
    assert not opt.eval and opt.bbox is None and opt.bbox_values is None and opt.scan_id is None and opt.cams is None
    assert not opt.no_world and not opt.all_components and not opt.normals and opt.resolution is None
    assert mesh.EVAL_RESOLUTION == 512
    assert mesh.eval_out_path("run", 7, 65) == os.path.join("run", "7", "scan65.ply") and mesh.eval_out_path("run", 7) == os.path.join("run", "7", "scan.ply")
    box = np.array([[-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]])
    np.savez(tmp_path / "bbs.npz", **{"65": box})
    opt = mesh.build_parser().parse_args(["--conf", "c", "--eval", "--bbox", str(tmp_path / "bbs.npz"), "--scan_id", "65"])
    assert np.array_equal(mesh.eval_bbox(opt), box * [[1.5], [1.0]])             # the reference's scaling of the min row, this route only
    opt = mesh.build_parser().parse_args(["--conf", "c", "--eval", "--bbox-values", "-1", "-2", "-3", "1", "2", "3"])
    assert np.array_equal(mesh.eval_bbox(opt), box)
    with pytest.raises(SystemExit):
        mesh.eval_bbox(mesh.build_parser().parse_args(["--conf", "c", "--eval", "--bbox", "x.npz"]))
