"""neat_scenegen_* on the device against the float64 restatement of tests/scenegen_f64.py (brute force over all triangles): the pictures
byte for byte, the runs index for index and their end points bit for bit, at the sizes where the 16 x 16 tiles, the 64-sample rounds of
the edge kernel and the workgroups of the tree's refit bite; and the refusals, which come back before any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import scenegen_f64 as SG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def shape(name):
    from neat_amd import scenegen
    base, _, sub = name.partition("/")
    verts, faces, junctions, edges = scenegen.shapes[base]
    verts, faces = scenegen.subdivide(verts, faces, int(sub or 0))
    verts, junctions = scenegen.normalise(verts, junctions)
    return verts, faces, junctions, edges


def views(H, W):
    """Three views of the unit-sized shapes that fill most of an H x W picture; the second has a skew."""
    from neat_amd import scenegen
    _, poses = scenegen.cameras(3, 64)
    f = 1.1 * min(H, W)
    K = np.broadcast_to(np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]), (3, 3, 3)).copy()
    K[1, 0, 1] = 0.3
    return K, poses


@functools.lru_cache(maxsize=None)
def picture_reference(name, H, W, ss):
    verts, faces, _, _ = shape(name)
    K, poses = views(H, W)
    return SG.pictures(verts, faces, K, poses, H, W, ss)


def build(verts, faces):
    from neat_amd import raycast
    scene = raycast.build(verts, faces, DEV)
    assert scene.status == 0
    return scene


# ---- pictures -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [1, 2, 3])
@pytest.mark.parametrize("size", [(29, 37), (8, 8)])
@pytest.mark.parametrize("name", ["box", "lblock", "lblock/3"])          # lblock/3: 1280 triangles, a tree of 2048 leaves
def test_pictures_equal_the_reference(name, size, ss):
    from neat_amd import scenegen
    H, W = size
    verts, faces, _, _ = shape(name)
    K, poses = views(H, W)
    want_rgb, want_mask = picture_reference(name, H, W, ss)
    rgb, mask = scenegen.pictures(build(verts, faces), K, poses, H, W, ss=ss)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, H, W, 3) and mask.dtype == torch.uint8 and tuple(mask.shape) == (3, H, W)
    rgb, mask = rgb.cpu().numpy(), mask.cpu().numpy()
    print("  %s %dx%d ss %d: %d of %d pixels hit, %d bytes differ" % (name, H, W, ss, int((want_mask > 0).sum()), want_mask.size,
                                                                     int((rgb != want_rgb).sum())))
    assert 0 < (want_mask > 0).mean() < 1 and len(np.unique(want_rgb)) > 3
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(rgb, want_rgb)


def test_pictures_of_an_empty_mesh_and_of_no_view():
    from neat_amd import scenegen
    verts, faces, _, _ = shape("box")
    K, poses = views(29, 37)
    rgb, mask = scenegen.pictures(build(verts, np.zeros((0, 3), np.int32)), K, poses, 29, 37, ss=2, background=0.5)
    assert (rgb.cpu().numpy() == 128).all() and (mask.cpu().numpy() == 0).all()
    rgb, mask = scenegen.pictures(build(verts, faces), K[:0], poses[:0], 29, 37)
    assert tuple(rgb.shape) == (0, 29, 37, 3) and tuple(mask.shape) == (0, 29, 37)
    # other shading constants reach the kernel
    want = SG.pictures(verts, faces, K, poses, 8, 8, 2, albedo=0.9, ambient=0.1, background=0.2)
    rgb, mask = scenegen.pictures(build(verts, faces), K, poses, 8, 8, ss=2, albedo=0.9, ambient=0.1, background=0.2)
    assert np.array_equal(rgb.cpu().numpy(), want[0]) and np.array_equal(mask.cpu().numpy(), want[1])


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------------
def check_runs(got, want):
    idx, p2, p3, junc = (x.cpu().numpy() for x in got)
    assert idx.dtype == np.int32 and p2.dtype == np.float64 and p3.dtype == np.float64 and junc.dtype == bool
    assert idx.shape == want["idx"].shape and np.array_equal(idx, want["idx"])
    assert np.array_equal(junc, want["junc"] != 0)
    assert p2.shape == want["p2"].shape and np.array_equal(p2.view(np.int64), want["p2"].view(np.int64))          # the same bits
    assert p3.shape == want["p3"].shape and np.array_equal(p3.view(np.int64), want["p3"].view(np.int64))


def rounds_scene():
    """Edges whose sample counts sit on the borders of the kernel's 64-sample rounds.  The camera looks down +z with fx = 128, so an edge
    at z = 1 between x = a / 128 and b / 128 is exactly b - a pixels long and has b - a + 1 samples at step 1.  A small quad at z = 0.5
    hides samples 64 .. 70 of the 129-sample edge: one run ends on the last sample of round 0 and the next spans rounds 1 and 2."""
    H, W = 48, 160
    K = np.array([[128.0, 0.0, 80.0], [0.0, 128.0, 24.0], [0.0, 0.0, 1.0]])
    row = lambda py: (py - 24.0) / 128.0
    col = lambda px: (px - 80.0) / 128.0
    J, E = [], []

    def edge(a, b):
        J.extend([a, b])
        E.append((len(J) - 2, len(J) - 1))
    edge((0.0, row(4), 1.0), (0.0, row(4) * 2.0, 2.0))                   # seen end on: n = 1
    for k, length in enumerate((1, 62, 63, 64)):                       # n = 2, 63, 64, 65
        edge((col(10), row(8 + 4 * k), 1.0), (col(10 + length), row(8 + 4 * k), 1.0))
    edge((col(10), row(24), 1.0), (col(138), row(24), 1.0))             # n = 129, partly hidden
    edge((col(20), row(30), -1.0), (col(60), row(30), -0.5))            # behind the camera
    edge((0.04, -0.01, 1.0), (0.0, 0.0, -1.0))                          # across z = near, close to the axis
    edge((col(100), row(38), 1.0), (col(300), row(40), 1.0))            # across the right border
    edge((col(138), row(24), 1.0), (col(10), row(24), 1.0))             # the hidden one again, the other way round
    x0, x1, y0, y1 = col(73.5) / 2.0, col(80.5) / 2.0, row(22) / 2.0, row(26) / 2.0
    verts = np.array([[x0, y0, 0.5], [x1, y0, 0.5], [x1, y1, 0.5], [x0, y1, 0.5]])
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    shifted = np.eye(4)
    shifted[:3, 3] = [3.0 / 128.0, -1.0 / 128.0, 0.0]
    return verts, faces, np.array(J), np.array(E, np.int32), np.stack([K, K]), np.stack([np.eye(4), shifted]), H, W


def test_runs_at_the_borders_of_the_sample_rounds():
    from neat_amd import scenegen
    verts, faces, J, E, K, poses, H, W = rounds_scene()
    scene = build(verts, faces)
    for min_len in (0.0, 2.0):
        want = SG.visible_edges(verts, faces, J, E, K, poses, H, W, 1.0, min_len, 0.002, 0.05)
        if min_len == 0.0:
            first = want["idx"][want["idx"][:, 0] == 0]
            n = {int(e): int(l) + 1 for _, e, _, l in first}                       # the last sample of an edge's last run
            assert [n[e] for e in (0, 1, 2, 3, 4, 5)] == [1, 2, 63, 64, 65, 129]
            assert [r[2:].tolist() for r in first if r[1] == 5] == [[0, 63], [71, 128]]      # ends on a round's last sample; spans a border
            assert 6 not in n and 7 in n and 8 in n
            assert want["junc"][(want["idx"][:, 0] == 0) & (want["idx"][:, 1] == 7)].tolist() == [[1, 0]]
            assert want["junc"][(want["idx"][:, 0] == 0) & (want["idx"][:, 1] == 8)].tolist() == [[1, 0]]
        check_runs(scenegen.visible_edges(scene, J, E, K, poses, H, W, step=1.0, min_len=min_len, bias=0.002, near=0.05), want)
    want = SG.visible_edges(verts, faces, J, E, K, poses, H, W, 0.37, 1.0, 0.01, 0.05)       # another step: other counts
    check_runs(scenegen.visible_edges(scene, J, E, K, poses, H, W, step=0.37, min_len=1.0, bias=0.01, near=0.05), want)
    none = scenegen.visible_edges(scene, J, E[:0], K, poses, H, W)                           # E = 0
    assert tuple(none.idx.shape) == (0, 4) and tuple(none.p3.shape) == (0, 2, 3)
    none = scenegen.visible_edges(scene, J, E, K[:0], poses[:0], H, W)                       # V = 0
    assert tuple(none.idx.shape) == (0, 4)


@pytest.mark.parametrize("name", ["lblock", "lblock/3"])
def test_runs_of_a_shape_that_hides_parts_of_itself(name):
    from neat_amd import scenegen
    verts, faces, J, E = shape(name)
    K, poses = views(96, 128)
    K, poses = np.concatenate([K, K[:1]]), np.concatenate([poses, scenegen.cameras(1, 64)[1][:1]])
    from neat_amd.synth import look_at_pose
    poses[3] = look_at_pose((0.3, -2.0, 0.8)).astype(np.float64)                    # the arm in front of an upright edge
    want = SG.visible_edges(verts, faces, J, E, K, poses, 96, 128, **{k: scenegen.DEFAULTS[k] for k in ("step", "min_len", "bias", "near")})
    assert want["idx"].shape[0] > 30 and 0 < (want["junc"] == 0).sum() and len(np.unique(want["idx"][:, 0])) == 4
    check_runs(scenegen.visible_edges(build(verts, faces), J, E, K, poses, 96, 128), want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_the_error_before_any_launch():
    from neat_amd import _lib, scenegen
    lib = _lib.lib()
    verts, faces, J, E = shape("box")
    scene = build(verts, faces)
    K, poses = views(29, 37)
    Kd, Pd = torch.from_numpy(K).to(DEV), torch.from_numpy(poses).to(DEV)
    Jd = torch.from_numpy(J).to(DEV)
    ws = torch.zeros(lib.neat_scenegen_scratch_bytes(3, 12), device=DEV, dtype=torch.uint8)
    total = torch.full((1,), 77, device=DEV, dtype=torch.int64)
    rgb = torch.full((3, 29, 37, 3), 7, device=DEV, dtype=torch.uint8)
    mask = torch.full((3, 29, 37), 7, device=DEV, dtype=torch.uint8)

    def count(edges, step, H=29, W=37, nJ=8):
        e = np.ascontiguousarray(edges, np.int32)
        return lib.neat_scenegen_edge_count(_lib.ptr(scene.bvh), scene.nf, _lib.ptr(Jd), nJ, e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                            e.shape[0], _lib.ptr(Kd), _lib.ptr(Pd), 3, H, W, step, 2.0, 0.002, 0.05, _lib.ptr(ws), _lib.ptr(total),
                                            _lib.stream())

    def shade(ss):
        return lib.neat_scenegen_shade(_lib.ptr(scene.bvh), scene.nf, _lib.ptr(Kd), _lib.ptr(Pd), 3, 29, 37, ss, 0.7, 0.25, 1.0, _lib.ptr(rgb),
                                       _lib.ptr(mask), _lib.stream())
    assert count(E, 0.0) == -1 and count(E, -1.0) == -1 and count(E, float("nan")) == -1            # step
    assert count(E, 1e-4) == -1                                                                        # too many samples: 470 100 for the diagonal
    bad = E.copy()
    bad[5, 1] = 8
    assert count(bad, 1.0) == -1 and count(E, 1.0, nJ=7) == -1                                         # a junction index outside the list
    bad[5, 1] = -1
    assert count(bad, 1.0) == -1
    assert shade(0) == -1 and shade(scenegen.MAX_SS + 1) == -1 and shade(-3) == -1
    assert lib.neat_scenegen_scratch_bytes(-1, 3) == 0 and lib.neat_scenegen_scratch_bytes(70000, 3) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == 77 and (rgb == 7).all() and (mask == 7).all() and (ws == 0).all()      # nothing ran
    with pytest.raises(RuntimeError):
        scenegen.visible_edges(scene, J, bad, K, poses, 29, 37)
    with pytest.raises(RuntimeError):
        scenegen.visible_edges(scene, J, E, K, poses, 29, 37, step=0.0)
    with pytest.raises(RuntimeError):
        scenegen.pictures(scene, K, poses, 29, 37, ss=0)
    with pytest.raises(RuntimeError):
        scenegen.pictures(verts, K, poses, 29, 37)                                                      # not a Scene: no host path
    assert count(E, 1.0) == 0 and shade(scenegen.MAX_SS) == 0                                          # and the good calls go through
    torch.cuda.synchronize()
    assert int(total.item()) > 0 and not (mask == 7).any()
