"""The closed loop on the device: one scene directory per shape, written by scenegen.main, and every tool that reads it held to the
analytic truth of tests/closed_loop.py: where the solid is, not what another restatement says.  Each leg takes what the previous tool
wrote: the generator's mesh, lines and cameras from the directory, the dataset's tensors, the PNGs, the dataset's segments.  The
per-tool tests hold a kernel to its own restatement; a convention that a tool and its restatement share (a half pixel, a transposed
pose, a camera-to-world matrix read as world-to-camera) passes them and fails here.

Settings and bars are tests/closed_loop.py's, and tests/test_closed_loop_math.py asserts the same conditions on the float64 side alone.
No bar is taken from the device's output.  Box and L-block:

    quantity                                                      float64 side                MI355X                      bar          the half-pixel mistake
    runs: p2 against the written-out projection of p3             2.8e-14 px on both          2.8e-14 px on both          1e-9 px      0.5 px
    runs: p3 off its edge                                         0 on both                   0 on both                   1e-12
    camera_setup rays of a pixel, projected back                  2.1e-5 px (float32 oracle)  1.9e-5 px                   2.4e-4 px    0.5 px
    project2d_pair of the runs' p3 against p2                     9.2e-6 px (float32 oracle)  1.1e-5 and 9.0e-6 px        2.4e-4 px
    pixel-centre rays: depth against the slab form (box)          1.3e-15                     1.2e-7 (t is a float32)     4.8e-7
    pixels with a partial sub-sample count, left out              1.3 % and 1.5 %             the same: the counts are the float64 side's   3 %
    batches: foot points off their segments                       5.3e-6 and 4.7e-6 px        4.5e-6 and 4.1e-6 px        1e-3 px      0.5 px
    batches: the segment's distance over the nearest run's        0                           0                           1e-4 px
    detected segments: midpoint to nearest projected edge         0.457 and 0.225 px          0.457 and 0.225 px          0.5 px       0.79 and 0.72 px
    detected segments: mean offset, each component                0.0097 and 0.0034 px        0.0097 and 0.0034 px        0.25 px      0.29 and 0.27 px
    detected segments: solved shift, each component               0.022 and 0.0072 px         0.022 and 0.0072 px         0.25 px      0.48 and 0.49 px
    detection: regions, judged, kept (both shapes, one call)      197, 1, 155                 155 kept                    judged <= 1 %
    triangulation from the runs: lines, edges covered over 80 %   12, 12 of 12; 17, 17 of 18  the same                    12 and 17 edges
    the same: end points off the nearest edge's infinite line     8.1e-7 and 2.7e-7           8.1e-7 and 2.7e-7           1e-4         1.1e-2 and 1.2e-2
    triangulation from the detections: lines                      4 and 10                    4 and 10                    equal, positive
    the same: end points off the nearest edge's infinite line     6.4e-4 and 1.2e-2           6.4e-4 and 1.2e-2           recorded: it measures the detector
    closest point against the box's closed form, 257 points       1.11e-16                    1.11e-16                    4.8e-16 (4 x 1.2e-16)

The triangulation bar of 1e-4 sits between the 8e-7 that the rule reaches from runs rounded to float32 and the 1e-2 that runs moved by
half a pixel give.  Along an edge the lines overshoot by up to 0.23 (a member seen at a glancing angle stretches the component), which
is the rule's behaviour: distances are taken to the edge's infinite line.

The MI355X column is one run of this module on the device (NEAT_F64_TABLE's rows, the worst over views and sizes).
Every measured value goes through tests/f64_table.record, so NEAT_F64_TABLE lists it."""
import numpy as np
import pytest
import torch

from tests import closed_loop as C
from tests.f64_table import record, write_table  # noqa: F401  (write_table: the NEAT_F64_TABLE writer, autouse)

BUILD = "closed_loop_gpu"
CAMERA_VIEWS = (0, 5, 11)
_dirs = {}


def dev():
    return torch.device("cuda:0")


def rec(name, P):
    return lambda entry, err: record(BUILD, f"{name}:{entry}", P, err)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("closed_loop"))


def made(root, name):
    """The scene directory of a shape, written once by the command line, and what reads it: -> dict(paths, ds, pics, scene)."""
    if name not in _dirs:
        import os
        from PIL import Image
        from neat_amd import datasets, raycast, scenegen
        out = os.path.join(root, name)
        assert scenegen.main(["--shape", name, "--views", str(C.VIEWS), "--res", str(C.RES), "--ss", str(C.SS), "--out", out]) == 0
        paths = scenegen.scene_paths(out, C.VIEWS)
        ds = datasets.BlenderDataset(name, [C.RES, C.RES], line_detector="gt", data_root=root)
        assert len(ds) == C.VIEWS
        pics = np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths["images"]])
        verts, faces = raycast.read_mesh(paths["mesh"])
        _dirs[name] = {"paths": paths, "ds": ds, "pics": pics, "scene": raycast.build(verts, faces, dev())}
    return _dirs[name]


# ---- the generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_generator(root, name):
    from neat_amd import scenegen
    sc, m = C.scene(name), made(root, name)
    junctions, edges = scenegen.read_lines(m["paths"]["lines"])
    with np.load(m["paths"]["cameras"]) as z:
        K, poses = z["intrinsics"], z["extrinsics"]
    assert np.array_equal(K, sc["K"]) and np.array_equal(poses, sc["poses"]) and np.array_equal(junctions, sc["junctions"])
    runs = scenegen.visible_edges(m["scene"], junctions, edges, K, poses, C.RES, C.RES)
    idx, p2, p3 = (x.cpu().numpy() for x in (runs.idx, runs.p2, runs.p3))
    assert p2.dtype == np.float64 and idx.shape[0] > 0
    C.check_runs(sc, idx, p2, p3, rec(name, idx.shape[0]))
    # the pictures in the directory are the ones whose sub-sample counts the other legs rely on
    from PIL import Image
    masks = np.stack([np.asarray(Image.open(p)) for p in m["paths"]["masks"]])
    assert np.array_equal(masks, sc["mask"]) and np.array_equal(m["pics"], sc["rgb"])


# ---- the training path's float32 camera kernels -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R", [256, 257])
@pytest.mark.parametrize("name", C.SHAPES)
def test_training_camera(root, name, R):
    from neat_amd import ops
    sc, ds = C.scene(name), made(root, name)["ds"]
    for v in CAMERA_VIEWS:
        uv = C.camera_pixels(sc["K"][v], R, seed=R + v)
        uv2 = uv[::-1] * 0.75 + 0.25                                          # the rays through uv_proj: pixels that are no integers
        pose, K = ds.pose_all[v][None].to(dev()), ds.intrinsics_all[v][None].to(dev())
        t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None].to(dev())
        dirs, origins, dirs2, w2c, K3 = ops.camera_setup(t32(uv), t32(uv2), pose, K)
        assert tuple(dirs.shape) == (R, 3) and tuple(origins.shape) == (R, 3) and tuple(dirs2.shape) == (R, 3)
        o, d, d2 = (x.cpu().numpy().astype(np.float64) for x in (origins, dirs, dirs2))
        err = C.check_camera(sc, v, uv, o, d, rec(name, R), f"camera_setup_v{v}")
        assert err <= C.BAR_CAM, err
        err = C.check_camera(sc, v, uv2, o, d2, rec(name, R), f"camera_setup_uv_proj_v{v}")
        assert err <= C.BAR_CAM, err
        p2, p3 = C.view_runs(sc, v)
        X = torch.from_numpy(p3.reshape(-1, 3).astype(np.float32)).to(dev())
        px, calib = ops.project2d_pair(K3, torch.eye(3, device=dev()), w2c, X)
        err = record(BUILD, f"{name}:project2d_pair_v{v}", X.shape[0], np.abs(px.cpu().numpy().astype(np.float64).reshape(-1, 4) - p2).max())
        assert err <= C.BAR_CAM, err
        # with the identity for K the same points come in calibrated coordinates: K applied in float64 gives the pixels again
        c = calib.cpu().numpy().astype(np.float64)
        back = np.stack([sc["K"][v][0, 0] * c[:, 0] + sc["K"][v][0, 2], sc["K"][v][1, 1] * c[:, 1] + sc["K"][v][1, 2]], 1).reshape(-1, 4)
        assert np.abs(back - p2).max() <= C.BAR_CAM


# ---- the pictures against the training rays ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_pictures_against_the_training_rays(root, name):
    from neat_amd import ops, raycast
    sc, m = C.scene(name), made(root, name)
    v, ds = 3, m["ds"]
    uv = torch.from_numpy(C.pixel_grid())[None].to(dev())
    dirs, _, origins = ops.camera_rays(uv, ds.pose_all[v][None].to(dev()), ds.intrinsics_all[v][None].to(dev()), with_origins=True)
    t, tri, _ = raycast.cast(m["scene"], origins, dirs.reshape(-1, 3))
    t, tri = t.cpu().numpy(), tri.cpu().numpy()
    assert np.array_equal(np.isfinite(t), tri >= 0)
    C.check_pictures(sc, v, origins[0].cpu().numpy(), dirs.reshape(-1, 3).cpu().numpy(), t, rec(name, C.RES * C.RES), "pictures")


# ---- the attraction field and the batch gather ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_batches(root, name):
    sc, ds = C.scene(name), made(root, name)["ds"]
    batches = ds.device_batches(dev())
    np.random.seed(5)
    for v in sc["attraction_views"]:
        assert np.array_equal(ds.lines[v][:, :4].numpy().astype(np.float64), sc["segs"][v])      # the runs at float32 rounding, in their order
        for n in (1, 255, 257):
            idx, sample, gt = batches.batch(v, n)
            uv, uv_proj, lines, labels, pixels = (sample[k][0].cpu().numpy() for k in ("uv", "uv_proj", "lines", "labels", "pixels"))
            assert uv.shape == (n, 2) and lines.shape == (n, 5) and int(idx) == v
            run, _ = C.check_attraction(sc["segs"][v], uv, uv_proj, lines, ds.distance, rec(name, n), f"batch_v{v}")
            uniq = sample["lines_uniq"][0].cpu().numpy()
            assert np.array_equal(uniq[labels], lines) and np.array_equal(labels, run)
            assert np.array_equal(pixels, (uv[:, 1] * C.RES + uv[:, 0]).astype(np.int64)) and np.array_equal(uv, np.rint(uv))
            assert np.array_equal(gt["lines2d"][0].cpu().numpy(), lines)
            rgb = sc["rgb"][v].reshape(-1, 3)[pixels].astype(np.float32) / np.float32(255.0)
            assert np.array_equal(gt["rgb"][0].cpu().numpy(), rgb)                                  # the colour is that pixel's


# ---- the detector -------------------------------------------------------------------------------------------------------------------
_detected = {}


def detected(root):
    """detect.lines on the PNGs of both shapes, one call (views are independent; the judge cap of `compare` is 1 % of the regions, and
    the box alone has 1 judged region in 79), against the restatement through tests/test_detect_gpu.compare."""
    if not _detected:
        from tests.test_detect_gpu import compare
        pics = np.concatenate([made(root, name)["pics"] for name in C.SHAPES])
        ref = C.merge_detections([C.scene(name)["det"] for name in C.SHAPES])
        lines, _, _, _, _, offsets = compare(pics, ref, 1.0)
        for i, name in enumerate(C.SHAPES):
            a, b = i * C.VIEWS, (i + 1) * C.VIEWS
            _detected[name] = (lines[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a])
    return _detected


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_detector(root, name):
    sc = C.scene(name)
    lines, offsets = detected(root)[name]
    assert lines.shape[0] >= sc["det"]["lines"].shape[0] - int(sc["det"]["cand_judge"].sum())
    C.check_detections(sc, lines, offsets, rec(name, lines.shape[0]))


# ---- the triangulation --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPES)
def test_triangulation(root, name):
    from neat_amd import run_io, triangulate
    from tests.test_triangulate_gpu import check_lines, host
    sc, ds = C.scene(name), made(root, name)["ds"]
    segments, Ks, Ts = run_io.dataset_views(ds)
    seg64 = [np.ascontiguousarray(s[:, :4].numpy(), dtype=np.float64) for s in segments]
    Ks64 = np.stack([k.numpy() for k in Ks]).astype(np.float64)
    Ts64 = np.stack([t.numpy() for t in Ts]).astype(np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(seg64, sc["segs"])) and np.array_equal(Ks64, sc["K"]) and np.array_equal(Ts64, sc["poses"])
    got = host(triangulate.lines([torch.from_numpy(s).to(dev()) for s in seg64], Ks64, Ts64))
    check_lines(got, sc["tri_runs"])
    C.check_lines3d(sc, got["lines3d"], rec(name, got["lines3d"].shape[0]), "triangulate_runs")
    # from the detector's segments: as many lines as the restatement finds; how far they lie from the edges measures the detector
    lines, offsets = detected(root)[name]
    det = [torch.from_numpy(np.ascontiguousarray(lines[offsets[v]:offsets[v + 1]])).to(dev()) for v in range(C.VIEWS)]
    got = host(triangulate.lines(det, Ks64, Ts64))
    assert got["lines3d"].shape[0] == sc["tri_det"]["lines3d"].shape[0] > 0
    record(BUILD, f"{name}:triangulate_detections", got["lines3d"].shape[0],
           C.nearest_edge_line(got["lines3d"], sc["junctions"], sc["edges"])[1].max())


# ---- the distance to the mesh -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_distance_to_the_box(root):
    from neat_amd import raycast
    sc, m = C.scene("box"), made(root, "box")
    pts = C.closest_points(sc["h"])
    dist, tri, point, _ = raycast.closest(m["scene"], torch.from_numpy(pts).to(dev()))
    dist, point = dist.cpu().numpy(), point.cpu().numpy()
    assert (tri.cpu().numpy() >= 0).all()
    err = record(BUILD, "box:closest", pts.shape[0], np.abs(dist - np.abs(C.box_sdf(pts, sc["h"]))).max())
    assert err <= C.BAR_CLOSEST, err
    assert np.abs(C.box_sdf(point, sc["h"])).max() <= C.BAR_CLOSEST          # the closest point lies on the surface
