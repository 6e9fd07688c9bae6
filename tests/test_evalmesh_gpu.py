"""GPU: the evaluation-mesh kernels (csrc/kernels_evalmesh.hpp) against their float64 restatement (tests/evalmesh_f64.py) on the same
fp32 inputs -- oriented grid points and the SDF grid in a frame bit for bit, moments within float64 summation slack, affine rows bit
for bit, the cut with integer-equal faces --, and mesh.eval_surface on the synthetic models through its properties."""
import numpy as np
import pytest
import torch

from tests import evalmesh_f64 as E
from tests import mesh_f64 as M
from tests.test_evalmesh_math import rotation
from tests.test_mesh_gpu import field, rough_model

pytestmark = pytest.mark.gpu
WG, TILE = 256, 1024        # kernels_evalmesh.hpp EMESH_WG, MOMENTS_TILE; pinned by tests/test_evalmesh_math.py
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- oriented points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 7), (24, 31, 40)])
@pytest.mark.parametrize("frame", ["identity", "rotated"])
def test_oriented_points_equal_the_restatement_bit_for_bit(shape, frame):
    from neat_amd import ops
    lo, hi = (-1.5, -0.7, 0.1), (1.5, 2.3, 0.30000001)
    R, c = (np.eye(3), np.zeros(3)) if frame == "identity" else (rotation(5), np.array([0.11, -0.23, 0.37]))
    want = torch.tensor(E.oriented_points(shape, lo, hi, R, c))
    total = shape[0] * shape[1] * shape[2]
    # the whole grid, then a ragged split: an odd first node and counts at the SDF kernels' point tiles (64 fp32, 128 16-bit) -1 / 0 / +1
    calls = [(0, total)] + [(f, n) for f in (0, total // 3 | 1) for n in (1, 63, 64, 65, 127, 128, 129) if f + n <= total]
    differing = 0
    for first, count in calls:
        ldp = -(-count // 128) * 128
        x = torch.full((3, ldp), 7.0, device=DEV)
        ops.grid_points_affine(x, ldp, first, count, shape, lo, hi, R, c)
        differing += int((bits(x[:, :count].cpu().t()) != bits(want[first:first + count])).sum())
        assert bool((x[:, count:] == 0).all()), (first, count)
        if frame == "identity":                                    # with the identity it is neat_grid_points
            y = torch.full((3, ldp), 7.0, device=DEV)
            ops.grid_points(y, ldp, first, count, shape, lo, hi)
            assert torch.equal(bits(x), bits(y)), (first, count)
    print(f"{frame} {shape}: {differing} words differ in {len(calls)} calls")
    assert differing == 0


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_sdf_grid_in_a_frame_is_get_sdf_vals_bit_for_bit(prec):
    from neat_amd import mesh
    model = rough_model(prec)
    shape, lo, hi = (24, 31, 40), (-0.9, -1.1, -0.7), (0.8, 1.0, 1.2)
    R, c = rotation(9), np.array([0.05, -0.1, 0.15])
    pts = torch.tensor(E.oriented_points(shape, lo, hi, R, c)).to(DEV)
    with torch.no_grad():
        want = model.implicit_network.get_sdf_vals(pts).reshape(shape)
    for chunk in (4096, 1 << 20):
        got = mesh.sdf_grid(model, shape, (lo, hi), chunk=chunk, frame=(R, c))
        diff = int((bits(got) != bits(want)).sum())
        print(f"{prec} chunk {chunk}: {diff} of {got.numel()} values differ in bits")
        assert got.shape == shape and diff == 0
    plain = torch.tensor(E.oriented_points(shape, lo, hi, np.eye(3), np.zeros(3))).to(DEV)
    with torch.no_grad():
        assert torch.equal(mesh.sdf_grid(model, shape, (lo, hi)), model.implicit_network.get_sdf_vals(plain).reshape(shape))      # unchanged without a frame


# ---- meshes shared by the tests below (computed once, never written) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes():
    from neat_amd import mesh
    out = {}
    for kind in ("sphere", "torus"):
        for n in (33, 65):
            g = field((n, n, n), kind, seed=n)
            v, f = mesh.extract(torch.tensor(g).to(DEV), -1.5, 1.5)
            out[kind, n] = (v, f, v.cpu().numpy(), f.cpu().numpy().astype(np.int64))
    return out


# ---- moments ----------------------------------------------------------------------------------------------------------------------------------
def test_moments_equal_the_restatement(meshes):
    from neat_amd import ops
    v, f, hv, hf = meshes["sphere", 65]
    assert len(hf) > TILE + 1
    o = np.array([0.02, -0.01, 0.03])
    for nf in (1, WG - 1, WG, WG + 1, TILE + 1, len(hf)):
        got = ops.mesh_moments(v, f[:nf].contiguous(), o)
        want = E.moments(hv, hf[:nf], o)
        r = np.linalg.norm(hv[np.unique(hf[:nf])] - o, axis=1).max()
        bar = 1e-12 * want[0] * r * r                              # float64 summation-order slack: the inputs are the same fp32 values
        err = np.abs(got - want).max()
        print(f"nf {nf}: area {want[0]:.6e} max error {err:.3e} (bar {bar:.3e})")
        assert err <= bar, nf
        assert ops.mesh_moments(v, f[:nf].contiguous(), o).tobytes() == got.tobytes()      # two runs, the same bytes
    bad = v.clone()
    bad[int(hf[300, 1]), 2] = float("nan")
    with pytest.raises(RuntimeError):
        ops.mesh_moments(bad, f, o)
    with pytest.raises(RuntimeError):                              # an index past the vertices is refused, not read
        ops.mesh_moments(v[:100].contiguous(), f, o)
    degenerate = torch.tensor([[0, 0, 1], [5, 5, 5]], dtype=torch.int32, device=DEV)
    assert (ops.mesh_moments(v, degenerate, o) == 0).all()        # triangles without area add nothing


def test_moments_over_two_levels_above_the_leaves(meshes):
    """WG TILE + 1 triangles are 257 leaf sums, which the tree reduces to 2 and then to 1: two levels above the leaves, where the
    shapes above stop at one.  The triangles are the sphere's, repeated; judged as test_moments_equal_the_restatement judges."""
    from neat_amd import ops
    v, f, hv, hf = meshes["sphere", 65]
    nf = WG * TILE + 1
    reps = -(-nf // len(hf))
    f2, hf2 = f.repeat(reps, 1)[:nf].contiguous(), np.tile(hf, (reps, 1))[:nf]
    o = np.array([0.02, -0.01, 0.03])
    got = ops.mesh_moments(v, f2, o)
    want = E.moments(hv, hf2, o)
    r = np.linalg.norm(hv[np.unique(hf2)] - o, axis=1).max()
    bar = 1e-12 * want[0] * r * r
    err = np.abs(got - want).max()
    print(f"nf {nf}: area {want[0]:.6e} max error {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    assert ops.mesh_moments(v, f2, o).tobytes() == got.tobytes()


def test_principal_frame_of_an_ellipsoid():
    from neat_amd import mesh
    Q, centre = rotation(4), np.array([0.04, -0.03, 0.02])
    n = 65
    ax = M.linspace_f32(-1.5, 1.5, n).astype(np.float64)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1) - centre
    g = (np.linalg.norm((p @ Q) / [0.3, 0.6, 1.1], axis=-1) - 1.0).astype(np.float32)      # semi-axes along the columns of Q
    v, f = mesh.extract(torch.tensor(g).to(DEV), -1.5, 1.5)
    R, mean = mesh.principal_frame(v, f)
    wR, wmean = E.principal_frame(v.cpu().numpy(), f.cpu().numpy())
    print("axes error", np.abs(R - wR).max(), "mean error", np.abs(mean - wmean).max())
    assert np.abs(R - wR).max() <= 1e-6 and np.abs(mean - wmean).max() <= 1e-6
    assert abs(np.linalg.det(R) - 1) <= 1e-12
    align = np.abs(R @ Q)                                          # and they are the ellipsoid's: the shortest semi-axis first
    assert align[0, 0] > 0.999 and (align.max(axis=1) > 0.999).all()


# ---- affine rows and bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, WG - 1, WG, WG + 1])
def test_affine_rows_and_bounds(n):
    from neat_amd import ops
    rng = np.random.default_rng(n)
    hv = rng.normal(size=(n, 3)).astype(np.float32)
    A = np.concatenate([rotation(n) * 1.7, rng.normal(size=(3, 1))], axis=1)
    v = torch.tensor(hv).to(DEV)
    bounds = ops.affine_bounds3(v, A).cpu().numpy()
    assert torch.equal(v.cpu(), torch.tensor(hv))                  # bounds write nothing
    assert np.array_equal(bounds, E.affine_bounds(hv, A))
    ops.affine_rows3_(v, A)
    assert np.array_equal(v.cpu().numpy().view(np.int32), E.affine_rows(hv, A).view(np.int32))


def test_affine_bounds_of_many_rows(meshes):
    from neat_amd import ops
    v, _, hv, _ = meshes["torus", 65]
    assert len(hv) > 2 * WG
    A = np.concatenate([rotation(2), [[0.1], [0.2], [0.3]]], axis=1)
    assert np.array_equal(ops.affine_bounds3(v, A).cpu().numpy(), E.affine_bounds(hv, A))


# ---- the cut --------------------------------------------------------------------------------------------------------------------------------------
def compare_cut(got, want, scale, what):
    gv, gf = got[0].cpu().numpy(), got[1].cpu().numpy().astype(np.int64)
    wv, wf = want
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert gv.shape == wv.shape and gf.shape == wf.shape, (what, gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gf, wf), what
    bar = 4 * 2.0 ** -23 * scale
    err = float(np.abs(gv.astype(np.float64) - wv).max()) if len(wv) else 0.0
    assert err <= bar, (what, err, bar)
    return err


def test_cut_of_single_triangles():
    """Every vertex outside (-), inside (+) or exactly on the plane (0, which is inside): all 27 combinations, hence all eight inside /
    outside patterns with and without vertices on the plane, times both orientations, both signs and every axis."""
    from neat_amd import ops
    rng = np.random.default_rng(3)
    worst, cases = 0.0, 0
    for axis in range(3):
        for sign in (1, -1):
            plane = np.float32(0.3)
            for combo in np.ndindex(3, 3, 3):
                hv = rng.uniform(-1, 1, size=(4, 3)).astype(np.float32)      # a fourth, unused vertex: dropped
                hv[:3, axis] = [plane + np.float32(sign * (s - 1) * rng.uniform(0.1, 1.0)) if s != 1 else plane for s in combo]
                for face in ([0, 1, 2], [0, 2, 1]):
                    hf = np.array([face], dtype=np.int64)
                    got = ops.mesh_cut(torch.tensor(hv).to(DEV), torch.tensor(hf, dtype=torch.int32).to(DEV), axis, float(plane), sign)
                    want = E.cut_plane(hv, hf, axis, plane, sign)
                    worst = max(worst, compare_cut(got, want, 1.3, (axis, sign, combo, face)))
                    n_in = sum(s >= 1 for s in combo)
                    assert len(want[1]) == (0, 1, 2, 1)[n_in]
                    cutv = got[0].cpu().numpy()[n_in:] if n_in in (1, 2) else np.zeros((0, 3), dtype=np.float32)
                    assert len(cutv) == (2 if n_in in (1, 2) else 0) and (cutv[:, axis] == plane).all()      # float32(plane), exactly
                    cases += 1
    print(f"{cases} single-triangle cuts, max vertex error {worst:.3e}")


@pytest.mark.parametrize("kind,n", [("sphere", 33), ("sphere", 65), ("torus", 33), ("torus", 65)])
def test_clip_box_of_whole_meshes(meshes, kind, n):
    from neat_amd import mesh
    v, f, hv, hf = meshes[kind, n]
    # through the torus hole: a slab around the axis that keeps two opposite arcs apart
    lo, hi = ((-1.2, -0.3, -0.4), (1.2, 0.33, 0.11)) if kind == "torus" else ((-0.31, -0.6, -0.12), (0.37, 0.2, 0.6))
    got = mesh.clip_box(v, f, lo, hi)
    want = E.clip_box(hv, hf, lo, hi)
    err = compare_cut(got, want, 1.5, (kind, n))
    comps = len(np.unique(M.components(len(want[0]), want[1])))
    lab = mesh.face_components(got[1], got[0].shape[0])
    print(f"{kind} {n}: {len(want[0])} vertices {len(want[1])} faces, {comps} components, max vertex error {err:.3e}")
    assert int(torch.unique(lab).numel()) == comps == (2 if kind == "torus" else 1)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    gv = got[0].cpu().numpy()
    assert (gv >= lo32).all() and (gv <= hi32).all()
    again = mesh.clip_box(v.clone(), f.clone(), lo, hi)
    assert torch.equal(bits(again[0]), bits(got[0])) and torch.equal(again[1], got[1])      # two runs, the same bytes
    inside = mesh.clip_box(v, f, -1.4, 1.4)
    assert torch.equal(bits(inside[0]), bits(v)) and torch.equal(inside[1], f)              # wholly inside: identical bytes
    outside = mesh.clip_box(v, f, (1.2, 1.2, 1.2), (1.4, 1.4, 1.4))
    assert outside[0].shape == (0, 3) and outside[1].shape == (0, 3)


# ---- the pipeline on the synthetic models -----------------------------------------------------------------------------------------------------------
def on_box_plane(ends, lo, hi):
    """ends [edges, 2, 3]: both ends of every edge on one and the same plane of the box."""
    return ((ends == np.float32(lo)) | (ends == np.float32(hi))).all(axis=1).any(axis=1)


@pytest.fixture(scope="module")
def init_run():
    from neat_amd import mesh
    model = rough_model("fp32", "init")
    timings = {}
    res = mesh.eval_surface(model, resolution=48, timings=timings)
    assert set(timings) == {"coarse_s", "frame_s", "grid_s", "extract_s", "components_s"}
    return model, res


def test_eval_surface_of_the_smooth_model(init_run):
    from neat_amd import ops
    model, res = init_run
    v, f, fr = res["verts"].cpu().numpy(), res["faces"].cpu().numpy().astype(np.int64), res["frame"]
    assert res["normals"] is None and min(fr["shape"]) == 48
    assert len(np.unique(M.components(len(v), f))) == 1 and len(E.open_edges(f)) == 0 and M.euler(len(v), f) == 2
    # a vertex lies in a cell whose corners straddle the level: its value is within one cell diagonal times the gradient norm of it.
    # The norm is measured here: at the vertices and at random points of the aligned grid's box
    net = model.implicit_network
    h = (fr["hi3"][0] - fr["lo3"][0]) / (fr["shape"][0] - 1)
    rng = np.random.default_rng(0)
    local = rng.uniform(fr["lo3"], fr["hi3"], size=(20000, 3))
    probe = torch.tensor((local @ fr["R"] + fr["mean"]).astype(np.float32)).to(DEV)
    with torch.no_grad():
        sdf, _ = ops.sdf_point_normals(net.handle(), res["verts"], net.sdf_bounding_sphere, net.sphere_scale)
        gnorm = max(float(ops.sdf_point_normals(net.handle(), x, net.sdf_bounding_sphere, net.sphere_scale)[1].norm(dim=1).max())
                    for x in (res["verts"], probe))
    bar = np.sqrt(3.0) * h * gnorm
    print(f"{len(v)} vertices {len(f)} faces, grid {fr['shape']} h {h:.4f}, max |sdf| {float(sdf.abs().max()):.3e}, max |grad| {gnorm:.3f}, bar {bar:.3e}")
    assert float(sdf.abs().max()) <= bar
    assert abs(np.linalg.det(fr["R"]) - 1) <= 1e-12


def test_eval_surface_with_a_box_and_a_scale(init_run):
    from neat_amd import mesh
    model, res = init_run
    v = res["verts"].cpu().numpy()
    lo, hi = v.min(axis=0) - 0.1, v.max(axis=0) + 0.1
    hi[0] = 0.5 * (v[:, 0].min() + v[:, 0].max()) + 0.21 * (v[:, 0].max() - v[:, 0].min())      # cuts the surface
    bbox = np.stack([lo, hi]).astype(np.float32)
    timings = {}
    cut = mesh.eval_surface(model, resolution=48, bbox=bbox, timings=timings)
    assert "cut_s" in timings
    cv, cf = cut["verts"].cpu().numpy(), cut["faces"].cpu().numpy().astype(np.int64)
    assert (cv >= bbox[0]).all() and (cv <= bbox[1]).all() and (cv[:, 0] == bbox[1, 0]).any()
    ends = cv[E.open_edges(cf)]
    assert len(ends) > 0 and on_box_plane(ends, bbox[0], bbox[1]).all()
    assert len(np.unique(M.components(len(cv), cf))) == 1
    # scale_mat = a similarity: the vertices are the affine image of the unscaled run's, the faces the same
    S = np.eye(4)
    S[:3, :3] *= 250.0
    S[:3, 3] = [12.5, -40.0, 600.25]
    world = mesh.eval_surface(model, resolution=48, scale_mat=S, normals=True)
    assert torch.equal(world["faces"], res["faces"])
    assert np.array_equal(world["verts"].cpu().numpy().view(np.int32), E.affine_rows(v, S[:3]).view(np.int32))
    nrm = world["normals"].cpu().numpy()
    assert nrm.shape == v.shape and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    S[0, 1] = 0.1
    with pytest.raises(ValueError):
        mesh.eval_surface(model, resolution=48, scale_mat=S, normals=True)


def test_eval_surface_without_a_level_crossing_is_none():
    from neat_amd import mesh
    assert mesh.eval_surface(rough_model("fp32"), resolution=48, level=0.0) is None
