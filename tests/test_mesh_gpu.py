"""GPU: neat_amd.mesh on the device against the float64 restatement (tests/mesh_f64.py) on the SAME fp32 grid values -- counts and faces
equal as integers, vertices within the fp32 bar --, at tile edges, with NaN / inf nodes, at 512^3; the grid evaluation against
get_sdf_vals bit for bit; mesh.surface on the synthetic model."""
import numpy as np
import pytest
import torch

from tests import mesh_f64 as M
from tests.test_mesh_math import sample, sphere, torus

pytestmark = pytest.mark.gpu
TILE = 2048          # kernels_mesh.hpp MESH_TILE (nodes per workgroup; sub-chunks of 256); pinned by tests/test_mesh_math.py


def field(shape, kind, seed=0):
    """fp32 grid values over [-1.5, 1.5]^3: 'noise' crosses the level in most cells (every table case, every edge class)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.normal(size=shape).astype(np.float32)
    if kind == "sphere":
        return (sample(sphere([0.013, -0.007, 0.021], 0.5), shape) + 1e-3 * rng.normal(size=shape)).astype(np.float32)
    if kind == "torus":
        return sample(torus([0.013, -0.007, 0.021], 0.7, 0.25), shape).astype(np.float32)
    raise ValueError(kind)


def compare(g, b0=-1.5, b1=1.5, level=0.0, what=""):
    """Device extraction of the fp32 grid g against the restatement on the same values."""
    from neat_amd import mesh
    dev = torch.device("cuda:0")
    verts, faces = mesh.extract(torch.tensor(g).to(dev), b0, b1, level)
    rv, rf = M.extract(g, b0, b1, level)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert (verts.shape[0], faces.shape[0]) == (len(rv), len(rf)), (what, verts.shape, faces.shape, rv.shape, rf.shape)
    assert np.array_equal(faces.cpu().numpy().astype(np.int64), rf), what
    bar = 4 * 2.0 ** -23 * max(np.abs(np.asarray(b0)).max(), np.abs(np.asarray(b1)).max())
    err = float(np.abs(verts.cpu().numpy().astype(np.float64) - rv).max()) if len(rv) else 0.0
    print(f"{what} {g.shape}: nv {len(rv)} nf {len(rf)} max vertex error {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (what, err, bar)
    return verts, faces


SIZES = [((2, 2, 2), "noise"), ((2, 3, 2), "noise"), ((3, 5, 7), "noise"), ((33, 33, 33), "noise"), ((33, 33, 33), "sphere"),
         ((65, 65, 65), "sphere"), ((65, 65, 65), "noise"), ((129, 64, 33), "torus"), ((100, 100, 100), "sphere"),
         # one axis at the 256-node sub-chunk and at the 2048-node tile, minus / plus one; 2 x 4 x 256 nodes = exactly one tile
         ((2, 4, 255), "noise"), ((2, 4, 256), "noise"), ((2, 4, 257), "noise"),
         ((2, 2, TILE - 1), "noise"), ((2, 2, TILE), "noise"), ((2, 2, TILE + 1), "noise"), ((TILE + 1, 2, 2), "noise")]


@pytest.mark.parametrize("shape,kind", SIZES, ids=[f"{k}-{'x'.join(map(str, s))}" for s, k in SIZES])
def test_extract_equals_the_restatement(shape, kind):
    # measured on MI355X: max vertex error 3.0e-7 over these sizes (4.2e-7 over all cases of this file) against the bar 7.15e-7
    g = field(shape, kind, seed=sum(shape))
    verts, faces = compare(g, what=kind)
    assert faces.shape[0] > 0
    if kind in ("sphere", "torus"):
        ne, ok, _ = M.edge_report(faces.cpu().numpy())
        assert ok.all() and verts.shape[0] - ne + faces.shape[0] == (2 if kind == "sphere" else 0)


def test_every_2x2x2_sign_pattern():
    """All 256 inside / outside patterns of one cell: each of the 16 table cases in each of the six tetrahedra."""
    rng = np.random.default_rng(1)
    for pattern in range(256):
        sign = np.array([-1.0 if (pattern >> c) & 1 else 1.0 for c in range(8)]).reshape(2, 2, 2)
        g = (sign * rng.uniform(0.1, 1.0, (2, 2, 2))).astype(np.float32)
        from neat_amd import mesh
        verts, faces = mesh.extract(torch.tensor(g).cuda(), -1.5, 1.5)
        rv, rf = M.extract(g, -1.5, 1.5)
        assert np.array_equal(faces.cpu().numpy().astype(np.int64), rf), pattern
        assert np.abs(verts.cpu().numpy() - rv).max(initial=0.0) <= 4 * 2.0 ** -23 * 1.5, pattern


def test_level_bounds_and_anisotropic_boxes():
    g = field((21, 34, 27), "noise", 3)
    compare(g, level=0.37, what="level 0.37")
    compare(g, level=-1.2, what="level -1.2")
    compare(g, b0=(-0.7, -1.5, 0.25), b1=(2.3, 1.0, 0.75), level=0.1, what="box")
    compare(field((40, 40, 40), "sphere", 2), level=0.11, what="sphere level 0.11")


def test_empty_results():
    from neat_amd import mesh
    dev = torch.device("cuda:0")
    for g in (torch.ones(5, 6, 7), -torch.ones(5, 6, 7), torch.full((2, 2, 2), float("nan"))):
        verts, faces = mesh.extract(g.to(dev), -1.5, 1.5)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.extract(torch.ones(5, 1, 7, device=dev), -1.5, 1.5)


def test_non_finite_nodes_leave_the_same_holes():
    g = field((17, 19, 23), "noise", 7)
    rng = np.random.default_rng(8)
    idx = rng.integers(0, g.size, 300)
    g.reshape(-1)[idx[:100]] = np.nan
    g.reshape(-1)[idx[100:200]] = np.inf
    g.reshape(-1)[idx[200:]] = -np.inf
    verts, faces = compare(g, what="nan/inf")
    assert torch.isfinite(verts).all()
    clean = field((17, 19, 23), "noise", 7)
    assert faces.shape[0] < M.extract(clean, -1.5, 1.5)[1].shape[0]
    s = field((33, 33, 33), "sphere", 1)
    s[16, 16, 25] = np.nan                                       # next to the surface (r = 0.5: node 16 + 5.3)
    s[16, 16, 22] = np.nan
    verts, faces = compare(s, what="sphere with holes")
    _, ok, _ = M.edge_report(faces.cpu().numpy())
    assert not ok.all()                                          # the documented hole


def test_nodes_exactly_on_the_level():
    g = sample(sphere([0.0, 0.0, 0.0], 0.75), (33, 33, 33)).astype(np.float32)      # nodes at +-0.75 on the axes: exactly on the level
    assert (g == 0).sum() >= 6
    verts, faces = compare(g, what="on level")
    ne, ok, _ = M.edge_report(faces.cpu().numpy())
    assert ok.all() and verts.shape[0] - ne + faces.shape[0] == 2                  # zero-area triangles kept: still a closed manifold
    g2 = field((9, 9, 9), "noise", 4)
    g2[::2, ::3, ::2] = 0.25
    compare(g2, level=0.25, what="many on level")


def test_two_runs_give_the_same_bytes():
    from neat_amd import mesh
    g = torch.tensor(field((65, 65, 65), "noise", 11)).cuda()
    a = mesh.extract(g, -1.5, 1.5)
    b = mesh.extract(g.clone(), -1.5, 1.5)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_tile_offsets_past_1024_tiles():
    """129 x 129 x 127 nodes are 1032 tiles of 2048, so the one workgroup of 1024 that turns the tile counts into offsets (mesh_scan_kernel)
    takes a second round with a carry; every other comparison of this file stays within one round and 512^3 checks the surface alone.
    The float64 restatement needs about 7 s on the host at this size, so the extraction is judged by what a wrong offset breaks: the
    vertex count is numpy's count of the edges whose end nodes differ in sign, the surface is closed and a sphere."""
    from neat_amd import mesh
    shape = (129, 129, 127)
    assert shape[0] * shape[1] * shape[2] > 1024 * TILE
    g = field(shape, "sphere", seed=1)
    verts, faces = mesh.extract(torch.tensor(g).cuda(), -1.5, 1.5)
    inside = g < 0
    edges = 0
    for c in range(1, 8):                                            # the seven edge classes: offsets (dx, dy, dz) = the bits of c
        dx, dy, dz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        a = inside[:shape[0] - dx, :shape[1] - dy, :shape[2] - dz]
        b = inside[dx:, dy:, dz:]
        edges += int((a != b).sum())
    assert verts.shape[0] == edges and bool(torch.isfinite(verts).all())
    f = faces.cpu().numpy()
    ne, ok, _ = M.edge_report(f)
    assert ok.all() and verts.shape[0] - ne + f.shape[0] == 2
    assert f.min() == 0 and f.max() == verts.shape[0] - 1


def test_sphere_at_512():
    from neat_amd import _lib, mesh
    dev = torch.device("cuda:0")
    n = 512
    assert _lib.lib().neat_mesh_ws_bytes(n, n, n) <= 32 * n ** 3
    ax = torch.tensor(mesh.linspace_f32(-1.5, 1.5, n)).to(dev)
    c = (0.013, -0.007, 0.021)
    g = torch.sqrt((ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2) - 0.5
    assert g.shape == (n, n, n) and not bool((g == 0).any())
    verts, faces = mesh.extract(g, -1.5, 1.5)
    del g
    nv, nf = verts.shape[0], faces.shape[0]
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = torch.minimum(e[:, 0], e[:, 1]) * nv + torch.maximum(e[:, 0], e[:, 1])
    sign = torch.where(e[:, 0] < e[:, 1], 1, -1)
    uniq, inv, count = torch.unique(key, return_inverse=True, return_counts=True)
    ssum = torch.zeros_like(uniq).index_add_(0, inv, sign)
    print(f"512^3 sphere: nv {nv} ne {uniq.numel()} nf {nf}")
    assert bool((count == 2).all()) and bool((ssum == 0).all())
    assert nv - uniq.numel() + nf == 2
    assert int(f.min()) == 0 and int(f.max()) == nv - 1
    r = (verts.double() - torch.tensor(c, device=dev, dtype=torch.float64)).norm(dim=1)
    assert float((r - 0.5).abs().max()) < (3.0 / 511) ** 2                      # on the sphere to second order in the cell size


def rough_model(prec, variant="rough"):
    from neat_amd import networks, synth
    sd = synth.synth_state_dict(7, variant)
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    model.to(torch.device("cuda:0")).eval()
    model.set_precision(prec)
    return model


def host_points(shape, lo, hi):
    from neat_amd import mesh
    axes = [torch.tensor(mesh.linspace_f32(lo, hi, n)) for n in shape]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)


def test_grid_points_are_the_linspace_rule():
    from neat_amd import ops
    dev = torch.device("cuda:0")
    shape, lo, hi = (7, 100, 13), (-1.5, -0.7, 0.1), (1.5, 2.3, 0.30000001)
    total = 7 * 100 * 13
    want = torch.stack(torch.meshgrid(*[torch.tensor(M.linspace_f32(lo[a], hi[a], shape[a])) for a in range(3)], indexing="ij"), dim=-1).reshape(-1, 3)
    first, count, ldp = 1234, 5000, 5120
    x = torch.full((3, ldp), 7.0, device=dev)
    ops.grid_points(x, ldp, first, count, shape, lo, hi)
    assert torch.equal(x[:, :count].cpu().t(), want[first:first + count])
    assert bool((x[:, count:] == 0).all())
    ops.grid_points(x, ldp, total - 100, 100, shape, lo, hi)
    assert torch.equal(x[:, :100].cpu().t(), want[total - 100:])


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("shape,chunks", [((24, 31, 40), (4096, 1 << 20)), ((64, 64, 64), (65536, 100000))])
def test_sdf_grid_is_get_sdf_vals_bit_for_bit(prec, shape, chunks):
    from neat_amd import mesh
    model = rough_model(prec)
    pts = host_points(shape, -1.5, 1.5).cuda()
    with torch.no_grad():
        want = model.implicit_network.get_sdf_vals(pts).reshape(shape)
    for chunk in chunks:
        got = mesh.sdf_grid(model, shape, (-1.5, 1.5), chunk=chunk)
        assert got.shape == tuple(shape) and got.dtype == torch.float32
        diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"{prec} {shape} chunk {chunk}: {diff} of {got.numel()} values differ in bits")
        assert diff == 0, (prec, shape, chunk)
    assert torch.equal(mesh.sdf_grid(model.implicit_network, shape, (-1.5, 1.5)), want)      # the SDF network alone is accepted too


@pytest.mark.parametrize("level", [0.6, 1.0])
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_surface_of_the_synthetic_model(prec, level):
    """The 'rough' synthetic model's SDF stays within [0.34, 3.24] on [-1.5, 1.5]^3 (the CPU oracle, oracle.neat_oracle.sdf_values, on the
    64^3 grid): it has no zero level there, so mesh.surface at level 0 is None (asserted below) and the surface checks run at two levels it
    does cross.  The float64 restatement on the oracle's grid gives 16 closed components at 0.6 and 39 at 1.0, of which some touch the grid's faces.

    Normals: on this model the network's gradient does NOT lie on the side of the incident faces' average normal at every vertex, and that
    is a property of the input, not of the device code: the perturbations have wavelengths of about four cells at 64^3, and where the
    level set passes a saddle of the field the interpolant's normal and the true gradient part.  The CPU oracle's gradient at the
    restatement's vertices disagrees at 196 of 9948 vertices (level 0.6, 64^3) -- the device: the same 196; 53 of 44 912 at 128^3, 23 of
    186 058 at 256^3.  So the figure is printed here and the sign check is asserted on the smooth model below
    (test_normals_of_the_smooth_model), where the oracle and the restatement alone satisfy it."""
    from neat_amd import mesh
    model = rough_model(prec)
    assert mesh.surface(model, resolution=64, grid_boundary=(-1.5, 1.5)) is None
    res = mesh.surface(model, resolution=64, grid_boundary=(-1.5, 1.5), level=level)
    assert res is not None
    v, f, n = res["verts"].cpu().numpy().astype(np.float64), res["faces"].cpu().numpy().astype(np.int64), res["normals"].cpu().numpy()
    # closed wherever the surface does not touch the grid's faces
    _, ok, edges = M.edge_report(f)
    touching = (np.abs(np.abs(v[edges]) - 1.5) < 1e-6).any(axis=(1, 2))
    print(f"{prec} level {level}: nv {len(v)} nf {len(f)} open edges {int((~ok).sum())} (on the boundary {int(touching.sum())})")
    assert ok[~touching].all()
    assert ok.all() == (level == 0.6)                            # 0.6 stays inside the box, 1.0 is cut by it
    # normals: unit length, on the side of the incident faces' average normal
    fn = M.face_normals(v, f)
    avg = np.zeros_like(v)
    for c in range(3):
        np.add.at(avg, f[:, c], fn)
    used = np.linalg.norm(avg, axis=1) > 0
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    against = int((np.einsum("ij,ij->i", n.astype(np.float64), avg)[used] <= 0).sum())
    print(f"{prec} level {level}: normals against the faces' average at {against} of {int(used.sum())} vertices (see the docstring)")
    # the largest component: one component, its area the maximum over the components (float64, host)
    big = mesh.surface(model, resolution=64, grid_boundary=(-1.5, 1.5), level=level, largest_component=True, normals=False)
    bv, bf = big["verts"].cpu().numpy().astype(np.float64), big["faces"].cpu().numpy().astype(np.int64)
    assert len(np.unique(M.components(len(bv), bf))) == 1 and bf.min() == 0 and bf.max() == len(bv) - 1
    lab = M.components(len(v), f)[f[:, 0]]
    area = 0.5 * np.linalg.norm(fn, axis=1)
    per = {l: area[lab == l].sum() for l in np.unique(lab)}
    got = 0.5 * np.linalg.norm(M.face_normals(bv, bf), axis=1).sum()
    assert len(per) > 1
    print(f"{prec} level {level}: components {len(per)}, areas max {max(per.values()):.6f}, kept {got:.6f}")
    assert abs(got - max(per.values())) <= 1e-9 * max(per.values())
    assert mesh.surface(model, resolution=16, grid_boundary=(-1.5, 1.5), level=50.0) is None      # nothing crosses: no surface


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_normals_of_the_smooth_model(prec):
    """The geometric-initialisation model ('init': a smooth sphere-like SDF that crosses zero inside the box; one closed component and no
    vertex normal against its faces for the CPU oracle and the restatement alone): level 0, every normal on the side of the incident
    faces' average normal."""
    from neat_amd import mesh
    model = rough_model(prec, "init")
    res = mesh.surface(model, resolution=64, grid_boundary=(-1.5, 1.5))
    v, f, n = res["verts"].cpu().numpy().astype(np.float64), res["faces"].cpu().numpy().astype(np.int64), res["normals"].cpu().numpy()
    ne, ok, _ = M.edge_report(f)
    assert ok.all() and len(v) - ne + len(f) == 2 and len(np.unique(M.components(len(v), f))) == 1
    fn = M.face_normals(v, f)
    avg = np.zeros_like(v)
    for c in range(3):
        np.add.at(avg, f[:, c], fn)
    used = np.linalg.norm(avg, axis=1) > 0
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    dot = np.einsum("ij,ij->i", n.astype(np.float64), avg)[used]
    print(f"{prec}: nv {len(v)} nf {len(f)}, normals against the faces' average: {int((dot <= 0).sum())}")
    assert (dot > 0).all()
