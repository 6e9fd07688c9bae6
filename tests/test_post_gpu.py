"""GPU tests of neat_amd.post (fuse / refine / snap; kernels_post.hpp) against the reference's recorded outputs (G21) and the float64
restatement tests/post_f64.py.  Line outputs that are copies must be bit-equal; indices, counts, peaks and edges must be equal; means must
be within 1e-6 max(1, |ref|) (`close` of test_parse_gpu.py: groups here hold <= 8 members, so the tree mean's error is <= 4 * 2^-24 relative)."""
import os

import numpy as np
import pytest
import torch

from tests import post_f64 as F
from tests.test_parse_gpu import close
from tests.test_post_math import PLATEAU_JUNCTIONS, golden_views, plateau_case

WG, GT_CHUNK = 256, 1024          # kernels_parse.hpp PARSE_WG, PARSE_GT_CHUNK
W, H, FOCAL = 128, 96, 64.0
K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]], np.float32)


def dev():
    return torch.device("cuda:0")


def pack(views, img_res=(H, W)):
    from neat_amd import post
    return post.pack_views([torch.tensor(v["det"]).reshape(-1, 5) for v in views], [torch.tensor(v["K"]) for v in views],
                           [torch.tensor(v["pose"]) for v in views], img_res, dev())


def check_fuse(lines, views, by_label, min_margin=1e-4):
    """post.fuse against the twin: flags and counts equal, scores close, kept lines bit-equal copies."""
    from neat_amd import post
    f = F.fuse(lines, views, by_label=by_label)
    assert f["margin"] > min_margin, f["margin"]
    r = post.fuse(torch.tensor(lines).to(dev()), pack(views), score_by_label=by_label)
    assert np.array_equal(r["count"].cpu().numpy(), f["count"])
    assert np.array_equal(r["keep"].cpu().numpy(), f["keep"])
    close(r["score"], f["score"], "score")
    assert np.array_equal(r["lines3d"].cpu().numpy(), np.asarray(lines, np.float32).reshape(-1, 2, 3)[f["keep"]])
    return r, f


# ---- G21: what the reference's scripts wrote -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_g21_fuse_refine_snap_reproduce_the_reference(golden):
    from neat_amd import post
    g = golden("g21_postprocess")
    views = golden_views(g)
    pv = pack(views, g["img_res"])
    lines = torch.tensor(g["lines3d"]).to(dev())
    runs = []
    for _ in range(2):
        fu = post.fuse(lines, pv)
        fl = post.fuse(lines, pv, score_by_label=True)
        filtered = lines[torch.tensor(g["scores"] < 0.01).to(dev())]
        rf = post.refine(filtered, pv)
        sn = post.snap(lines, 512)
        runs.append([fu["lines3d"], fu["score"], fu["count"], fl["keep"], rf, sn["junctions"], sn["edges"], sn["count"], sn["lines3d"]])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert np.array_equal(fu["lines3d"].cpu().numpy(), g["ref_fused"])                       # copies: bit-equal
    close(rf, g["ref_refined"], "refined")
    assert np.array_equal(sn["junctions"].cpu().numpy(), g["ref_snap_junctions"])
    assert np.array_equal(sn["edges"].cpu().numpy(), g["ref_snap_edges"])
    assert np.array_equal(sn["lines3d"].cpu().numpy(), g["ref_snap_junctions"][g["ref_snap_edges"]])
    # and the twin, intermediates included
    for by_label, r in ((False, fu), (True, fl)):
        f = F.fuse(g["lines3d"], views, by_label=by_label)
        assert np.array_equal(r["keep"].cpu().numpy(), f["keep"]) and np.array_equal(r["count"].cpu().numpy(), f["count"])
        close(r["score"], f["score"], "score")
    assert not torch.equal(fu["keep"], fl["keep"])                                           # the enumerate rank is not the label
    f = F.refine(g["lines3d"][g["scores"] < 0.01], views, float(g["img_res"][1]), float(g["img_res"][0]))
    close(rf, f["lines3d"], "refined vs twin")
    f = F.snap(g["lines3d"], 512)
    assert np.array_equal(sn["count"].cpu().numpy(), f["count"])


# ---- fuse ------------------------------------------------------------------------------------------------------------------------------------
def fuse_scene(n, ms, seed):
    """n lines in front of near-identity cameras; in every view about half of them have a detection within a fraction of a pixel (at a
    random position of the detection list, in a random orientation); the other detections lie far outside the image."""
    rng = np.random.default_rng(seed)
    lines = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2, 2)), rng.uniform(2, 3, (n, 2, 1))], -1).astype(np.float32)
    views = []
    for v, m in enumerate(ms):
        pose = np.eye(4, dtype=np.float32)
        pose[:3, 3] = [0.1 * v, -0.05 * v, 0.0]
        k = min(m, n // 2 + 1)
        det = np.zeros((m, 5), np.float32)
        if m:
            uv = F.project(K, pose, lines[rng.choice(n, k, replace=False)])
            flip = rng.random(k) < 0.5
            uv[flip] = uv[flip][:, [2, 3, 0, 1]]
            det[:k, :4] = uv + rng.normal(0, 0.2, (k, 4))
            det[k:, :4] = rng.uniform(1000, 2000, (m - k, 4))
            det[:, 4] = np.where(rng.random(m) < 0.4, rng.uniform(0.05, 0.4, m), rng.uniform(0.6, 0.99, m))
            det = det[rng.permutation(m)]
        views.append({"K": K, "pose": pose, "det": det})
    return lines, views


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("m", [0, 1, GT_CHUNK - 1, GT_CHUNK, GT_CHUNK + 1])
@pytest.mark.parametrize("n", [1, WG - 1, WG, WG + 1])
def test_fuse_shapes(n, m, V):
    for seed in range(20):                      # a draw whose decisions are clear in float64 (the twin alone decides)
        lines, views = fuse_scene(n, [m] * V, 1000 * n + 10 * m + V + 7919 * seed)
        if min(F.fuse(lines, views)["margin"], F.fuse(lines, views, by_label=True)["margin"]) > 1e-4:
            break
    else:
        raise AssertionError("no clear draw")
    for by_label in (False, True):
        r, f = check_fuse(lines, views, by_label)
    if m == 0:
        assert int(r["count"].sum()) == 0 and r["lines3d"].shape[0] == 0
    else:
        assert 1 <= f["count"].max() <= V


@pytest.mark.gpu
def test_fuse_ranks_past_one_scan_round():
    """Views of 1300 and 1100 detections, a few hundred of them matched at random positions: the workgroup of 1024 that ranks a view's
    matched detections (post_rank_kernel) takes a second round, and detections past index 1024 carry the count of the first."""
    for seed in range(20):
        lines, views = fuse_scene(600, [1300, 1100], 31 + 7919 * seed)
        if min(F.fuse(lines, views)["margin"], F.fuse(lines, views, by_label=True)["margin"]) > 1e-4:
            break
    else:
        raise AssertionError("no clear draw")
    for view in views:
        _, d1, d2 = F.view_costs(lines, view)
        idx, cost, bad, _ = F._best(d1, d2, 10.0)
        matched = np.unique(idx[~bad & (cost < 10.0)])
        assert (matched >= 1024).sum() >= 10 and (matched < 1024).sum() >= 100
    for by_label in (False, True):
        check_fuse(lines, views, by_label)


@pytest.mark.gpu
def test_fuse_cases():
    """A duplicated detection (lowest index wins), a NaN line, an empty view between two others, a line matched nowhere, both modes."""
    lines, views = fuse_scene(40, [30, 0, 30], 5)
    lines[7] = np.nan
    lines[11] = [[40.0, 40.0, 2.0], [41.0, 40.0, 2.0]]                 # projects far outside: matched in no view
    for v in (0, 2):
        det = views[v]["det"]
        near = np.nonzero(det[:, 0] < 500)[0]
        a, b = int(near[0]), int(near[1])
        det[b, :4] = det[a, :4]                                         # detection b duplicates detection a; their scores differ
        det[a, 4], det[b, 4] = 0.9, 0.1
    assert views[1]["det"].shape[0] == 0
    out = {}
    for by_label in (False, True):
        r, f = check_fuse(lines, views, by_label)
        assert f["count"][7] == 0 and f["count"][11] == 0 and not f["keep"][7] and not f["keep"][11]
        assert f["count"].max() == 2
        out[by_label] = f["score"]
    # a line lies on the duplicated pair: the twin's argmin (and so the score by label, 0.9 against 0.1) is the lower index
    det = views[0]["det"]
    a, b = np.nonzero((det[:, :4] == det[np.nonzero(det[:, 0] < 500)[0][0], :4]).all(1))[0]
    _, d1, d2 = F.view_costs(lines, views[0])
    with np.errstate(invalid="ignore"):
        on_dup = np.nonzero(np.nan_to_num(np.minimum(d1, d2)[:, a], nan=np.inf) < 10)[0]
    assert a < b and len(on_dup) >= 1 and not np.array_equal(out[False], out[True])


# ---- refine ----------------------------------------------------------------------------------------------------------------------------------
def refine_scene(n, seed=0):
    """Identity cameras (K exact in fp32): view 0 merges a group whose members are all reversed, a mixed group, a group of one and a line
    whose projection lies exactly on the image border; view 1's detections are far away; view 2 merges again."""
    rng = np.random.default_rng(seed)
    A = np.array([[-0.5, -0.3, 1.0], [0.4, 0.2, 1.0]])
    B = np.array([[0.3, -0.5, 1.0], [-0.2, 0.5, 1.0]])
    C = np.array([[-0.7, 0.4, 1.0], [-0.3, 0.6, 1.0]])
    border = np.array([[-1.0, -0.75, 1.0], [1.0, 0.75, 1.0]])          # projects to (0, 0, 128, 96) exactly
    outside = np.array([[-1.01, -0.7, 1.0], [0.9, 0.7, 1.0]])          # u1 < 0: close to its detection, but not possible
    jit = lambda s, k: s[None] + rng.normal(0, 0.004, (k, 2, 3))
    groupA = jit(A, 8)[:, [1, 0]]                                       # every member reversed against detection A
    groupB = jit(B, 5)
    groupB[::2] = groupB[::2][:, [1, 0]]
    rest = np.concatenate([rng.uniform(-0.9, 0.9, (n - 17, 2, 1)), rng.uniform(-0.7, 0.7, (n - 17, 2, 1)), np.ones((n - 17, 2, 1))], -1)
    rest[::3, :, 2] = -1.0                                              # behind the camera
    lines = np.concatenate([groupA, groupB, jit(C, 1), border[None], outside[None], border[None] + [[0.0, 0.001, 0.0], [0.0, -0.001, 0.0]], rest])
    lines = lines[rng.permutation(len(lines))].astype(np.float32)
    pose = np.eye(4, dtype=np.float32)
    pr = lambda s: F.project(K, pose, s[None])[0]
    d0 = np.array([[*pr(A), 0.9], [*pr(B), 0.8], [*pr(C), 0.7], [0, 0, 128, 96, 0.9], [*pr(outside), 0.9]], np.float32)
    d1 = np.concatenate([rng.uniform(1000, 2000, (6, 4)), np.full((6, 1), 0.9)], -1).astype(np.float32)
    d2 = np.array([[*pr(B)[[2, 3, 0, 1]], 0.9], [*pr(A), 0.9]], np.float32)
    return lines, [{"K": K, "pose": pose, "det": d} for d in (d0, d1, d2)]


def check_refine(lines, views):
    from neat_amd import post
    f = F.refine(lines, views, W, H)
    assert f["margin"] > 1e-4, f["margin"]
    r = post.refine(torch.tensor(lines).to(dev()), pack(views))
    close(r, f["lines3d"], "refined")
    got, src = r.cpu().numpy(), {l.tobytes() for l in np.asarray(lines, np.float32).reshape(-1, 2, 3)}
    copies = [i for i, l in enumerate(f["lines3d"]) if l.astype(np.float32).tobytes() in src and (l.astype(np.float32) == l).all()]
    for i in copies:                                                     # lines that no view touched are bit-equal copies
        assert got[i].tobytes() in src, i
    return r, f, copies


@pytest.mark.gpu
def test_refine_cases_n257():
    lines, views = refine_scene(257)
    r, f, copies = check_refine(lines, views)
    assert f["sizes"][0] < 257 and f["sizes"][1] == f["sizes"][0] and f["groups"] == 8      # the middle view changes nothing
    assert f["sizes"][0] == 257 - (8 + 5 + 1 + 2) + 4               # four groups: A, B, C and the two border lines; `outside` stays
    assert len(copies) == 257 - 15                                  # all but the members of A, B and the border pair (C's mean is C)
    # view 0 alone: the all-reversed group's mean is the mean of the reversed members, the group of one is the line itself
    r0, f0, _ = check_refine(lines, views[:1])
    assert np.allclose(f0["lines3d"][-4][0], [-0.5, -0.3, 1.0], atol=0.01)                  # detection A's orientation, not the members'


@pytest.mark.gpu
def test_refine_shrinks_to_one_line_and_handles_tiny_sets():
    from neat_amd import post
    rng = np.random.default_rng(1)
    A = np.array([[-0.5, -0.3, 1.0], [0.4, 0.2, 1.0]])
    lines = (A[None] + rng.normal(0, 0.004, (5, 2, 3))).astype(np.float32)
    pose = np.eye(4, dtype=np.float32)
    views = [{"K": K, "pose": pose, "det": np.array([[*F.project(K, pose, A[None])[0], 0.9]], np.float32)}]
    r, f, _ = check_refine(lines, views)
    assert r.shape == (1, 2, 3)
    r1, f1, _ = check_refine(lines[:1], views)                           # a group of one: the mean of one line
    assert torch.equal(r1.cpu(), torch.tensor(lines[:1]))
    empty = [{"K": K, "pose": pose, "det": np.zeros((0, 5), np.float32)}]
    assert torch.equal(post.refine(torch.tensor(lines).to(dev()), pack(empty)).cpu(), torch.tensor(lines))
    assert post.refine(torch.zeros(0, 2, 3, device=dev()), pack(views)).shape == (0, 2, 3)


@pytest.mark.gpu
def test_refine_walks_the_views_without_synchronising():
    from neat_amd import post
    lines, views = refine_scene(257)
    pv, dl = pack(views), torch.tensor(lines).to(dev())
    post.refine(dl, pv)                                                  # warm-up: library load, first launches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        buf, count = post.refine_device(dl, pv)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    close(buf[:int(count.item())], F.refine(lines, views, W, H)["lines3d"], "refined")


@pytest.mark.gpu
def test_refine_sdf_prefilter_against_get_sdf_vals():
    from neat_amd import networks, post, synth
    torch.manual_seed(0)
    model = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF).to(dev()).eval()
    rng = np.random.default_rng(2)
    lines = torch.tensor(rng.uniform(-0.6, 0.6, (300, 2, 3)).astype(np.float32)).to(dev())
    scores = torch.tensor(np.where(rng.random(300) < 0.2, 0.02, 0.001).astype(np.float32))
    t = torch.linspace(0, 1, 16, device=dev()).reshape(1, -1, 1)
    pts = lines[:, :1] + t * (lines[:, 1:] - lines[:, :1])
    with torch.no_grad():
        sdf = model.implicit_network.get_sdf_vals(pts.reshape(-1, 3)).reshape(300, 16).abs().max(-1)[0]
    sdf_max = float(sdf.median())
    pose = np.eye(4, dtype=np.float32)
    pv = pack([{"K": K, "pose": pose, "det": np.zeros((0, 5), np.float32)}] * 2)          # views that change nothing: the filter alone
    ok = sdf < sdf_max
    assert 0 < int(ok.sum()) < 300
    assert torch.equal(post.refine(lines, pv, model=model, sdf_max=sdf_max), lines[ok])
    ok2 = ok & (scores.to(dev()) < 0.01)
    assert int(ok2.sum()) < int(ok.sum())
    assert torch.equal(post.refine(lines, pv, model=model, sdf_max=sdf_max, scores=scores), lines[ok2])


# ---- snap ------------------------------------------------------------------------------------------------------------------------------------
def check_snap(lines, G, **kw):
    from neat_amd import post
    f = F.snap(lines, G, **kw)
    assert f["margin"] > 1e-4, f["margin"]
    r = post.snap(torch.tensor(np.asarray(lines, np.float32)).to(dev()), G, **kw)
    assert np.array_equal(r["junctions"].cpu().numpy(), f["junctions"])                    # float32 nodes: bit-equal
    assert np.array_equal(r["count"].cpu().numpy(), f["count"])
    assert np.array_equal(r["edges"].cpu().numpy(), f["edges"])
    assert np.array_equal(r["lines3d"].cpu().numpy(), f["lines3d"])
    assert r["edges"].dtype == torch.int32
    return r, f


@pytest.mark.gpu
@pytest.mark.parametrize("G", [2, 8, 512])
@pytest.mark.parametrize("n", [1, 300])
def test_snap_random_soup(G, n):
    rng = np.random.default_rng(G + n)
    verts = rng.uniform(-1, 1, (12, 3))
    lines = (verts[rng.integers(0, 12, (n, 2))] + rng.normal(0, 0.01, (n, 2, 3))).astype(np.float32)
    r, f = check_snap(lines, G)
    assert r["edges"].shape[0] == n
    check_snap(lines, G, unique=True)
    if n > 1 and G == 512:
        moved = np.sort(np.linalg.norm(f["junctions"][f["nearest"]] - lines.reshape(-1, 3), axis=1))
        q = len(moved) // 4
        k = q + 1 + int(np.argmax(np.diff(moved[q:3 * q])))             # the widest gap of the middle half: a clear --max-snap
        r2, f2 = check_snap(lines, G, max_snap=float((moved[k] + moved[k - 1]) / 2))
        assert 0 < r2["edges"].shape[0] < n


@pytest.mark.gpu
def test_snap_sorts_in_room_sized_by_the_count_alone():
    """The sort region is sort_scratch_bytes(2 n), whatever rocprim would ask for: at n = 1 that is 4 MiB for a sort of two int keys and
    one of a single 64-bit key, and at n = 300 with unique on both sorts run in it."""
    rng = np.random.default_rng(7)
    verts = rng.uniform(-1, 1, (12, 3))
    for n, kw in ((1, {}), (300, {"unique": True})):
        lines = (verts[rng.integers(0, 12, (n, 2))] + rng.normal(0, 0.01, (n, 2, 3))).astype(np.float32)
        check_snap(lines, 64, **kw)


@pytest.mark.gpu
def test_snap_cases():
    from neat_amd import post
    # end points on half-integer cells (G = 5 over [0, 4]: delta = 1): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    half = np.array([[[0, 0, 0], [4, 4, 4]], [[0.5, 1.5, 2.5], [3.5, 0.49999997, 2.5000002]]], np.float32)
    r, f = check_snap(half, 5)
    assert f["cells"][2].tolist() == [0, 2, 2] and f["cells"][3].tolist() == [4, 0, 3]
    # a plateau of two adjacent cells (both peaks), peaks on a face, an edge and a corner of the grid; --unique drops the degenerate
    # edges (i, i) and writes (min, max)
    r, f = check_snap(plateau_case(), 5)
    assert r["junctions"].cpu().tolist() == PLATEAU_JUNCTIONS and r["edges"].cpu().tolist() == [[0, 0], [1, 1], [4, 2], [3, 3]]
    twice = np.concatenate([plateau_case(), plateau_case()[2:3, [1, 0]]])                  # the edge (4, 2) again, as (2, 4)
    r, f = check_snap(twice, 5, unique=True)
    assert r["edges"].cpu().tolist() == [[2, 4]]
    # a zero-extent axis: cell 0, node = min
    flat = plateau_case().copy()
    flat[..., 1] = 0.375
    r, f = check_snap(flat, 5)
    assert (r["junctions"][:, 1] == 0.375).all()
    # one point twice: every axis has zero extent
    r, f = check_snap(np.full((1, 2, 3), 0.25, np.float32), 8)
    assert r["junctions"].cpu().tolist() == [[0.25, 0.25, 0.25]] and r["edges"].cpu().tolist() == [[0, 0]]
    # a grid beyond 1024 is refused before any launch
    dl = torch.tensor(half).to(dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(ValueError, match="refused"):
            post.snap(dl, 2048)
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_runs_each_subcommand_on_a_toy_run_directory(tmp_path, capsys):
    from neat_amd import conf as conf_mod, post, run_io
    from tests.util_run import synth_init_model, write_synth_run
    paths = write_synth_run(tmp_path, n_views=3)
    run, conf_path, model = paths["dir"], paths["conf"], synth_init_model()
    rng = np.random.default_rng(0)
    blocks = np.empty(2, dtype=object)                                   # per-view blocks, as -all.npz holds lines3d_all
    blocks[0], blocks[1] = (rng.uniform(-0.4, 0.4, (k, 2, 3)).astype(np.float32) for k in (30, 50))
    data = tmp_path / "latest-abcd1234-all.npz"
    np.savez(data, lines3d=blocks, scores=np.full(80, 0.001, np.float32))
    lines = torch.tensor(np.concatenate(list(blocks))).to(dev())
    common = ["--conf", str(conf_path), "--data", str(data), "--data_root", str(tmp_path / "data")]
    views = post.views_of(run_io.build_dataset(conf_mod.parse_file(conf_path), paths["data_root"], distance_threshold=1.0), dev())
    assert len(views["m"]) == 3 and min(views["m"]) > 0 and (views["height"], views["width"]) == (64.0, 64.0)

    assert post.main(["fuse"] + common + ["--dis", "400"]) == 0
    got = np.load(run / "wireframes" / "latest-abcd1234-all-fused.npz")
    lib = post.fuse(lines, views, dis=400.0)
    assert sorted(got.files) == ["count", "keep", "lines3d", "score"]
    assert np.array_equal(got["lines3d"], lib["lines3d"].cpu().numpy()) and np.array_equal(got["count"], lib["count"].cpu().numpy())
    assert "fuse" in capsys.readouterr().out

    assert post.main(["refine"] + common + ["--dis", "400", "--sdf-max", "10"]) == 0
    got = np.load(run / "wireframes" / "latest-abcd1234-all-ref.npz")
    out = capsys.readouterr().out
    assert "refine" in out and "skipped" not in out
    assert np.array_equal(got["lines3d"], post.refine(lines, views, dis=400.0, model=model.to(dev()), sdf_max=10.0,
                                                      scores=np.full(80, 0.001, np.float32)).cpu().numpy())
    assert post.main(["refine"] + common + ["--no-filter"]) == 0       # the file exists: kept
    assert "keeping" in capsys.readouterr().out
    assert post.main(["refine"] + common + ["--no-filter", "--overwrite"]) == 0
    assert "SDF pre-filter skipped" in capsys.readouterr().out

    assert post.main(["snap", "--data", str(data), "--grid", "64", "--unique"]) == 0
    got = np.load(tmp_path / "latest-abcd1234-all-snap.npz")
    lib = post.snap(lines, 64, unique=True)
    assert np.array_equal(got["junctions"], lib["junctions"].cpu().numpy()) and np.array_equal(got["edges"], lib["edges"].cpu().numpy())
    assert np.array_equal(got["lines3d"], got["junctions"][got["edges"]]) and got["edges"].dtype == np.int32
    assert "snap" in capsys.readouterr().out and len(got["count"]) == len(got["junctions"])
