"""CPU checks of the post-processing rules (tests/post_f64.py) against what the reference's fusion.py, refinement.py and nms.py recorded
(tests/golden/g21_postprocess.npz), of the literal float32 arithmetic of snap, and of the ABI of the new entry points."""
import os
import re

import numpy as np
import torch

from tests import post_f64 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_views(g):
    return [{k: g[f"v{v}_{k}"] for k in ("K", "pose", "det")} for v in range(int(g["n_views"]))]


def test_twin_reproduces_the_reference_scripts(golden):
    g = golden("g21_postprocess")
    views = golden_views(g)
    H, W = g["img_res"]
    fr = F.fuse(g["lines3d"], views)
    assert fr["margin"] > 1e-3
    assert fr["lines3d"].shape == g["ref_fused"].shape and np.abs(fr["lines3d"] - g["ref_fused"]).max() < 1e-6
    assert np.array_equal(g["lines3d"][fr["keep"]], g["ref_fused"])              # kept lines are copies
    assert (fr["count"] == 0).any() and 0 < fr["keep"].sum() < len(fr["keep"])
    rf = F.refine(g["lines3d"][g["scores"] < 0.01], views, W, H)                 # the stub SDF is 0: the pre-filter is the score test
    assert rf["margin"] > 1e-3 and rf["groups"] >= 3
    assert rf["lines3d"].shape == g["ref_refined"].shape and np.abs(rf["lines3d"] - g["ref_refined"]).max() < 1e-5
    sn = F.snap(g["lines3d"], 512)
    assert sn["margin"] > 1e-3
    assert np.array_equal(sn["junctions"], g["ref_snap_junctions"])              # float32 nodes, bit for bit
    assert np.array_equal(sn["edges"], g["ref_snap_edges"])


def test_fuse_enumerate_rank_differs_from_label(golden):
    """One view, three detections with scores (0.9, 0.1, 0.9); lines sit on detections 0 and 2 only.  The matched labels are {0, 2}: the
    reference's enumerate gives label 2 the score of detection 1 (rank 1), so it drops the second line; by label both stay."""
    K = np.array([[80.0, 0, 32], [0, 80.0, 24], [0, 0, 1]])
    pose = np.eye(4)
    seg = np.array([[[-0.2, 0.0, 2.0], [0.0, 0.1, 2.0]], [[0.1, -0.1, 2.0], [0.3, 0.1, 2.0]]])
    uv = F.project(K, pose, seg)
    det = np.array([[*uv[0], 0.9], [5.0, 5.0, 9.0, 9.0, 0.1], [*uv[1][[2, 3, 0, 1]], 0.9]])
    views = [{"K": K, "pose": pose, "det": det}]
    rank, label = F.fuse(seg, views), F.fuse(seg, views, by_label=True)
    assert rank["count"].tolist() == [1, 1] and label["count"].tolist() == [1, 1]
    assert np.allclose(rank["score"], [0.9, 0.1]) and np.allclose(label["score"], [0.9, 0.9])
    assert rank["keep"].tolist() == [True, False] and label["keep"].tolist() == [True, True]


def test_snap_cells_round_half_to_even_and_linspace_nodes():
    # G = 5 over [0, 4]: delta = 1, so the coordinate is the cell quotient itself
    pts = np.array([[0, 0, 0], [4, 4, 4], [0.5, 1.5, 2.5], [3.5, 0.49999997, 2.5000002]], np.float32)
    cells, lo, hi, delta = F.cells_f32(pts, 5)
    assert delta.tolist() == [1.0, 1.0, 1.0]
    assert cells[2].tolist() == [0, 2, 2] and cells[3].tolist() == [4, 0, 3]
    literal = np.array(((pts - lo[None]) / ((hi - lo) / 4)).round(), dtype=np.int64)        # nms.py :172-175
    assert np.array_equal(cells, literal)
    # a zero-extent axis: cell 0 (the literal divides by zero there)
    flat, _, _, d0 = F.cells_f32(np.array([[0, 1, 5], [2, 1, 7]], np.float32), 8)
    assert d0[1] == 0 and flat[:, 1].tolist() == [0, 0] and flat[:, 0].tolist() == [0, 7]
    rng = np.random.default_rng(3)
    for G in (2, 3, 8, 9, 17, 511, 512, 1024):
        for _ in range(20):
            a = np.float32(rng.normal())
            b = np.float32(a + abs(rng.normal()) * 3)
            assert np.array_equal(F.linspace_f32(a, b, G), torch.linspace(a, b, G).numpy()), G
    assert np.array_equal(F.linspace_f32(1.5, 1.5, 8), np.full(8, 1.5, np.float32))


def test_snap_plateau_and_peaks_on_the_grid_boundary():
    lines = plateau_case()
    sn = F.snap(lines, 5)
    assert sn["junctions"].tolist() == PLATEAU_JUNCTIONS and sn["count"].tolist() == [2, 2, 1, 2, 1]
    assert sn["edges"].tolist() == [[0, 0], [1, 1], [4, 2], [3, 3]]
    assert F.snap(lines, 5, unique=True)["edges"].tolist() == [[2, 4]]


# G = 5 over the unit cube (delta = 1/4): the corner cell (0,0,0) and its neighbour (1,0,0) hold two end points each (a plateau: both
# are peaks), the face cell (4,2,2) one, the edge cell (4,4,2) two and the far corner (4,4,4) one; no other two cells are adjacent
PLATEAU_JUNCTIONS = [[0, 0, 0], [0.25, 0, 0], [1, 0.5, 0.5], [1, 1, 0.5], [1, 1, 1]]


def plateau_case():
    pts = [[0, 0, 0]] * 2 + [[0.25, 0, 0]] * 2 + [[1, 1, 1], [1, 0.5, 0.5]] + [[1, 1, 0.5]] * 2
    return np.array(pts, np.float32).reshape(-1, 2, 3)


def test_new_symbols_are_declared_bound_and_additive():
    from neat_amd import _lib
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ("neat_post_fuse_ws_bytes", "neat_post_fuse", "neat_post_select", "neat_post_refine_ws_bytes", "neat_post_refine_view",
             "neat_post_snap_ws_bytes", "neat_post_snap")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert n in _lib.exported_symbols(), n
    assert _lib.ABI_VERSION == 15
    lib = _lib.lib()
    assert lib.neat_abi_version() == 15
    # host-side refusals, before any launch (no device here): a grid beyond 1024 has no workspace and the call returns -1
    assert lib.neat_post_snap_ws_bytes(10, 2048) == 0 and lib.neat_post_snap_ws_bytes(10, 1) == 0
    assert lib.neat_post_snap(None, 10, 2048, -1.0, 0, None, None, None, None, None, None, None) == -1
    assert lib.neat_post_fuse_ws_bytes(10, 70000, 5) == 0            # views beyond the y dimension of a launch
    assert lib.neat_post_fuse_ws_bytes(256, 3, 100) > 256 * 3 * 4
    assert lib.neat_post_refine_ws_bytes(257, 40) > 2 * 257 * 4
