"""CPU: the float64 restatement of the wireframe parsing (tests/parse_f64.py, steps 3-7 of neat_amd/parsing.py) reproduces what the
reference's initial_recon + visibility_checking recorded in golden G19 (tests/golden/make_parse_golden.py), for both junction settings."""
import numpy as np
import pytest

from tests import parse_f64 as F

THR = dict(line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0, ckview=5)


def golden_views(g):
    keys = ("lines3d", "lines2d", "l3d", "gt_lines_001", "gt_lines_005", "K", "pose")
    return [{k: g[f"v{v}_{k}"] for k in keys} for v in range(int(g["n_views"]))]


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_final_parsing")


@pytest.mark.parametrize("refine", [1, 0])
def test_restatement_reproduces_reference(g19, refine):
    views = golden_views(g19)
    f = F.distil(g19[f"junctions_refine{refine}"], views, **THR)
    assert f["margin"] > 1e-4
    for k in ("junctions3d_initial", "lines3d_all", "lines3d_wfi", "lines3d_wfi_checked"):
        ref = g19[f"r{refine}_{k}"]
        assert f[k].shape == ref.shape, k
        np.testing.assert_allclose(f[k], ref, rtol=0, atol=2e-6 * max(1.0, float(np.abs(ref).max())), err_msg=k)
    np.testing.assert_array_equal(f["graph_initial"], g19[f"r{refine}_graph_initial"])


def test_golden_covers_the_corner_cases(g19):
    views = golden_views(g19)
    f = F.distil(g19["junctions_refine1"], views, **THR)
    # a line whose two ends snap to one junction: the reference keeps the degenerate [j, j] segment
    assert any(i == j for i, j in f["edges"])
    diag = [e for e, (i, j) in enumerate(f["edges"]) if i == j]
    assert np.array_equal(g19["r1_lines3d_wfi"][diag[0], 0], g19["r1_lines3d_wfi"][diag[0], 1])
    # junctions come in the order of their first vote, not in index order
    assert f["order"] != sorted(f["order"])
    # both orientations match: rows n..2n (the reversed lines) carry labels too
    n = len(views[0]["l3d"])
    assert (f["labels"][0][:n] >= 0).any() and (f["labels"][0][n:] >= 0).any()
    # NaN rows never match, the score filter and the visibility check both drop something
    bad = np.isnan(views[0]["lines2d"]).any(1)
    assert bad.any() and (f["labels"][0][:n][bad] == -1).all() and (f["labels"][0][n:][bad] == -1).all()
    assert 0 < len(f["lines3d_wfi_checked"]) < len(f["lines3d_wfi"])
    assert len(f["lines3d_all"]) < sum(len(np.unique(l[l >= 0])) for l in f["labels"])
