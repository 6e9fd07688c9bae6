"""GPU tests of neat_amd.triangulate (csrc/kernels_triangulate.hpp) against the float64 definition tests/triangulate_f64.py.

The hypothesis list must be the reference's: the same (a, i, m, j) rows in the same order and the same bits in s_1, s_2, which are sums,
products and quotients in one order without contraction.  Scores carry an exp per term: 64 * 2^-52 relative (at most 32 slot terms, each
exp within an ulp of numpy's, and the additions).  tests/test_triangulate_math.py asserts that no decision of these scenes lies within
1e-9 of its threshold, so the kept estimates, picks, labels, members and views must be equal, and with equal picks the estimates and the
lines are equal bits.  Segment counts straddle the wavefront (63, 64, 65) and the pair kernel's tile (255, 256, 257)."""
import os

import numpy as np
import pytest
import torch

from tests import triangulate_f64 as T

SCORE_RTOL = 64 * 2.0 ** -52


def dev():
    return torch.device("cuda:0")


def on_device(name):
    seg, Ks, poses = T.scene(name)
    return [torch.tensor(s, device=dev()) for s in seg], Ks, poses              # the scenes are read-only: tensor() copies


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


# ---- 1. the hypothesis list -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 6])
@pytest.mark.parametrize("name", ["v2", "v3", "v7"])
def test_hypotheses_equal_the_reference(name, M):
    from neat_amd import triangulate
    want = T.reference(name, "hypotheses", neighbours=M)
    rows, depths, nb = triangulate.hypotheses(*on_device(name), neighbours=M)
    rows, depths = rows.cpu().numpy(), depths.cpu().numpy()
    print(f"{name} M = {M}: {rows.shape[0]} hypotheses (reference {want['rows'].shape[0]})")
    assert np.array_equal(nb.cpu().numpy(), want["neighbours"]) and nb.shape[1] == min(M, len(T.scene(name)[0]) - 1)
    assert rows.dtype == np.int32 and rows.shape == want["rows"].shape and np.array_equal(rows, want["rows"])
    assert depths.dtype == np.float64 and np.array_equal(depths.view(np.int64), want["depths"].view(np.int64))      # the same bits
    assert rows.shape[0] > 0


# ---- 2. the lines -------------------------------------------------------------------------------------------------------------------------------
def check_lines(got, want):
    assert np.array_equal(got["rows"], want["rows"]) and np.array_equal(got["depths"].view(np.int64), want["depths"].view(np.int64))
    rel = np.abs(got["score"] - want["score"]) / np.maximum(np.abs(want["score"]), 1e-300)
    print(f"{want['rows'].shape[0]} hypotheses, {int(want['kept'].sum())} estimates, {want['lines3d'].shape[0]} lines; "
          f"largest relative score difference {rel.max() if rel.size else 0.0:.3e} (bound {SCORE_RTOL:.3e})")
    assert (rel <= SCORE_RTOL).all()
    assert got["kept"].dtype == bool and np.array_equal(got["kept"], want["kept"])
    k = want["kept"]
    assert np.array_equal(got["estimate"][k].view(np.int64), want["estimate"][k].view(np.int64))          # equal picks: equal bits
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["members"], want["members"])
    assert np.array_equal(got["views"], want["views"]) and got["views"].dtype == np.int32
    assert got["lines3d"].shape == want["lines3d"].shape and np.array_equal(got["lines3d"].view(np.int64), want["lines3d"].view(np.int64))
    rel = np.abs(got["support"] - want["support"]) / np.maximum(np.abs(want["support"]), 1e-300)
    assert (rel <= SCORE_RTOL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixture", "v7"])
def test_lines_equal_the_reference(name):
    from neat_amd import triangulate
    want = T.reference(name)
    assert want["lines3d"].shape[0] > 0
    check_lines(host(triangulate.lines(*on_device(name))), want)


@pytest.mark.gpu
def test_capacity_edges():
    """A segment with more than 64 hypotheses (a wavefront strides over them) and a component of more than 64 members (a wavefront
    walks them in rounds): one line seen in 70 views, many partners in the six views around view 0."""
    from neat_amd import triangulate
    want = T.reference("capacity")
    per_segment = np.bincount(want["offsets"][want["rows"][:, 0]] + want["rows"][:, 1])
    assert per_segment.max() > 64 and np.bincount(want["labels"][want["labels"] >= 0]).max() > 64
    check_lines(host(triangulate.lines(*on_device("capacity"))), want)


@pytest.mark.gpu
def test_empty_and_tiny_inputs():
    from neat_amd import triangulate
    res = host(triangulate.lines([], np.zeros((0, 3, 3)), np.zeros((0, 4, 4)), device=dev()))
    assert res["lines3d"].shape == (0, 2, 3) and res["rows"].shape == (0, 4) and res["offsets"].tolist() == [0]
    for V, counts in ((1, [5]), (2, [5, 0]), (3, [0, 0, 0])):
        seg, Ks, poses = T.random_scene(counts, 5, seed=V)
        want = T.lines(seg, Ks, poses)
        got = host(triangulate.lines([torch.from_numpy(s).to(dev()) for s in seg], Ks, poses))
        assert got["lines3d"].shape == (0, 2, 3) and np.array_equal(got["rows"], want["rows"]) and (got["members"] == -1).all()
        assert got["estimate"].shape == (sum(counts), 2, 3) and not got["kept"].any()
    seg, Ks, poses = T.scene("f32")                                              # float32 segments, as the datasets give them
    want = T.reference("f32", "hypotheses")
    rows, depths, _ = triangulate.hypotheses([torch.from_numpy(s.astype(np.float32)).to(dev()) for s in seg], Ks, poses)
    assert want["rows"].shape[0] > 0 and np.array_equal(rows.cpu().numpy(), want["rows"]) and np.array_equal(depths.cpu().numpy(), want["depths"])


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_a_slice_equals_its_views_alone():
    from neat_amd import triangulate
    seg, Ks, poses = on_device("fixture")
    a, b = host(triangulate.lines(seg, Ks, poses)), host(triangulate.lines(seg, Ks, poses))
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    sl = slice(3, 17)
    alone = ([s.clone() for s in seg[sl]], np.array(Ks[sl]), np.array(poses[sl]))
    c, d = host(triangulate.lines(seg[sl], Ks[sl], poses[sl])), host(triangulate.lines(*alone))
    assert c["lines3d"].shape[0] > 0
    for key in c:
        assert c[key].tobytes() == d[key].tobytes(), key
    check_lines(c, T.reference("fixture_slice"))


# ---- 4. the command line --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_writes_a_file_the_other_tools_read(tmp_path, capsys):
    from neat_amd import evaluate, run_io, show, triangulate
    from tests.util_run import write_synth_run
    run = write_synth_run(tmp_path, n_views=8)
    args = ["--conf", run["conf"], "--data_root", run["data_root"], "--min-score", "0.5", "--min-views", "2", "--angle", "1"]
    assert triangulate.main(args) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    path = os.path.join(run["data_root"], "abc", "toy", "hawp-l3d.npz")
    assert line.startswith("8 views, 48 segments, ") and line.endswith(path) and os.path.exists(path)
    assert not [n for n in os.listdir(os.path.dirname(path)) if ".tmp" in n]
    with np.load(path) as data:
        assert sorted(data.files) == ["cameras", "lines3d", "support", "views"]
        N = data["lines3d"].shape[0]
        assert data["lines3d"].dtype == np.float64 and data["views"].dtype == np.int32 and data["views"].shape == (N,)
        assert data["support"].shape == (N,) and data["cameras"].shape == (8, 4, 4)
        stored = data["lines3d"]
    lines3d, scores = run_io.load_lines(path)
    assert lines3d.dtype == np.float64 and lines3d.shape == (N, 2, 3) and scores is None
    # the same answer as the library call on the dataset's views
    segments, Ks, poses = run_io.dataset_views(run_io.build_dataset(run_io.parse_conf(run["conf"]), run["data_root"]))
    res = triangulate.lines([s[:, :4].to(dev()) for s in segments], Ks, poses, min_score=0.5, min_views=2, angle_min=1.0)
    assert np.array_equal(res["lines3d"].cpu().numpy(), stored) and f"{N} lines" in line
    # --views and --out
    out = str(tmp_path / "sub.npz")
    assert triangulate.main(args + ["--views", "0:8:2", "--out", out]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith("4 views, 24 segments, ")
    assert np.load(out)["cameras"].shape == (4, 4, 4)
    # evaluate and show take the path
    assert evaluate.build_parser().parse_args(["abc", "--data", path, "--scan", str(tmp_path)]).data == path
    assert evaluate.build_parser().parse_args(["dtu-lines", "--data", path]).data == path
    assert show.build_parser().parse_args(["--data", path]).data == path
