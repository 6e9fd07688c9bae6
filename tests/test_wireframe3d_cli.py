"""`python -m neat_amd.triangulate --wireframe` on a generated box scene: the file it writes, what evaluate abc and show make of it, and
that the tool without the flag writes what it wrote before."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

KEYS = ["cameras", "degree", "edges", "junctions3d", "kind", "lines3d", "src", "support", "views", "votes"]


def test_parser_defaults_and_options():
    from neat_amd import triangulate
    opt = triangulate.build_parser().parse_args(["--conf", "x"])
    assert not opt.wireframe and (opt.end_frac, opt.reach, opt.min_votes, opt.junction_angle) == (0.2, 0.25, 2, 10.0)
    assert triangulate.WIREFRAME_DEFAULTS == {"end_frac": 0.2, "reach": 0.25, "min_votes": 2, "angle": 10.0}
    assert triangulate.out_path(opt, "d", "gt") == os.path.join("d", "gt-l3d.npz")
    opt = triangulate.build_parser().parse_args(["--conf", "x", "--wireframe", "--end-frac", "0.3", "--reach", "0.5", "--min-votes", "3", "--junction-angle", "20"])
    assert opt.wireframe and (opt.end_frac, opt.reach, opt.min_votes, opt.junction_angle) == (0.3, 0.5, 3, 20.0)
    assert triangulate.out_path(opt, "d", "gt") == os.path.join("d", "gt-wf3d.npz")
    with pytest.raises(RuntimeError, match="no CPU path"):
        triangulate.wireframe([torch.zeros(2, 2)], [torch.zeros(1, 2, dtype=torch.long)], np.eye(3)[None], np.eye(4)[None])


def test_dataset_graphs_are_the_views_segments():
    from neat_amd import run_io
    from neat_amd.wireframe import WireframeGraph

    class Views:
        def __init__(self):
            self.wf = WireframeGraph(torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), torch.ones(3), torch.tensor([[0, 1], [1, 2], [2, 0]]),
                                     torch.tensor([0.9, 0.01, 0.8]), 8, 8)

        def __len__(self):
            return 2

        def __getitem__(self, i):
            return i, {"wireframe": self.wf, "intrinsics": torch.eye(4), "pose": torch.eye(4)}, None

    vertices, edges, Ks, poses = run_io.dataset_graphs(Views())
    segments = run_io.dataset_views(Views())[0]
    assert len(vertices) == len(edges) == len(Ks) == len(poses) == 2 and edges[0].tolist() == [[0, 1], [2, 0]] and tuple(Ks[0].shape) == (3, 3)
    for v, e, s in zip(vertices, edges, segments):
        assert torch.equal(v[e].reshape(-1, 4), s[:, :4])


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.mark.gpu
def test_wireframe_file_and_the_tools_that_read_it(tmp_path, capsys):
    from neat_amd import evaluate, run_io, scenegen, show, synth, triangulate
    root = tmp_path / "data" / "box"
    assert scenegen.main(["--shape", "box", "--views", "6", "--res", "64", "--out", str(root)]) == 0
    conf = tmp_path / "box.conf"
    conf.write_text(synth.hocon_text({"train": {"expname": "box", "dataset_class": "datasets.blender_hawp_dataset.BlenderDataset"},
                                      "dataset": {"data_dir": "box", "img_res": [64, 64], "line_detector": "gt"}}))
    args = ["--conf", str(conf), "--data_root", str(tmp_path / "data")]
    capsys.readouterr()
    # 1. --wireframe writes the graph
    assert triangulate.main(args + ["--wireframe"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    path = str(root / "gt-wf3d.npz")
    assert line.endswith(path) and os.path.exists(path) and not [n for n in os.listdir(root) if ".tmp" in n]
    with np.load(path) as z:
        data = {k: z[k] for k in z.files}
    assert sorted(data) == KEYS
    J, E = data["junctions3d"].shape[0], data["edges"].shape[0]
    assert data["lines3d"].shape == (E, 2, 3) and data["lines3d"].dtype == np.float64 and data["edges"].dtype == np.int32 and data["cameras"].shape == (6, 4, 4)
    assert all(data[k].shape == (J,) and data[k].dtype == np.int32 for k in ("degree", "kind", "votes"))
    assert all(data[k].shape == (E,) for k in ("src", "views", "support"))
    assert np.array_equal(data["lines3d"], data["junctions3d"][data["edges"]])
    assert f"{J} vertices, {int((data['kind'] == 1).sum())} junctions, {E} edges, " in line and (data["kind"] == 1).sum() >= 4
    ends = np.unique(data["lines3d"].reshape(-1, 3), axis=0)
    assert ends.shape[0] == np.unique(data["edges"]).shape[0] <= J < 2 * E             # the file's unique end points are its vertices
    # the library call on the dataset's graphs gives the file
    ds = run_io.build_dataset(run_io.parse_conf(str(conf)), str(tmp_path / "data"))
    vertices, edges, Ks, poses = run_io.dataset_graphs(ds)
    res = triangulate.wireframe([v.to("cuda:0") for v in vertices], [e.to("cuda:0") for e in edges], Ks, poses)
    assert np.array_equal(res["junctions3d"].cpu().numpy(), data["junctions3d"]) and np.array_equal(res["edges3d"].cpu().numpy(), data["edges"])
    assert np.array_equal(res["support"].cpu().numpy()[data["src"]], data["support"])
    # 2. evaluate abc reads it: every true corner has a vertex of the file
    assert evaluate.main(["abc", "--data", path, "--scan", str(root), "--json"]) == 0
    found = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert found["junctions_recall"][-1] == 1.0, found                     # at the widest threshold
    # 3. without --wireframe the file is what triangulate.lines gives, as before
    assert triangulate.main(args) == 0
    capsys.readouterr()
    segments = run_io.dataset_views(ds)[0]
    plain = triangulate.lines([s[:, :4].to("cuda:0") for s in segments], Ks, poses)
    direct = str(tmp_path / "direct.npz")
    triangulate.write_lines(direct, plain["lines3d"].cpu().numpy(), plain["views"].cpu().numpy(), plain["support"].cpu().numpy(),
                            triangulate._np64(poses).reshape(-1, 4, 4))
    assert sha(str(root / "gt-l3d.npz")) == sha(direct) and sha(path) != sha(direct)
    # 4. show and the line soup's reader take the file
    lines3d, scores = run_io.load_lines(path)
    assert lines3d.shape == (E, 2, 3) and scores is None
    out = str(tmp_path / "frames")
    assert show.main(["--data", path, "--pose", "dtu", "--frames", "2", "--step", "90", "--width", "64", "--height", "48", "--save-path", out, "--no-gif"]) == 0
    assert sorted(n for _, _, names in os.walk(out) for n in names if n.endswith(".png")) == ["0000.png", "0001.png"]
