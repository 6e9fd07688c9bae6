"""`python -m neat_amd.detect --junctions`: the parser and the refusals on the CPU; on the device the files it writes, what the dataset
reads from them, `--from` on another detector's files, and one training step on the built wireframes."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz")


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_options():
    from neat_amd import detect
    opt = detect.build_parser().parse_args(["--scan", "x"])
    assert not opt.junctions and opt.source is None and not opt.no_t and opt.name == "lsd"
    assert (opt.gap, opt.gap_frac, opt.angle) == (4.0, 0.4, 10.0) == tuple(detect.JUNCTION_DEFAULTS[k] for k in ("gap", "frac", "angle"))
    opt = detect.build_parser().parse_args(["--scan", "x", "--junctions", "--gap", "3", "--gap-frac", "0.25", "--angle", "15", "--no-t", "--from", "hawp",
                                            "--name", "hawpj"])
    assert opt.junctions and opt.no_t and (opt.gap, opt.gap_frac, opt.angle, opt.source, opt.name) == (3.0, 0.25, 15.0, "hawp", "hawpj")


def test_refusals_need_no_device(tmp_path, capsys):
    from neat_amd import detect
    (tmp_path / "images").mkdir()
    (tmp_path / "lsd").mkdir()
    scan = str(tmp_path)
    assert detect.main(["--scan", scan, "--device", "cpu", "--junctions"]) == 2
    assert "device only" in capsys.readouterr().err
    for args, word in ((["--from", "lsd"], "--junctions"), (["--junctions", "--from", "lsd"], "one folder"), (["--junctions", "--gap", "0"], "gap"),
                       (["--junctions", "--gap-frac", "0.5"], "frac"), (["--junctions", "--angle", "0"], "angle"),
                       (["--junctions", "--from", "nowhere", "--name", "out"], "nowhere")):
        assert detect.main(["--scan", scan] + args) == 2, args
        assert word in capsys.readouterr().err, args
    assert not (tmp_path / "out").exists()
    with pytest.raises(RuntimeError, match="no CPU path"):
        detect.junctions(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), [0, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        detect.wireframes(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), [0, 2], 8, 8)


def test_load_json_ignores_the_extra_keys(tmp_path):
    from neat_amd import run_io
    from neat_amd.wireframe import WireframeGraph
    wf = WireframeGraph(torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), torch.tensor([0.5, 0.6, 0.7]), torch.tensor([[0, 1], [1, 2]]),
                        torch.tensor([0.9, 0.8]), 64, 48)
    path = str(tmp_path / "a" / "v.json")
    run_io.write_wireframe_json(path, wf, {"vertices-degree": [1, 2, 1], "vertices-kind": [0, 1, 2]})
    doc = json.load(open(path))
    assert doc["vertices-degree"] == [1, 2, 1] and doc["vertices-kind"] == [0, 1, 2]
    back = WireframeGraph.load_json(path)
    assert torch.equal(back.vertices, wf.vertices) and torch.equal(back.edges, wf.edges) and torch.equal(back.weights, wf.weights)
    assert (back.frame_width, back.frame_height) == (64, 48) and not hasattr(back, "kind")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def folder_bytes(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


@pytest.mark.gpu
def test_files_dataset_from_and_one_training_step(tmp_path, capsys):
    from neat_amd import detect, run_io, synth
    from neat_amd.datasets import BlenderDataset
    from neat_amd.train import Trainer
    from tests import junctions2d_f64 as J
    dev = torch.device("cuda:0")
    root = str(tmp_path / "abc" / "scene")
    res = synth.write_scene_fixture(FIXTURE, root)
    # 1. without --junctions: what detect.lines and to_wireframe give, byte for byte
    assert detect.main(["--scan", root, "--batch", "3"]) == 0
    plain = capsys.readouterr().out.strip().splitlines()[-1]
    images = torch.from_numpy(np.load(FIXTURE)["images"]).to(dev)
    lines, _, nfa, _, _, off = detect.lines(images)
    off = off.cpu().tolist()
    names = [f"image_{i:04d}.json" for i in range(8)]
    soup = folder_bytes(os.path.join(root, "lsd"))
    assert sorted(soup) == names and plain.startswith(f"8 views, {off[-1]} segments, ") and "vertices" not in plain
    for v, name in enumerate(names):
        wf = detect.to_wireframe(lines[off[v]:off[v + 1]], nfa[off[v]:off[v + 1]], images.shape[1], images.shape[2])
        run_io.write_wireframe_json(str(tmp_path / "direct" / name), wf, {"edges-nfa": nfa[off[v]:off[v + 1]].cpu().tolist()})
        assert wf.vertices.shape[0] == 2 * (off[v + 1] - off[v])
    assert folder_bytes(str(tmp_path / "direct")) == soup
    # 2. with --junctions: the library's graphs, which are the reference's
    assert detect.main(["--scan", root, "--name", "lsdj", "--junctions", "--batch", "5"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    built = folder_bytes(os.path.join(root, "lsdj"))
    weight = detect.nfa_weight(nfa).double().numpy()
    want = J.build(lines.float().double().cpu().numpy(), off, weight)
    nv, ne = want["vertices"].shape[0], want["edges"].shape[0]
    assert sorted(built) == names and line.startswith(f"8 views, {off[-1]} segments, {nv} vertices, {ne} edges, "), line
    assert folder_bytes(os.path.join(root, "lsd")) == soup and nv < 2 * off[-1]
    for v, name in enumerate(names):
        doc, part = json.loads(built[name]), J.view_of(want, v)
        assert sorted(doc) == ["edges", "edges-weights", "height", "vertices", "vertices-degree", "vertices-kind", "vertices-score", "width"]
        assert np.array_equal(np.array(doc["vertices"], np.float32).reshape(-1, 2), part["vertices"].astype(np.float32))
        assert doc["vertices-degree"] == part["degree"].tolist() and doc["vertices-kind"] == part["kind"].tolist()
        assert doc["edges"] == part["edges"].tolist() and np.array_equal(np.array(doc["edges-weights"], np.float32), part["eweight"].astype(np.float32))
    # 3. the dataset reads them: the junctions are the built vertices
    ds = BlenderDataset("abc/scene", [res, res], line_detector="lsdj", data_root=str(tmp_path))
    assert len(ds) == 8
    for v in range(8):
        assert ds.wireframes[v].vertices.shape == (want["voff"][v + 1] - want["voff"][v], 2)
        assert ds.lines[v].shape[0] == int((J.view_of(want, v)["eweight"].astype(np.float32) > 0.05).sum())
    # 4. --from on the soup's files gives the same files; a slice of the views gives its files
    assert detect.main(["--scan", root, "--name", "fromj", "--junctions", "--from", "lsd", "--batch", "8"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith(f"8 views, {off[-1]} segments, {nv} vertices, {ne} edges, ")
    assert folder_bytes(os.path.join(root, "fromj")) == built
    assert detect.main(["--scan", root, "--name", "part", "--junctions", "--from", "lsd", "--views", "2:4", "--no-t", "--gap", "3"]) == 0
    capsys.readouterr()
    assert sorted(os.listdir(os.path.join(root, "part"))) == names[2:4]
    # 5. one training step of the default build on these wireframes
    np.random.seed(0)
    torch.manual_seed(0)
    _, sample, gt = ds.device_batches(dev).batch(0, 128)
    assert sample["wireframe"][0].vertices.shape[0] == want["voff"][1]
    _, losses = Trainer(device="cuda:0").step(sample, gt)
    torch.cuda.synchronize()
    assert np.isfinite(float(losses["loss"]))
