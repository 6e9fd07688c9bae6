"""The command line of neat_amd.creases: the arguments it refuses (host only), and one run on the device whose lines.json scenegen takes
as its --lines."""
import json
import os

import pytest


def test_arguments():
    from neat_amd import creases
    opt = creases.parse_args(["--mesh", "m.obj", "--out", "lines.json"])
    assert (opt.angle, opt.turn, opt.deviation, opt.no_boundary, opt.drop_curved, opt.min_len, opt.ply, opt.gpu, opt.overwrite) == \
        (30.0, 1.0, 1e-6, False, False, 0.0, None, 0, False)
    opt = creases.parse_args(["--mesh", "m.PLY", "--out", "l.json", "--angle", "45", "--turn", "2", "--deviation", "1e-4", "--no-boundary",
                              "--drop-curved", "--min-len", "0.01", "--ply", "c.ply", "--gpu", "1", "--overwrite"])
    assert (opt.mesh, opt.angle, opt.turn, opt.deviation, opt.no_boundary, opt.drop_curved, opt.min_len, opt.ply, opt.gpu, opt.overwrite) == \
        ("m.PLY", 45.0, 2.0, 1e-4, True, True, 0.01, "c.ply", 1, True)
    ok = ["--mesh", "m.obj", "--out", "l.json"]
    for bad in (["--out", "l.json"], ["--mesh", "m.obj"], ["--mesh", "m.stl", "--out", "l.json"], ok + ["--angle", "0"], ok + ["--angle", "180"],
                ok + ["--angle", "-30"], ok + ["--angle", "nan"], ok + ["--turn", "-1"], ok + ["--deviation", "-1e-6"], ok + ["--deviation", "inf"],
                ok + ["--min-len", "-0.5"], ok + ["--ply", "c.obj"], ok + ["--gpu", "-1"]):
        with pytest.raises(SystemExit):
            creases.parse_args(bad)


def test_an_existing_output_is_left_alone(tmp_path, capsys):
    from neat_amd import creases
    out = tmp_path / "lines.json"
    out.write_bytes(b"{\"junctions\": [], \"lines\": []}  \n")
    before = out.read_bytes()
    assert creases.main(["--mesh", str(tmp_path / "absent.obj"), "--out", str(out)]) == 0      # the mesh is not even opened
    assert capsys.readouterr().out.startswith("exists: ")
    assert out.read_bytes() == before and os.listdir(tmp_path) == ["lines.json"]


@pytest.mark.gpu
def test_cli_output_is_scenegens_lines(tmp_path, capsys):
    from neat_amd import creases, ply, scenegen
    verts, faces, junctions, _ = scenegen.shapes["lblock"]
    verts, faces = scenegen.subdivide(verts, faces, 1)
    mesh, lines, tubes, scene = (str(tmp_path / n) for n in ("lblock.obj", "lines.json", "creases.ply", "scene"))
    scenegen.write_obj(mesh, verts, faces)
    assert creases.main(["--mesh", mesh, "--out", lines, "--ply", tubes]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith(
        lines + ": 18 lines (0 curved) between 12 junctions from 80 triangles: 36 creases, 0 boundary and 0 non-manifold edges in 18 chains; ")
    doc = json.load(open(lines))
    assert len(doc["lines"]) == 18 and len(doc["junctions"]) == 12 and doc["kind"] == [0] * 18 and doc["curved"] == [False] * 18
    assert {tuple(p) for p in doc["junctions"]} == {tuple(float(x) for x in p) for p in junctions}
    tube = ply.read_ply(tubes)
    assert tube["points"].shape == (18 * 6, 3) and tube["faces"].shape == (18 * 8, 3)
    assert scenegen.main(["--mesh", mesh, "--lines", lines, "--out", scene, "--views", "2", "--res", "32", "--ss", "1"]) == 0
    made = json.load(open(scenegen.scene_paths(scene, 2)["lines"]))
    assert len(made["lines"]) == 18 and len(made["junctions"]) == 12
    assert not [n for _, _, names in os.walk(tmp_path) for n in names if ".tmp" in n]
