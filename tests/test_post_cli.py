"""CPU checks of `python -m neat_amd.post`: argument parsing, output file names, --overwrite, and that the files it writes are files the
loader of neat_amd.evaluate and neat_amd.show (run_io.load_lines) accepts.  No device is touched."""
import os

import numpy as np
import pytest

from neat_amd import post


def parse(*argv):
    return post.build_parser().parse_args(list(argv))


def test_arguments_and_defaults():
    o = parse("fuse", "--conf", "run/runconf.conf", "--data", "w/latest-abcd1234-all.npz")
    assert (o.dis, o.keep, o.score_by_label, o.checkpoint, o.gpu, o.overwrite, o.data_root) == (10.0, 0.5, False, "latest", 0, False, "../data")
    assert parse("fuse", "--conf", "c", "--data", "d.npz", "--score-by-label").score_by_label is True
    o = parse("refine", "--conf", "c", "--data", "d.npz", "--sdf-max", "0.02", "--score-max", "0.03")
    assert (o.dis, o.sdf_max, o.score_max, o.no_filter) == (10.0, 0.02, 0.03, False)
    o = parse("snap", "--data", "d.npz")
    assert (o.grid, o.max_snap, o.unique, o.conf) == (512, None, False, None)
    o = parse("snap", "--data", "d.npz", "--grid", "64", "--max-snap", "0.05", "--unique")
    assert (o.grid, o.max_snap, o.unique) == (64, 0.05, True)
    for argv in (["fuse", "--data", "d.npz"], ["refine", "--data", "d.npz"], ["snap"], []):      # fuse / refine need --conf, all need --data
        with pytest.raises(SystemExit):
            parse(*argv)


def test_output_file_names(tmp_path):
    run = tmp_path / "exps" / "run"
    data = tmp_path / "in" / "latest-abcd1234-all.npz"
    o = parse("fuse", "--conf", str(run / "runconf.conf"), "--data", str(data))
    assert post.out_path(o) == str(run / "wireframes" / "latest-abcd1234-all-fused.npz")
    o = parse("refine", "--conf", str(run / "runconf.conf"), "--data", str(data), "--expdir", str(tmp_path / "other"))
    assert post.out_path(o) == str(tmp_path / "other" / "wireframes" / "latest-abcd1234-all-ref.npz")
    o = parse("snap", "--data", str(data))
    assert post.out_path(o) == str(tmp_path / "in" / "latest-abcd1234-all-snap.npz")
    o = parse("snap", "--data", str(data), "--expdir", str(run))
    assert post.out_path(o) == str(run / "wireframes" / "latest-abcd1234-all-snap.npz")


def test_existing_output_is_kept_without_overwrite(tmp_path, capsys):
    data = tmp_path / "soup.npz"
    np.savez(data, lines3d=np.zeros((2, 2, 3), np.float32))
    out = tmp_path / "soup-snap.npz"
    out.write_bytes(b"earlier result")
    assert post.main(["snap", "--data", str(data)]) == 0                     # returns before any device call
    assert "keeping" in capsys.readouterr().out and out.read_bytes() == b"earlier result"
    # a refused grid is reported before any device call, too (--overwrite gets past the existing file)
    assert post.main(["snap", "--data", str(data), "--overwrite", "--grid", "2048"]) == 2
    assert "refused" in capsys.readouterr().err and out.read_bytes() == b"earlier result"


def test_snap_help_needs_no_device(capsys):
    with pytest.raises(SystemExit) as e:
        parse("snap", "--help")
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--grid" in text and "--max-snap" in text and "--unique" in text


def test_written_files_are_read_by_evaluate_and_show(tmp_path):
    from neat_amd import run_io
    lines = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    fused = tmp_path / "x-fused.npz"
    np.savez(fused, lines3d=lines[:3], score=np.ones(4, np.float32), count=np.ones(4, np.int32), keep=np.array([1, 1, 1, 0], bool))
    ref = tmp_path / "x-ref.npz"
    np.savez(ref, lines3d=lines[:2])
    snap = tmp_path / "x-snap.npz"
    junc = lines.reshape(-1, 3)[:3]
    edges = np.array([[0, 1], [1, 2]], np.int32)
    np.savez(snap, junctions=junc, edges=edges, lines3d=junc[edges], count=np.ones(3, np.int32))
    for path, n in ((fused, 3), (ref, 2), (snap, 2)):
        got, scores = run_io.load_lines(str(path))
        assert scores is None and np.asarray(got).shape == (n, 2, 3)          # `score` is not `scores`: dtu-lines does not filter by it
        assert run_io.load_lines(str(path), pth_key="lines3d_wfi")[0].shape == (n, 2, 3)
