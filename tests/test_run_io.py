"""neat_amd.run_io and neat_amd.ply, the layer every tool stands on: load_lines on every file shape the tools meet (read with both .pth
keys), the mesh and scan readers, the atomic writers, --views and the cameras.  No device is touched."""
import numpy as np
import pytest
import torch

from neat_amd import run_io

KEYS = ("lines3d_wfi_checked", "lines3d_wfi")


@pytest.fixture(scope="module")
def blocks():
    rng = np.random.default_rng(0)
    return [rng.normal(size=(n, 2, 3)).astype(np.float32) for n in (3, 0, 5)]


def _object_array(parts):
    obj = np.empty(len(parts), dtype=object)
    for i, b in enumerate(parts):
        obj[i] = b
    return obj


@pytest.mark.parametrize("pth_key", KEYS)
def test_load_lines_reads_every_file_shape(tmp_path, blocks, pth_key):
    def read(name, **arrays):
        np.savez(tmp_path / name, **arrays)
        lines, scores = run_io.load_lines(str(tmp_path / name), pth_key=pth_key)
        assert lines.dtype == np.float64 and lines.ndim == 3 and lines.shape[1:] == (2, 3)
        return lines, scores

    # flat [n,2,3], float32 and float64: the cast to float64 is exact, pth_key does not matter to an .npz
    flat64 = np.concatenate(blocks).astype(np.float64) * (1.0 + 2.0 ** -40)
    for name, flat in (("flat32.npz", blocks[2]), ("flat64.npz", flat64)):
        lines, scores = read(name, lines3d=flat)
        assert scores is None and np.array_equal(lines, flat.astype(np.float64))
    # per-view blocks (one of them empty) are concatenated in order
    lines, scores = read("blocks.npz", lines3d=_object_array(blocks))
    assert scores is None and lines.shape == (8, 2, 3) and np.array_equal(lines, np.concatenate(blocks).astype(np.float64))
    # no view at all: no lines
    lines, scores = read("none.npz", lines3d=_object_array([]))
    assert scores is None and lines.shape == (0, 2, 3)
    # `scores` comes back as the file holds it; `score` (neat_amd.post fuse) is not `scores`
    s = np.linspace(0.0, 1.0, 5)
    lines, scores = read("scored.npz", lines3d=blocks[2], scores=s)
    assert np.array_equal(lines, blocks[2].astype(np.float64)) and scores.dtype == s.dtype and np.array_equal(scores, s)
    assert read("fused.npz", lines3d=blocks[2], score=s)[1] is None
    # a -neat.pth holding both keys gives the one asked for, and never scores
    held = {"lines3d_wfi_checked": blocks[0], "lines3d_wfi": blocks[2]}
    torch.save({k: torch.tensor(v) for k, v in held.items()}, str(tmp_path / "x-neat.pth"))
    lines, scores = run_io.load_lines(str(tmp_path / "x-neat.pth"), pth_key=pth_key)
    assert scores is None and lines.dtype == np.float64 and np.array_equal(lines, held[pth_key].astype(np.float64))
    assert np.array_equal(run_io.load_lines(str(tmp_path / "x-neat.pth"))[0], blocks[0].astype(np.float64))          # the default: the checked lines
    # a -neat.pth without the key asked for is an error, not another key's lines
    torch.save({k: torch.tensor(v) for k, v in held.items() if k != pth_key}, str(tmp_path / "y-neat.pth"))
    with pytest.raises(KeyError):
        run_io.load_lines(str(tmp_path / "y-neat.pth"), pth_key=pth_key)


# ------------------------------------------------------------------ the shared file, camera and --views helpers
def test_read_mesh_reads_back_what_the_writers_wrote(tmp_path):
    from neat_amd import ply
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, -2.0]])      # dyadic: exact in the PLY's float32 too
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    ply.write_ply(str(tmp_path / "m.ply"), verts, faces)
    ply.write_obj(str(tmp_path / "m.obj"), verts, faces)
    for name in ("m.ply", "m.obj"):
        v, f = ply.read_mesh(str(tmp_path / name))
        assert v.dtype == np.float64 and f.dtype == np.int32 and np.array_equal(v, verts) and np.array_equal(f, faces), name
    ply.write_ply_cloud(str(tmp_path / "cloud.ply"), verts)
    with pytest.raises(ValueError, match="no faces"):
        ply.read_mesh(str(tmp_path / "cloud.ply"))


def test_scan_ground_truth_readers(tmp_path):
    from neat_amd import raycast, scenegen
    (tmp_path / "lines.json").write_text('{"junctions": [[4, 8, 12], [0, 0, 0], [0.5, 1, -2]], "lines": [[0, 1], [2, 0]]}')
    (tmp_path / "offset_scale.txt").write_text("1 2 3 4\n")
    lines, scale = str(tmp_path / "lines.json"), str(tmp_path / "offset_scale.txt")
    J = [[4.0, 8.0, 12.0], [0.0, 0.0, 0.0], [0.5, 1.0, -2.0]]
    # the reader itself: what evaluate abc hands to abc_scores
    j, e = run_io.read_lines_json(lines)
    off = run_io.read_offset_scale(scale)
    assert j.dtype == np.float64 and np.array_equal(j, J) and e.dtype == np.int64 and np.array_equal(e, [[0, 1], [2, 0]])
    assert off.dtype == np.float64 and np.array_equal(off, [1.0, 2.0, 3.0, 4.0])
    j, e = scenegen.read_lines(lines)
    assert j.dtype == np.float64 and np.array_equal(j, J) and e.dtype == np.int32 and np.array_equal(e, [[0, 1], [2, 0]])
    # scale_mat = [x / 4 - (1, 2, 3)], so its inverse is 4 x + (4, 8, 12): powers of two, exact
    inv_scale, j32, e64 = raycast.scan_wireframe(str(tmp_path))
    assert inv_scale.dtype == np.float64 and np.array_equal(inv_scale, [[4.0, 0, 0, 4.0], [0, 4.0, 0, 8.0], [0, 0, 4.0, 12.0], [0, 0, 0, 1.0]])
    assert j32.dtype == np.float32 and np.array_equal(j32, [[20.0, 40.0, 60.0], [4.0, 8.0, 12.0], [6.0, 12.0, 4.0]])
    assert e64.dtype == np.int64 and np.array_equal(e64, [[0, 1], [2, 0]])
    x = raycast.to_mesh_frame(np.array([[4.0, 8.0, 12.0], [0.0, 0.0, 2.0]], dtype=np.float32), scale)
    assert x.dtype == np.float64 and np.array_equal(x, [[0.0, 0.0, 0.0], [-1.0, -2.0, -2.5]])


def test_replace_file(tmp_path):
    path = tmp_path / "new" / "deeper" / "a.npz"                       # the missing parents are made
    run_io.replace_file(str(path), lambda tmp: np.savez(tmp, x=np.arange(3)))
    assert np.array_equal(np.load(path)["x"], [0, 1, 2])
    assert sorted(p.name for p in path.parent.iterdir()) == ["a.npz"]                # np.savez added no suffix of its own: nothing is left over
    before = path.read_bytes()

    def fails(tmp):
        with open(tmp, "wb") as fh:
            fh.write(b"half")
        raise RuntimeError("the writer broke off")
    with pytest.raises(RuntimeError, match="broke off"):
        run_io.replace_file(str(path), fails)
    assert path.read_bytes() == before and not [p.name for p in path.parent.iterdir() if ".tmp" in p.name]
    run_io.replace_file(str(tmp_path / "plain"), lambda tmp: open(tmp, "w").close())          # a name without a suffix
    assert (tmp_path / "plain").exists() and not [p.name for p in tmp_path.iterdir() if ".tmp" in p.name]


def test_write_png_keeps_an_existing_file(tmp_path):
    from PIL import Image
    path = tmp_path / "sub" / "a.png"
    rgb = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert run_io.write_png(str(path), rgb) is True and np.array_equal(np.asarray(Image.open(path)), rgb)
    assert run_io.write_png(str(path), rgb[::-1], overwrite=False) is False and np.array_equal(np.asarray(Image.open(path)), rgb)
    assert run_io.write_png(str(path), rgb[::-1]) is True and np.array_equal(np.asarray(Image.open(path)), rgb[::-1])
    assert run_io.write_png(str(path), torch.from_numpy(rgb.copy())) is True and np.array_equal(np.asarray(Image.open(path)), rgb)      # a tensor
    assert sorted(p.name for p in path.parent.iterdir()) == ["a.png"]


def test_skip_existing(tmp_path, capsys):
    path = tmp_path / "out.npz"
    assert run_io.skip_existing(str(path), False) is False and capsys.readouterr().out == ""
    path.write_bytes(b"kept")
    assert run_io.skip_existing(str(path), True) is False and capsys.readouterr().out == ""
    assert run_io.skip_existing(str(path), False) is True
    assert capsys.readouterr().out == "exists: {} (--overwrite to replace it)\n".format(path)


def test_parse_views():
    assert list(run_io.parse_views(None, 5)) == [0, 1, 2, 3, 4]
    assert list(run_io.parse_views("1:3", 5)) == [1, 2]
    assert list(run_io.parse_views(":2", 5)) == [0, 1]
    assert list(run_io.parse_views("3:", 5)) == [3, 4]
    assert list(run_io.parse_views("2:99", 5)) == [2, 3, 4]
    for bad in ("3", "1:2:3", "a:b", "0:4:2"):
        with pytest.raises(ValueError):
            run_io.parse_views(bad, 5)
    with pytest.raises(ValueError, match="^--views 0:4:2: expected a:b$"):
        run_io.parse_views("0:4:2", 5)
    assert list(run_io.parse_views(None, 5, step=True)) == [0, 1, 2, 3, 4]
    assert list(run_io.parse_views("1:3", 5, step=True)) == [1, 2]
    assert list(run_io.parse_views(":2", 5, step=True)) == [0, 1]
    assert list(run_io.parse_views("0:100:4", 100, step=True)) == list(range(0, 100, 4))
    assert list(run_io.parse_views("::2", 5, step=True)) == [0, 2, 4]
    assert list(run_io.parse_views("2:99:", 5, step=True)) == [2, 3, 4]
    for bad in ("3", "1:2:3:4", "a:b", "0:4:0", "0:4:-1"):
        with pytest.raises(ValueError):
            run_io.parse_views(bad, 5, step=True)


def test_dataset_cams_and_camera_centres():
    from neat_amd.synth import look_at_pose

    class Poses:                                                       # what dataset_cams reads of a dataset: pose_all and its length
        pose_all = [torch.from_numpy(look_at_pose(c).astype(np.float32)) for c in ((2.0, 0.5, 1.0), (-1.0, 1.5, 0.25), (0.5, -2.0, -1.0))]

        def __len__(self):
            return len(self.pose_all)
    stack = np.stack([p.numpy().astype(np.float64) for p in Poses.pose_all])
    cams = run_io.dataset_cams(Poses())
    assert cams.dtype == np.float64 and cams.shape == (3, 4, 4) and np.array_equal(cams, np.linalg.inv(stack))
    centres = run_io.camera_centres(cams)
    # -R^T t, each component the sum of its three products in order (a BLAS product may fuse them and differ in the last bit)
    want = np.array([[-((c[0, i] * c[0, 3] + c[1, i] * c[1, 3]) + c[2, i] * c[2, 3]) for i in range(3)] for c in cams])
    assert centres.dtype == np.float64 and centres.shape == (3, 3) and np.array_equal(centres, want)
