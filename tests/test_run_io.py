"""run_io.load_lines, the one reader of wireframe files: every file shape the tools meet, read with both .pth keys.  No device is touched."""
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
