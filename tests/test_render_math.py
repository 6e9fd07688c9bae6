"""CPU checks of neat_amd.render's host side and of its numpy restatement (tests/render_f64.py): the make_grid layout against hand-written
sizes and offsets, the PSNR of two constant images, the byte rule on the values where numpy's cast is defined, the CSV text against
pandas, the pixel order against the dataset's."""
import io
import math

import numpy as np
import pytest
import torch

from neat_amd import render
from tests import render_f64 as R


def test_grid_layout_has_the_hand_written_sizes_and_offsets():
    rng = np.random.default_rng(0)
    one = rng.integers(1, 255, (1, 5, 7, 3), dtype=np.uint8)
    assert R.make_grid(one, 8).shape == (5, 7, 3) and np.array_equal(R.make_grid(one, 8), one[0])           # a single image: unpadded
    assert render.grid_shape(1, 5, 7, 8) == (5, 7)
    two = rng.integers(1, 255, (2, 5, 7, 3), dtype=np.uint8)
    g = R.make_grid(two, 1)
    assert g.shape == (16, 11, 3) and render.grid_shape(2, 5, 7, 1) == (16, 11)
    assert np.array_equal(g[2:7, 2:9], two[0]) and np.array_equal(g[9:14, 2:9], two[1])
    mask = np.ones((16, 11), dtype=bool)
    mask[2:7, 2:9] = mask[9:14, 2:9] = False
    assert not g[mask].any()                                                                                   # the padding is zeros
    three = rng.integers(1, 255, (3, 5, 7, 3), dtype=np.uint8)
    g = R.make_grid(three, 2)
    assert g.shape == (16, 20, 3) and render.grid_shape(3, 5, 7, 2) == (16, 20)
    assert np.array_equal(g[2:7, 2:9], three[0]) and np.array_equal(g[2:7, 11:18], three[1]) and np.array_equal(g[9:14, 2:9], three[2])
    assert not g[9:14, 11:18].any()                                                                            # the empty cell
    assert render.grid_shape(4, 5, 7, 8) == (9, 38) and R.make_grid(np.zeros((4, 5, 7, 3), np.uint8), 8).shape == (9, 38, 3)
    assert render.grid_shape(2, 64, 64, 1) == (134, 68)                                                        # the trainer's rendering picture


def test_psnr_of_two_constant_images_a_tenth_apart_is_20_db():
    a = np.full((6, 5, 3), 0.5, dtype=np.float64)
    b = a + 0.1
    e = (a - b) ** 2
    assert abs(-10.0 * math.log10(R.exact_sum(e) / e.size) - 20.0) <= 1e-12
    assert abs(render.psnr_of(R.exact_sum(e), e.size) - 20.0) <= 1e-12
    # through the float32 squares the same 20 dB up to float32's rounding of 0.1 and of the square (2^-23 relative each -> < 1e-5 dB)
    assert abs(R.psnr(np.full((6, 5, 3), 0.5, np.float32), np.full((6, 5, 3), 0.6, np.float32)) - 20.0) <= 1e-5
    assert render.psnr_of(0.0, 12) == float("inf")


def test_byte_rule_is_numpys_cast_where_that_is_defined_and_clamps_elsewhere():
    x = R.byte_inputs(np.random.default_rng(1), 4096)
    ok = np.isfinite(x) & (x * np.float32(255.0) >= 0) & (x * np.float32(255.0) < 256)
    assert ok.sum() > 3000
    assert np.array_equal(R.byte(x)[ok], (x[ok] * 255).astype(np.uint8))
    special = np.array([np.nan, np.inf, -np.inf, -1e-3, 1.5, 0.0, 1.0, 254.5 / 255, 1 / 255], dtype=np.float32)
    assert R.byte(special).tolist() == [0, 255, 0, 0, 255, 0, 255, 254, 1]
    assert R.normal_byte(np.array([-1.0, 0.0, 1.0, 1.001, -1.001], np.float32)).tolist() == [0, 127, 255, 255, 0]
    d = np.array([1.0, 2.0, 3.0, np.nan, np.inf], dtype=np.float32)
    assert R.finite_range(d) == (1.0, 3.0) and R.grey(d, 1.0, 3.0).tolist() == [0, 127, 255, 0, 0]
    assert R.finite_range(np.array([np.nan, np.inf], np.float32)) == (0.0, 0.0) and not R.grey(d, 2.0, 2.0).any()


@pytest.mark.parametrize("n", [1, 2, 5])
def test_psnr_csv_is_the_text_pandas_writes(tmp_path, n):
    pd = pytest.importorskip("pandas")
    p = np.random.default_rng(n).uniform(15.0, 40.0, n)
    rows = np.concatenate([p, [p.mean()], [p.std()]])
    assert np.array_equal(render.psnr_rows(p), rows)
    buf = io.StringIO()
    pd.DataFrame(rows).to_csv(buf)
    path = tmp_path / "psnr_7.csv"
    render.write_psnr_csv(str(path), p)
    assert path.read_bytes().decode() == buf.getvalue()
    lines = path.read_text().splitlines()
    assert lines[0] == ",0" and len(lines) == n + 3 and float(lines[-1].split(",")[1]) == p.std() and float(lines[-2].split(",")[1]) == p.mean()


def test_pixel_grid_is_the_datasets_uv(tmp_path):
    """The full-view sample of a BlenderDataset (the attraction fields of its constructor run on the device, so the class itself is
    not built here: its __getitem__ is called on a bare instance, which reads img_res and the per-view lists only)."""
    from neat_amd.datasets import BlenderDataset
    H, W = 5, 7
    ds = BlenderDataset.__new__(BlenderDataset)
    ds.img_res, ds.sampling_idx = [H, W], None
    one = [torch.zeros(H * W)]
    ds.lines, ds.masks, ds.labels, ds.att_points = [torch.zeros(1, 4)], one, [torch.zeros(H * W, dtype=torch.long)], [torch.zeros(H * W, 2)]
    ds.intrinsics_all, ds.pose_all, ds.rgb_images = [torch.eye(4)], [torch.eye(4)], [torch.zeros(H * W, 3)]

    class _Wf:
        vertices = torch.zeros(1, 2)
    ds.wireframes = [_Wf()]
    _, sample, _ = ds[0]
    uv = render.pixel_grid(H, W)
    assert uv.dtype == torch.float32 and uv.shape == (H * W, 2) and torch.equal(uv, sample["uv"])
    assert uv[1].tolist() == [1.0, 0.0] and uv[W].tolist() == [0.0, 1.0] and uv[-1].tolist() == [W - 1.0, H - 1.0]      # x fastest


def test_runner_takes_vis_images():
    import inspect
    from neat_amd.runner import TrainRunner
    assert inspect.signature(TrainRunner.__init__).parameters["vis_images"].default is False      # off by default, as the reference's do_vis
