"""GPU tests of neat_amd.detect (csrc/kernels_detect.hpp) against the float64 definition tests/detect_f64.py.

Labels are integers and must be equal.  For the lines, the set of kept (view, partition, label) regions, their order and every n and k
must be equal, end points within 1e-9 px and -log10 NFA within 1e-9 relative.  The reference marks the regions in which a float64
decision lies within 1e-9 of its boundary (`judge`); those are left out of the comparison and may be 1 % of the regions at most.
Decisions on integers (sizes, votes and their ties) are exact on both sides and are not judged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import detect_f64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz")
_cache = {}


def dev():
    return torch.device("cuda:0")


def reference(name, scale):
    """The pictures of a test and the reference's answer, computed once."""
    key = (name, scale)
    if key not in _cache:
        images = {"polygons": lambda: D.two_polygons()[0][None], "rectangles": D.rectangles,
                  "fixture": lambda: np.load(FIXTURE)["images"]}[name]()
        images.setflags(write=False)
        _cache[key] = (images, D.detect(images, scale))
    return _cache[key]


# ---- 1. labelling -------------------------------------------------------------------------------------------------------------------------------
def serpentine(n=129):
    """A one-pixel path through every 16-pixel tile of an n x n grid: every other row full, joined at alternating ends; one component."""
    m = np.full((n, n), 255, dtype=np.uint8)
    m[0::2, :] = 3
    for j, y in enumerate(range(1, n, 2)):
        m[y, n - 1 if j % 2 == 0 else 0] = 3
    return m


def checkerboard(h, w):
    """Pixels of one code that touch only at their corners: 8-connected across every tile corner."""
    y, x = np.mgrid[:h, :w]
    return np.where((x + y) % 2 == 0, 5, 255).astype(np.uint8)


def comb(h, w):
    m = np.full((h, w), 255, dtype=np.uint8)
    m[:, 0::2] = 1                                                     # the teeth
    m[h - 1, :] = 1                                                    # the back, at the far end of every tooth
    return m


def code_maps(h, w, V, seed):
    rng = np.random.default_rng(seed)
    out = []
    for density in (0.3, 0.9):
        out.append(np.where(rng.random((V, h, w)) < density, rng.integers(0, 8, (V, h, w)), 255).astype(np.uint8))
    patterns = [checkerboard(h, w), comb(h, w), np.full((h, w), 255, np.uint8), np.full((h, w), 6, np.uint8)]
    out.append(np.stack([patterns[(v + 0) % 4] for v in range(V)]))
    out.append(np.stack([patterns[(v + 2) % 4] for v in range(V)]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("shape", [(2, 2), (1, 300), (17, 65), (64, 64), (65, 129)])
def test_labels_equal_the_reference(shape, V):
    from neat_amd import detect
    for codes in code_maps(*shape, V, seed=shape[1] + V):
        got = detect.labels(torch.from_numpy(codes).to(dev())).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, D.labels(codes))


@pytest.mark.gpu
def test_labels_serpentine_is_one_component():
    from neat_amd import detect
    s = serpentine()
    codes = np.stack([s, s.T.copy(), s[::-1].copy()])
    got = detect.labels(torch.from_numpy(codes).to(dev())).cpu().numpy()
    want = D.labels(codes)
    assert np.array_equal(got, want)
    for v in range(3):
        assert len(np.unique(want[v][want[v] >= 0])) == 1
    assert detect.labels(torch.zeros(0, 5, 5, dtype=torch.uint8, device=dev())).shape == (0, 5, 5)


# ---- 2. / 3. lines ------------------------------------------------------------------------------------------------------------------------------
def compare(images, ref, scale):
    """detect.lines against the reference's dict; returns the device's outputs."""
    from neat_amd import detect
    out = detect.lines(torch.from_numpy(images.copy()).to(dev()), scale=scale, grey=True)
    lines, width, nfa, n, k, offsets, grey = (t.cpu().numpy() for t in out)
    assert np.array_equal(grey, ref["grey"])                           # bit for bit, the Gaussian of scale < 1 included
    V = images.shape[0]
    assert offsets.shape == (V + 1,) and offsets[0] == 0 and offsets[-1] == lines.shape[0] and (np.diff(offsets) >= 0).all()
    judged = {tuple(t) for t in ref["cand"][ref["cand_judge"]].tolist()}
    print(f"regions {len(ref['cand'])}, judged {len(judged)}, kept {ref['lines'].shape[0]} (device {lines.shape[0]})")
    assert len(judged) <= 0.01 * len(ref["cand"])
    # the device reports no (partition, label); a kept region is identified by its view, its order and its counts, and the order is
    # (view, partition, label): walk both lists in step, skipping the judged regions of the reference
    want = [i for i in range(ref["lines"].shape[0]) if (ref["view"][i], ref["part"][i], ref["label"][i]) not in judged]
    if not judged:
        assert lines.shape[0] == ref["lines"].shape[0] and np.array_equal(offsets, ref["offsets"])
        have = list(range(lines.shape[0]))
    else:                                                              # a judged region may be kept on one side only: match by view and end points
        have = []
        for i in want:
            a, b = offsets[ref["view"][i]], offsets[ref["view"][i] + 1]
            d = np.abs(lines[a:b] - ref["lines"][i]).max(axis=1) if b > a else np.zeros(0)
            assert d.size and d.min() < 1e-9, ("a kept region is missing", i)
            have.append(int(a + d.argmin()))
        assert have == sorted(have) and lines.shape[0] - len(have) <= len(judged)
    assert len(have) == len(want)
    for j, i in zip(have, want):
        assert n[j] == ref["n"][i] and k[j] == ref["k"][i], (i, n[j], ref["n"][i], k[j], ref["k"][i])
        assert np.abs(lines[j] - ref["lines"][i]).max() < 1e-9, (i, lines[j], ref["lines"][i])
        assert abs(width[j] - ref["width"][i]) < 1e-9
        assert abs(nfa[j] - ref["nfa"][i]) <= 1e-9 * abs(ref["nfa"][i]), (i, nfa[j], ref["nfa"][i])
    return lines, width, nfa, n, k, offsets


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale", [("polygons", 1.0), ("rectangles", 1.0), ("fixture", 1.0), ("fixture", 0.8)])
def test_lines_equal_the_reference(name, scale):
    images, ref = reference(name, scale)
    lines = compare(images, ref, scale)[0]
    assert lines.shape[0] >= 7
    if name == "polygons":
        assert lines.shape[0] == 7


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_agree_and_a_batch_is_its_views():
    from neat_amd import detect
    images = torch.from_numpy(reference("fixture", 1.0)[0].copy()).to(dev())
    for scale in (1.0, 0.8):
        a = detect.lines(images, scale=scale)
        b = detect.lines(images, scale=scale)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        parts = [detect.lines(images[v:v + 1], scale=scale) for v in range(images.shape[0])]
        for j in range(5):
            assert torch.equal(a[j], torch.cat([p[j] for p in parts]))
        assert a[5].tolist() == np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).tolist()
    grey = detect.lines(images[:2, :, :, 1].contiguous(), scale=1.0, grey=True)[6]          # one channel: the grey is the picture
    assert torch.equal(grey, images[:2, :, :, 1].double())


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_writes_what_the_dataset_reads(tmp_path):
    from neat_amd import synth
    from neat_amd.datasets import BlenderDataset
    root = str(tmp_path / "scene")
    res = synth.write_scene_fixture(FIXTURE, root)
    run = subprocess.run([sys.executable, "-m", "neat_amd.detect", "--scan", root, "--batch", "3"], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    images, ref = reference("fixture", 1.0)
    summary = run.stdout.strip().splitlines()[-1]
    assert summary.startswith(f"8 views, {ref['lines'].shape[0]} segments, "), summary
    assert sorted(os.listdir(os.path.join(root, "lsd"))) == [f"image_{i:04d}.json" for i in range(8)]
    ds = BlenderDataset("scene", [res, res], line_detector="lsd", data_root=str(tmp_path))
    assert len(ds) == 8
    assert not ref["cand_judge"].any()
    for v in range(8):
        a, b = ref["offsets"][v], ref["offsets"][v + 1]
        got = ds.lines[v].numpy()
        assert got.shape == (b - a, 5)
        assert np.abs(got[:, :4] - ref["lines"][a:b]).max() < 1e-4                         # float32 in the JSON's reader
        assert np.allclose(got[:, 4], 1.0 - 10.0 ** -ref["nfa"][a:b], atol=1e-6)
    np.random.seed(0)
    batch = ds.device_batches(dev())
    idx, sample, gt = batch.batch(0, 64)
    torch.cuda.synchronize()
    assert sample["uv"].shape[-2:] == (64, 2) and gt["lines2d"].shape[-2:] == (64, 5)


# ---- 6. edges of the domain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_tiny_constant_and_all_used_pictures():
    from neat_amd import detect
    out = detect.lines(torch.zeros(0, 16, 16, 3, dtype=torch.uint8, device=dev()))
    assert out[0].shape == (0, 4) and out[5].tolist() == [0]
    rng = np.random.default_rng(4)
    tiny = rng.integers(0, 256, (2, 2, 2), dtype=np.uint8)
    const = np.full((2, 20, 33), 90, dtype=np.uint8)
    y, x = np.mgrid[:30, :40]
    ramp = (5 * x + 2 * y).astype(np.uint8)[None]                      # at most 253; the gradient (5, 2) everywhere: every position is used
    assert (D.orientation_codes(*D.gradient(ramp[0].astype(np.float64)), D.constants(30, 40)["rho2"], 0.4) != 255).all()
    for images in (tiny, const, ramp):
        ref = D.detect(images, 1.0)
        got = detect.lines(torch.from_numpy(images).to(dev()), scale=1.0)
        assert got[0].shape[0] == ref["lines"].shape[0] and got[5].tolist() == ref["offsets"].tolist()
        assert np.array_equal(got[3].cpu().numpy(), ref["n"]) and np.array_equal(got[4].cpu().numpy(), ref["k"])
    small = detect.lines(torch.from_numpy(tiny).to(dev()), scale=0.3)                       # 1 x 1 after scaling: no gradient grid
    assert small[0].shape == (0, 4) and small[5].tolist() == [0, 0, 0]
