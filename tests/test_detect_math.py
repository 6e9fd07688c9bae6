"""CPU checks of the line-segment detector: the float64 definition tests/detect_f64.py on pictures with known answers, the pictures of
tests/test_detect_gpu.py against the judge cap, the C ABI's three new symbols and the workspace query, and the JSON round trip."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import detect_f64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_abc_00075213_8views.npz")
NAMES = ["neat_detect_label", "neat_detect_lines", "neat_detect_scratch_bytes"]


def fixture_images():
    return np.load(FIXTURE)["images"]


def test_two_polygons_give_their_seven_edges_and_noise_gives_none():
    img, edges = D.two_polygons()
    r = D.detect(img[None], 1.0)
    assert r["lines"].shape == (7, 4) and r["offsets"].tolist() == [0, 7]
    assert (r["nfa"] > 20).all() and (r["nfa"] < 100).all()
    hit = set()
    for e in edges:
        best = None
        for j, l in enumerate(r["lines"]):
            for a, b in ((l[:2], l[2:]), (l[2:], l[:2])):
                d = max(math.hypot(*(a - e[:2])), math.hypot(*(b - e[2:])))
                if best is None or d < best[0]:
                    best = (d, j)
        assert best[0] < 1.5, (e, best)
        hit.add(best[1])
    assert len(hit) == 7                                    # one segment per edge
    assert D.detect(D.noise()[None], 1.0)["lines"].shape[0] == 0


def test_label_map_is_the_smallest_index_of_the_component():
    """The scipy-based labelling against a flood fill written out."""
    rng = np.random.default_rng(2)
    code = np.where(rng.random((13, 19)) < 0.7, rng.integers(0, 3, (13, 19)), 255).astype(np.uint8)
    h, w = code.shape
    want = np.full(h * w, -1, dtype=np.int32)
    for i in range(h * w):
        if code.flat[i] == 255 or want[i] >= 0:
            continue
        stack, want[i] = [i], i                            # raster order: i is the smallest index of a component not yet seen
        while stack:
            p = stack.pop()
            y, x = divmod(p, w)
            for yy in range(max(y - 1, 0), min(y + 2, h)):
                for xx in range(max(x - 1, 0), min(x + 2, w)):
                    n = yy * w + xx
                    if want[n] < 0 and code.flat[n] == code.flat[i]:
                        want[n] = i
                        stack.append(n)
    assert np.array_equal(D.label_map(code).reshape(-1), want)


def test_orientation_codes_are_sectors_of_45_degrees():
    ang = np.deg2rad(np.arange(0.25, 360.0, 0.5))                      # no sample on a boundary
    gx, gy = 10 * np.cos(ang)[None], 10 * np.sin(ang)[None]
    codes = D.orientation_codes(gx, gy, gx * gx + gy * gy, 1.0, math.sqrt(2.0) - 1.0)
    for p, first in ((0, 0.0), (1, 22.5)):
        sector = np.floor(((np.rad2deg(ang) - first) % 360.0) / 45.0).astype(int)
        for s in range(8):
            assert len(set(codes[p, 0][sector == s].tolist())) == 1
        assert len(set(codes[p, 0].tolist())) == 8
    assert (D.orientation_codes(gx, gy, gx * gx + gy * gy, 101.0, 0.4) == 255).all()


@pytest.mark.parametrize("scale", [1.0, 0.8])
def test_the_gpu_tests_pictures_stay_within_the_judge_cap(scale):
    """tests/test_detect_gpu.py leaves out regions with a decision within 1e-9 of its boundary and allows 1 % of them: the reference
    alone must stay within that on every picture used there."""
    pictures = [D.two_polygons()[0][None], D.rectangles(), fixture_images()] if scale == 1.0 else [fixture_images()]
    for images in pictures:
        r = D.detect(images, scale)
        assert len(r["cand"]) > 0 and r["cand_judge"].sum() <= 0.01 * len(r["cand"])
        assert r["lines"].shape[0] >= 7
    if scale == 1.0:
        r = D.detect(D.rectangles(), 1.0)
        assert (np.diff(r["offsets"]) >= 16).all()                     # four rectangles of four edges a view


def test_grey_downscale_shape_and_constant_picture():
    img = np.full((1, 10, 13, 3), 77, dtype=np.uint8)
    g = D.grey(img, 0.8)
    assert g.shape == (1, 8, 11)
    assert np.abs(g - 77.0).max() < 1e-12                              # normalised taps
    assert D.grey(img, 1.0).shape == (1, 10, 13) and (D.grey(img, 1.0) == 77.0).all()
    c = np.zeros((1, 2, 2, 3), dtype=np.uint8)
    c[0, 0, 0] = (255, 0, 0)
    c[0, 0, 1] = (0, 255, 0)
    c[0, 1, 0] = (0, 0, 255)
    c[0, 1, 1] = (255, 255, 255)
    assert D.grey(c, 1.0).reshape(-1).tolist() == [77.0, 149.0, 29.0, 255.0]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    from neat_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neat_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(neat_detect_[a-z0-9_]+)\s*\(", text)))
    assert declared == NAMES
    assert [n for n in _lib.exported_symbols() if n.startswith("neat_detect_")] == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n)
        assert not hasattr(lib, "f16_" + n)                            # compiled once: no twin
    twins = open(os.path.join(ROOT, "neat_amd", "csrc", "twin_list.h")).read()
    assert "detect" not in twins
    assert _lib.lib().neat_abi_version() == _lib.ABI_VERSION == 15
    assert not any(n.endswith("_ws_bytes") for n in NAMES)


# (V, H, W, scale, min_reg) -> bytes, around the 16-pixel tile of the labelling (gradient grids of 15, 16 and 17) and the 256-element
# workgroups, recorded from the library; Python allocates from this query
SCRATCH = [((1, 2, 2, 1.0, 2), 4864), ((1, 16, 16, 1.0, 7), 25600), ((1, 17, 17, 1.0, 7), 26368), ((1, 18, 18, 1.0, 7), 31488),
           ((3, 17, 33, 1.0, 8), 143360), ((1, 128, 128, 1.0, 12), 1383424), ((1, 128, 128, 0.8, 12), 894208),
           ((8, 128, 128, 1.0, 12), 11038720), ((2, 97, 131, 1.0, 12), 2137600), ((0, 0, 0, 1.0, 2), 1792), ((0, 128, 128, 1.0, 2), 1792),
           ((1, 1200, 1600, 1.0, 18), 156503296)]
REFUSED = [(-1, 16, 16, 1.0, 5), (1, 1, 16, 1.0, 5), (1, 16, 1, 1.0, 5), (1, 16, 16, 0.0, 5), (1, 16, 16, 1.5, 5), (1, 16, 16, -0.5, 5),
           (1, 16, 16, 1.0, 0), (1, 40000, 16, 1.0, 5), (4096, 32768, 32768, 1.0, 5), (1, 16, 16, float("nan"), 5)]


def test_scratch_bytes_are_pinned_and_bad_arguments_refused():
    from neat_amd import _lib, detect
    lib = _lib.lib()
    for args, want in SCRATCH:
        assert lib.neat_detect_scratch_bytes(*args) == want, args
        V, H, W, scale, min_reg = args
        if V > 0:                                                      # the min_reg of the table is the one the host computes
            assert detect.constants(D.scaled_size(H, scale), D.scaled_size(W, scale))["min_reg"] == min_reg
    for args in REFUSED:
        assert lib.neat_detect_scratch_bytes(*args) == 0, args
    # the entry points validate on the host, before any launch: no device is touched here
    off = (ctypes.c_int * 4)()
    a = ctypes.addressof(off)
    c = detect.constants(16, 16)
    tail = [c["rho2"], c["c1"], c["cos_tau"], 0.7, c["logNT"], c["p"], c["min_reg"], None, 0, None, None, None, None, None, a, None]
    call = lambda V, H, W, ch, scale: lib.neat_detect_lines(None, V, H, W, ch, scale, None, None, 0, *tail)
    assert call(-1, 16, 16, 3, 1.0) == -1
    assert call(1, 1, 16, 3, 1.0) == -1 and call(1, 16, 1, 3, 1.0) == -1
    assert call(1, 16, 16, 2, 1.0) == -1 and call(1, 16, 16, 4, 1.0) == -1
    assert call(1, 16, 16, 3, 0.0) == -1 and call(1, 16, 16, 3, 1.25) == -1
    assert call(1, 16, 16, 3, 1.0) == -1                               # no images, no workspace
    assert lib.neat_detect_label(None, -1, 4, 4, None, None) == -1
    assert lib.neat_detect_label(None, 1, 4, 4, None, None) == -1
    assert lib.neat_detect_label(None, 0, 4, 4, None, None) == 0
    assert lib.neat_detect_label(None, 3, 65536, 65536, None, None) == -1


def test_host_constants_are_the_definitions():
    from neat_amd import detect
    for Hs, Ws in ((2, 2), (96, 96), (103, 103), (1200, 1600)):
        assert detect.constants(Hs, Ws) == D.constants(Hs, Ws)
    assert D.constants(128, 128)["min_reg"] == 12
    for out, scale in ((103, 0.8), (64, 0.5), (7, 0.3)):
        assert np.array_equal(detect.gaussian_taps(out, scale), D.gaussian_taps(out, scale)[0])


def test_wireframe_json_round_trip(tmp_path):
    from neat_amd import detect, run_io
    from neat_amd.wireframe import WireframeGraph
    r = D.detect(D.two_polygons()[0][None], 1.0)
    nfa = r["nfa"].copy()
    nfa[0], nfa[1] = 0.01, 0.5                                         # NFA 0.977 (dropped by the datasets' threshold) and 0.316 (kept)
    wf = detect.to_wireframe(torch.from_numpy(r["lines"]), torch.from_numpy(nfa), 96, 96)
    assert wf.vertices.shape == (14, 2) and wf.edges.tolist() == [[2 * i, 2 * i + 1] for i in range(7)]
    assert np.allclose(wf.weights.numpy(), 1.0 - 10.0 ** -nfa, atol=1e-7) and torch.equal(wf.v_confidences, wf.weights.repeat_interleave(2))
    path = str(tmp_path / "lsd" / "view.json")
    run_io.write_wireframe_json(path, wf, {"edges-nfa": nfa.tolist()})
    d = json.load(open(path))
    assert d["edges-nfa"] == nfa.tolist() and d["height"] == 96 and d["width"] == 96
    back = WireframeGraph.load_json(path).line_segments(0.05)
    assert back.shape == (6, 5)
    assert np.array_equal(back[:, :4].numpy(), r["lines"][1:].astype(np.float32))
    assert np.allclose(back[:, 4].numpy(), (1.0 - 10.0 ** -nfa[1:]).astype(np.float32))
