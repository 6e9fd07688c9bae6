"""CPU: the float64 model of the sphere tracing (tests/trace_f64.py) against the closed-form first intersections of its analytic fields,
the new entry points in the header and the binding, and the `check` command line of neat_amd.trace: flags, keep rule, file layout."""
import os
import re

import numpy as np
import pytest

from tests import trace_f64 as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_SYMBOLS = ("neat_trace_ws_bytes", "neat_trace_list_offset", "neat_trace_init", "neat_trace_step", "neat_trace_finish", "neat_trace_target_rays")
EPS, REFINE = 1e-4, 8


@pytest.mark.parametrize("name", sorted(T.FIELDS))
def test_model_meets_the_closed_forms_within_the_derived_bound(name):
    o, d = T.scene(name)
    m = T.trace(T.np_field(name), o, d, eps=EPS, refine_steps=REFINE)
    j = T.judge(name, o, d, m, EPS, REFINE)
    keep = ~j["excluded"]
    print("%s: %d rays, %d hit, %d excluded, %d evaluations, states %s" % (name, len(o), j["hit"].sum(), j["excluded"].sum(), m["evals"],
                                                                           np.bincount(m["state"], minlength=4).tolist()))
    assert j["excluded"].mean() <= 0.02                                   # the fans keep the exclusions rare
    assert j["hit"].sum() > 200 and (~j["alive"]).sum() > 50 and (j["alive"] & ~j["hit"]).sum() > 100
    expect = np.where(j["hit"], T.HIT, T.MISS)
    assert np.array_equal(m["state"][keep], expect[keep])
    h = keep & j["hit"]
    err = np.abs(m["depth"][h] - j["tstar"][h])
    print("  worst depth error / bound: %.3g" % (err / j["bound"][h]).max())
    assert (err <= j["bound"][h]).all()
    assert np.isnan(m["depth"][m["state"] == T.MISS]).all() and (m["steps"][~j["alive"]] == 0).all()
    assert (m["steps"] <= 1 + 64 + REFINE).all() and m["evals"] == sum(len(l) for l in m["lists"])
    # the bound's bracket term is the width the model ends with; at the default rounds it is never above bisection's w0 / 2^refine_steps
    assert (m["wfin"] <= m["w0"] / 2.0 ** REFINE).all()
    if name == "sphere_x2":
        assert (m["w0"][h] > 0).mean() > 0.9                              # the overshoot goes through the bracket and its refinement
        # too few rounds: brackets are left open, the hit is their near end, and the bound holds with their width as its term
        few = T.trace(T.np_field(name), o, d, eps=EPS, refine_steps=2)
        jf = T.judge(name, o, d, few, EPS, 2)
        left = h & (few["wfin"] > 0)
        err = np.abs(few["depth"][h] - jf["tstar"][h])
        print("  2 rounds: %d brackets left open, widths up to %.3g, worst depth error / bound %.3g" % (left.sum(), few["wfin"].max(), (err / jf["bound"][h]).max()))
        assert left.sum() > 100 and (few["state"][keep] == expect[keep]).all() and (few["steps"] <= 1 + 64 + 2).all()
        assert (err <= jf["bound"][h]).all() and (few["depth"][left] <= jf["tstar"][left]).all()
        assert (few["wfin"][left] <= 0.95 ** 2 * few["w0"][left] * (1 + 1e-12)).all()      # what the 90 % clamp does guarantee per round
    if name in ("sphere", "box"):
        assert (m["w0"] == 0).all()                                       # an exact SDF with relax 1 never steps across the surface


def test_model_states_at_the_ends():
    f = T.np_field("sphere")
    n = 40
    o, d = T.fan(n, 3, ((0.0, 0.3),))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    tstar, _ = T.first_hit("sphere", o64, d64, 0.0, np.inf)
    # t_end in front of the surface: MISS; behind it: HIT; exactly at the fp32 value next above it: not lost
    assert (T.trace(f, o, d, t_end=tstar - 0.05)["state"] == T.MISS).all()
    assert (T.trace(f, o, d, t_end=tstar + 0.05)["state"] == T.HIT).all()
    up = np.nextafter(tstar.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    at_end = T.trace(f, o, d, t_end=up)
    assert (at_end["state"] == T.HIT).all() and np.abs(at_end["depth"] - tstar).max() < 2e-4
    # every ray misses the bounding sphere: no evaluation
    o2, d2 = T.fan(n, 4, ((1.05, 1.5),))
    m = T.trace(f, o2, d2)
    assert (m["state"] == T.MISS).all() and m["evals"] == 0 and m["lists"] == []
    # every ray starts inside the surface: INSIDE at the start of the chord, one evaluation each
    m = T.trace(f, 0.1 * o, d, near=0.0)
    assert (m["state"] == T.INSIDE).all() and (m["depth"] == 0).all() and m["evals"] == n and (m["steps"] == 1).all()
    # the under-stepping field at a small max_steps: UNCONVERGED after 1 + max_steps evaluations, no depth
    m = T.trace(T.np_field("sphere_half"), o, d, max_steps=4)
    assert (m["state"] == T.UNCONVERGED).all() and (m["steps"] == 5).all() and np.isnan(m["depth"]).all()
    # a NaN from the field ends the ray
    m = T.trace(lambda p: np.full(len(p), np.nan), o, d)
    assert (m["state"] == T.UNCONVERGED).all() and (m["steps"] == 1).all()
    # refine_steps = 0: the hit is the last point in front of the surface
    m = T.trace(T.np_field("sphere_x2"), o, d, refine_steps=0)
    assert (m["state"] == T.HIT).all() and (m["depth"] < tstar).all()


def header_text():
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_and_binding_agree_on_the_new_entries():
    import ctypes
    from neat_amd import _lib
    text = header_text()
    for name in TRACE_SYMBOLS:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        res, args = _lib._SIGNATURES[name]
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int), name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):
            want = (_lib.c_fp if "*" in p else ctypes.c_double if p.startswith("double") else ctypes.c_float if p.startswith("float")
                    else ctypes.c_int)
            assert a is want, (name, p)
    assert _lib.ABI_VERSION == 15


def _load():
    from neat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_library_exports_the_entries_and_rejects_bad_arguments_before_any_launch():
    lib = _load()
    assert lib.neat_abi_version() == 15
    for name in TRACE_SYMBOLS:
        getattr(lib, name)
        assert not hasattr(lib, "f16_" + name)               # no 16-bit storage type: compiled once
    w = lib.neat_trace_ws_bytes
    assert w(0) == 0 and w(-3) == 0 and w(2 ** 24) > 0 and w(2 ** 24 + 1) == 0          # the cap of one batch
    off = lib.neat_trace_list_offset
    assert off(0, 0) == 0 and off(5, 2) == 0 and off(2 ** 24 + 1, 0) == 0
    for R in (1, 63, 256, 257, 100000):
        # six float, five int and three byte arrays of R entries, and one int per workgroup of 256 list positions
        assert w(R) >= 4 * 11 * R + 3 * R + 4 * ((R + 255) // 256) and w(R) % 256 == 0
        assert w(R + 256) > w(R)
        # the two id lists: int32 [R] each, apart, inside the workspace, 256-byte aligned
        a, b = off(R, 0), off(R, 1)
        assert a % 256 == 0 and b % 256 == 0 and a >= 4 * 6 * R and abs(b - a) >= 4 * R and max(a, b) + 4 * R <= w(R)
    assert lib.neat_trace_init(None, None, None, 4, 1.0, 0.0, None, None, None, None) == -1
    assert lib.neat_trace_step(None, None, None, 0, 4, 0, 1e-4, 1.0, 64, 8, None, None, None, None) == -1
    assert lib.neat_trace_finish(None, None, 4, None, None, None, None, None, None) == -1
    assert lib.neat_trace_target_rays(None, 0, None, 3, 0, 1, 1.0, 0.0, 0.01, None, None, None, None, None) == 0          # nothing to do
    assert lib.neat_trace_target_rays(None, 2, None, 3, 2, 1, 1.0, 0.0, 0.01, None, None, None, None, None) == -1
    assert lib.neat_trace_target_rays(None, 2, None, 3, 2, 16, 1.0, 0.0, 0.01, None, None, None, None, None) == -1         # segments need 6 floats


def test_check_flags_and_defaults():
    from neat_amd import trace
    opt = trace.parse_args(["check", "--conf", "x/runconf.conf", "--data", "w/latest-abc-wfi.npz"])
    expect = {"command": "check", "min_views": 5, "min_frac": 0.5, "bias": 0.01, "samples": 16, "checkpoint": "latest", "expdir": None,
              "data_root": "../data", "gpu": 0, "precision": None, "json": False, "overwrite": False}
    for k, v in expect.items():
        assert getattr(opt, k) == v, k
    opt = trace.parse_args(["check", "--conf", "c", "--data", "d.pth", "--min-views", "2", "--min-frac", "0.25", "--bias", "0.02", "--samples", "8",
                            "--checkpoint", "1000", "--expdir", "run", "--data_root", "r", "--gpu", "3", "--precision", "fp32", "--json", "--overwrite"])
    assert (opt.min_views, opt.min_frac, opt.bias, opt.samples, opt.checkpoint, opt.expdir, opt.data_root, opt.gpu, opt.precision) == (
        2, 0.25, 0.02, 8, "1000", "run", "r", 3, "fp32") and opt.json and opt.overwrite
    for bad in ([], ["check"], ["check", "--conf", "c"], ["check", "--conf", "c", "--data", "d", "--samples", "1"],
                ["check", "--conf", "c", "--data", "d", "--min-frac", "1.5"], ["check", "--conf", "c", "--data", "d", "--bias", "-1"],
                ["check", "--conf", "c", "--data", "d", "--precision", "int8"], ["look", "--conf", "c"]):
        with pytest.raises(SystemExit):
            trace.parse_args(bad)
    assert trace.out_path("run/wireframes/latest-abc-wfi.npz") == "run/wireframes/latest-abc-wfi_occl.npz"
    assert trace.out_path("w/latest-abc-neat.pth") == "w/latest-abc-neat_occl.npz"
    assert trace.DEFAULTS == dict(eps=1e-4, relax=1.0, max_steps=64, refine_steps=8, near=0.0)
    assert (trace.MISS, trace.HIT, trace.INSIDE, trace.UNCONVERGED) == (T.MISS, T.HIT, T.INSIDE, T.UNCONVERGED) == (0, 1, 2, 3)


def test_keep_rule_on_a_hand_made_table():
    from neat_amd import trace
    frac = np.array([[1.0, 0.5, 0.4375, 0.0, 0.5],
                     [1.0, 0.5, 0.5000, 0.0, 0.0],
                     [1.0, 0.0, 0.5625, 0.0, 1.0]])           # three views, five lines
    views, kept = trace.keep_rule(frac, min_views=2, min_frac=0.5)
    assert views.dtype == np.int32 and views.tolist() == [3, 2, 2, 0, 2] and kept.dtype == bool and kept.tolist() == [True, True, True, False, True]
    views, kept = trace.keep_rule(frac, min_views=3, min_frac=0.5)
    assert kept.tolist() == [True, False, False, False, False]
    views, kept = trace.keep_rule(frac, min_views=1, min_frac=0.5625)
    assert views.tolist() == [3, 0, 1, 0, 1] and kept.tolist() == [True, False, True, False, True]
    views, kept = trace.keep_rule(frac, min_views=0, min_frac=1.0)
    assert kept.all() and views.tolist() == [3, 0, 0, 0, 1]
    views, kept = trace.keep_rule(np.zeros((0, 4)), 5, 0.5)
    assert views.tolist() == [0] * 4 and not kept.any()


def test_occl_file_layout_and_readers(tmp_path):
    from neat_amd import run_io, trace
    rng = np.random.default_rng(0)
    lines = rng.uniform(-1, 1, (6, 2, 3))
    np.savez(tmp_path / "latest-h-wfi.npz", lines3d=lines)
    assert np.array_equal(run_io.load_lines(str(tmp_path / "latest-h-wfi.npz"), pth_key="lines3d_wfi")[0], lines)
    views = np.array([5, 0, 7, 1, 9, 3])
    kept = views >= 5
    path = trace.out_path(str(tmp_path / "latest-h-wfi.npz"))
    trace.write_occl(path, lines, views, kept)
    with np.load(path) as z:
        assert sorted(z.files) == ["kept", "lines3d", "views"]
        assert z["views"].dtype == np.int32 and z["views"].tolist() == views.tolist()
        assert z["kept"].dtype == bool and z["kept"].tolist() == kept.tolist()
        assert z["lines3d"].shape == (3, 2, 3) and np.array_equal(z["lines3d"], lines[kept])
    assert np.array_equal(run_io.load_lines(path)[0], lines[kept])            # neat_amd.show reads the file as it is
    assert os.listdir(tmp_path).count(os.path.basename(path)) == 1 and not [f for f in os.listdir(tmp_path) if "tmp" in f]
    import torch
    torch.save({"lines3d_wfi": torch.from_numpy(lines).float(), "lines3d_wfi_checked": torch.zeros(0, 2, 3)}, str(tmp_path / "latest-h-neat.pth"))
    assert np.array_equal(run_io.load_lines(str(tmp_path / "latest-h-neat.pth"), pth_key="lines3d_wfi")[0], lines.astype(np.float32).astype(np.float64))
