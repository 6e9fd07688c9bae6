"""CPU: the command line of the wireframe parsing (python -m neat_amd.parse) against the reference's code/neat-final-parsing.py --
flag defaults and output names -- and the ABI v15 entry points of the library (symbols, workspace queries; no device work)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSE_SYMBOLS = ("neat_parse_match", "neat_parse_group_ws_bytes", "neat_parse_group", "neat_parse_vote_ws_bytes", "neat_parse_vote",
                 "neat_parse_graph_ws_bytes", "neat_parse_graph", "neat_parse_visibility_ws_bytes", "neat_parse_visibility")


def _load():
    from neat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_flag_defaults_equal_the_reference():
    from neat_amd.parse import build_parser
    opt = build_parser().parse_args(["--conf", "x/runconf.conf"])
    # neat-final-parsing.py :430-443 (--gpu takes a device index here: there is no GPUtil 'auto')
    expect = {"checkpoint": "latest", "chunksize": 2048, "reproj_dis": 10, "ckdist": 100, "ckview": 5, "overwrite": False,
              "disable_junction_refine": False, "junc_match_threshold": 0.02}
    for k, v in expect.items():
        assert getattr(opt, k) == v, k
    types = {a.dest: a.type for a in build_parser()._actions}
    assert types["reproj_dis"] is int and types["ckdist"] is float and types["ckview"] is int and types["chunksize"] is int
    assert types["junc_match_threshold"] is float and opt.gpu == 0
    opt = build_parser().parse_args(["--conf", "c", "--reproj-dis", "5", "--disable-junction-refine", "--overwrite", "--gpu", "3"])
    assert opt.reproj_dis == 5 and opt.disable_junction_refine and opt.overwrite and opt.gpu == 3
    with pytest.raises(SystemExit):
        build_parser().parse_args([])


def test_file_names_equal_the_reference(golden):
    from neat_amd.parse import out_basename
    g = golden("g19_final_parsing")
    kwargs = json.loads(str(g["name_kwargs"]))
    assert len(kwargs) >= 3
    for kw, h in zip(kwargs, g["name_hashes"]):
        assert out_basename(kw["conf"], kw["checkpoint"], kw["distance"], kw["sdf_junction_refine"]) == f"{kw['checkpoint']}-{h}"


def test_library_exports_the_v15_symbols():
    from neat_amd import _lib
    lib = _load()
    assert _lib.ABI_VERSION == 15 and lib.neat_abi_version() == 15
    for name in PARSE_SYMBOLS:
        assert name in _lib.exported_symbols()
        getattr(lib, name)
        assert not hasattr(lib, "f16_" + name)      # the parse stages have no 16-bit storage type: compiled once, no f16 twin


def test_workspace_queries_are_sane():
    lib = _load()
    from neat_amd import _lib as L
    # group: a stable counting sort over tiles of 4096 rows: [tiles x m] counters + 3 m + the 2 n row order
    g = lib.neat_parse_group_ws_bytes
    assert g(0, 0) == 0 and g(-1, 3) == 0 and g(5, -1) == 0
    for n, m in ((1, 1), (63, 64), (2048, 5), (200000, 5000)):
        tiles = (2 * n + 4095) // 4096
        assert g(n, m) >= 4 * (tiles * m + 3 * m + 2 * n)
        assert g(n, m) % 256 == 0
        assert g(n, m + 64) > g(n, m) and g(n + 4096, m) > g(n, m)
    # vote: the [J, 2 mcap] cost matrix, the column mask, the pairs and neat_lsap's own workspace
    v = lib.neat_parse_vote_ws_bytes
    assert v(0, 5) == 0 and v(5, 0) == 0
    for J, mcap in ((1, 1), (64, 40), (1024, 300)):
        assert v(J, mcap) >= 4 * J * 2 * mcap + lib.neat_lsap_ws_bytes(J, 2 * mcap) + 16 * min(J, 2 * mcap)
        assert v(J, mcap + 64) > v(J, mcap)
    gr = lib.neat_parse_graph_ws_bytes
    assert gr(6, 40, 64) >= 4 * (6 * 40 + 64) and gr(-1, 1, 1) == 0
    vi = lib.neat_parse_visibility_ws_bytes
    assert vi(100, 6) >= 6 * 100 + 4 * 100
    assert vi(101, 6) >= vi(100, 6) and vi(-1, 2) == 0
    # argument checks happen before any launch (no device needed): bad sizes are rejected, empty problems are no-ops
    assert lib.neat_parse_match(None, -1, None, 0, 4, 10.0, None, None, None) == -1
    assert lib.neat_parse_match(None, 0, None, 0, 4, 10.0, None, None, None) == 0
    assert lib.neat_parse_match(None, 4, None, 3, 2, 10.0, None, None, None) == -1          # gt row stride < 4
    assert lib.neat_parse_vote(None, 0, None, None, 3, 0.02, 0, None, None, None, None) == 0
    assert lib.neat_parse_group(None, None, None, -1, 2, None, None, None, None, None) == -1
