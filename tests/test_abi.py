"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/neat_hip.h declares; the Python binding declares the same set.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(neat_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from neat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = header_functions()
    assert len(names) >= 12
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/neat_hip.h but not exported"
    assert names == _lib.exported_symbols()
    assert _lib.lib().neat_abi_version() == _lib.ABI_VERSION


def test_workspace_queries_are_consistent():
    from neat_amd import _lib
    lib = _lib.lib()
    for prec, tile in ((0, 64), (1, 128)):
        assert lib.neat_packed_floats(prec) > 19 * 256
        assert lib.neat_sdf_ws_floats(64, 0, prec) < lib.neat_sdf_ws_floats(64, 1, prec)
        assert lib.neat_render_ws_floats(8, 8, 0, prec) > lib.neat_sdf_ws_floats(64, 1, prec)
        assert lib.neat_render_ws_floats(8, 8, 0, prec) == lib.neat_render_ws_floats(8, 7, 8, prec)     # E extra points share the tile grid
        # point stride is padded to the workgroup's point tile (64 fp32 / 128 bf16)
        assert lib.neat_sdf_ws_floats(1, 0, prec) == lib.neat_sdf_ws_floats(tile, 0, prec)
        assert lib.neat_sdf_ws_floats(tile + 1, 0, prec) == lib.neat_sdf_ws_floats(2 * tile, 0, prec)
    assert lib.neat_packed_floats(7) == 0          # unknown precision is rejected
    # NEAT_F16 (3) = the bf16 build's layouts with IEEE half as the 16-bit type; NEAT_BF16X3 (2) = the fp32 build's
    assert lib.neat_packed_floats(3) == lib.neat_packed_floats(1) and lib.neat_packed_floats(2) == lib.neat_packed_floats(0)
    assert lib.neat_render_ws_floats(64, 32, 8, 3) == lib.neat_render_ws_floats(64, 32, 8, 1)
    assert lib.neat_render_eval_ws_floats(64, 32, 3) == lib.neat_render_eval_ws_floats(64, 32, 1)
    assert lib.neat_sdf_ws_floats(100, 1, 3) == lib.neat_sdf_ws_floats(100, 1, 1) and lib.neat_heads_ws_floats(100, 3) == lib.neat_heads_ws_floats(100, 1)
    # neat_sdf_ldp = the x-row stride the sampler's launches write a query at (ops.sdf_query_workspace): it must be the stride the
    # values-mode forward reads and neat_sdf_ws_floats sized the workspace with, for every precision code (bf16x3 runs the fp32
    # layouts; fp16 / fp16x3 / fp16x3-fast the 16-bit ones)
    for P in (1, 63, 64, 65, 127, 128, 129):
        assert lib.neat_sdf_ldp(P, 2) == lib.neat_sdf_ldp(P, 0), P
        assert lib.neat_sdf_ldp(P, 4) == lib.neat_sdf_ldp(P, 5) == lib.neat_sdf_ldp(P, 1) == lib.neat_sdf_ldp(P, 3), P
        for prec, tile in ((0, 64), (2, 64), (1, 128), (3, 128), (4, 128), (5, 128)):
            ldp = lib.neat_sdf_ldp(P, prec)
            assert ldp >= P and ldp % tile == 0 and ldp - P < tile, (P, prec, ldp)
            # the workspace was sized with the same granule: P and ldp land on the same size
            assert lib.neat_sdf_ws_floats(P, 0, prec) == lib.neat_sdf_ws_floats(ldp, 0, prec), (P, prec)
            if ldp > tile:
                assert lib.neat_sdf_ws_floats(ldp - tile, 0, prec) < lib.neat_sdf_ws_floats(P, 0, prec), (P, prec)
    assert lib.neat_sdf_ldp(0, 2) == 0


def test_tool_workspace_sizes_and_offsets_are_pinned():
    """Python allocates the tools' workspaces from the *_ws_bytes queries and reads parts of them at the offsets neat_show_ws_layout and
    neat_trace_list_offset report, so these values are part of the ABI.  tests/ws_sizes.json is a table (query, arguments) -> value
    recorded from the library before the layouts moved to csrc/ws_layout.hpp: arguments around every tile size (0, 1, 255, 256, 257,
    4096, 4097; grids of 2048 nodes, one tile of the mesh, and of 2050, the nearest above that three axes of two nodes and more can
    make) and arguments each query refuses (0, or None for neat_show_ws_layout's -1).  The queries touch no device.
    neat_post_snap_ws_bytes is pinned where it does not include rocprim's own temporary storage (no lines, refusals)."""
    import json
    from neat_amd import _lib
    lib = _lib.lib()
    table = json.load(open(os.path.join(ROOT, "tests", "ws_sizes.json")))
    queries = {q for q, _, _ in table}
    wanted = {n for n in _lib.exported_symbols() if n.endswith("_ws_bytes")} | {"neat_raycast_bvh_bytes", "neat_show_ws_layout", "neat_trace_list_offset"}
    assert queries == wanted, sorted(queries ^ wanted)
    assert sum(1 for _, args, v in table if not v and min(args) < 0) >= 25          # refusals (a negative count); an empty workspace is 0 too
    for query, args, want in table:
        if query == "neat_show_ws_layout":
            off = (ctypes.c_size_t * 4)()
            got = list(off) if lib.neat_show_ws_layout(*args, off) == 0 else None
        else:
            got = getattr(lib, query)(*args)
        assert got == want, (query, args, got, want)


def test_tuning_keys_retired_and_surviving():
    """neat_set_tuning only writes host switches, so this runs without a GPU.  Every retired key (closed experiments: the key list in
    include/neat_hip.h) is rejected with -1 for every value it once took, its old default included; every surviving key accepts its
    documented default.  Setting a key to its default is also what leaves it there: the switches of this process stay as the other
    tests expect them."""
    from neat_amd import _lib
    lib = _lib.lib()
    retired = (3, 4, 5, 7, 10, 15, 18, 19, 20, 23)
    for key in retired:
        for value in (0, 1, 2, 3, 4, 16, 256):
            assert lib.neat_set_tuning(key, value) == -1, (key, value)
    # key -> documented default (include/neat_hip.h); 17 and 28 are the probe switch and the junction-MLP switch
    defaults = {0: 2, 1: 1, 2: 1, 6: 2, 8: -1, 9: 1, 11: 15, 12: 1, 13: 1, 14: 2, 16: 1, 17: 0, 21: 1, 22: 1, 24: 1, 25: 1, 28: 1}
    assert not set(defaults) & set(retired)
    for key, value in defaults.items():
        assert lib.neat_set_tuning(key, value) == 0, (key, value)
    # the header's key list names exactly these keys, and the retired numbers on one line
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    doc = text[text.index("A/B switches for benchmarking"):text.index("int neat_set_tuning")]
    listed = {int(m) for m in re.findall(r"^ \* {1,3}(\d+) \S", doc, flags=re.M)}
    assert listed == set(defaults), sorted(listed ^ set(defaults))
    assert "Retired keys" in doc and ", ".join(map(str, retired)) in doc
    assert lib.neat_set_tuning(99, 0) == -1


def test_copy_batch_rejects_bad_arguments_before_any_launch():
    """neat_copy_batch validates on the host: more than 16 copies, null tables, misaligned pointers and sizes that are not multiples of 4
    return -1 without touching a device (so this runs without a GPU); zero copies is a no-op."""
    from neat_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    base = ctypes.addressof(buf)
    def call(srcs, dsts, sizes):
        n = len(srcs)
        return lib.neat_copy_batch((ctypes.c_void_p * n)(*srcs), (ctypes.c_void_p * n)(*dsts), (ctypes.c_longlong * n)(*sizes), n, None)
    assert lib.neat_copy_batch(None, None, None, 0, None) == 0
    assert lib.neat_copy_batch(None, None, None, 3, None) == -1
    assert call([base] * 17, [base + 32] * 17, [4] * 17) == -1            # at most 16 per launch (ops.copy_batch chunks)
    assert call([base + 2], [base + 32], [4]) == -1                        # source not 4-byte aligned
    assert call([base], [base + 33], [4]) == -1                            # destination not 4-byte aligned
    assert call([base], [base + 32], [6]) == -1                            # size not a multiple of 4
    assert call([base], [base + 32], [-4]) == -1
    assert call([base, 0], [base + 32, base + 48], [4, 4]) == -1           # a null source


def test_ops_refuse_cpu_tensors():
    import torch
    from neat_amd import networks, synth
    m = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    with pytest.raises(RuntimeError):
        m.implicit_network.get_sdf_vals(torch.zeros(4, 3))      # no CPU fallback: must fail loudly


def test_torch_ops_are_registered_for_the_gpu_only():
    """torch.ops.neat_hip.* (neat_amd/torch_ops.py) exist with tensor/scalar schemas and have no CPU kernel: the dispatcher refuses."""
    import torch
    from neat_amd import torch_ops
    for name in torch_ops.OPS:
        schema = str(getattr(torch.ops.neat_hip, name).default._schema)
        assert schema.startswith(f"neat_hip::{name}("), schema
    with pytest.raises(NotImplementedError):
        torch.ops.neat_hip.volume_weights(torch.zeros(2, 4), torch.zeros(2, 4), torch.ones(1))
    with pytest.raises(NotImplementedError):
        torch.ops.neat_hip.sdf_values(torch.zeros(4, 3), [torch.zeros(1)] * 27, 3.0, 20.0, 0)
