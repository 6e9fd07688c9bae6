"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/neat_hip.h declares; the Python binding, which neat_amd/_lib.py reads from that header, declares the same set with the
types an independent reading of the header gives.  No compute calls (no GPU here)."""
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


def test_binding_agrees_with_an_independent_reading_of_the_header():
    """neat_amd/_lib.py derives restype / argtypes from include/neat_hip.h; this reads the header a second time, with its own
    expressions and without _lib's parser, and checks every entry: return type, argument count, every scalar's ctype, c_void_p for
    every unmarked pointer, and for every NEAT_HOST pointer a POINTER whose element type is the declared base type."""
    from neat_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neat_hip.h")).read(), flags=re.S)
    scalar = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
              "size_t": ctypes.c_size_t, "unsigned char": ctypes.c_ubyte}
    struct = {"neat_net_params": _lib.NetParams, "neat_net_grads": _lib.NetGrads, "neat_eval_grid_t": _lib.EvalGrid}
    assert _lib.c_fp is ctypes.c_void_p
    seen, host = [], 0
    for res, name, params in re.findall(r"^(int|size_t) (neat_[a-z0-9_]+)\(([^)]*)\);", text, flags=re.M):
        seen.append(name)
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is scalar[res], name
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        assert len(params) == len(argtypes), (name, params)
        for p, got in zip(params, argtypes):
            ty = p[:p.rindex(" ")]                                   # without the parameter's name
            if "*" not in ty:
                assert got is scalar[ty], (name, p)
            elif not ty.startswith("NEAT_HOST "):
                assert "NEAT_HOST" not in ty and got is ctypes.c_void_p, (name, p)
            else:
                host += 1
                base, stars = re.fullmatch(r"NEAT_HOST (?:const )?([a-z_ ]+?)(\*| ?\* ?const ?\*)", ty).groups()
                want = ctypes.c_void_p if stars.count("*") == 2 else scalar.get(base) or struct[base]
                assert got is ctypes.POINTER(want) and got._type_ is want, (name, p)
    assert len(seen) >= 134 and len(set(seen)) == len(seen) and sorted(seen) == _lib.exported_symbols() == header_functions()
    assert host >= 49          # the 46 positions the hand-written table typed, and neat_copy_batch's three tables


HEADER_FORMS = """
/* a comment, with (parentheses), commas and a prototype: int neat_not_this(int a, float b); */
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NEAT_HOST   /* expands to nothing */
#define NEAT_NUM_LAYERS 3   /* layers */
#define NEAT_F32 0
typedef struct neat_tagged {
  const float* v[NEAT_NUM_LAYERS];
  float* dv[2];
} neat_tagged;
typedef struct {
  double origin[3];
  double cell;
  int n;
  const int* start;
} neat_plain_t;
int neat_none(void);
size_t neat_scalars(int a, float b, double c, long long d, size_t e);
int neat_pointers(const float* a /* [n,3], (row-major), see f(x, y) */, float* b, unsigned char* c, const long long* d,
                  const void* bvh, void* stream);
int neat_host(NEAT_HOST const double* a, NEAT_HOST int* b, NEAT_HOST const void* const* c, NEAT_HOST void* const* d,
              NEAT_HOST const long long* e, NEAT_HOST size_t* f, NEAT_HOST unsigned char* g, NEAT_HOST const neat_tagged* s,
              NEAT_HOST const neat_plain_t* t, const neat_plain_t* dev);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_on_every_declaration_form():
    from ctypes import POINTER, c_double, c_float, c_int, c_longlong, c_size_t, c_ubyte, c_void_p
    from neat_amd import _lib
    consts, structs, sigs = _lib.parse_header(HEADER_FORMS)
    assert consts == {"NEAT_NUM_LAYERS": 3, "NEAT_F32": 0}
    assert list(structs) == ["neat_tagged", "neat_plain_t"] and all(issubclass(s, ctypes.Structure) for s in structs.values())
    tagged, plain = structs["neat_tagged"], structs["neat_plain_t"]
    assert [(n, t._type_, t._length_) for n, t in tagged._fields_] == [("v", c_void_p, 3), ("dv", c_void_p, 2)]
    assert [n for n, _ in plain._fields_] == ["origin", "cell", "n", "start"]
    assert plain._fields_[0][1]._type_ is c_double and plain._fields_[0][1]._length_ == 3
    assert [t for _, t in plain._fields_[1:]] == [c_double, c_int, c_void_p]
    assert ctypes.sizeof(tagged) == 40 and ctypes.sizeof(plain) == 48 and plain.start.offset == 40
    assert list(sigs) == ["neat_none", "neat_scalars", "neat_pointers", "neat_host"]
    assert sigs["neat_none"] == (c_int, [])
    assert sigs["neat_scalars"] == (c_size_t, [c_int, c_float, c_double, c_longlong, c_size_t])
    assert sigs["neat_pointers"] == (c_int, [c_void_p] * 6)
    assert sigs["neat_host"] == (c_int, [POINTER(c_double), POINTER(c_int), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_longlong),
                                         POINTER(c_size_t), POINTER(c_ubyte), POINTER(tagged), POINTER(plain), c_void_p])
    # what the parser does not know raises and names the entry and the parameter; nothing becomes void* by default
    for bad, words in (("int neat_bad(int a, short b);", ("neat_bad", "short b")),
                       ("int neat_bad(const short* p);", ("neat_bad", "short* p")),
                       ("int neat_bad(NEAT_HOST const neat_unknown_t* p);", ("neat_bad", "neat_unknown_t* p")),
                       ("int neat_bad(const float NEAT_HOST* p);", ("neat_bad", "float NEAT_HOST* p")),
                       ("int neat_bad(NEAT_HOST const void* p);", ("neat_bad", "void* p")),
                       ("int neat_bad(float*** p);", ("neat_bad", "float*** p")),
                       ("int neat_bad(int a,);", ("neat_bad",)),
                       ("typedef struct { int n[NEAT_UNKNOWN]; } neat_bad_t;", ("neat_bad_t", "n[NEAT_UNKNOWN]")),
                       ("short neat_bad(int a);", ("short neat_bad",)),
                       ("unsigned int neat_bad(void);", ("unsigned",)),
                       ("int neat_bad(int a)", ("neat_bad",))):
        with pytest.raises(RuntimeError) as e:
            _lib.parse_header(HEADER_FORMS + bad)
        assert all(w in str(e.value) for w in words), (bad, str(e.value))


def test_missing_header_raises_like_a_missing_library(monkeypatch):
    from neat_amd import _lib
    monkeypatch.delitem(vars(_lib), "_SIGNATURES", raising=False)          # as before the first read; put back afterwards
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="no_such_header.h is missing"):
        _lib.exported_symbols()


def test_struct_layouts_and_header_constants_are_pinned():
    """The structs Python fills are built from the header's typedefs: their sizes, field names and order are what the call sites
    (.v[i], .dv[i], positional EvalGrid(...)) and the library's own layout rely on."""
    from neat_amd import _lib
    assert _lib.NUM_LAYERS == 19
    assert ctypes.sizeof(_lib.NetParams) == ctypes.sizeof(_lib.NetGrads) == 3 * 19 * 8
    assert ctypes.sizeof(_lib.EvalGrid) == 80
    assert [n for n, _ in _lib.EvalGrid._fields_] == ["origin", "cell", "dim", "buckets", "dense", "n", "start", "sidx", "spts"]
    assert _lib.EvalGrid.start.offset == 56
    assert [n for n, _ in _lib.NetParams._fields_] == ["v", "g", "b"] and [n for n, _ in _lib.NetGrads._fields_] == ["dv", "dg", "db"]
    for cls in (_lib.NetParams, _lib.NetGrads):
        assert all(t._type_ is ctypes.c_void_p and t._length_ == 19 for _, t in cls._fields_)
    text = open(os.path.join(ROOT, "include", "neat_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (NEAT_[A-Z0-9_]+) (\d+)\b", text, flags=re.M)}
    assert defines["NEAT_NUM_LAYERS"] == _lib.NUM_LAYERS
    names = {"fp32": "NEAT_F32", "bf16": "NEAT_BF16", "bf16x3": "NEAT_BF16X3", "fp16": "NEAT_F16", "fp16x3": "NEAT_F16X3"}
    assert set(names) == set(_lib.PRECISIONS)
    for key, define in names.items():
        assert _lib.PRECISIONS[key] == defines[define], key
    assert _lib.ABI_VERSION == 15


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
    neat_post_snap_ws_bytes with lines was added when its sort region became sort_scratch_bytes(2 n): those three values are worked out
    by hand from post_snap_layout's region list, every region rounded up to 256 bytes."""
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


def test_model_refuses_cpu_inputs():
    """The model's three entry points refuse host tensors up front, with the exception type and phrase of ops._f32c."""
    import torch
    from neat_amd import networks, synth
    from neat_amd.wireframe import WireframeGraph
    sc = synth.synth_scene(seed=9, n_rays=8)
    inp = {k: torch.tensor(sc[k]) for k in ("intrinsics", "pose", "uv", "uv_proj")}
    inp["wireframe"] = [WireframeGraph(*(torch.tensor(sc[k]) for k in ("wf_vertices", "wf_vconf", "wf_edges", "wf_weights")), 512, 512)]
    m = networks.VolSDFNetwork(synth.ABC_NEAT_A_MODEL_CONF)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(inp)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(inp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.render_rgb(inp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.render_pixels(inp["uv"], inp["pose"], inp["intrinsics"])


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
