"""ctypes binding of libneat_hip.so, read from include/neat_hip.h: the header is the only written copy of the C ABI.

parse_header turns its prototypes into restype / argtypes and its struct typedefs into ctypes.Structure classes, once, on the first lib() or
exported_symbols() (or the first use of NUM_LAYERS, NetParams, NetGrads, EvalGrid or _SIGNATURES).  A pointer is passed as an integer address
(c_void_p) unless the header marks it NEAT_HOST: those the library dereferences on the host, and they are typed POINTER(...), so ctypes
refuses anything but an array or byref of that element type (or None).

There is NO fallback: if the shared library or the header is missing, a declaration is not understood or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import re

import torch

ABI_VERSION = 15      # what this package expects of the library (checked against neat_abi_version()); not read from the header
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "fp16x3": 4}
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NEAT_HIP_LIB") or os.path.join(_HERE, "csrc", "libneat_hip.so")      # NEAT_HIP_LIB: a probe build (scripts/probes/abl_build.sh)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "neat_hip.h")

c_fp = ctypes.c_void_p      # a device pointer or an opaque handle (passed as integer addresses)

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
            "size_t": ctypes.c_size_t, "unsigned char": ctypes.c_ubyte}
_STRUCTS = {"neat_net_params": "NetParams", "neat_net_grads": "NetGrads", "neat_eval_grid_t": "EvalGrid"}      # typedef -> module attribute


def _ctype(decl, structs, consts, owner):
    """(name, ctype) of one parameter or struct field `T name` / `T name[N]`.  A pointer is c_fp unless NEAT_HOST leads its type: then
    POINTER(T), or POINTER(c_fp) for a table of pointers (`T* const*`).  Anything else than that raises: nothing defaults to void*."""
    m = re.fullmatch(r"(.*[\s*])(\w+)(?:\[(\w+)\])?", decl.strip(), flags=re.S)
    words = re.sub(r"\bconst\b", " ", m.group(1)).replace("*", " * ").split() if m else []
    host, stars = words[:1] == ["NEAT_HOST"], words.count("*")
    base = " ".join(w for w in words[host:] if w != "*")
    elem = _SCALARS.get(base) or structs.get(base)
    if stars == 0:
        t = _SCALARS.get(base)
    elif stars > 2 or not (elem or base == "void"):
        t = None
    elif not host:
        t = c_fp
    else:
        t = ctypes.POINTER(c_fp) if stars == 2 else elem and ctypes.POINTER(elem)
    count = m and m.group(3) and consts.get(m.group(3), m.group(3))
    if t is None or (count and not str(count).isdigit()):
        raise RuntimeError(f"neat_hip.h: cannot bind `{' '.join(decl.split())}` of {owner}: not a type the binding knows")
    return m.group(2), t * int(count) if count else t


def parse_header(text):
    """(constants, structs, signatures) of a header written like include/neat_hip.h: `#define NAME integer`, `typedef struct [tag] {...} name;`
    -> ctypes.Structure classes with the header's field names and order, `int|size_t name(parameters);` -> name -> (restype, argtypes).
    Whatever else is left outside comments and preprocessor lines raises a RuntimeError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^#define (\w+) (-?\d+)\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    structs, signatures = {}, {}

    def struct(m):
        fields = [_ctype(d, structs, consts, m.group(2)) for d in m.group(1).split(";") if d.strip()]
        structs[m.group(2)] = type(_STRUCTS.get(m.group(2), m.group(2)), (ctypes.Structure,), {"_fields_": fields})
        return ""

    def function(m):
        res, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        signatures[name] = (_SCALARS[res], [_ctype(p, structs, consts, name)[1] for p in params])
        return ""

    text = re.sub(r"\btypedef struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    text = re.sub(r"\b(int|size_t)\s+(\w+)\s*\(([^()]*)\)\s*;", function, text)
    rest = re.sub(r'extern "C" \{|\}', "", text).split()
    if rest:
        raise RuntimeError(f"neat_hip.h: not a declaration the binding knows, near `{' '.join(rest[:8])}`")
    return consts, structs, signatures


def _bind():
    """Reads the header once: from then on NUM_LAYERS, NetParams, NetGrads, EvalGrid and _SIGNATURES are module attributes."""
    g = globals()
    if "_SIGNATURES" not in g:
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f"{HEADER_PATH} is missing: neat_amd reads its ctypes binding from that header and keeps no second copy of it.")
        consts, structs, signatures = parse_header(open(HEADER_PATH).read())
        g.update({attr: structs[name] for name, attr in _STRUCTS.items()}, NUM_LAYERS=consts["NEAT_NUM_LAYERS"], _SIGNATURES=signatures)
    return g["_SIGNATURES"]


def __getattr__(name):      # the header-derived attributes, on their first use
    if name in ("NUM_LAYERS", "_SIGNATURES", *_STRUCTS.values()):
        _bind()
        return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


_lib = None


def exported_symbols():
    """Names of the entry points that include/neat_hip.h declares (the binding is read from that header)."""
    return sorted(_bind())


tuning_overrides = []      # the NEAT_TUNING key=value pairs applied when the library was loaded (bench.py records them)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or neat_amd/csrc/build.sh).  neat_amd has no CPU/PyTorch fallback for the hot path.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _bind().items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
        # A/B switches from the environment (probe scripts; the defaults are what the tests and the bench run):
        # NEAT_TUNING="16=0,21=2" -> neat_set_tuning(16, 0), neat_set_tuning(21, 2)
        applied = []
        for kv in filter(None, os.environ.get("NEAT_TUNING", "").split(",")):
            k, v = kv.split("=")
            check(l.neat_set_tuning(int(k), int(v)), f"NEAT_TUNING {kv}")
            applied.append(kv)
        if applied:       # never silent: a stray variable changes what the tests and the bench measure
            import sys
            print(f"[neat_amd] NEAT_TUNING overrides applied: {','.join(applied)}", file=sys.stderr, flush=True)
        global tuning_overrides
        tuning_overrides = applied
    return _lib


def check(code, what):
    if code != 0:
        raise RuntimeError(f"libneat_hip: {what} failed with code {code}")


def stream():
    """The current stream of the current device, as the library's hipStream_t argument."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """A tensor's device address; NULL for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None
