"""ctypes binding of libdemf_hip.so, derived from the C ABI declared in include/demf_hip.h.

The reference reaches its native operators through pybind extensions of mmdet3d/mmcv; this is the equivalent thin
layer.  cffi is not installed in the target image, so the binding is ctypes.  There is no fallback: if the library
is missing, ``load()`` raises.

The header is the one source: every ``.hip`` includes it, so a definition that disagrees with its prototype
does not compile, and the argument types, structs and constants below are read from it at import.  A
declaration the parser does not know raises; it never guesses.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEMF_LIB_PATH") or os.path.join(_HERE, "lib", "libdemf_hip.so")     # (A/B builds)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "demf_hip.h")

_BY_VALUE = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
             "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint, "demf_stream_t": ctypes.c_void_p}
_DECLARATOR = re.compile(r"(.*?)\b(\w+)\s*(?:\[\s*(\d+)\s*\])?", re.S)


def _declarator(text, where, base=None):
    """'const float* x' / 'long long n' / 'int reserved[7]' -> (name, the base type's text, ctypes class).  Pointers
    are c_void_p; ``base``: the type of a further declarator of 'int M, N, K'."""
    m = _DECLARATOR.fullmatch(text.strip())
    if m is None:
        raise ValueError(f"{where}: cannot read the declaration {text.strip()!r}")
    ctype, name, dim = m.groups()
    ctype = base if base is not None and not ctype.strip() else ctype
    key = " ".join(t for t in ctype.split() if t != "const")
    if "*" in key:
        cls = ctypes.c_void_p
    elif key in _BY_VALUE:
        cls = _BY_VALUE[key]
    else:
        raise ValueError(f"{where}: unknown by-value type {key!r} in {text.strip()!r}")
    return name, ctype, cls * int(dim) if dim else cls


def _struct(name, body):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base = None
        for part in decl.split(","):
            field, base, cls = _declarator(part, f"struct {name}", base)
            fields.append((field, cls))
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"include/demf_hip.h: {name}"})


def _int_expr(text, where):
    """Value of '3', '(-1)' or '(1u << 16)': an integer, optionally shifted, optionally in parentheses."""
    m = re.fullmatch(r"(\()?\s*(-?\d+|0[xX][0-9a-fA-F]+)[uUlL]*\s*(?:<<\s*(\d+)\s*)?(?(1)\))", text)
    if m is None:
        raise ValueError(f"{where}: cannot evaluate {text!r}")
    return int(m.group(2), 0) << int(m.group(3) or 0)


def parse_header(text):
    """-> (prototypes: name -> (restype, [argtypes]), structs: name -> ctypes.Structure class, constants: name -> int)
    of a header in the style of include/demf_hip.h."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, flags=re.M):
        if m.group(2).strip():                      # (a bare name is a marker: the include guard, DEMF_INTERNAL)
            constants[m.group(1)] = _int_expr(m.group(2).strip(), "#define " + m.group(1))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\bDEMF_INTERNAL\b|extern\s+"C"\s*\{', " ", text)
    struct = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
    structs = {m.group(1): _struct(m.group(1), m.group(2)) for m in struct.finditer(text)}
    *decls, tail = struct.sub("", text).split(";")
    protos = {}
    for decl in decls:
        decl = " ".join(decl.split())
        f = re.fullmatch(r"(int|const char ?\*) ?(demf_\w+) ?\(([^(){}]*)\)", decl)
        if f:
            args = f.group(3).strip()
            protos[f.group(2)] = (ctypes.c_int if f.group(1) == "int" else ctypes.c_char_p,
                                  [] if args in ("", "void") else
                                  [ctypes.c_void_p if "*" in a or "[" in a else _declarator(a, f.group(2))[2]
                                   for a in args.split(",")])
        elif decl != "typedef void* demf_stream_t":
            raise ValueError(f"unknown declaration: {decl!r}")
    if tail.strip() not in ("", "}"):                   # (the brace that closes extern "C")
        raise ValueError(f"unknown declaration: {tail.strip()!r}")
    return protos, structs, constants


with open(HEADER_PATH) as _f:
    _PROTOS, STRUCTS, CONSTANTS = parse_header(_f.read())
# name -> argtypes of every entry point that returns a status (demf_version / demf_last_error: see load())
SIGNATURES = {n: a for n, (_, a) in _PROTOS.items() if n not in ("demf_version", "demf_last_error")}
DwJob, DetectLayer, GemmDesc, Ctx, OptState = (STRUCTS["demf_" + n] for n in
                                               ("dw_job", "detect_layer", "gemm_desc", "ctx", "opt_state"))

_lib = None


def load():
    """Load libdemf_hip.so; raises if it has not been built (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). demf_amd has no CPU fallback.")
    # torch first: PyTorch-ROCm bundles its own HIP / HSA runtime; if this library were loaded before
    # it, the process would hold two runtimes and the second one finds no device ("no ROCm-capable
    # device is detected" at the first launch - seen with build() and smoke() in one process)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def call(name, *args):
    """Invoke an entry point; a non-zero return becomes a RuntimeError with the
    library's thread-local message (the upstream pybind wrappers raise likewise)."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.demf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (code {rc}): {msg}")
