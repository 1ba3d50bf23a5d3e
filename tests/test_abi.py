"""The C-ABI library loads without a GPU and exports exactly what include/demf_hip.h
declares; the ctypes table, structs and constants that demf_amd/_ffi.py derives from the header agree with it
as this file's own regex reads it and as a C++ compiler lays it out."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from demf_amd import _ffi


def _header_decls():
    text = open(os.path.join(ROOT, "include", "demf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|const char\*)\s+(demf_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(3).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        decls[m.group(2)] = n
    return decls


def test_library_exports_every_declared_symbol():
    decls = _header_decls()
    assert len(decls) >= 20
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in decls:
        assert hasattr(lib, name), f"{name} declared in demf_hip.h but not exported"


def test_ffi_table_matches_header():
    decls = _header_decls()
    lib = _ffi.load()
    assert lib.demf_version() == 2
    assert lib.demf_last_error() is not None
    for name, argtypes in _ffi.SIGNATURES.items():
        assert name in decls, f"{name} bound in _ffi.py but not declared in the header"
        assert len(argtypes) == decls[name], f"{name}: arity differs from the header"
    bound = set(_ffi.SIGNATURES) | {"demf_version", "demf_last_error"}
    assert bound == set(decls)


PUBLIC = {"demf_version", "demf_last_error", "demf_fps_f32", "demf_ball_query_f32", "demf_group_points_fwd",
          "demf_group_points_bwd", "demf_gather_points_fwd", "demf_gather_points_bwd", "demf_three_nn_f32",
          "demf_three_interpolate_fwd", "demf_three_interpolate_bwd", "demf_msda_fwd_f32", "demf_msda_bwd_f32"}


def test_header_marks_everything_but_the_upstream_shaped_operators_internal():
    """include/demf_hip.h: the entry points with an upstream counterpart (mmdet3d.ops / mmcv.ops) are the public ABI;
    every other declaration carries DEMF_INTERNAL."""
    text = open(os.path.join(ROOT, "include", "demf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    marked = set(re.findall(r"DEMF_INTERNAL[ \t]+int[ \t]+(demf_\w+)\s*\(", text))
    every = set(_header_decls())
    assert PUBLIC <= every
    assert marked == every - PUBLIC, sorted((every - PUBLIC) ^ marked)


def test_bad_arguments_are_reported_not_launched():
    # argument validation happens before any device work, so this runs without a GPU
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_fps_f32", 1, 0, 4, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_ball_query_f32", 1, 8, 2, 0.0, 1.0, 4, None, None, None, None)
    assert b"null pointer" in _ffi.load().demf_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    from demf_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.furthest_point_sample(torch.zeros(1, 8, 3), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ball_query(0.0, 1.0, 4, torch.zeros(1, 8, 3), torch.zeros(1, 2, 3))


SYNTHETIC = """
/* a comment with ; and ( inside: int demf_not_a_function(int x); */
#ifndef T_H_
#define T_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* demf_stream_t;
#define DEMF_INTERNAL
#define DEMF_THREE 3
#define DEMF_NEG (-2)   // trailing; (comment
#define DEMF_BIT (1u << 16)   /* a comment that goes on
                                 over a second line; */
typedef struct demf_t {
  int M, N;
  const float* A; long long s, s2;
  int reserved[7];
  unsigned u;
  double d;   /* int hidden; */
} demf_t;
DEMF_INTERNAL int demf_a(const float* const* srcs, void** out, int64_t* const* out2, const int hws[],
                         long long total,
                         float r, double d, unsigned u,
                         demf_stream_t stream);
int demf_b(void);
const char* demf_c();
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_synthetic_header():
    protos, structs, constants = _ffi.parse_header(SYNTHETIC)
    P = ctypes.c_void_p
    assert protos == {"demf_a": (ctypes.c_int, [P, P, P, P, ctypes.c_longlong, ctypes.c_float, ctypes.c_double,
                                                ctypes.c_uint, P]),
                      "demf_b": (ctypes.c_int, []), "demf_c": (ctypes.c_char_p, [])}
    assert constants == {"DEMF_THREE": 3, "DEMF_NEG": -2, "DEMF_BIT": 65536}
    assert list(structs) == ["demf_t"]
    assert structs["demf_t"]._fields_ == [("M", ctypes.c_int), ("N", ctypes.c_int), ("A", P),
                                          ("s", ctypes.c_longlong), ("s2", ctypes.c_longlong),
                                          ("reserved", ctypes.c_int * 7), ("u", ctypes.c_uint), ("d", ctypes.c_double)]
    assert ctypes.sizeof(structs["demf_t"]) == 8 + 8 + 16 + 28 + 4 + 8


@pytest.mark.parametrize("decl, names", [
    ("int demf_d(int n, size_t bytes);", "demf_d.*size_t"),             # an unknown by-value type
    ("int demf_d(int n, long count);", "demf_d.*long"),
    ("int demf_d(int, int n);", "demf_d"),                              # an unnamed argument
    ("float demf_e(int n);", "float demf_e"),                           # an unknown return type
    ("typedef struct demf_s { short a; } demf_s;", "demf_s.*short"),
    ("typedef int demf_int;", "demf_int"),
    ("#define DEMF_F(x) (x)", "DEMF_F"),
    ("#define DEMF_G DEMF_THREE", "DEMF_G"),
    ("#define DEMF_H (1 << 2", "DEMF_H"),
    ("int demf_d(int n); }", "}"),
])
def test_parser_raises_on_what_it_does_not_know(decl, names):
    with pytest.raises(ValueError, match=names):
        _ffi.parse_header(SYNTHETIC.replace("int demf_b(void);", decl))


def _host_compiler():
    return next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++",
                             "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)


def test_structs_and_constants_match_the_compilers_layout(tmp_path):
    """A generated C++ program prints sizeof / offsetof of every struct of the header and the value of every
    DEMF_* integer macro; the derived ctypes classes and the constants mapping must say the same."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demf_hip.h")).read(), flags=re.S)
    struct_names = re.findall(r"typedef\s+struct\s+(demf_\w+)", text)
    macro_names = re.findall(r"^#define[ \t]+(DEMF_\w+)[ \t]+\S", text, flags=re.M)
    assert set(struct_names) == set(_ffi.STRUCTS) and len(struct_names) == 5
    assert {"DEMF_ABI_VERSION", "DEMF_METER_FLAG_GRAD_NORM", "DEMF_RANKS_MAX"} <= set(macro_names)
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "demf_hip.h"', "int main() {"]
    for s in struct_names:
        lines.append('  std::printf("sizeof %s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in _ffi.STRUCTS[s]._fields_:
            lines.append('  std::printf("field %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (s, f, s, f, s, f))
    for m in macro_names:
        lines.append('  std::printf("define %s %%lld\\n", (long long)(%s));' % (m, m))
    lines += ["  return 0;", "}"]
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   timeout=120)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    got = [ln for ln in out if ln]
    want = []
    for s in struct_names:
        cls = _ffi.STRUCTS[s]
        want.append("sizeof %s %d" % (s, ctypes.sizeof(cls)))
        want += ["field %s %s %d %d" % (s, f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
    want += ["define %s %d" % (m, _ffi.CONSTANTS[m]) for m in macro_names]
    assert got == want
    assert set(macro_names) == set(_ffi.CONSTANTS)
    # no padding the field list does not account for: a field the parser dropped would show here or in sizeof
    for s in struct_names:
        cls = _ffi.STRUCTS[s]
        ends = [getattr(cls, f).offset + getattr(cls, f).size for f, _ in cls._fields_]
        starts = [getattr(cls, f).offset for f, _ in cls._fields_][1:] + [ctypes.sizeof(cls)]
        assert all(0 <= b - a < 8 for a, b in zip(ends, starts)), s
    assert (ctypes.sizeof(_ffi.DwJob), ctypes.sizeof(_ffi.DetectLayer), ctypes.sizeof(_ffi.GemmDesc),
            ctypes.sizeof(_ffi.Ctx), ctypes.sizeof(_ffi.OptState)) == (96, 120, 280, 32, 64)


HEADER_NAMES = {
    "ops": dict(NMS_MAX_SEGMENT="DEMF_NMS_MAX_SEGMENT", TTA_MAX_CANDIDATES="DEMF_TTA_MAX_CANDIDATES",
                EVAL_MAX_PRED_PER_SEGMENT="DEMF_EVAL_MAX_PRED_PER_SEGMENT",
                EVAL_MAX_GT_PER_SEGMENT="DEMF_EVAL_MAX_GT_PER_SEGMENT", RANKS_MAX="DEMF_RANKS_MAX",
                DETECT_MAX_LAYERS="DEMF_DETECT_MAX_LAYERS", FRAME_TILE="DEMF_FRAME_TILE",
                METER_ROW_WORDS="DEMF_METER_ROW_WORDS", METER_HEAD_WORDS="DEMF_METER_HEAD_WORDS",
                METER_MAX_SCALARS="DEMF_METER_MAX_SCALARS", METER_FLAG_GRAD_NORM="DEMF_METER_FLAG_GRAD_NORM"),
    "fused": dict(RELU="DEMF_GEMM_RELU", DROPOUT="DEMF_GEMM_DROPOUT", GATE="DEMF_GEMM_GATE", ACCUM="DEMF_GEMM_ACCUM",
                  ROWBIAS="DEMF_GEMM_ROWBIAS", ACCUM2="DEMF_GEMM_ACCUM2"),
    "meter": dict(ROW_WORDS="DEMF_METER_ROW_WORDS", HEAD_WORDS="DEMF_METER_HEAD_WORDS",
                  MAX_SCALARS="DEMF_METER_MAX_SCALARS", FLAG_GRAD_NORM="DEMF_METER_FLAG_GRAD_NORM"),
}


def test_python_names_are_the_headers_values_and_no_literal_copy_is_left():
    import importlib
    for mod, names in HEADER_NAMES.items():
        m = importlib.import_module("demf_amd." + mod)
        for py, c in names.items():
            assert getattr(m, py) == _ffi.CONSTANTS[c], (mod, py)
    assert (_ffi.CONSTANTS["DEMF_NMS_MAX_SEGMENT"], _ffi.CONSTANTS["DEMF_RANKS_MAX"],
            _ffi.CONSTANTS["DEMF_METER_FLAG_GRAD_NORM"], _ffi.CONSTANTS["DEMF_GEMM_ACCUM2"]) == (1024, 64, 1 << 16, 32)
    every = {py for names in HEADER_NAMES.values() for py in names}
    bad = []
    for p in glob.glob(os.path.join(ROOT, "demf_amd", "**", "*.py"), recursive=True):
        for i, line in enumerate(open(p), 1):
            m = re.match(r"([A-Z][A-Z0-9_]*(?:, [A-Z][A-Z0-9_]*)*) = (.*)", line)       # a module-level assignment
            if m and every & set(m.group(1).split(", ")) and re.search(r"\b\d", m.group(2).split("#")[0]):
                bad.append("%s:%d" % (os.path.relpath(p, ROOT), i))
    for p in glob.glob(os.path.join(ROOT, "demf_amd", "csrc", "*")):
        for i, line in enumerate(open(p, errors="replace"), 1):
            if re.search(r"\b(kNmsMax|kMergeMaxCand|kMatchMaxGt|kMatchMaxPred|kFrameTile|\w*RANKS_MAX|\w*DETECT_MAX_LAYERS)"
                         r"\s*=\s*\d", line) or re.search(r"\bstruct\s+\w*OptState\b", line):
                bad.append("%s:%d" % (os.path.relpath(p, ROOT), i))
    assert bad == []
