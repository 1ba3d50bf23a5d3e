"""The package's environment switches: ONE table for the Python-only ones, and the library's own table
(csrc/switches.h, through demf_switch_at) for every switch a kernel launch reads.

Read times: module-level constants of ops.py / modules/image_stream.py call ``env_int`` at import; engine.py and
ops.set_compute_dtype call the readers when they run, so a test may change the environment inside one process.
``lib`` answers what the LIBRARY runs with: it parses its table once per process, at the first call that needs one.
"""
import ctypes
import os

# name -> (default, meaning).  None: a "present means on" switch (``env_on``) or a string (``env_str``)
TABLE = {
    "DEMF_LIB_PATH": (None, "string: another libdemf_hip.so to load (A/B builds; read in _ffi.py at import)"),
    "DEMF_ALLOW_LIBRARY_FALLBACK": (0, "allow rocBLAS / MIOpen fall-backs of the module paths"),
    "DEMF_DEFER_DW": (1, "queue the few-row weight-gradient products into one grouped launch"),
    "DEMF_BQ_GRID_MIN_N": (8192, "smallest cloud for the cell-grid ball query"),
    "DEMF_MSDA_HEAD": (1, "the (scene, head)-major encoder attention"),
    "DEMF_OWN_GEMM_ROWS": (65536, "rows above which ops.linear runs this package's own GEMM"),
    "DEMF_NO_FPS_CHECK": (0, "1 = no FPS order check against the level below"),
    "DEMF_NO_RED_FUSE": (0, "1 = dX without the fused BN-backward reduce"),
    "DEMF_NO_FIRST_FUSE": (0, "1 = first layer without the fused epilogue"),
    "DEMF_NO_BWD_FUSE": (0, "1 = no one-pass backward kernels"),
    "DEMF_BF16_STORE": (0, "bf16 row storage of SA1's stack in the bf16 mode"),
    "DEMF_VEC_FIN": (7, "in-kernel backward vectors: bit 0 sparse reduce, 1 fused, 2 dx_red"),
    "DEMF_FUSED_COLS_MIN_R": (0, "rows from which 256-output layers take the per-chunk one-pass backward; 0 = never"),
    "DEMF_FUSED_WIDE_MIN_R": (16384, "rows from which they take the one-launch wide one-pass backward; 0 = never"),
    "DEMF_POOL_NOY": (1, "SA1's pooled last layer without its stored output"),
    "DEMF_SA1_X4": (1, "SA1's first layer without its stored output"),
    "DEMF_NO_GROUP_FIRST": (0, "1 = no group-first first layer"),
    "DEMF_NO_FUSED_POOL": (0, "1 = max-pool as a launch of its own"),
    "DEMF_ENC_FUSED": (1, "encoder layers on the row-GEMM chain kernels"),
    "DEMF_IMG_NHWC": (1, "channels-last image stream"),
    "DEMF_IMG_CONV": (1, "ResNet + neck on this package's convolution kernels"),
    "DEMF_MIOPEN_SEARCH": (0, "MIOpen exhaustive search (library path only)"),
    "DEMF_ENC_PRE_ADD": (0, "encoder: query + pos added ahead of the projection"),
    "DEMF_ENC_SPLIT_LN": (1, "encoder FFN: LayerNorm as its own launch"),
    "DEMF_DETR2D_FUSED": (1, "2D detector: decoder and head on the row-GEMM / attention / selection kernels"),
    "DEMF_DETR2D_VALUE_ONE": (1, "2D detector: the six layers' value projections of the memory as one launch"),
    "DEMF_AR_OVERLAP": (0, "all-reduce overlapped with the backward"),
    "DEMF_GRAPH_UPDATE": (1, "optimizer update inside the captured step"),
    "DEMF_GRAPH_ALLREDUCE": (0, "all-reduce inside the captured step"),
    "DEMF_ZERO_COPY_TOKENS": (1, "captured step reads the image tokens in place"),
    "DEMF_DIST_BACKEND": (None, "string: torch.distributed backend (default nccl on a GPU, gloo otherwise)"),
    # present means on, whatever the value ("0" included): bench.py reads DEMF_GEO_AT_BWD this way too
    "DEMF_GEO_AT_BWD": (None, "retired: capture() refuses (was: forward and backward as two graphs, pre-pass between)"),
    "DEMF_GEO_TWO_DEEP": (None, "retired: capture() refuses (was: coordinate pre-pass two steps ahead)"),
    "DEMF_SKIP_GEO": (None, "present = replay without the pre-pass (measurement only)"),
    "DEMF_SHARE_DEVICE": (None, "present = every rank on GPU 0 (test hook, with DEMF_DIST_BACKEND=gloo)"),
}

_lib_table = None


def lib_table():
    """{name: (value, default)} of the library's switches, as the library itself parsed them."""
    global _lib_table
    if _lib_table is None:
        from . import _ffi
        fn, table, i = _ffi.load().demf_switch_at, {}, 0
        name, value, dflt = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        while fn(i, ctypes.byref(name), ctypes.byref(value), ctypes.byref(dflt)) == 0:
            table[name.value.decode()] = (value.value, dflt.value)
            i += 1
        _lib_table = table
    return _lib_table


def lib(name):
    """The value the library runs with (fixed for the process)."""
    return lib_table()[name][0]


def default(name):
    """A switch's default, from whichever table has it."""
    return TABLE[name][0] if name in TABLE else lib_table()[name][1]


def env_int(name):
    """An integer switch read from the environment NOW: unset = the table's default, empty = 0."""
    v = os.environ.get(name)
    return default(name) if v is None else int(v or 0)


def env_nonzero(name):
    """Set and non-zero, read NOW: for a switch that is off unless set, so that no default - and for a library switch
    (DEMF_F32_NATIVE at the import of ops.py) no library - is needed."""
    return bool(int(os.environ.get(name) or 0))


def env_on(name):
    """A "present means on" switch: any non-empty value, "0" included."""
    assert TABLE[name][0] is None, name
    return bool(os.environ.get(name))


def env_str(name):
    assert TABLE[name][0] is None, name
    return os.environ.get(name) or None
