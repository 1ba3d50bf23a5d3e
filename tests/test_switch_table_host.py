"""The A/B switches have ONE table each - csrc/switches.h for what the library reads (enumerated through
demf_switch_at), demf_amd/switches.py for the Python-only ones - one parse and one read.  No GPU: the library loads
without one (tests/test_abi.py)."""
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT
from demf_amd import _ffi, switches

# a child that loads the library alone (no torch) and prints its table as {name: [value, default]}
CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
name, value, dflt, table, i = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), [], 0
while lib.demf_switch_at(i, ctypes.byref(name), ctypes.byref(value), ctypes.byref(dflt)) == 0:
    table.append([name.value.decode(), value.value, dflt.value])
    i += 1
assert lib.demf_switch_at(i, None, None, None) == -1 and lib.demf_switch_at(-1, None, None, None) == -1
print(json.dumps(table))
"""


def _table(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DEMF_")}
    env.update(extra)
    out = subprocess.run([sys.executable, "-c", CHILD, _ffi.LIB_PATH], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_names_are_unique_and_an_empty_environment_gives_every_default():
    rows = _table()
    names = [r[0] for r in rows]
    assert len(rows) >= 60 and len(set(names)) == len(names)
    assert all(n.startswith("DEMF_") for n in names)
    assert [r for r in rows if r[1] != r[2]] == []
    assert not set(names) & set(switches.TABLE), "a switch belongs to exactly one table"


@pytest.mark.parametrize("bwd", [None, "232"])
def test_set_variables_arrive_and_the_backward_grid_follows_the_documented_fallback(bwd):
    """DEMF_PERSIST_CUS_BWD, then DEMF_PERSIST_CUS, then 240: the table reports the EFFECTIVE value of the _BWD entry,
    the one launch_fused and pool_bwd_grid (csrc/mlp_bwd.hip) size their grids with."""
    extra = dict(DEMF_FWD_RES="0", DEMF_PERSIST_CUS="256")
    if bwd is not None:
        extra["DEMF_PERSIST_CUS_BWD"] = bwd
    got = {n: (v, d) for n, v, d in _table(**extra)}
    want = {"DEMF_FWD_RES": (0, 1), "DEMF_PERSIST_CUS": (256, 240), "DEMF_PERSIST_CUS_BWD": (int(bwd or 256), 240)}
    for n, (v, d) in got.items():
        assert (v, d) == want.get(n, (d, d)), n
    assert {n: d for n, (_, d) in got.items()} == {n: d for n, _, d in _table()}       # defaults do not move


def test_unset_backward_grid_falls_back_to_the_default_of_the_forward_one():
    got = {n: v for n, v, _ in _table(DEMF_PERSIST_CUS_BWD="232")}
    assert got["DEMF_PERSIST_CUS"] == 240 and got["DEMF_PERSIST_CUS_BWD"] == 232


def test_python_readers(monkeypatch):
    monkeypatch.delenv("DEMF_VEC_FIN", raising=False)
    assert switches.env_int("DEMF_VEC_FIN") == 7
    monkeypatch.setenv("DEMF_VEC_FIN", "5")
    assert switches.env_int("DEMF_VEC_FIN") == 5
    monkeypatch.setenv("DEMF_VEC_FIN", "")
    assert switches.env_int("DEMF_VEC_FIN") == 0
    monkeypatch.delenv("DEMF_F16_TERMS", raising=False)
    assert switches.env_int("DEMF_F16_TERMS") == 1          # a library switch: the library's default
    monkeypatch.delenv("DEMF_GEO_AT_BWD", raising=False)
    assert not switches.env_on("DEMF_GEO_AT_BWD")
    monkeypatch.setenv("DEMF_GEO_AT_BWD", "0")              # present means on: bench.py reads it the same way
    assert switches.env_on("DEMF_GEO_AT_BWD")
    with pytest.raises(KeyError):
        switches.env_int("DEMF_NO_SUCH_SWITCH")
    lib = switches.lib_table()
    assert lib["DEMF_X3_MASK"][1] == 7 and switches.lib("DEMF_FWD_RES") in (0, 1)


def test_every_switch_is_documented_in_design_log_section_5():
    text = open(os.path.join(ROOT, "DESIGN_LOG.md")).read()
    sec = text[text.index("\n## 5. Measurement"):text.index("\n## 6. ")]
    missing = [n for n in list(switches.lib_table()) + list(switches.TABLE) if not re.search(r"\b%s\b" % n, sec)]
    assert missing == []


def test_only_the_table_reads_the_environment():
    csrc = os.path.join(ROOT, "demf_amd", "csrc")
    hits = [os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*")) if "getenv" in open(p, errors="replace").read()]
    assert hits == ["switches.hip"]
    bad = []
    for p in glob.glob(os.path.join(ROOT, "demf_amd", "**", "*.py"), recursive=True):
        rel = os.path.relpath(p, os.path.join(ROOT, "demf_amd"))
        if rel == "switches.py":
            continue
        for i, line in enumerate(open(p), 1):
            if re.search(r"environ|getenv", line) and "DEMF_" in line and not line.lstrip().startswith("#"):
                if rel == "_ffi.py" and "DEMF_LIB_PATH" in line and "DEMF_LIB_PATH" in switches.TABLE:
                    continue
                bad.append("%s:%d" % (rel, i))
    assert bad == []


def test_first_use_from_eight_threads_under_the_thread_sanitizer(tmp_path):
    """tests/host/switches_threads.cpp + the host code of csrc/switches.hip as one stand-alone program."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "switches_threads")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-x", "c++",
                    os.path.join(ROOT, "demf_amd", "csrc", "switches.hip"),
                    os.path.join(ROOT, "tests", "host", "switches_threads.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "8 threads, 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
