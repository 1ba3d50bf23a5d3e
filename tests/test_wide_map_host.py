"""csrc/wide_map.h - the grid arithmetic of demf_mlp_bwd_fused_wide (block id -> column chunk and slab sequence) -
checked by a stand-alone host program (tests/host/wide_map_check.cpp) built with the address and undefined-behaviour
sanitizers: every (chunk, slab) pair visited exactly once, chunk-mates 8 block ids apart.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_wide_block_mapping_covers_every_chunk_and_slab_once(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "wide_map_check")
    src = os.path.join(ROOT, "tests", "host", "wide_map_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "90 cases, 0 failures" in r.stdout
