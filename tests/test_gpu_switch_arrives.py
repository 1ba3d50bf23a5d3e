"""A kernel-form switch must ARRIVE at the dispatch: tests/test_gpu_switches.py compares a step under each setting
with the default step, which a library that ignored its environment would pass.  Here two fresh processes run
tools/switch_forms.py - three shared-MLP forwards whose middle layer reaches the weight-resident, the producer /
consumer and the few-row tile forward of csrc/mlp.hip launch_gemm_t - and report the form demf_mlp_last_form() saw:
with the defaults RES, PC and TILE (recorded on the parent of the commit that introduced the switch table, whose
library still read the environment at each dispatch site: the same three), with DEMF_FWD_RES = DEMF_FWD_PC =
DEMF_FWD_TILE = 0 mlp_gemm_kernel for all three."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GENERIC, TILE, RES, PC = 1, 2, 3, 4     # include/demf_hip.h DEMF_FORM_*
OFF = {"DEMF_FWD_RES": "0", "DEMF_FWD_PC": "0", "DEMF_FWD_TILE": "0"}


def _child(extra):
    env = {k: v for k, v in os.environ.items() if k not in OFF}
    env.update(extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_forms.py")], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, (extra, out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_forward_form_switches_reach_the_dispatch():
    on, off = _child({}), _child(OFF)
    print("defaults", on, " switched off", off)
    assert on["forms"] == [RES, PC, TILE]
    assert off["forms"] == [GENERIC, GENERIC, GENERIC]
    assert on["finite"] and off["finite"]
    assert on["shapes"] == off["shapes"] == [[1024, 64], [1024, 128], [128, 64]]
