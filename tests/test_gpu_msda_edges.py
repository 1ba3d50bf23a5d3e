"""The multi-scale deformable attention kernels of csrc/msda.hip, launched directly through _ffi.call with raw pointers
(pitches, column offsets, alignment and null arguments are the test's choice), against the float64 C oracle with the
per-element bounds of tests/msda_reference.py, at every kernel instantiation and launch edge (shapes and their reasons:
tests/msda_cases.py; ``form_of`` there names the instantiation each case runs).

Pass rules (derived in msda_reference's docstring):
  every output element            |got - ref64| <= c(n) * 2^-24 * sum|term| + coordinate term (+ softmax term for the
                                  raw forms), for EVERY element; no element is excluded
  bit for bit                     an output element with no valid term is +0.0; grad_loc and grad_attw of a sample
                                  with no valid corner are 0; a grad_value element with no contribution keeps its
                                  prefill; the bf16 entries equal the f32 entries on the widened rows (out, grad_loc,
                                  grad_attw)
Every output lives between sentinel bands, which must keep their bits.  Overwritten outputs start as NaN and must end
without one; grad_value starts from its prefill, which enters the reference as one more term; a NULL grad_value is
allocated all the same and keeps every bit.  Every bounded check prints its worst ratio before asserting."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import msda_cases as mc
import msda_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT_BITS = np.array([mc.SENTINEL], F32).view(np.uint32)[0]
NAN_BITS = np.uint32(0x7FC00000)
SWITCHES = ("DEMF_MSDA_RAW_LANES", "DEMF_MSDA_XCD", "DEMF_MSDA_NT", "DEMF_MSDA_HEAD_WGS")


def _call(name, *args):
    from demf_amd import _ffi
    _ffi.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, shift=0):
    """-> (tensor that owns the memory, pointer): the bytes of ``a`` on the GPU, ``shift`` 4-byte words off 16-byte
    alignment."""
    words = np.ascontiguousarray(a).reshape(-1).view(np.uint32)
    host = np.zeros(words.size + 4, np.uint32)
    host[shift:shift + words.size] = words
    t = torch.from_numpy(host.view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


class _Out:
    """``shape`` 4-byte words between two sentinel bands (the `_Out` pattern of test_gpu_gather_edges): .ptr for the
    kernel, .get(dtype) the values, .check() the bands, .untouched() every bit.  ``fill``: None = sentinel, "nan" =
    quiet NaNs (an output the kernel overwrites), or the values an accumulating kernel starts from.  ``shift``: words
    by which .ptr is off 16-byte alignment.  ``device=False``: host side only, for a buffer another process fills
    (.before goes out, .result comes back)."""

    def __init__(self, shape, fill=None, shift=0, device=True):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.guard = 64 + shift
        host = np.full(self.guard + self.n + 64, SENT_BITS, np.uint32)
        inner = slice(self.guard, self.guard + self.n)
        if isinstance(fill, str):
            host[inner] = NAN_BITS
        elif fill is not None:
            host[inner] = _bits(np.broadcast_to(fill, self.shape)).reshape(-1)
        self.before, self.inner, self.result = host, inner, None
        if device:
            self.buf = torch.from_numpy(host.view(np.int32)).cuda()
            assert self.buf.data_ptr() % 16 == 0
            self.ptr = self.buf.data_ptr() + 4 * self.guard

    def _now(self):
        return self.result if self.result is not None else self.buf.cpu().numpy().view(np.uint32)

    def get(self, dtype=F32):
        return self._now()[self.inner].view(dtype).reshape(self.shape)

    def check(self, label):
        now = self._now()
        assert now.shape == self.before.shape, label
        assert np.array_equal(now[:self.guard], self.before[:self.guard]), label + ": band in front was written"
        assert np.array_equal(now[self.inner.stop:], self.before[self.inner.stop:]), label + ": band behind was written"

    def untouched(self, label):
        assert np.array_equal(self._now(), self.before), label + ": was written"


def _bounded(label, what, got, want, bound):
    """One output against the float64 reference: no NaN left from the prefill, then the bound on EVERY element."""
    assert got.shape == want.shape == bound.shape, (label, what, got.shape, want.shape, bound.shape)
    assert not np.isnan(got).any(), "%s %s: a NaN of the prefill is left, or one was computed" % (label, what)
    ratio = np.abs(got.astype(F64) - want) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    print("msda-edges %-28s %-7s worst |err| / bound %.3f  (%d elements)" % (label, what, worst, got.size))
    assert worst <= 1.0, "%s %s: worst ratio %.3f over the bound, at %s: got %r want %r" % (
        label, what, worst, np.unravel_index(ratio.argmax(), ratio.shape), got.reshape(-1)[ratio.argmax()], want.reshape(-1)[ratio.argmax()])


@pytest.fixture(scope="module", autouse=True)
def _default_switches():
    """``form_of`` names the kernels under the switch values the cases were written for: this process runs with them."""
    from demf_amd import switches
    got = {k: switches.lib(k) for k in SWITCHES}
    assert got == mc.DEFAULT_SWITCHES, got


# ---- direct entries --------------------------------------------------------------------------------------------------
def _run_direct(name, c, d, sfx, value):
    """Forward and backward of demf_msda_{fwd,bwd}_<sfx> on one case -> dict of the outputs as _Out."""
    B, Q, H, Dh, L, P, S = tuple(c[k] for k in ("B", "Q", "H", "Dh", "L", "P")) + (d["S"],)
    keep = [_dev(value, c["value_shift"]), _dev(d["shapes"]), _dev(d["lsi"]), _dev(d["loc"]), _dev(d["attw"]),
            _dev(d["gout"], c["gout_shift"])]
    (_, pv), (_, ps), (_, pl), (_, ploc), (_, pw), (_, pg) = keep
    o = dict(out=_Out((B, Q, H * Dh), "nan", shift=c["out_shift"]), gloc=_Out((B, Q, H, L, P, 2), "nan"),
             gattw=_Out((B, Q, H, L, P), "nan"), gvalue=_Out((B, S, H, Dh), d["prefill"]))
    _call("demf_msda_fwd_" + sfx, B, S, H, Dh, L, Q, P, pv, ps, pl, ploc, pw, o["out"].ptr)
    _call("demf_msda_bwd_" + sfx, B, S, H, Dh, L, Q, P, pv, ps, pl, ploc, pw, pg,
          o["gvalue"].ptr if d["prefill"] is not None else None, o["gloc"].ptr, o["gattw"].ptr)
    torch.cuda.synchronize()
    del keep
    return o


def _judge_direct(name, c, d, o):
    j = ref.judge(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], d["gout"], d["prefill"], d["eps"],
                  want_gvalue=d["prefill"] is not None)
    for k in ("out", "gloc", "gattw"):
        o[k].check("%s %s" % (name, k))
    out, gloc, gattw = o["out"].get(), o["gloc"].get(), o["gattw"].get()
    assert not _bits(out)[j.out_zero].any(), name + ": an output element with no valid term is not +0.0"
    _bounded(name, "out", out, j.out, j.out_bound)
    assert not gloc[j.dead].any() and not gattw[j.dead].any(), name + ": a gradient of a sample with no valid corner"
    _bounded(name, "gloc", gloc, j.gloc, j.gloc_bound)
    _bounded(name, "gattw", gattw, j.gattw, j.gattw_bound)
    if d["prefill"] is None:
        o["gvalue"].untouched(name + " gvalue (NULL was passed)")
        return
    o["gvalue"].check(name + " gvalue")
    gv, none = o["gvalue"].get(), j.gvalue.hits == 0
    assert none.any() and np.array_equal(_bits(gv)[none], _bits(d["prefill"])[none]), name + ": a grad_value element without a contribution changed"
    _bounded(name, "gvalue", gv, j.gvalue.value, j.gvalue_bound)


@pytest.mark.parametrize("name", list(mc.DIRECT))
def test_direct_f32(name):
    c = mc.DIRECT[name][0]
    d = mc.direct_inputs(name, c)
    print("msda-edges %s runs %s" % (name, mc.form_of(c)))
    _judge_direct(name, c, d, _run_direct(name, c, d, "f32", d["value"]))


@pytest.mark.parametrize("name", list(mc.BF16))
def test_direct_bf16(name):
    """The 2-byte rows against float64 on the widened values, and bit for bit against the f32 entries on them."""
    c = mc.BF16[name][0]
    d = mc.direct_inputs(name, c)
    print("msda-edges %s runs %s" % (name, mc.form_of(c)))
    o = _run_direct(name, c, d, "bf16", d["value_bits"])
    _judge_direct(name, c, d, o)
    wide = _run_direct(name, c, d, "f32", d["value"])
    for k in ("out", "gloc", "gattw"):
        assert np.array_equal(_bits(o[k].get()), _bits(wide[k].get())), "%s %s: bf16 and f32 entries differ on the same rows" % (name, k)


# ---- raw entries -----------------------------------------------------------------------------------------------------
def _raw_args(c, d, dev=_dev):
    """Upload a raw case -> (keep, the raw entry's arguments without out)."""
    keep = [dev(d["vbuf"]), dev(d["shapes"]), dev(d["lsi"]), dev(d["raw"], c["raw_shift"]), dev(d["ref"], c["ref_shift"])]
    (_, pv), (_, ps), (_, pl), (_, praw), (_, pref) = keep
    return keep, (pv + 4 * c["v_off"], c["vpitch"], ps, pl, praw, c["ldraw"], c["off_col0"], c["lgt_col0"], pref)


def _judge_raw(name, c, d, out):
    j = ref.judge(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], eps=d["eps"], attw_err=d["attw_err"])
    out.check(name)
    got = out.get()
    assert not _bits(got)[j.out_zero].any(), name + ": an output element with no valid term is not +0.0"
    _bounded(name, "out", got, j.out, j.out_bound)


@pytest.mark.parametrize("name", list(mc.RAW))
def test_raw_entry(name):
    c = mc.RAW[name][0]
    d = mc.raw_inputs(name, c)
    print("msda-edges %s runs %s" % (name, mc.form_of(c)))
    keep, args = _raw_args(c, d)
    out = _Out((c["B"], c["Q"], c["H"] * 32), "nan")
    _call("demf_msda_fwd_raw_f32", c["B"], d["S"], c["H"], 32, 4, c["Q"], c["P"], *args, out.ptr)
    torch.cuda.synchronize()
    _judge_raw(name, c, d, out)


@pytest.mark.parametrize("name", list(mc.HEAD))
def test_head_entry(name):
    """demf_msda_fwd_raw_head_f32 called directly (the S >= 2048 gate is in ops.msda_fwd_raw, not in the library),
    judged against float64 like every other form."""
    c = mc.HEAD[name][0]
    d = mc.raw_inputs(name, c)
    print("msda-edges %s runs %s, (chunks, queries per chunk, passes) = %s" % (name, mc.form_of(c), mc.head_chunks(c)))
    keep, args = _raw_args(c, d)
    out = _Out((c["B"], c["Q"], 256), "nan")
    _call("demf_msda_fwd_raw_head_f32", c["B"], d["S"], c["Q"], c["P"], *args, out.ptr, c["first"], d["staged"])
    torch.cuda.synchronize()
    _judge_raw(name, c, d, out)


# ---- the wave form under DEMF_MSDA_XCD=1 DEMF_MSDA_NT=0: one child process -----------------------------------------
CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from demf_amd import _ffi, switches
jobs = np.load(sys.argv[2])
meta = json.loads(str(jobs["meta"]))
res = {}
for i, m in enumerate(meta):
    t = {k: torch.from_numpy(jobs["%d_%s" % (i, k)]).cuda() for k in ("vbuf", "shapes", "lsi", "raw", "ref", "out")}
    p = {k: v.data_ptr() for k, v in t.items()}
    _ffi.call("demf_msda_fwd_raw_f32", m["B"], m["S"], 8, 32, 4, m["Q"], m["P"], p["vbuf"] + 4 * m["v_off"], m["vpitch"],
              p["shapes"], p["lsi"], p["raw"], m["ldraw"], m["off_col0"], m["lgt_col0"], p["ref"], p["out"] + 4 * m["guard"],
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res["%d_out" % i] = t["out"].cpu().numpy()
np.savez(sys.argv[3], **res)
print("SWITCHES " + json.dumps({k: switches.lib(k) for k in sys.argv[4:]}))
"""


def test_wave_form_in_xcd_order_with_plain_loads(tmp_path):
    """One child, started once, runs every row of XCD under DEMF_MSDA_XCD=1 DEMF_MSDA_NT=0 (the grid rounded up to a
    multiple of 8 blocks, the blocks past the end leaving; msda_fwd_raw_wave_kernel<.., NT = false>) and writes the
    output buffers, bands included, to a file; they are judged here by the rules of the in-process cases."""
    cases = {n: (c, mc.raw_inputs(n, c)) for n, (c, _) in mc.XCD.items()}
    outs, arrays, meta = {}, {}, []
    for i, (n, (c, d)) in enumerate(cases.items()):
        assert mc.form_of(c, mc.CHILD_SWITCHES) == ["msda_fwd_raw_wave_kernel<4,%d,false>" % c["P"], "xcd block order"]
        outs[n] = _Out((c["B"], c["Q"], 256), "nan", device=False)
        for k in ("vbuf", "raw", "ref"):
            arrays["%d_%s" % (i, k)] = d[k]
        arrays["%d_shapes" % i], arrays["%d_lsi" % i] = d["shapes"], d["lsi"]
        arrays["%d_out" % i] = outs[n].before.view(np.int32)
        meta.append(dict({k: c[k] for k in ("B", "Q", "P", "v_off", "vpitch", "ldraw", "off_col0", "lgt_col0")},
                         S=d["S"], guard=outs[n].guard))
    jobs, done = str(tmp_path / "jobs.npz"), str(tmp_path / "done.npz")
    np.savez(jobs, meta=json.dumps(meta), **arrays)
    env = dict(os.environ, DEMF_MSDA_XCD="1", DEMF_MSDA_NT="0")
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, jobs, done] + list(SWITCHES), capture_output=True, text=True,
                         timeout=120, env=env)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, run.stderr[-2000:]
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("SWITCHES ")][-1]
    assert json.loads(line[9:]) == mc.CHILD_SWITCHES, line
    got = np.load(done)
    for i, (n, (c, d)) in enumerate(cases.items()):
        outs[n].result = got["%d_out" % i].view(np.uint32)
        _judge_raw(n, c, d, outs[n])


# ---- refusals and early returns -------------------------------------------------------------------------------------
def _arguments(entry, change):
    """The accepted call of mc.ACCEPTED with ``change`` applied: every pointer a banded buffer of its own."""
    from demf_amd import _ffi
    values = dict(mc.ACCEPTED[entry])
    null = change.get("null")
    values.update({k: v for k, v in change.items() if k != "null"})
    values, bufs, args = list(values.values()), [], []
    for t in _ffi.SIGNATURES[entry][:-1]:                      # (the last pointer is the stream)
        if t is ctypes.c_void_p:
            bufs.append(_Out((4096,), None))
            args.append(None if null == len(bufs) - 1 else bufs[-1].ptr)
        else:
            args.append(values.pop(0))
    assert not values
    return bufs, args


@pytest.mark.parametrize("entry,change,why", mc.REFUSED,
                         ids=["%s-%s" % (e[10:], "_".join("%s%s" % kv for kv in ch.items())) for e, ch, _ in mc.REFUSED])
def test_refused_calls_write_nothing(entry, change, why):
    bufs, args = _arguments(entry, change)
    with pytest.raises(RuntimeError):
        _call(entry, *args)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        b.untouched("%s %s (%s) pointer %d" % (entry, change, why, k))


@pytest.mark.parametrize("entry,change", mc.RETURNS_EARLY,
                         ids=["%s-%s0" % (e[10:], list(ch)[0]) for e, ch in mc.RETURNS_EARLY])
def test_empty_calls_return_without_writing(entry, change):
    bufs, args = _arguments(entry, change)
    _call(entry, *args)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        b.untouched("%s %s pointer %d" % (entry, change, k))
