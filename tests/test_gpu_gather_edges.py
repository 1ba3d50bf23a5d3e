"""The gather / scatter kernels of csrc/group_gather.hip and the interpolation kernels of csrc/three_nn_interp.hip,
launched directly through _ffi.call with raw pointers (pitches, column offsets, alignment and null arguments are the
test's choice), against the float64 restatement of tests/gather_reference.py at every dispatch branch and launch edge
(shapes and their reasons: tests/gather_cases.py).

Pass rules, all derived:
  copies and index outputs        bit for bit (gathers, the rows of group_concat with +0.0 pad columns, maxpool values
                                  and arg, CSR offsets and lists)
  rel_xyz                         bit for bit against (fl32(p) - fl32(q)) / fl32(r) in numpy float32
  interpolation forward           bit for bit against fma(w2, f2, fma(w0, f0, fl32(w1 * f1)))
  every summed output             |got - ref64| <= (n + 2) * 2^-24 * sum|term| + 2^-126 for EVERY element, n the number
                                  of terms, prefill included; an element with no term keeps its prefill to the bit
                                  (+0.0 in the gather form)
Every output lives between sentinel bands, which must keep their bits.  Overwritten outputs start as NaN and must end
without one; accumulating outputs start from a random prefill, which enters the reference as one more term.  Every
summed check prints its worst ratio before asserting."""
import ctypes
import hashlib
import subprocess
import sys

import numpy as np
import pytest
import torch

import gather_cases as gc
import gather_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT_BITS = np.array([gc.SENTINEL], F32).view(np.uint32)[0]
NAN_BITS = np.uint32(0x7FC00000)
UNWRITTEN = F32(1234.5)             # prefill of the columns a pitched output must not write


def _call(name, *args):
    from demf_amd import _ffi
    _ffi.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, shift=0):
    """-> (tensor that owns the memory, pointer): ``a`` on the GPU, ``shift`` 4-byte words off 16-byte alignment."""
    a = np.ascontiguousarray(a)
    host = np.zeros(a.size + 4, np.uint32)
    host[shift:shift + a.size] = a.reshape(-1).view(np.uint32)
    t = torch.from_numpy(host.view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


class _Out:
    """``shape`` 4-byte words between two sentinel bands (the `_Out` pattern of test_gpu_dense_rows_edges): .ptr for
    the kernel, .get(dtype) the values, .check() the bands, .untouched() every bit.  ``fill``: None = sentinel,
    "nan" = quiet NaNs (an output the kernel overwrites), or the values an accumulating kernel starts from.
    ``shift``: words by which .ptr is off 16-byte alignment."""

    def __init__(self, shape, fill=None, pitch=4, shift=0):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.guard = (max(4 * pitch, 16) + 3) // 4 * 4 + shift
        host = np.full(self.guard + self.n + 16, SENT_BITS, np.uint32)
        inner = slice(self.guard, self.guard + self.n)
        if isinstance(fill, str):
            host[inner] = NAN_BITS
        elif fill is not None:
            host[inner] = _bits(np.broadcast_to(fill, self.shape)).reshape(-1)
        self.before, self.inner = host, inner
        self.buf = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 4 * self.guard

    def _now(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def get(self, dtype=F32):
        return self._now()[self.inner].view(dtype).reshape(self.shape)

    def check(self, label):
        now = self._now()
        assert np.array_equal(now[:self.guard], self.before[:self.guard]), label + ": band in front was written"
        assert np.array_equal(now[self.inner.stop:], self.before[self.inner.stop:]), label + ": band behind was written"

    def untouched(self, label):
        assert np.array_equal(self._now(), self.before), label + ": was written"


def _same_bits(label, got, want):
    """A copy / an index output: every element bit for bit, and no NaN left from the prefill."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first at %s: got %r want %r" % (
        label, bad.size, got.size, np.unravel_index(bad[0], got.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
    if got.dtype == F32:
        assert not np.isnan(got).any(), label


def _judge_sum(label, out, s, prefill=None):
    """One summed output against its Sum: bands, the elements without a term, then the bound on every element."""
    torch.cuda.synchronize()
    out.check(label)
    got = out.get()
    err = np.abs(got.astype(F64) - s.value)
    ratio = float((err / s.bound()).max()) if err.size else 0.0
    print("gather-edges %-46s worst |err| / bound %.3f  (n up to %d, %d elements, %d without a term)" % (
        label, ratio, int(s.n.max()) if s.n.size else 0, got.size, int((s.hits == 0).sum())))
    none = s.hits == 0
    keep = np.zeros(got.shape, F32) if prefill is None else np.broadcast_to(np.asarray(prefill, F32), got.shape)
    assert np.array_equal(_bits(got)[none], _bits(keep)[none]), label + ": an element without a term changed"
    assert ratio <= 1.0, "%s: worst ratio %.3f over the bound" % (label, ratio)
    return got


def _split(J):
    """M * ns = J with ns > 1 where J allows."""
    for ns in (4, 3):
        if J % ns == 0:
            return J // ns, ns
    return J, 1


# ---- channel-major: group_points, gather_points ---------------------------------------------------------------------
@pytest.mark.parametrize("J", gc.CM_J)
@pytest.mark.parametrize("C", gc.CM_C)
def test_group_points_and_gather_points(C, J):
    B, N = 2, gc.CM_N
    M, ns = _split(J)
    for same in (False, True):
        rng = gc.gen("group_cm_%d_%d_%d" % (C, J, same))
        idx = gc.indices(rng, B, J, N, same=same)
        feat, gout, pre = gc.normal(rng, B, C, N), gc.normal(rng, B, C, J), gc.normal(rng, B, C, N)
        want, s = ref.group_points(feat, idx), ref.group_points_bwd(gout, idx, N, pre)
        (_, d_idx), (_, d_feat), (_, d_gout) = keep = [_dev(idx), _dev(feat), _dev(gout)]
        for entry, dims in (("demf_group_points", (B, C, N, M, ns)), ("demf_gather_points", (B, C, N, J))):
            label = "%s C%d J%d%s" % (entry[5:], C, J, " same" if same else "")
            out = _Out((B, C, J), "nan", pitch=J)
            _call(entry + "_fwd", *dims, d_feat, d_idx, out.ptr)
            torch.cuda.synchronize()
            out.check(label)
            _same_bits(label + " fwd", out.get(), want)
            gfeat = _Out((B, C, N), pre, pitch=N)
            _call(entry + "_bwd", *dims, d_gout, d_idx, gfeat.ptr)
            _judge_sum(label + " bwd", gfeat, s, pre)
        del keep


# ---- group_concat_cl_fwd --------------------------------------------------------------------------------------------
def _concat_inputs(kind, name, c):
    rng = gc.gen("concat_%s_%s" % (kind, name))
    B, N, M, ns, C = c["B"], c["N"], c["M"], c["ns"], c["C"]
    idx = gc.indices(rng, B, M * ns, N, same=c["same"]).reshape(B, M, ns)
    return rng, idx, gc.normal(rng, B, N, 3), gc.normal(rng, B, M, 3), gc.normal(rng, B, N, C)


@pytest.mark.parametrize("name", list(gc.GROUP_CONCAT_FWD))
def test_group_concat_cl_fwd(name):
    c = gc.GROUP_CONCAT_FWD[name][0]
    B, N, M, ns, C, ldo = c["B"], c["N"], c["M"], c["ns"], c["C"], c["ldo"]
    _, idx, xyz, center, feat = _concat_inputs("fwd", name, c)
    want = ref.group_concat(xyz, center, feat if C else None, idx, ldo, c["xyz_col"], c["feat_col"], gc.RADIUS, c["normalize"])
    keep = [_dev(xyz), _dev(center), _dev(feat, c["feat_shift"]), _dev(idx)]
    out = _Out((B, M, ns, ldo), "nan", pitch=ldo, shift=c["out_shift"])
    _call("demf_group_concat_cl_fwd", B, N, M, ns, C, ldo, c["xyz_col"], c["feat_col"], gc.RADIUS, c["normalize"],
          keep[0][1], keep[1][1], keep[2][1] if C else None, keep[3][1], out.ptr)
    torch.cuda.synchronize()
    out.check(name)
    got = out.get()
    pad = np.ones(ldo, bool)
    pad[c["xyz_col"]:c["xyz_col"] + 3] = False
    pad[c["feat_col"]:c["feat_col"] + C] = False
    assert not _bits(got[..., pad]).any(), name + ": a pad column is not +0.0"
    _same_bits(name + " feature columns", got[..., c["feat_col"]:c["feat_col"] + C], want[..., c["feat_col"]:c["feat_col"] + C])
    _same_bits(name + " rel_xyz", got[..., c["xyz_col"]:c["xyz_col"] + 3], want[..., c["xyz_col"]:c["xyz_col"] + 3])
    _same_bits(name, got, want)


# ---- group_concat_cl_bwd (atomic scatter) ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", gc.GROUP_CONCAT_BWD_FORMS)
@pytest.mark.parametrize("name", list(gc.GROUP_CONCAT_BWD))
def test_group_concat_cl_bwd(name, form):
    c = gc.GROUP_CONCAT_BWD[name][0]
    B, N, M, ns, C, ldo = c["B"], c["N"], c["M"], c["ns"], c["C"], c["ldo"]
    rng, idx, _, _, _ = _concat_inputs("bwd", name, c)
    gout = gc.normal(rng, B, M, ns, ldo)
    pre = dict(feat=gc.normal(rng, B, N, C), xyz=gc.normal(rng, B, N, 3), center=gc.normal(rng, B, M, 3))
    with_feat, with_xyz = form in ("feat_and_xyz", "feat_only"), form in ("feat_and_xyz", "xyz_only")
    sums = dict(zip(("feat", "xyz", "center"), ref.group_concat_bwd(
        gout, idx, N, C, c["xyz_col"], c["feat_col"], gc.RADIUS, c["normalize"], pre["feat"], pre["xyz"], pre["center"])))
    outs = dict(feat=_Out((B, N, C), pre["feat"], pitch=max(C, 1)), xyz=_Out((B, N, 3), pre["xyz"]),
                center=_Out((B, M, 3), pre["center"]))
    keep = [_dev(gout, c["out_shift"]), _dev(idx)]
    _call("demf_group_concat_cl_bwd", B, N, M, ns, C, ldo, c["xyz_col"], c["feat_col"], gc.RADIUS, c["normalize"],
          keep[0][1], keep[1][1], outs["feat"].ptr if with_feat else None, outs["xyz"].ptr if with_xyz else None,
          outs["center"].ptr if with_xyz else None)
    torch.cuda.synchronize()
    for k, o in outs.items():
        label = "concat_bwd %s %s %s" % (name, form, k)
        if (with_feat and C > 0) if k == "feat" else with_xyz:
            _judge_sum(label, o, sums[k], pre[k])
        else:
            o.untouched(label)             # a null output is allocated all the same and keeps every bit


# ---- demf_invert_index / demf_invert_index_ws -----------------------------------------------------------------------
def _invert(form, B, N, E, d_idx):
    """Run the inversion in ``form`` -> (off, rows) as _Out.  The dispatcher picks the form from the shape and the
    workspace: lists that fit LDS stay there; without a workspace the rest takes the global-list form, with one the
    five launches."""
    from demf_amd import switches
    assert gc.fits_lds(N, E) == (form == "lds")
    off, rows = _Out((B, N + 1), "nan", pitch=16), _Out((B, E), "nan", pitch=16)
    if form == "split":
        assert switches.lib("DEMF_INVERT_SPLIT") == 1, "the split form is chosen by its default switch value"
        ws = _Out((B, max(E, 1)), None, pitch=16)
        _call("demf_invert_index_ws", B, N, E, d_idx, off.ptr, rows.ptr, ws.ptr)
        torch.cuda.synchronize()
        ws.check("invert %s workspace" % form)
    else:
        _call("demf_invert_index", B, N, E, d_idx, off.ptr, rows.ptr)
    torch.cuda.synchronize()
    return off, rows


def _check_lists(label, off, rows, want_off, want_rows):
    off.check(label + " off")
    rows.check(label + " rows")
    _same_bits(label + " off", off.get(np.int32), want_off)
    _same_bits(label + " rows", rows.get(np.int32), want_rows)


@pytest.mark.parametrize("form,N,E", [(f, n, e) for f, shapes in gc.INVERT.items() for n, e in shapes])
def test_invert_index(form, N, E):
    B = 2
    idx = gc.invert_indices(form, N, E, B)
    want_off, want_rows = ref.invert_index(idx, N)
    keep = _dev(idx)
    off, rows = _invert(form, B, N, E, keep[1])
    _check_lists("invert %s N%d E%d" % (form, N, E), off, rows, want_off, want_rows)
    if E:
        print("gather-edges invert %-6s N %5d E %5d  longest list %d" % (form, N, E, int(np.diff(want_off, axis=1).max())))


def test_invert_index_rejects_more_points_than_its_histogram_holds():
    B, N, E = 1, 16385, 8
    keep = _dev(np.zeros((B, E), np.int32))
    off, rows = _Out((B, N + 1)), _Out((B, E))
    with pytest.raises(RuntimeError, match="exceeds"):
        _call("demf_invert_index", B, N, E, keep[1], off.ptr, rows.ptr)
    torch.cuda.synchronize()
    off.untouched("off")
    rows.untouched("rows")


FRESH_N, FRESH_E, FRESH_B, FRESH_LONG = 16384, 30000, 2, 400
CHILD = """
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
N, E, B, LONG = (int(a) for a in sys.argv[2:6])
idx = np.random.default_rng(5).integers(0, N, (B, E)).astype(np.int32)
idx[:, :LONG] = 7
import torch
from demf_amd import _ffi
lib = _ffi.load()
d_idx = torch.from_numpy(idx).cuda()
off = torch.empty((B, N + 1), dtype=torch.int32, device="cuda")
rows = torch.empty((B, E), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
# the first kernel launch of this process
rc = lib.demf_invert_index(B, N, E, d_idx.data_ptr(), off.data_ptr(), rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
msg = lib.demf_last_error().decode("utf-8", "replace") if rc else ""
torch.cuda.synchronize()
h = hashlib.sha256(off.cpu().numpy().tobytes() + rows.cpu().numpy().tobytes()).hexdigest()
print("RC %d SHA %s MSG %s" % (rc, h, msg))
"""


def test_global_list_invert_index_as_the_first_launch_of_a_fresh_process():
    """The global-list form asks for 4 * (2N + 1) bytes of dynamic LDS (131 076 at N = 16 384) next to 4 KB of static;
    here it is the first launch of a process in which nothing has raised invert_index_k's dynamic-LDS limit through
    the LDS-list path.  The launch must be accepted and the lists exact.  (On the MI355X it is: the runtime takes the
    launch without a raised limit, so the dispatcher reserves LDS for the LDS-list form alone.)"""
    assert not gc.fits_lds(FRESH_N, FRESH_E)
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT] + [str(v) for v in (FRESH_N, FRESH_E, FRESH_B, FRESH_LONG)],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RC ")][-1].split(" ", 5)
    assert line[1] == "0", "the launch was refused: " + " ".join(line)
    idx = np.random.default_rng(5).integers(0, FRESH_N, (FRESH_B, FRESH_E)).astype(np.int32)
    idx[:, :FRESH_LONG] = 7
    off, rows = ref.invert_index(idx, FRESH_N)
    assert line[3] == hashlib.sha256(off.tobytes() + rows.tobytes()).hexdigest(), "offsets or lists differ from the reference"


# ---- group_concat_cl_bwd_gather -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.BWD_GATHER))
def test_group_concat_cl_bwd_gather(name):
    c = gc.BWD_GATHER[name][0]
    B, N, E, C, ldo, col, lists = c["B"], c["N"], c["E"], c["C"], c["ldo"], c["feat_col"], c["lists"]
    rng = gc.gen("bwd_gather_" + name)
    idx = gc.list_indices(rng, B, N, E, lists)
    gout = gc.normal(rng, B, E, ldo)
    want_off, want_rows = ref.invert_index(idx, N)
    keep = [_dev(gout), _dev(idx)]
    if lists in gc.INVERT:                      # offsets and lists made on the GPU, in that form
        off, rows = _invert(lists, B, N, E, keep[1][1])
        _check_lists("bwd_gather %s lists" % name, off, rows, want_off, want_rows)
        p_off, p_rows = off.ptr, rows.ptr
    else:
        keep += [_dev(want_off), _dev(want_rows)]
        p_off, p_rows = keep[2][1], keep[3][1]
    if lists == "lengths":
        assert set(gc.LIST_LENGTHS) <= set(np.diff(want_off[0]))
    s = ref.gather_sum(gout, want_off, want_rows, C, col)
    assert (s.hits == 0).any(), "a point that nobody gathered"
    gfeat = _Out((B, N, C), "nan", pitch=C)
    _call("demf_group_concat_cl_bwd_gather", B, N, E, C, ldo, col, keep[0][1], p_off, p_rows, gfeat.ptr)
    got = _judge_sum("bwd_gather %s" % name, gfeat, s)
    assert not np.isnan(got).any()
    # the atomic scatter of the same gradient (entries as M = E rows of one neighbour), onto zeros
    atomic = _Out((B, N, C), np.zeros((B, N, C), F32), pitch=C)
    _call("demf_group_concat_cl_bwd", B, N, E, 1, C, ldo, 0, col, 1.0, 0, keep[0][1], keep[1][1], atomic.ptr, None, None)
    got_atomic = _judge_sum("bwd_gather %s (atomic form)" % name, atomic, s)
    diff = np.abs(got.astype(F64) - got_atomic.astype(F64))
    assert (diff <= 2 * s.bound()).all(), "%s: gather and atomic forms differ by %.3f bounds" % (name, (diff / s.bound()).max())


# ---- gather_rows_cl -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.GATHER_ROWS))
def test_gather_rows_cl(name):
    c = gc.GATHER_ROWS[name][0]
    B, N, M, C = c["B"], c["N"], c["M"], c["C"]
    rng = gc.gen("gather_rows_" + name)
    idx = gc.indices(rng, B, M, N, same=c["same"])
    feat, gout, pre = gc.normal(rng, B, N, C), gc.normal(rng, B, M, C), gc.normal(rng, B, N, C)
    keep = [_dev(feat), _dev(idx), _dev(gout)]
    out = _Out((B, M, C), "nan", pitch=C)
    _call("demf_gather_rows_cl_fwd", B, N, M, C, keep[0][1], keep[1][1], out.ptr)
    torch.cuda.synchronize()
    out.check(name)
    _same_bits("gather_rows " + name, out.get(), ref.gather_rows(feat, idx))
    gfeat = _Out((B, N, C), pre, pitch=C)
    _call("demf_gather_rows_cl_bwd", B, N, M, C, keep[2][1], keep[1][1], gfeat.ptr)
    _judge_sum("gather_rows_bwd " + name, gfeat, ref.gather_rows_bwd(gout, idx, N, pre), pre)


# ---- interpolation --------------------------------------------------------------------------------------------------
def _interp_want(feat_cl, idx, w):
    """The pinned fma chain, point-major: float64 restatement, the C oracle's fma where a float64 sum was inexact."""
    from oracle import kernels as ok
    out, exact = ref.three_interpolate_cl(feat_cl, idx, w)
    if not exact.all():
        fma = ok.three_interpolate_fwd(np.ascontiguousarray(np.swapaxes(feat_cl, 1, 2)), idx, w)
        out = np.where(exact, out, np.swapaxes(fma, 1, 2))
    return out


@pytest.mark.parametrize("n", gc.CM_J)
@pytest.mark.parametrize("C", gc.CM_C)
def test_three_interpolate_channel_major(C, n):
    for m in (gc.CM_N, 1):                       # (one source: every entry the same index)
        _run_interp_cm(2, C, m, n)


def _run_interp_cm(B, C, m, n):
    label = "C%d n%d m%d" % (C, n, m)
    rng = gc.gen("interp_cm_" + label)
    idx, w = gc.triplets(rng, B, n, m)
    feat, gout, pre = gc.normal(rng, B, C, m), gc.normal(rng, B, C, n), gc.normal(rng, B, C, m)
    keep = [_dev(feat), _dev(idx), _dev(w), _dev(gout)]
    out = _Out((B, C, n), "nan", pitch=n)
    _call("demf_three_interpolate_fwd", B, C, m, n, keep[0][1], keep[1][1], keep[2][1], out.ptr)
    torch.cuda.synchronize()
    out.check("interp_cm " + label)
    want = np.swapaxes(_interp_want(np.ascontiguousarray(np.swapaxes(feat, 1, 2)), idx, w), 1, 2)
    _same_bits("interp_cm " + label, out.get(), want)
    gfeat = _Out((B, C, m), pre, pitch=m)
    _call("demf_three_interpolate_bwd", B, C, n, m, keep[3][1], keep[1][1], keep[2][1], gfeat.ptr)
    _judge_sum("interp_cm_bwd " + label, gfeat, ref.three_interpolate_bwd(gout, idx, w, m, pre), pre)


def _run_interp_cl(label, B, m, n, C, ldo, col0, Cs=0):
    """Forward into columns [col0, col0 + C (+ Cs)) of rows of ``ldo`` floats that start as UNWRITTEN; backward from
    the same columns of a full random grad_out onto a random prefill."""
    rng = gc.gen("interp_cl_" + label)
    idx, w = gc.triplets(rng, B, n, m)
    feat, gout, pre = gc.normal(rng, B, m, C), gc.normal(rng, B, n, ldo), gc.normal(rng, B, m, C)
    skip = gc.normal(rng, B, n, Cs) if Cs else None
    keep = [_dev(feat), _dev(idx), _dev(w), _dev(gout)] + ([_dev(skip)] if Cs else [])
    out = _Out((B, n, ldo), UNWRITTEN, pitch=ldo)
    if Cs:
        assert ldo == C + Cs and col0 == 0
        _call("demf_three_interpolate_cat_cl_fwd", B, m, n, C, Cs, keep[0][1], keep[1][1], keep[2][1], keep[4][1], out.ptr)
    else:
        _call("demf_three_interpolate_cl_fwd", B, m, n, C, ldo, col0, keep[0][1], keep[1][1], keep[2][1], out.ptr)
    torch.cuda.synchronize()
    out.check(label)
    want = np.full((B, n, ldo), UNWRITTEN, F32)
    want[..., col0:col0 + C] = _interp_want(feat, idx, w)
    if Cs:
        want[..., C:] = skip
    _same_bits("interp_cl " + label, out.get(), want)
    gfeat = _Out((B, m, C), pre, pitch=C)
    _call("demf_three_interpolate_cl_bwd", B, m, n, C, ldo, col0, keep[3][1], keep[1][1], keep[2][1], gfeat.ptr)
    s = ref.three_interpolate_cl_bwd(gout[..., col0:col0 + C], idx, w, m, pre)
    _judge_sum("interp_cl_bwd " + label, gfeat, s, pre)
    if m >= 4:
        assert (s.hits[:, gc.unused(m)] == 0).all()


@pytest.mark.parametrize("name", list(gc.INTERP_CL))
def test_three_interpolate_cl(name):
    c = gc.INTERP_CL[name][0]
    _run_interp_cl(name, c["B"], c["m"], c["n"], c["C"], c["C"] + c["pad"], c["col0"])


@pytest.mark.parametrize("Cs", gc.INTERP_CAT_CS)
@pytest.mark.parametrize("C", [1, 65, 256])
def test_three_interpolate_cat_cl(C, Cs):
    _run_interp_cl("cat_C%d_Cs%d" % (C, Cs), 2, 300, 9, C, C + Cs, 0, Cs=Cs)


# ---- maxpool_ns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.MAXPOOL))
def test_maxpool_ns(name):
    c = gc.MAXPOOL[name][0]
    R, ns, C = c["R"], c["ns"], c["C"]
    x = gc.maxpool_input(name, R, ns, C)
    gout = gc.normal(gc.gen("maxpool_g" + name), R, C)
    best, arg = ref.maxpool_ns(x)
    assert (arg[1] == 0).all() and np.isneginf(best[1]).all() and (arg[3:, 0] == 0).all()
    if ns > 1:
        assert (arg[2] == ns - 1).all()
        assert C == 1 or (np.isposinf(best).any() and (arg > 0).any())
    keep = [_dev(x), _dev(gout), _dev(arg)]
    out, oarg = _Out((R, C), "nan", pitch=C), _Out((R, C), "nan", pitch=C)
    _call("demf_maxpool_ns_fwd", R, ns, C, keep[0][1], out.ptr, oarg.ptr)
    gx = _Out((R, ns, C), "nan", pitch=C)
    _call("demf_maxpool_ns_bwd", R, ns, C, keep[1][1], keep[2][1], gx.ptr)
    torch.cuda.synchronize()
    for o in (out, oarg, gx):
        o.check("maxpool " + name)
    _same_bits("maxpool %s values" % name, out.get(), best)
    _same_bits("maxpool %s arg" % name, oarg.get(np.int32), arg)
    _same_bits("maxpool %s bwd" % name, gx.get(), ref.maxpool_ns_bwd(gout, arg, ns))


# ---- colsum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", gc.COLSUM_LD_EXTRA)
@pytest.mark.parametrize("N", gc.COLSUM_N)
def test_colsum(N, extra):
    """Rows around the rows-per-block of the switch table; x aligned and 4 bytes off; out holds a non-zero prefill and
    8 more floats behind the N columns, which stay as they are."""
    from demf_amd import switches
    rpb, ld = switches.lib("DEMF_COLSUM_ROWS"), N + extra
    worst = 0.0
    for R in gc.colsum_rows(rpb):
        if R < 1:
            continue
        for shift in (0, 1):
            rng = gc.gen("colsum_%d_%d_%d_%d" % (N, extra, R, shift))
            xfull, pre = gc.normal(rng, R, ld), gc.normal(rng, N + 8)
            keep = _dev(xfull, shift)
            out = _Out((N + 8,), pre, pitch=4)
            _call("demf_colsum_f32", R, N, ld, keep[1], out.ptr)
            s = ref.colsum(xfull[:, :N], pre[:N])
            tail = ref.Sum(pre[N:].astype(F64), np.ones(8, np.int64), np.abs(pre[N:].astype(F64)), np.zeros(8, np.int64))
            both = ref.Sum(*[np.concatenate([a, b]) for a, b in zip(s, tail)])
            _judge_sum("colsum N%d ld%d R%d x+%d" % (N, ld, R, 4 * shift), out, both, pre)


# ---- early returns --------------------------------------------------------------------------------------------------
# entry -> argument values in front of the pointers, one of the sizes 0
EARLY = [
    ("demf_group_points_fwd", (0, 4, 9, 3, 2)), ("demf_group_points_fwd", (2, 0, 9, 3, 2)), ("demf_group_points_fwd", (2, 4, 9, 0, 2)),
    ("demf_group_points_bwd", (0, 4, 9, 3, 2)), ("demf_group_points_bwd", (2, 0, 9, 3, 2)), ("demf_group_points_bwd", (2, 4, 9, 0, 2)),
    ("demf_gather_points_fwd", (0, 4, 9, 3)), ("demf_gather_points_fwd", (2, 0, 9, 3)), ("demf_gather_points_fwd", (2, 4, 9, 0)),
    ("demf_gather_points_bwd", (0, 4, 9, 3)), ("demf_gather_points_bwd", (2, 0, 9, 3)), ("demf_gather_points_bwd", (2, 4, 9, 0)),
    ("demf_group_concat_cl_fwd", (0, 9, 3, 2, 4, 8, 4, 0, 0.3, 1)), ("demf_group_concat_cl_fwd", (2, 9, 0, 2, 4, 8, 4, 0, 0.3, 1)),
    ("demf_group_concat_cl_bwd", (0, 9, 3, 2, 4, 8, 4, 0, 0.3, 1)), ("demf_group_concat_cl_bwd", (2, 9, 0, 2, 4, 8, 4, 0, 0.3, 1)),
    ("demf_gather_rows_cl_fwd", (0, 9, 3, 4)), ("demf_gather_rows_cl_fwd", (2, 9, 0, 4)), ("demf_gather_rows_cl_fwd", (2, 9, 3, 0)),
    ("demf_gather_rows_cl_bwd", (0, 9, 3, 4)), ("demf_gather_rows_cl_bwd", (2, 9, 0, 4)), ("demf_gather_rows_cl_bwd", (2, 9, 3, 0)),
    ("demf_three_interpolate_fwd", (0, 4, 9, 3)), ("demf_three_interpolate_fwd", (2, 0, 9, 3)), ("demf_three_interpolate_fwd", (2, 4, 9, 0)),
    ("demf_three_interpolate_bwd", (0, 4, 3, 9)), ("demf_three_interpolate_bwd", (2, 0, 3, 9)), ("demf_three_interpolate_bwd", (2, 4, 0, 9)),
    ("demf_three_interpolate_cl_fwd", (0, 9, 3, 4, 8, 2)), ("demf_three_interpolate_cl_fwd", (2, 9, 0, 4, 8, 2)),
    ("demf_three_interpolate_cl_fwd", (2, 9, 3, 0, 8, 2)),
    ("demf_three_interpolate_cl_bwd", (0, 9, 3, 4, 8, 2)), ("demf_three_interpolate_cl_bwd", (2, 9, 0, 4, 8, 2)),
    ("demf_three_interpolate_cl_bwd", (2, 9, 3, 0, 8, 2)),
    ("demf_three_interpolate_cat_cl_fwd", (0, 9, 3, 4, 2)), ("demf_three_interpolate_cat_cl_fwd", (2, 9, 0, 4, 2)),
    ("demf_maxpool_ns_fwd", (0, 2, 4)), ("demf_maxpool_ns_fwd", (3, 2, 0)),
    ("demf_maxpool_ns_bwd", (0, 2, 4)), ("demf_maxpool_ns_bwd", (3, 2, 0)),
    ("demf_colsum_f32", (0, 4, 4)), ("demf_colsum_f32", (3, 0, 4)),
    ("demf_invert_index", (0, 9, 5)), ("demf_invert_index_ws", (0, 9, 5)),
    ("demf_group_concat_cl_bwd_gather", (0, 9, 5, 4, 8, 4)),
]


@pytest.mark.parametrize("entry,values", EARLY, ids=["%s-%s" % (e[5:], "_".join(str(v) for v in a)) for e, a in EARLY])
def test_early_returns_write_nothing(entry, values):
    """B = 0, M = 0, C = 0 or n = 0: the entry point returns success before it launches; every buffer it was handed,
    inputs included, keeps every bit."""
    from demf_amd import _ffi
    sig = _ffi.SIGNATURES[entry][:-1]                       # (the last pointer is the stream)
    values, bufs, args = list(values), [], []
    for t in sig:
        if t is ctypes.c_void_p:
            bufs.append(_Out((64,), None))
            args.append(bufs[-1].ptr)
        else:
            args.append(values.pop(0))
    assert not values
    _call(entry, *args)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        b.untouched("%s %s pointer %d" % (entry, args, k))
