"""Which kernel form every layer of the model's own shared-MLP stacks takes, forward and backward, read off the two pure
plan functions of demf_amd/ops.py (_fwd_plan, _bwd_forms / _bwd_form) - no GPU: the functions take sizes and flags
only, and the library (for switches.lib) loads without a device.

The stacks are SA1 .. SA4 and the vote aggregation at the benchmarked size (8 scenes), rows and channels from
demf_amd/config.py.  The expected forms are read from the conditions in ops.py; where tests/shared_mlp_trace.json has a
case of the same shape (SA1 at 16 384 / 16 320 rows, 256 -> 256 -> 256 at 16 384 / 16 368 rows) they were confirmed
against the launches recorded there.  A pull request that adds a kernel form states its dispatch rule here."""
import contextlib

import pytest

from demf_amd import ops, switches
from demf_amd.config import DeMFCfg

B = 8
CFG = DeMFCfg()


def _stacks():
    """name -> (R, ld, ns, shapes, has_geo, x_requires_grad) as demf_amd/modules/pointnet2.py calls the node."""
    bb, head, out = CFG.backbone, CFG.head, {}
    c = bb.in_channels - 3
    for i, (M, ns, chans) in enumerate(zip(bb.num_points, bb.num_samples, bb.sa_channels)):
        geo = c % 4 == 0 and c > 0                  # group-first first layer: feature rows of the source points
        k, shapes = c + 3, []
        for n in chans:
            shapes.append((n, k))
            k = n
        out["sa%d" % (i + 1)] = (B * M * ns, c if geo else c + 3, ns, shapes, geo, i > 0)
        c = chans[-1]
    k, shapes = head.agg_mlp_channels[0] + 3, []
    for n in head.agg_mlp_channels[1:]:
        shapes.append((n, k))
        k = n
    out["agg"] = (B * head.num_proposal * head.agg_num_sample, head.agg_mlp_channels[0], head.agg_num_sample, shapes,
                  True, True)
    return out


STACKS = _stacks()
# the boundary: SA1's stack and the aggregation's widths as plain stacks at 16 384 rows and one group less
STACKS.update({
    "sa1_at": (16384, 4, 64, STACKS["sa1"][3], False, False),
    "sa1_under": (16384 - 64, 4, 64, STACKS["sa1"][3], False, False),
    "wide_at": (16384, 128, 16, [(256, 128), (256, 256), (256, 256)], False, True),
    "wide_under": (16384 - 16, 128, 16, [(256, 128), (256, 256), (256, 256)], False, True),
})


@contextlib.contextmanager
def _setting(attrs, mode):
    prev = {k: getattr(ops, k) for k in list(attrs) + ["_COMPUTE_MODE"]}
    try:
        for k, v in attrs.items():
            setattr(ops, k, v)
        ops._COMPUTE_MODE = ops._COMPUTE_MODES[mode]      # (the plan reads the mode; no kernel runs here)
        yield
    finally:
        for k, v in prev.items():
            setattr(ops, k, v)


def _forms(name):
    R, ld, ns, shapes, geo, xgrad = STACKS[name]
    plan = ops._fwd_plan(R, ld, ns, shapes, True, geo, xgrad)
    _, bwd = ops._bwd_forms(plan, R, ld, ns, shapes, xgrad, geo)
    return plan.fwd, [(l, f.form, f.variant, f.first_tail) for l, f in bwd.items()]


def _two(l, variant):
    return (l, "two_launch", variant, False)


GEO_FWD = ("group_first", "bn", "pool")
GEO_BWD = [(2, "fused", None, False), (1, "fused", None, False), (0, "geo_first", None, False)]
GEO_BWD_TWO = [_two(2, "dx_red_v"), _two(1, "dx_red_v"), (0, "geo_first", None, False)]
SA1_STORED = (("bn", "bn", "pool"), [(2, "fused", None, False), (1, "fused_first", None, False)])
SA1_TWO = (("bn", "bn", "pool"), [_two(2, "dx_red_v"), (1, "two_launch", None, True)])
WIDE_FWD = ("bn", "bn", "pool")
DEFAULT = {
    "sa1": (("first_stats", "bn_x4", "pool_noy"), [(2, "pool_noy", None, False), (1, "fused_first", "x4", False)]),
    "sa2": (GEO_FWD, GEO_BWD),
    "sa3": (GEO_FWD, GEO_BWD),
    "sa4": (GEO_FWD, GEO_BWD),
    "agg": (GEO_FWD, [(2, "fused_wide", None, False), (1, "fused_wide", None, False), (0, "geo_first", None, False)]),
    "sa1_under": SA1_STORED,                                   # the no-store forms start at 16 384 rows
    "wide_at": (WIDE_FWD, [(2, "fused_wide", None, False), (1, "fused_wide", None, False), _two(0, "dx_w")]),
    "wide_under": (WIDE_FWD, [_two(2, "dx_red_v"), _two(1, "dx_red_v"), _two(0, "dx_w")]),
}
DEFAULT["sa1_at"] = DEFAULT["sa1"]
NO_FUSE = dict(DEFAULT, sa1=SA1_TWO, sa1_at=SA1_TWO, sa1_under=SA1_TWO, sa2=(GEO_FWD, GEO_BWD_TWO), sa3=(GEO_FWD, GEO_BWD_TWO),
               sa4=(GEO_FWD, GEO_BWD_TWO), agg=(GEO_FWD, GEO_BWD_TWO), wide_at=DEFAULT["wide_under"])
SA1_Y = (("first_stats", "bn_x4", "pool"), [(2, "fused", None, False), (1, "fused_first", "x4", False)])
SA1_Y0 = (("bn", "bn", "pool_noy"), [(2, "pool_noy", None, False), (1, "fused_first", None, False)])
SA1_ST16 = (("bn", "bn_st16", "pool_st16"), [(2, "fused", None, False), (1, "fused_first", None, False)])

SETTINGS = [
    ("default", {}, "f32x3", DEFAULT),
    ("_NO_BWD_FUSE", {"_NO_BWD_FUSE": True}, "f32x3", NO_FUSE),
    ("_POOL_NOY=False", {"_POOL_NOY": False}, "f32x3", dict(DEFAULT, sa1=SA1_Y, sa1_at=SA1_Y)),
    ("_SA1_X4=False", {"_SA1_X4": False}, "f32x3", dict(DEFAULT, sa1=SA1_Y0, sa1_at=SA1_Y0)),
    ("bf16", {}, "bf16", DEFAULT),                             # same forms: the bf16 kernels have every one of them
    ("bf16 rows", {"_NO_BF16_STORE": False}, "bf16", dict(DEFAULT, sa1=SA1_ST16, sa1_at=SA1_ST16)),
    ("f32_native", {}, "f32_native", NO_FUSE),                    # no one-pass form, no no-store form
]
# what the expected forms above assume of the switches (their defaults, demf_amd/switches.py and csrc/switches.h)
BASE = {"_NO_BWD_FUSE": False, "_POOL_NOY": True, "_SA1_X4": True, "_NO_BF16_STORE": True, "_NO_FIRST_FUSE": False,
        "_NO_RED_FUSE": False, "_NO_FUSED_POOL": False, "_VEC_FIN": 7, "_FUSED_COLS_MIN_R": 0, "_FUSED_WIDE_MIN_R": 16384}


def test_the_stacks_are_the_models():
    assert {k: (v[0], v[1], v[2], v[4]) for k, v in STACKS.items() if k in ("sa1", "sa2", "sa3", "sa4", "agg")} == {
        "sa1": (1 << 20, 4, 64, False), "sa2": (1 << 18, 128, 32, True), "sa3": (1 << 16, 256, 16, True),
        "sa4": (1 << 15, 256, 16, True), "agg": (1 << 15, 256, 16, True)}
    assert STACKS["sa1"][3] == [(64, 4), (64, 64), (128, 64)] and STACKS["agg"][3] == [(256, 259), (256, 256), (256, 256)]


@pytest.mark.parametrize("label,attrs,mode,want", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_forms_of_the_model_stacks(label, attrs, mode, want):
    if not (switches.lib("DEMF_X3_MASK") & 1 and switches.lib("DEMF_FWD_RES") and not switches.lib("DEMF_STATIC_TILES")):
        pytest.fail("the expected forms are those of the library's default switches; unset DEMF_X3_MASK / DEMF_FWD_RES / "
                    "DEMF_STATIC_TILES")
    with _setting(dict(BASE, **attrs), mode):
        got = {name: _forms(name) for name in STACKS}
    assert got == {name: (tuple(f), b) for name, (f, b) in want.items()}


def test_eval_and_single_layer_stacks():
    with _setting(BASE, "f32x3"):
        R, ld, ns, shapes, geo, xgrad = STACKS["sa2"]
        assert ops._fwd_plan(R, ld, ns, shapes, False, geo, xgrad).fwd == ("group_first", "eval", "eval")
        plan = ops._fwd_plan(4096, 64, 16, [(128, 64)], True, False, True)     # one layer: the pooling is its own launch
        assert plan.fwd == ("bn",) and not plan.fuse_pool
        assert ops._bwd_forms(plan, 4096, 64, 16, [(128, 64)], True, False)[1] == {0: ("two_launch", "dx_w", False)}
        assert ops._bwd_forms(plan, 4096, 64, 16, [(128, 64)], False, False)[1] == {0: ("two_launch", None, False)}


def test_the_plan_reads_the_switches_when_called():
    """The tests and tools assign ops._POOL_NOY etc. at run time: a plan cached at import would void every A/B."""
    R, ld, ns, shapes, geo, xgrad = STACKS["sa1"]
    with _setting(BASE, "f32x3"):
        assert ops._fwd_plan(R, ld, ns, shapes, True, geo, xgrad).noy
        ops._POOL_NOY = False
        assert not ops._fwd_plan(R, ld, ns, shapes, True, geo, xgrad).noy
