"""engine._capture_plan - what Trainer.capture decides before it touches anything - over its whole small grid, and
the attributes engine.Trainer starts with.  No GPU: the plan is a pure function, the trainer runs the CPU path.

The expected results are written out from the rules, in the order the function documents:
  1. a retired replay-order switch is refused (RuntimeError naming it), whatever else was asked;
  2. accumulate = 1: role must be None or "last" (else ValueError matching "role") and resolves to None, ``dry`` is
     handed back as given;
  3. accumulate = W > 1: role defaults to "last" at micro = W-1 and to "accumulate" before it, anything but those
     two is a ValueError matching "role"; then the overlapped update is refused on the fused path (RuntimeError
     matching "overlapped"); ``dry`` is forced on;
  4. update_in_graph (None = DEMF_GRAPH_UPDATE) holds only if fused and stub == 0 and (world == 1 or
     DEMF_GRAPH_ALLREDUCE)."""
import itertools

import pytest
import torch

from demf_amd import engine
from test_accumulate_host import Toy, _batch

ROLES = (None, "accumulate", "last", "first")
RETIRED = (frozenset(), frozenset({"DEMF_GEO_AT_BWD"}), frozenset({"DEMF_GEO_TWO_DEEP"}))


def _expected(W, micro, role, dry, uig, fused, world, stub, overlap, graph_update, graph_allreduce, retired):
    """-> ("ok", (role, dry, update_in_graph)) or (exception type, word its message must match)."""
    if retired:
        return RuntimeError, next(iter(retired))
    if W == 1:
        if role in ("accumulate", "first"):
            return ValueError, "role"
        want_role, want_dry = None, dry
    else:
        if role == "first":
            return ValueError, "role"
        want_role = role or ("last" if micro == W - 1 else "accumulate")
        if fused and overlap:
            return RuntimeError, "overlapped"
        want_dry = True
    asked = bool(graph_update) if uig is None else uig
    return "ok", (want_role, want_dry, bool(asked and fused and stub == 0 and (world == 1 or graph_allreduce == 1)))


@pytest.mark.parametrize("W", [1, 3])
def test_capture_plan_over_the_grid(W):
    seen = {"ok": 0, "role": 0, "overlapped": 0, "DEMF_GEO_AT_BWD": 0, "DEMF_GEO_TWO_DEEP": 0}
    for micro, role, dry, uig, fused, (world, stub), graph_update, graph_allreduce, overlap, retired in \
            itertools.product((0, W - 1), ROLES, (False, True), (None, False, True), (False, True),
                              ((1, 0), (2, 0), (1, 50)), (0, 1), (0, 1), (False, True), RETIRED):
        args = (W, micro, role, dry, uig, fused, world, stub, overlap, graph_update, graph_allreduce, retired)
        kind, want = _expected(*args)
        if kind == "ok":
            got = engine._capture_plan(*args)
            assert got == want and all(type(g) is type(w) for g, w in zip(got, want)), (args, got, want)
            seen["ok"] += 1
        else:
            with pytest.raises(kind, match=want) as err:
                engine._capture_plan(*args)
            assert type(err.value) is kind, args
            seen[want] += 1
    # every class of input was met (the overlap refusal exists with W > 1 only)
    assert all(n > 0 for k, n in seen.items() if k != "overlapped") and (seen["overlapped"] > 0) == (W > 1), seen


def test_the_refusals_say_what_the_callers_match_on():
    plan = engine._capture_plan
    with pytest.raises(RuntimeError, match=r"DEMF_GEO_AT_BWD.*retired.*6\.49 against 6\.39.*4\.95 against 4\.88"):
        plan(1, 0, None, False, None, True, 1, 0, False, 1, 0, {"DEMF_GEO_AT_BWD"})
    with pytest.raises(RuntimeError, match=r"DEMF_GEO_TWO_DEEP.*retired.*7\.80 against 7\.67"):
        plan(1, 0, None, False, None, True, 1, 0, False, 1, 0, {"DEMF_GEO_TWO_DEEP"})
    with pytest.raises(RuntimeError, match=r"overlapped.*accumulate = 2 > 1.*DEMF_AR_OVERLAP / allreduce_overlap"):
        plan(2, 0, None, False, None, True, 1, 50, True, 1, 0, set())
    with pytest.raises(ValueError, match=r"role='first'.*'accumulate' or 'last'"):
        plan(2, 0, "first", False, None, True, 1, 0, False, 1, 0, set())
    with pytest.raises(ValueError, match=r"role='accumulate'.*accumulate = 1"):
        plan(1, 0, "accumulate", False, None, True, 1, 0, False, 1, 0, set())


def test_capture_refuses_a_retired_switch_before_it_looks_at_the_batch(monkeypatch):
    """On the CPU trainer a capture could not even begin: the refusal comes first, at accumulate = 1 as well."""
    for W in (1, 2):
        tr = engine.Trainer(Toy(), accumulate=W)
        before = [p.detach().clone() for p in tr.flat.params]
        for name in engine.RETIRED_ORDERS:
            monkeypatch.setenv(name, "0")                      # present means on
            with pytest.raises(RuntimeError, match=name):
                tr.capture(None)
            monkeypatch.delenv(name)
        assert tr.micro == 0 and not tr.flat.flat.any() and tr.flat.mode is None and not tr.flat.captured_pack
        assert all(torch.equal(a, p) for a, p in zip(before, tr.flat.params))


def test_trainer_starts_with_every_attribute_the_engine_reads():
    tr = engine.Trainer(Toy())
    assert tr.side_stream is None and tr._comm_stream is None and tr._graph is None
    assert tr._pending_update is False
    assert tr.allreduce_stub_us == 0 and tr.allreduce_overlap is None and tr.allreduce_events is None
    assert all(name in vars(tr) for name in ("side_stream", "_comm_stream", "_pending_update", "allreduce_stub_us",
                                             "allreduce_overlap", "allreduce_events", "_graph"))
    assert tr.allreduce_config() == (1, 0, False)
    tr.step(_batch(0))                                         # and the CPU step runs with them
    assert tr._pending_update is False


def test_flat_grads_capturing_sets_and_always_clears():
    flat = engine.Trainer(Toy()).flat
    marker = object()
    with pytest.raises(KeyError):
        with flat.capturing("last", marker):
            assert flat.captured_pack is True and flat.mode == "last" and flat.sumsq_state is marker
            raise KeyError("inside")
    assert flat.captured_pack is False and flat.mode is None and flat.sumsq_state is None
