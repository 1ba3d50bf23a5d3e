"""What Trainer.capture hands back (engine.CapturedStep) and what it refuses, at test_gpu_engine's tiny configuration
(3 scenes x 1 024 points)."""
import pytest
import torch

from test_gpu_engine import _setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["DEMF_GEO_TWO_DEEP", "DEMF_GEO_AT_BWD"])
def test_retired_switch_is_refused_at_accumulate_one_with_the_state_untouched(monkeypatch, name):
    tr, model, batch = _setup()
    assert tr.accumulate == 1
    tr.step(batch)                                   # (moments, gradients and BatchNorm statistics that are not zero)

    def snap():
        torch.cuda.synchronize()
        return [tr.opt.flat.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone(), tr.opt.state.clone(),
                tr.flat.flat.clone()] + [b.clone() for b in model.buffers()]

    before = snap()
    monkeypatch.setenv(name, "1")
    with pytest.raises(RuntimeError, match=name) as err:
        tr.capture(batch, warmup=1)
    assert "retired" in str(err.value)
    after = snap()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    assert tr._graph is None and tr.micro == 0 and tr.flat.mode is None and not tr.flat.captured_pack
    monkeypatch.delenv(name)
    assert bool(torch.isfinite(tr.capture(batch, warmup=1)()))          # without the switch the same call captures


def test_capture_returns_a_captured_step():
    tr, _, batch = _setup()
    replay = tr.capture(batch, warmup=1, max_gt=8)
    assert type(replay).__name__ == "CapturedStep"
    assert (replay.role, replay.accumulate, replay.update_in_graph, replay.metered) == (None, 1, True, False)
    assert replay.max_gt == 8 and replay.geo is not None and callable(replay.load)
    assert set(replay.static) == {"points", "img_features", "img_metas", "gt_bboxes_3d", "gt_labels_3d"}
    assert tuple(replay.static["gt_bboxes_3d"].shape) == (3, 8, 7)
    assert tr._graph is replay.graph and isinstance(replay.graph, torch.cuda.CUDAGraph)
    loss = replay()
    assert loss is replay.loss and bool(torch.isfinite(loss))
