"""The parts of the sync-free test path that need no device: argument validation of the csrc/detect.hip entry
points (before any launch), checkpoint layouts of demf_amd.infer.load_checkpoint, and its command line."""
import ctypes

import pytest
import torch

from demf_amd import _ffi


def _layers(n, K):
    arr = (_ffi.DetectLayer * n)()
    for d in arr:
        d.K = K
        d.res_scale = 1.0
    return arr


def test_detect_layer_struct_matches_the_header_layout():
    # int K; float res_scale; 7 x (pointer, int, int)
    assert ctypes.sizeof(_ffi.DetectLayer) == 8 + 7 * 16
    assert _ffi.DetectLayer.center.offset == 8 and _ffi.DetectLayer.base_sb.offset == 8 + 16 + 8
    assert _ffi.DetectLayer.sem_sk.offset == 8 + 6 * 16 + 12


def test_detect_decode_validates_before_launching():
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_detect_decode", 1, 8, 0, 10, 12, 1, None, None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_detect_decode", -1, 8, 1, 10, 12, 1, _layers(1, 8), None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):                     # the layers' K do not add up
        _ffi.call("demf_detect_decode", 1, 9, 2, 10, 12, 1, _layers(2, 4), None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_detect_decode", 1, 8, 1, 10, 12, 1, None, None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):                  # layer fields and outputs are null
        _ffi.call("demf_detect_decode", 1, 8, 2, 10, 12, 1, _layers(2, 4), None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"code -?\d+\): detect_decode: K=1026 boxes per scene exceeds 1024"):
        _ffi.call("demf_detect_decode", 1, 1026, 2, 10, 12, 1, _layers(2, 513), None, None, None, None, None, None,
                  None)


def test_detect_pack_validates_before_launching():
    none5 = [None] * 5
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_detect_pack", 1, 8, 0, 1, 0.05, *none5, 0, 4, 100, *none5, None)
    with pytest.raises(RuntimeError, match="bad sizes"):                     # scenes 3 .. 4 of a 4-scene store
        _ffi.call("demf_detect_pack", 2, 8, 10, 1, 0.05, *none5, 3, 4, 100, *none5, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_detect_pack", 2, 8, 10, 1, 0.05, *none5, 0, 4, 100, *none5, None)
    assert b"null pointer" in _ffi.load().demf_last_error()
    with pytest.raises(RuntimeError, match="detect_pack: K=1025 boxes per scene exceeds 1024"):
        _ffi.call("demf_detect_pack", 2, 1025, 10, 1, 0.05, *none5, 0, 4, 100, *none5, None)
    # an empty batch is not an error and launches nothing
    _ffi.call("demf_detect_pack", 0, 8, 10, 1, 0.05, *none5, 0, 4, 100, *none5, None)


def test_ops_refuse_cpu_tensors():
    from demf_amd import ops
    z = lambda *s: torch.zeros(s)                                            # noqa: E731
    layer = dict(center=z(1, 4, 3), size=z(1, 4, 3), dir_class=z(1, 4, 12), dir_res=z(1, 4, 12), obj=z(1, 4, 2),
                 sem=z(1, 4, 10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.detect_decode([layer], 12)
    with pytest.raises(ValueError, match="1 to 8 layers"):
        ops.detect_decode([], 12)


# ---- checkpoints -------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv1d(3, 4, 1)
        self.bn = torch.nn.BatchNorm1d(4)


def _seeded():
    torch.manual_seed(3)
    net = _Net()
    with torch.no_grad():
        net.bn.running_mean.uniform_(-1, 1)
        net.bn.running_var.uniform_(0.5, 2)
        net.bn.num_batches_tracked.fill_(7)
    return net


@pytest.mark.parametrize("layout", ["mmcv", "trainer", "bare"])
def test_load_checkpoint_layouts(tmp_path, layout):
    from demf_amd.infer import load_checkpoint
    src = _seeded()
    sd = src.state_dict()
    ckpt = {"mmcv": dict(meta=dict(epoch=36, note="x"), state_dict=sd, optimizer=dict(state={}, param_groups=[])),
            "trainer": dict(model=sd, optimizer=dict(t=3, lr_factor=1.0)), "bare": dict(sd)}[layout]
    path = str(tmp_path / "c.pth")
    torch.save(ckpt, path)
    dst = _Net()
    assert load_checkpoint(dst, path) is dst
    got = dst.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_load_checkpoint_missing_and_unexpected_keys_are_errors(tmp_path):
    from demf_amd.infer import load_checkpoint
    sd = dict(_seeded().state_dict())
    missing = {k: v for k, v in sd.items() if k != "bn.running_var"}
    path = str(tmp_path / "m.pth")
    torch.save(dict(state_dict=missing), path)
    with pytest.raises(RuntimeError, match="bn.running_var"):
        load_checkpoint(_Net(), path)
    torch.save(dict(sd, extra=torch.zeros(1)), path)
    with pytest.raises(RuntimeError, match="extra"):
        load_checkpoint(_Net(), path)
    torch.save(dict(weights=[1, 2, 3]), path)
    with pytest.raises(ValueError, match="layout not recognised"):
        load_checkpoint(_Net(), path)


def test_load_checkpoint_applies_the_detectors_key_remap(tmp_path):
    """load_checkpoint goes through the model's own load_state_dict (DeMFVoteNet's remaps stage-1 keys)."""
    from demf_amd.data import remap_checkpoint
    from demf_amd.infer import load_checkpoint

    class Remapping(_Net):
        def load_state_dict(self, state_dict, strict=True, **kw):
            return super().load_state_dict(remap_checkpoint(state_dict), strict=strict, **kw)

    sd = dict(_seeded().state_dict())
    sd["img_bbox_head.fc_cls.weight"] = torch.zeros(2)                      # a stage-1 key the remap drops
    path = str(tmp_path / "s.pth")
    torch.save(dict(state_dict=sd), path)
    load_checkpoint(Remapping(), path)
    with pytest.raises(RuntimeError, match="img_bbox_head"):
        load_checkpoint(_Net(), path)


# ---- command line ------------------------------------------------------------------------------------------
def test_argument_parsing():
    from demf_amd.infer import parse_args
    a = parse_args(["--data-root", "R", "--ann-file", "v.pkl", "--checkpoint", "c.pth"])
    assert (a.data_root, a.ann_file, a.checkpoint) == ("R", "v.pkl", "c.pth")
    assert a.batch_size == 8 and a.workers == 8 and a.out is None and a.no_eval is False
    a = parse_args(["--data-root", "R", "--ann-file", "v.pkl", "--checkpoint", "c.pth", "--batch-size", "3",
                    "--workers", "2", "--out", "o.pkl", "--no-eval"])
    assert a.batch_size == 3 and a.workers == 2 and a.out == "o.pkl" and a.no_eval is True
    for bad in (["--ann-file", "v.pkl", "--checkpoint", "c"],                       # no --data-root
                ["--data-root", "R", "--ann-file", "v", "--checkpoint", "c", "--batch-size", "0"],
                ["--data-root", "R", "--ann-file", "v", "--checkpoint", "c", "--no-eval"]):   # results discarded
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_detection_store_argument_checks():
    from demf_amd.detections import DetectionStore
    with pytest.raises(ValueError, match="max_scenes"):
        DetectionStore(0, device="cpu")
    with pytest.raises(ValueError, match="max_rows"):
        DetectionStore(2, max_rows=-1, device="cpu")
