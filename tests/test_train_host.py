"""Host side of the training runner (demf_amd/train.py) and of the step meter (demf_amd/meter.py): ring decoding,
schedule, checkpoint files, argument parsing and log lines.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures


# ---- ring decode --------------------------------------------------------------------------------------------------
NAMES = ("a", "b", "_total")


def _put(ring, t, vals, lr_factor=1.0, grad_norm=2.0, clip=0.5, flags=0):
    r = t % ring.shape[0]
    ring[r, :2].view(np.int64)[0] = t
    ring[r, 2:3].view(np.uint32)[0] = flags
    f = ring[r].view(np.float32)
    f[3], f[4], f[5] = lr_factor, grad_norm, clip
    f[6:6 + len(vals)] = vals


def test_decode_returns_every_step_once_in_order_across_a_wrap():
    from demf_amd import meter
    ring = meter.empty_ring(4)
    assert ring.shape == (4, 16) and ring.dtype == np.int32
    rows, nxt = meter.decode_ring(ring, NAMES, 0)
    assert rows == [] and nxt == 0                         # stamps -1: nothing has happened
    for t in range(3):
        _put(ring, t, [t + 0.25, 10.0 * t, t + 0.5], lr_factor=0.1)
    rows, nxt = meter.decode_ring(ring, NAMES, 0)
    assert [r["t"] for r in rows] == [0, 1, 2] and nxt == 3
    assert rows[1] == dict(t=1, lr_factor=float(np.float32(0.1)), grad_norm=2.0, clip=0.5, nonfinite=(), a=1.25, b=10.0,
                           _total=1.5)
    again, nxt2 = meter.decode_ring(ring, NAMES, nxt)
    assert again == [] and nxt2 == 3                       # nothing twice
    for t in range(3, 6):                                  # rows 3, 0, 1: the ring wraps
        _put(ring, t, [t + 0.25, 10.0 * t, t + 0.5])
    rows, nxt = meter.decode_ring(ring, NAMES, 3)
    assert [r["t"] for r in rows] == [3, 4, 5] and nxt == 6
    assert [r["a"] for r in rows] == [3.25, 4.25, 5.25]


def test_decode_raises_on_a_wrong_stamp():
    from demf_amd import meter
    ring = meter.empty_ring(4)
    for t in range(6):                                     # six steps into four rows: 0 and 1 are gone
        _put(ring, t, [0.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match=r"overrun: step 0 was expected in row 0, which holds step 4 \(6 steps"):
        meter.decode_ring(ring, NAMES, 0)
    rows, _ = meter.decode_ring(ring, NAMES, 2)            # the four newest are intact
    assert [r["t"] for r in rows] == [2, 3, 4, 5]
    hole = meter.empty_ring(4)
    _put(hole, 0, [0.0] * 3)
    _put(hole, 2, [0.0] * 3)                               # step 1 never written
    with pytest.raises(RuntimeError, match="step 1 was expected in row 1, which holds step -1"):
        meter.decode_ring(hole, NAMES, 0)
    with pytest.raises(ValueError):
        meter.decode_ring(np.zeros((4, 8), np.int32), NAMES, 0)
    with pytest.raises(ValueError):
        meter.decode_ring(meter.empty_ring(4), ["x"] * 11, 0)


def test_flag_word_maps_to_term_names():
    from demf_amd import meter
    names = meter.loss_names()
    assert len(names) == 9 and names[-2:] == ("vote_loss", "_total") and "center_loss" in names
    ring = meter.empty_ring(8)
    vals = [float(i) for i in range(9)]
    _put(ring, 0, vals)
    _put(ring, 1, vals, flags=1 << 4)
    _put(ring, 2, vals, flags=(1 << 0) | (1 << 8))
    _put(ring, 3, vals, flags=meter.FLAG_GRAD_NORM)
    _put(ring, 4, vals, flags=meter.FLAG_GRAD_NORM | (1 << 7))
    rows, _ = meter.decode_ring(ring, names, 0)
    assert [r["nonfinite"] for r in rows] == [(), (names[4],), (names[0], "_total"), ("grad_norm",),
                                              ("vote_loss", "grad_norm")]
    assert all(r[n] == float(i) for r in rows for i, n in enumerate(names))


# ---- schedule -----------------------------------------------------------------------------------------------------
def test_schedule_and_loader_epochs():
    from demf_amd import engine, train
    want = [1.0] * 24 + [0.1] * 8 + [0.1 * 0.1] * 4
    got = [train.lr_factor(e) for e in range(36)]
    assert got == pytest.approx(want, rel=1e-12) and got[23] == 1.0 and got[24] == 0.1
    assert train.lr_factor(1, (1,), 0.1) == 0.1 and train.lr_factor(0, (1,), 0.1) == 1.0
    # the trainer's own schedule is the same expression

    class _T(engine.Trainer):
        def __init__(self):
            self.fused = False
            self.opt = type("O", (), dict(param_groups=[dict(lr=0.0)]))()
            self._base_lrs = [1.0]
    assert [_T().set_epoch(e) for e in range(36)] == got
    # every pass of the run has its own loader epoch: 36 x 5 distinct numbers, in run order
    seq = [train.loader_epoch(e, p, 5) for e in range(36) for p in range(5)]
    assert seq == list(range(180))
    assert train.loader_epoch(3, 0, 1) == 3
    with pytest.raises(ValueError):
        train.loader_epoch(0, 5, 5)


# ---- checkpoint files ---------------------------------------------------------------------------------------------
def _cpu_trainer(seed):
    from demf_amd import engine
    from demf_amd.modules import DeMFHotPath
    model = DeMFHotPath(fixtures.tiny_cfg())
    fixtures.seed_weights(model, seed)
    tr = engine.Trainer(model, lr=1e-3)
    assert not tr.fused and isinstance(tr.opt, torch.optim.AdamW)
    return tr, model


def _fake_steps(tr, seed, n=2):
    """Optimizer steps on made-up gradients (the operators have no CPU path): moments and step counts fill up."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        tr.flat.flat.copy_(torch.randn(tr.flat.flat.shape, generator=g))
        tr._update()


def _flat_state(tr):
    out = {"model." + k: v for k, v in tr.model.state_dict().items()}
    osd = tr.opt.state_dict()
    for i, st in osd["state"].items():
        for k, v in st.items():
            out[f"opt.{i}.{k}"] = v if torch.is_tensor(v) else torch.tensor(v)
    for i, g in enumerate(osd["param_groups"]):
        out[f"group.{i}.lr"] = torch.tensor(g["lr"])
    return out


def test_checkpoint_roundtrip_is_bit_exact(tmp_path):
    from demf_amd import infer, train
    from demf_amd.modules import DeMFHotPath
    tr, model = _cpu_trainer(3)
    tr.set_epoch(24)                                       # a decayed rate must survive the file
    _fake_steps(tr, 1)
    meta = dict(epoch=25, iter=1234, seed=7, repeat=5)
    path = train.save_checkpoint(str(tmp_path), 25, train.make_checkpoint(model, tr, None, meta))
    ckpt = torch.load(path, map_location="cpu", weights_only=True)        # nothing in it needs pickle
    assert list(ckpt)[:2] == ["meta", "state_dict"] and set(ckpt) == {"meta", "state_dict", "trainer", "meter"}
    assert ckpt["meta"] == meta and "model" not in ckpt["trainer"] and ckpt["meter"] is None
    want = _flat_state(tr)
    tr2, model2 = _cpu_trainer(4)                          # other weights, empty optimizer
    assert not torch.equal(model2.state_dict()["pts_bbox_head.conv_pred0.conv_reg.weight"],
                           model.state_dict()["pts_bbox_head.conv_pred0.conv_reg.weight"])
    assert train.restore_checkpoint(train.load_checkpoint_file(path), model2, tr2) == meta
    got = _flat_state(tr2)
    assert set(got) == set(want) and len(want) > 100
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert got["group.0.lr"].item() == pytest.approx(1e-4) and got["opt.0.step"].item() == 2
    # the parameters are still the flat buffer's views, and both runs continue identically
    assert all(p.grad.data_ptr() >= tr2.flat.flat.data_ptr() for p in tr2.flat.params)
    _fake_steps(tr, 2, n=1)
    _fake_steps(tr2, 2, n=1)
    for k, v in _flat_state(tr).items():
        assert torch.equal(_flat_state(tr2)[k], v), k
    # the same file through the test path's loader
    fresh = DeMFHotPath(fixtures.tiny_cfg())
    infer.load_checkpoint(fresh, path)
    assert all(torch.equal(v, ckpt["state_dict"][k]) for k, v in fresh.state_dict().items())


def test_rotation_keeps_max_keep_ckpts_and_latest(tmp_path):
    from demf_amd import train
    wd = str(tmp_path)
    for e in range(1, 12):                                 # past 9 -> 10: the order is numeric, not lexical
        train.save_checkpoint(wd, e, dict(meta=dict(epoch=e), state_dict=dict(w=torch.full((3,), float(e)))), 2)
        assert sorted(os.listdir(wd)) == sorted(["latest.pth"] + [f"epoch_{k}.pth" for k in range(max(1, e - 1), e + 1)])
        assert train.load_checkpoint_file(os.path.join(wd, "latest.pth"))["meta"]["epoch"] == e
    train.save_checkpoint(wd, 12, dict(meta=dict(epoch=12), state_dict={}), 1)
    assert sorted(os.listdir(wd)) == ["epoch_12.pth", "latest.pth"]
    keep_all = str(tmp_path / "all")
    for e in (1, 2, 3):
        train.save_checkpoint(keep_all, e, dict(meta=dict(epoch=e), state_dict={}), 0)
    assert sorted(os.listdir(keep_all)) == ["epoch_1.pth", "epoch_2.pth", "epoch_3.pth", "latest.pth"]


def test_interrupted_write_never_truncates_latest(tmp_path, monkeypatch):
    from demf_amd import train
    wd = str(tmp_path)
    good = dict(meta=dict(epoch=1), state_dict=dict(w=torch.arange(1000.0)))
    train.save_checkpoint(wd, 1, good, 1)
    real = torch.save

    def dying(obj, path, *a, **k):
        """Writes half the file, then the process 'dies'."""
        real(obj, path, *a, **k)
        size = os.path.getsize(path)
        with open(path, "r+b") as f:
            f.truncate(size // 2)
        raise KeyboardInterrupt

    monkeypatch.setattr(torch, "save", dying)
    with pytest.raises(KeyboardInterrupt):
        train.save_checkpoint(wd, 2, dict(meta=dict(epoch=2), state_dict=dict(w=torch.zeros(1000))), 1)
    monkeypatch.setattr(torch, "save", real)
    # the truncated bytes sit under the temporary name only; both published files are whole and still epoch 1
    assert sorted(os.listdir(wd)) == ["epoch_1.pth", "epoch_2.pth.tmp", "latest.pth"]
    for name in ("latest.pth", "epoch_1.pth"):
        ck = train.load_checkpoint_file(os.path.join(wd, name))
        assert ck["meta"]["epoch"] == 1 and torch.equal(ck["state_dict"]["w"], good["state_dict"]["w"])
    # ... and the next save goes through over the leftover
    train.save_checkpoint(wd, 2, dict(meta=dict(epoch=2), state_dict=dict(w=torch.zeros(1000))), 1)
    assert sorted(os.listdir(wd)) == ["epoch_2.pth", "latest.pth"]
    assert train.load_checkpoint_file(os.path.join(wd, "latest.pth"))["meta"]["epoch"] == 2


# ---- arguments ----------------------------------------------------------------------------------------------------
REQ = ["--data-root", "R", "--ann-file", "a.pkl", "--work-dir", "W"]


def test_defaults_are_the_references():
    import inspect
    from demf_amd import train
    a = train.parse_args(REQ)
    # schedule_3x.py (AdamW 0.008 / 0.01, clip 10, steps 24 and 32, 36 epochs), sunrgbd-3d-10class.py:75-86 (16 samples,
    # 4 workers, RepeatDataset x 5), default_runtime.py:6-7 (log every 50), demf_votenet.py:275-280 (evaluate every 36,
    # keep one checkpoint)
    assert (a.batch_size, a.epochs, a.seed, a.workers, a.log_interval) == (16, 36, 0, 4, 50)
    assert not a.no_graphs and not a.no_validate and a.val_ann_file is a.load_from is a.resume_from is None
    sig = {k: p.default for k, p in inspect.signature(train.fit).parameters.items()}
    want = dict(batch_size=16, max_epochs=36, repeat=5, lr=0.008, weight_decay=0.01, max_grad_norm=10, lr_steps=(24, 32),
                gamma=0.1, log_interval=50, ckpt_interval=1, max_keep_ckpts=1, eval_interval=36, seed=0, workers=4,
                graphs=True, resume_from=None, val_set=None)
    assert {k: sig[k] for k in want} == want
    b = train.parse_args(REQ + ["--no-graphs", "--no-validate", "--epochs", "2", "--batch-size", "4", "--seed", "9",
                                "--workers", "2", "--log-interval", "10", "--val-ann-file", "v.pkl", "--resume-from", "c"])
    assert (b.no_graphs, b.no_validate, b.epochs, b.batch_size, b.seed, b.workers, b.log_interval, b.val_ann_file,
            b.resume_from) == (True, True, 2, 4, 9, 2, 10, "v.pkl", "c")


@pytest.mark.parametrize("bad", [["--batch-size", "0"], ["--workers", "0"], ["--log-interval", "0"], ["--epochs", "-1"],
                                 ["--batch-size", "two"], ["--load-from", "a", "--resume-from", "b"], ["--bogus"]])
def test_bad_arguments_are_rejected(bad, capsys):
    from demf_amd import train
    with pytest.raises(SystemExit) as e:
        train.parse_args(REQ + bad)
    assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train.parse_args(REQ[:4])                          # --work-dir is required
    capsys.readouterr()


# ---- log lines ----------------------------------------------------------------------------------------------------
def test_log_line_from_rows():
    from demf_amd import meter, train
    names = meter.loss_names()
    rows = []
    for t in range(4):
        r = dict(t=100 + t, lr_factor=0.1, grad_norm=1.0 + t, clip=1.0, nonfinite=())
        r.update({n: float(i + t) for i, n in enumerate(names)})
        rows.append(r)
    line = train.format_log(rows, 3, 104, 0.008, 0.25, names)
    assert list(line)[:4] == ["mode", "epoch", "iter", "lr"]
    assert (line["mode"], line["epoch"], line["iter"]) == ("train", 3, 104)
    assert line["lr"] == pytest.approx(0.0008) and line["time"] == 0.25
    assert line["grad_norm"] == 2.5 and line["loss"] == 8 + 1.5 and "_total" not in line
    for i, n in enumerate(names[:-1]):
        assert line[n] == i + 1.5
    assert set(line) == {"mode", "epoch", "iter", "lr", "loss", "grad_norm", "time"} | set(names[:-1])
    assert json.loads(json.dumps(line)) == line
    with pytest.raises(ValueError):
        train.format_log([], 1, 1, 0.008, 0.1)
    # a flagged row stops the run and names where and what
    train.check_finite(rows, 50)
    rows[2]["nonfinite"] = ("center_loss", "grad_norm")
    with pytest.raises(FloatingPointError, match=r"non-finite center_loss, grad_norm at epoch 3, iteration 103 "):
        train.check_finite(rows, 50)
