"""Gradient accumulation (engine.Trainer(accumulate=W)) on the CPU / gloo path and the runner's step arithmetic:
W micro-steps feed one AdamW step on the mean of their gradients, which is what the reference's DDP all-reduce over
W ranks produces (each pass with its own BatchNorm batch statistics, as each rank has)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from demf_amd import engine, train


class Toy(nn.Module):
    """Stands in for DeMFHotPath on CPU: same forward_train / param_groups contract, with BatchNorm."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.backbone = nn.Linear(5, 7, bias=False)  # a bias before BN has a ~0 gradient; Adam would amplify noise
        self.decoder = nn.Linear(7, 3)     # 'decoder' params train at lr * 0.05
        self.bn = nn.BatchNorm1d(7)

    def forward_train(self, points, img_features, img_metas, gt_bboxes_3d, gt_labels_3d):
        y = self.decoder(torch.relu(self.bn(self.backbone(points))))
        return dict(a=(y - gt_bboxes_3d).pow(2).sum(), b=y.abs().sum() * 0.1)

    def param_groups(self, lr=0.008, weight_decay=0.01):
        dec = [p for n, p in self.named_parameters() if "decoder" in n]
        rest = [p for n, p in self.named_parameters() if "decoder" not in n]
        return [dict(params=rest, lr=lr, weight_decay=weight_decay),
                dict(params=dec, lr=lr * 0.05, weight_decay=weight_decay)]


def _batch(i):
    g = torch.Generator().manual_seed(100 + i)
    return dict(points=torch.randn(6, 5, generator=g), img_features=None, img_metas=None,
                gt_bboxes_3d=torch.randn(6, 3, generator=g), gt_labels_3d=None)


def _learned(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running" not in k and "num_b" not in k}


def _mean_gradient_reference(groups_of_batches):
    """The hand-written loop of tests/test_engine_gloo.py: per optimizer step the mean of the batches' gradients,
    clip_grad_norm_, torch.optim.AdamW."""
    ref = Toy()
    opt = torch.optim.AdamW(ref.param_groups(), lr=0.008, weight_decay=0.01)
    params = [p for g in ref.param_groups() for p in g["params"]]
    for group in groups_of_batches:
        grads = []
        for i in group:
            ref.zero_grad()
            sum(ref.forward_train(**_batch(i)).values()).backward()
            grads.append([p.grad.clone() for p in params])
        for k, p in enumerate(params):
            p.grad = sum(g[k] for g in grads) / len(grads)
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
    return ref


def test_accumulate_two_matches_mean_gradient_steps():
    model = Toy()
    tr = engine.Trainer(model, max_grad_norm=10.0, accumulate=2)
    assert tr.accumulate == 2 and tr.micro == 0
    before = _learned(model)
    for i in range(6):
        tr.step(_batch(i))
        assert tr.micro == (i + 1) % 2
        if i == 0:                               # a micro-step that is not the group's last updates nothing
            assert all(torch.equal(v, before[k]) for k, v in _learned(model).items())
            assert tr.flat.flat.abs().sum() > 0
        if i % 2 == 1:                           # the invariant: the buffer is zero between optimizer steps
            assert not tr.flat.flat.any()
    ref = _mean_gradient_reference([(0, 1), (2, 3), (4, 5)])
    got = _learned(model)
    for k, v in _learned(ref).items():
        torch.testing.assert_close(got[k], v, rtol=1e-5, atol=1e-6, msg=k)


def test_accumulate_one_is_the_plain_step():
    a, b = Toy(), Toy()
    ta, tb = engine.Trainer(a, max_grad_norm=10.0), engine.Trainer(b, max_grad_norm=10.0, accumulate=1)
    for i in range(3):
        ta.step(_batch(i))
        tb.step(_batch(i))
        assert tb.micro == 0
    for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(x, y), k


def test_unused_parameter_keeps_the_earlier_passes():
    """A ``None`` gradient in a later pass must not wipe what the earlier passes accumulated."""
    class Sometimes(Toy):
        def forward_train(self, points, img_features, img_metas, gt_bboxes_3d, gt_labels_3d):
            if img_features == "skip":                         # the decoder is not part of this pass's graph
                return dict(a=self.bn(self.backbone(points)).pow(2).sum())
            return super().forward_train(points, img_features, img_metas, gt_bboxes_3d, gt_labels_3d)

    model = Sometimes()
    tr = engine.Trainer(model, max_grad_norm=1e9, lr=0.0, weight_decay=0.0, accumulate=2)
    tr.step(_batch(0))
    first = tr.flat.flat.clone()
    dec = [v for p, v in zip(tr.flat.params, tr.flat.views) if any(p is q for q in model.decoder.parameters())]
    assert all(v.abs().sum() > 0 for v in dec)
    seen = {}
    orig = tr.opt.step
    tr.opt.step = lambda: (seen.update(flat=tr.flat.flat.clone()), orig())[1]
    tr.step(dict(_batch(1), img_features="skip"))
    solo = Sometimes()
    g = torch.autograd.grad(sum(solo.forward_train(**dict(_batch(1), img_features="skip")).values()),
                            [p for gr in solo.param_groups() for p in gr["params"]], allow_unused=True)
    want = first.clone()
    off = 0
    for p, gi in zip(tr.flat.params, g):
        if gi is not None:
            want[off:off + p.numel()] += gi.reshape(-1)
        off += p.numel()
    torch.testing.assert_close(seen["flat"], want / 2, rtol=1e-6, atol=1e-7)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    engine.init_distributed()
    assert dist.get_backend() == "gloo" and dist.get_world_size() == world
    tr_model = Toy()
    tr = engine.Trainer(tr_model, max_grad_norm=10.0, accumulate=2)
    for s in range(3):
        for m in range(2):
            tr.step(_batch(4 * s + 2 * m + rank))             # step s: batches 4s .. 4s+3 over (micro, rank)
    assert tr.micro == 0 and not tr.flat.flat.any()
    torch.save(_learned(tr_model), os.path.join(out, f"r{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world_two_times_accumulate_two_over_gloo(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for k in a:
        assert torch.equal(a[k], b[k]), f"replicas diverged on {k}"
    ref = _mean_gradient_reference([range(4 * s, 4 * s + 4) for s in range(3)])
    for k, v in _learned(ref).items():
        torch.testing.assert_close(a[k], v, rtol=1e-5, atol=1e-6, msg=k)


def test_guards():
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Trainer(Toy(), accumulate=bad)
    model, twin = Toy(), Toy()
    tr, tw = engine.Trainer(model, accumulate=2), engine.Trainer(twin, accumulate=2)
    tr.step(_batch(7))
    assert tr.micro == 1
    with pytest.raises(RuntimeError, match="micro = 1"):
        tr.state_dict()
    with pytest.raises(RuntimeError, match="micro = 1"):
        tr.set_epoch(3)
    with pytest.raises(RuntimeError, match="micro = 1"):
        tr.accumulate = 3
    assert tr.micro == 1 and tr.flat.flat.abs().sum() > 0     # the refusals left the open group alone
    tr.reset_accumulation()
    assert tr.micro == 0 and not tr.flat.flat.any()
    # the abandoned pass has moved BatchNorm's running statistics (as any forward does), nothing else: give the
    # twin the same statistics and both must walk the same way through a fresh group
    twin.load_state_dict(model.state_dict())
    for i in range(2):
        tr.step(_batch(i))
        tw.step(_batch(i))
    for (k, x), y in zip(model.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(x, y), k
    sd = tr.state_dict()                                       # on a step boundary: fine
    tr.step(_batch(3))
    tr.load_state_dict(sd)                                     # abandons the open group
    assert tr.micro == 0 and not tr.flat.flat.any()


def test_a_raising_pass_abandons_its_group():
    tr = engine.Trainer(Toy(), accumulate=3)
    tr.step(_batch(0))
    bad = dict(_batch(1), points=torch.randn(6, 4))            # wrong width: the forward raises
    with pytest.raises(RuntimeError):
        tr.step(bad)
    assert tr.micro == 0 and not tr.flat.flat.any() and tr.flat.mode is None


@pytest.mark.parametrize("W", [1, 2, 8])
def test_accumulation_plan(W):
    for per_pass, repeat in ((16, 5), (331, 5), (7, 1), (3, 2), (0, 1), (1, 1)):
        steps, dropped = train.accumulation_plan(per_pass, repeat, W)
        total = per_pass * repeat
        assert steps * W + dropped == total and 0 <= dropped < W
        # the loop itself, micro-step by micro-step, across the passes
        micro = n = 0
        for _ in range(repeat):
            for _ in range(per_pass):
                micro += 1
                if micro == W:
                    micro, n = 0, n + 1
        assert (n, micro) == (steps, dropped)
    assert train.accumulation_plan(16, 5, W) == (80 // W, 0)                  # divides
    assert train.accumulation_plan(331, 5, W) == (1655 // W, 1655 % W)        # SUN RGB-D: 5285 scenes / 16
    with pytest.raises(ValueError):
        train.accumulation_plan(4, 1, 0)


def test_resume_with_another_accumulate_raises():
    assert train.check_resume_accumulate(dict(epoch=1, iter=5, accumulate=2), 2) == 2
    assert train.check_resume_accumulate(dict(epoch=1, iter=5), 1) == 1       # a file from before the field
    with pytest.raises(ValueError, match=r"accumulate = 2.*accumulate = 4"):
        train.check_resume_accumulate(dict(epoch=1, iter=5, accumulate=2), 4, "x.pth")
    with pytest.raises(ValueError, match=r"accumulate = 1.*accumulate = 8"):
        train.check_resume_accumulate(dict(epoch=1, iter=5), 8)


def test_command_line_and_autoscale():
    base = ["--data-root", "r", "--ann-file", "a", "--work-dir", "w"]
    args = train.parse_args(base)
    assert args.accumulate == 1 and args.autoscale_lr is False
    args = train.parse_args(base + ["--accumulate", "8", "--autoscale-lr"])
    assert args.accumulate == 8 and args.autoscale_lr is True
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--accumulate", "0"])
    assert train.autoscale_lr(0.008, 8) == 0.008                              # the reference's own step
    assert train.autoscale_lr(0.008, 2) == pytest.approx(0.002, rel=1e-12)
    assert train.autoscale_lr(0.008, 1, world=1) == pytest.approx(0.001, rel=1e-12)
