"""Gradient accumulation on the GPU: the kernels of csrc/accum.hip at launch edges (as tests/test_gpu_optim_edges.py
checks the copying pack), then engine.Trainer(accumulate=W) eager and captured, then the runner."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import optim_cases as oc
from oracle import fixtures
from test_gpu_optim_edges import (COPY_WORDS, GUARD, S0, _bits, _call, _dev, _k_multi_copy, _place, _read_state,
                                  _spans, _state, _sumsq_bound)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ---- demf_multi_add / demf_multi_add_sumsq ------------------------------------------------------------------------
def _add_data(n, seed):
    """Finite, normal-range fp32 values with -0.0 among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    x[np.abs(x) < 1e-3] = np.float32(0.5)              # (no sum of two of them can come out denormal)
    x[::13] = -0.0
    return x


def _run_add(entry, specs, bps, seed, special=None):
    """specs: (words, src_off or None for a null source, dst_off).  One launch over the whole table.  Stored sums
    against numpy's float32 addition, bit for bit (one fp32 add is correctly rounded; denormal inputs and results are
    left out on purpose: whether the device flushes them is not what this checks).  Guard bands, null-source
    destinations and the source buffer bit-identical; sumsq against the fp64 sum of squares of the STORED results,
    null-source segments included.  ``special``: "zero" - every destination holds the negated source, every sum is
    +0.0 and the state's bits stay; inf / nan - one source element."""
    with_sum = entry == "demf_multi_add_sumsq"
    words = [s[0] for s in specs]
    sstart, slen = _spans(words, [s[1] or 0 for s in specs])
    dstart, dlen = _spans(words, [s[2] for s in specs])
    src = _add_data(slen, seed)
    dst = np.full(dlen, oc.SENTINEL, np.float32)
    for (w, so, do), ss, ds in zip(specs, sstart, dstart):
        piece = _add_data(w, seed + 1000 + ds)
        if so is not None:
            piece[3::7] = -src[ss:ss + w][3::7]                          # exact cancellations: x + (-x) = +0.0
            if special == "zero":
                piece = -src[ss:ss + w]
        elif special == "zero":
            piece = np.zeros(w, np.float32)
        dst[ds:ds + w] = piece
    if special not in (None, "zero"):
        w, so, do = specs[0]
        src[sstart[0] + w // 2] = special
    want = dst.copy()
    ref_sum = bound = 0.0
    for (w, so, do), ss, ds in zip(specs, sstart, dstart):
        if so is not None:
            with np.errstate(invalid="ignore"):
                want[ds:ds + w] = dst[ds:ds + w] + src[ss:ss + w]        # float32 + float32 -> float32
        if with_sum:
            s = float((want[ds:ds + w].astype(np.float64) ** 2).sum())
            # a null source takes the scalar loop whatever the alignment
            k = _k_multi_copy(w, so is not None and so % 4 == 0 and do % 4 == 0, bps)
            ref_sum += s
            bound += (k + 2) * U * s
    dsrc, ddst = _place(src, 0), _place(dst, 0)
    table = np.array([[0 if so is None else dsrc.data_ptr() + 4 * ss for (_, so, _), ss in zip(specs, sstart)],
                      [ddst.data_ptr() + 4 * ds for ds in dstart], words], np.int64)
    dtable = _dev(table)
    for (w, so, do), a_s, a_d in zip(specs, table[0], table[1]):
        assert a_d % 16 == 4 * do and (so is None or a_s % 16 == 4 * so)
    state, sbytes = _state(S0, 7, 0.1)
    if with_sum:
        _call(entry, len(specs), dtable.data_ptr(), bps, state.data_ptr())
    else:
        _call(entry, len(specs), dtable.data_ptr(), bps)
    torch.cuda.synchronize()
    got = ddst.cpu().numpy()
    # (a NaN result - the non-finite case only - is compared as a NaN, not by its payload)
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want)))
    assert bad.size == 0, (entry, bps, "first wrong word %d of %d, %d wrong" % (bad[0], dlen, bad.size))
    assert np.array_equal(_bits(dsrc.cpu().numpy()), _bits(src))
    after = state.cpu().numpy()
    assert after[8:].tobytes() == sbytes[8:].tobytes()                   # t, ticket, lr_factor and the pad
    if not with_sum or special == "zero":
        assert special != "zero" or ref_sum == 0.0
        assert after.tobytes() == sbytes.tobytes()
        return
    s = _read_state(state)
    if special is not None:
        assert (np.isinf(s["sumsq"]) and s["sumsq"] > 0) if np.isinf(special) else np.isnan(s["sumsq"]), s["sumsq"]
        return
    err = abs(s["sumsq"] - (S0 + ref_sum))
    # test_gpu_optim_edges._sumsq_bound, its fp32 part summed piece by piece (k differs between pieces)
    bound += _sumsq_bound(0.0, 0, len(specs) * bps, S0 + ref_sum)
    print("%s %d pieces bps %d: sumsq err %.3e bound %.3e" % (entry, len(specs), bps, err, bound))
    assert err <= bound, (s["sumsq"], S0 + ref_sum, err, bound)


@pytest.mark.parametrize("bps", [1, 4, 64])
@pytest.mark.parametrize("entry", ["demf_multi_add", "demf_multi_add_sumsq"])
def test_multi_add_offsets_and_sizes(entry, bps):
    """Every size x source offset x destination offset (0-3 floats each) as the 128 pieces of one table: the
    float4 body with its 4q tail where both sit on 16 bytes, the scalar loop everywhere else."""
    specs = [(w, so, do) for w in COPY_WORDS for so in range(4) for do in range(4)]
    if bps != 64:                                       # the 1 MB pieces once per entry point, at their production width
        specs = [s for s in specs if s[0] != COPY_WORDS[-1]]
    _run_add(entry, specs, bps, seed=bps)


@pytest.mark.parametrize("nseg", [1, 2, 119])
@pytest.mark.parametrize("entry", ["demf_multi_add", "demf_multi_add_sumsq"])
def test_multi_add_segment_counts_and_null_sources(entry, nseg):
    """1, 2 and 119 pieces (the full model's parameter count) in one table; every third piece of the long table and
    the second of the pair has a null source: left bit-identical, its squares counted."""
    rng = np.random.default_rng(nseg)
    specs = []
    for i in range(nseg):
        w = int(rng.choice(COPY_WORDS[1:-1]))
        null = (nseg == 2 and i == 1) or (nseg == 119 and i % 3 == 2)
        specs.append((w, None if null else int(rng.integers(0, 4)) * (i % 2), int(rng.integers(0, 4)) * (i % 2)))
    _run_add(entry, specs, 4, seed=100 + nseg)


def test_multi_add_only_null_sources():
    for entry in ("demf_multi_add", "demf_multi_add_sumsq"):
        _run_add(entry, [(1025, None, 0), (5, None, 3), (4, None, 1)], 4, seed=1)


def test_multi_add_sumsq_zero_and_non_finite_results():
    """All-zero results (null-source pieces of zeros among them) leave the state's bits alone; an inf or NaN result
    makes sumsq non-finite."""
    specs = [(2049, 0, 0), (1025, 1, 2), (5, None, 3)]
    for special in ("zero", float("inf"), float("nan")):
        _run_add("demf_multi_add_sumsq", specs, 4, seed=5, special=special)


def test_multi_add_bad_arguments():
    from demf_amd import _ffi
    for entry, tail in (("demf_multi_add", ()), ("demf_multi_add_sumsq", (None,))):
        with pytest.raises(RuntimeError, match="bad arguments"):
            _ffi.call(entry, -1, None, 1, *tail, None)
        with pytest.raises(RuntimeError, match="bad arguments"):
            _ffi.call(entry, 1, None, 0, *tail, None)
        with pytest.raises(RuntimeError, match="null"):
            _ffi.call(entry, 1, None, 1, *tail, None)
        _ffi.call(entry, 0, None, 1, *tail, None)                       # an empty table is no launch


# ---- demf_scalars_accum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10])
def test_scalars_accum(n):
    """Three calls in a row onto a sentinel-guarded block: per call |got - ref64| <= 2 * 2^-24 * (|acc| + |scale * v|)
    (one rounded product, one rounded sum).  Bad n and null pointers are rejected with the block untouched."""
    from demf_amd import _ffi
    rng = np.random.default_rng(n)
    block = np.full(GUARD + n + GUARD, oc.SENTINEL, np.float32)
    block[GUARD:GUARD + n] = (rng.standard_normal(n) * 2).astype(np.float32)
    dev = _place(block, 0)
    acc_ptr = dev.data_ptr() + 4 * GUARD
    vals = torch.from_numpy((rng.standard_normal((3, 16)) * 5).astype(np.float32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    prev = block.copy()
    for call, scale in enumerate((1.0 / 3.0, 0.125, -2.5)):
        ptrs = (ctypes.c_void_p * n)(*[vals[call, 15 - i:].data_ptr() for i in range(n)])   # views at any offset
        _ffi.call("demf_scalars_accum", n, ctypes.addressof(ptrs), acc_ptr, scale, stream)
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        assert np.array_equal(_bits(got[:GUARD]), _bits(block[:GUARD]))
        assert np.array_equal(_bits(got[GUARD + n:]), _bits(block[GUARD + n:]))
        v = vals[call].cpu().numpy()[15 - np.arange(n)].astype(np.float64)
        a = prev[GUARD:GUARD + n].astype(np.float64)
        sv = float(np.float32(scale)) * v
        err = np.abs(got[GUARD:GUARD + n].astype(np.float64) - (a + sv))
        bound = 2 * U * (np.abs(a) + np.abs(sv))
        print("scalars_accum n %d call %d: worst err / bound %.3f" % (n, call, float((err / bound).max())))
        assert (err <= bound).all(), (call, err, bound)
        prev = got.copy()
    ptrs = (ctypes.c_void_p * 10)(*[vals[0, i:].data_ptr() for i in range(10)])
    holed = (ctypes.c_void_p * 10)(*[vals[0, i:].data_ptr() if i != 0 else None for i in range(10)])
    for args, what in (((0, ctypes.addressof(ptrs), acc_ptr), "n=0"), ((11, ctypes.addressof(ptrs), acc_ptr), "n=11"),
                       ((1, None, acc_ptr), "null pointer"), ((1, ctypes.addressof(ptrs), None), "null pointer"),
                       ((1, ctypes.addressof(holed), acc_ptr), "null pointer")):
        with pytest.raises(RuntimeError, match=what):
            _ffi.call("demf_scalars_accum", *args, 0.5, stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(prev))


# ---- the engine ---------------------------------------------------------------------------------------------------
def _cfg(dropout=0.0):
    cfg = fixtures.tiny_cfg()
    return dataclasses.replace(cfg, head=dataclasses.replace(cfg.head, attn_dropout=dropout, ffn_dropout=dropout))


def _scene_batch(cfg, seed):
    from demf_amd import synthetic
    raw = synthetic.make_scene_batch(3, 1024, fixtures.TINY_PYRAMID, fixtures.TINY_INPUT, cfg.head.embed_dims,
                                     seed=seed, n_gt=4)
    return dict(points=torch.from_numpy(raw["points"]).cuda(),
                img_features=[torch.from_numpy(f).cuda() for f in raw["img_features"]],
                img_metas=raw["img_metas"],
                gt_bboxes_3d=[torch.from_numpy(b).cuda() for b in raw["gt_boxes"]],
                gt_labels_3d=[torch.from_numpy(l).cuda() for l in raw["gt_labels"]])


def _trainer(cfg, seed=3, **kw):
    from demf_amd import engine
    from demf_amd.modules import DeMFHotPath
    torch.manual_seed(11)
    model = DeMFHotPath(cfg)
    fixtures.seed_weights(model, seed)
    model.cuda().train()
    return engine.Trainer(model, **kw), model


_MEAN = {}


def _mean_gradient():
    """The three batches and the mean of their gradients, each taken on its own by an accumulate=1 twin's _fwd_bwd
    (computed once, shared, never modified)."""
    if not _MEAN:
        cfg = _cfg()
        batches = [_scene_batch(cfg, s) for s in (3, 4, 5)]
        twin, _ = _trainer(cfg, lr=0.0, weight_decay=0.0, max_grad_norm=0.0)
        grads = []
        for b in batches:
            twin._fwd_bwd(b)
            grads.append(twin.flat.flat.double().clone())
        _MEAN.update(cfg=cfg, batches=batches, mean=sum(grads) / 3)
    return _MEAN


def _assert_group_closed(tr, t):
    torch.cuda.synchronize()
    assert tr.micro == 0 and tr.opt.t == t
    assert not bool(tr.flat.flat.any()), "the flat gradient buffer is zero between optimizer steps"
    assert tr._loss_acc is None or not bool(tr._loss_acc.any())
    state = tr.opt.state.cpu().numpy()
    assert not state[0:8].any() and not state[16:20].any(), "sumsq and the ticket are zero between optimizer steps"


def test_eager_group_takes_the_mean_gradient():
    ref = _mean_gradient()
    tr, model = _trainer(ref["cfg"], lr=0.0, weight_decay=0.0, max_grad_norm=0.0, accumulate=3)
    before = tr.opt.flat.clone()
    for i, b in enumerate(ref["batches"]):
        assert tr.micro == i
        tr.step(b)
        if i < 2:
            assert tr.opt.t == 0 and bool(tr.flat.flat.any())         # no update, the sum is building up
    _assert_group_closed(tr, 1)
    got = tr.opt.exp_avg.double() / (1.0 - tr.opt.betas[0])
    rel = ((got - ref["mean"]).norm() / ref["mean"].norm()).item()
    print("eager W=3 mean gradient: rel-L2 %.3e" % rel)
    assert rel < 1e-3
    assert torch.equal(tr.opt.flat, before), "lr = 0, weight_decay = 0: the parameters stay"


def test_group_clip_and_meter_row():
    from demf_amd import meter
    ref = _mean_gradient()
    norm = ref["mean"].norm().item()
    max_norm = 0.1 * norm
    tr, _ = _trainer(ref["cfg"], lr=0.0, weight_decay=0.0, max_grad_norm=max_norm, accumulate=3)
    m = meter.StepMeter(meter.loss_names(), ring_rows=8)
    tr.attach_meter(m)
    per_pass = []
    for b in ref["batches"]:
        tr.step(b)
        per_pass.append([float(s) for s in tr._loss_scalars])
    m.snapshot()
    rows = m.collect(wait=True)
    _assert_group_closed(tr, 1)
    assert len(rows) == 1 and rows[0]["t"] == 0 and not rows[0]["nonfinite"], rows
    row = rows[0]
    print("row grad_norm %.6f twin %.6f clip %.6f" % (row["grad_norm"], norm, row["clip"]))
    assert abs(row["grad_norm"] - norm) <= 1e-3 * norm
    gn = np.float32(row["grad_norm"])
    want_clip = min(np.float32(1.0), np.float32(max_norm) / (gn + np.float32(1e-6)))
    assert abs(np.float32(row["clip"]) - want_clip) <= np.spacing(want_clip), (row["clip"], want_clip)
    for k, name in enumerate(m.names):
        mean = sum(np.float64(p[k]) for p in per_pass) / 3
        assert abs(row[name] - mean) <= 4 * U * abs(mean), (name, row[name], mean)
    want = (1.0 - tr.opt.betas[0]) * float(want_clip) * ref["mean"]
    rel = ((tr.opt.exp_avg.double() - want).norm() / want.norm()).item()
    print("clipped W=3 exp_avg: rel-L2 %.3e" % rel)
    assert rel < 1e-3


@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_step_cache_groups_match_eager_groups(dropout):
    """Trainer.bucketed() with accumulate = 2 over test_gpu_engine's ten batches of two shapes against an eager
    accumulate = 2 twin: graphs are captured lazily per (shape, role), two of them in the MIDDLE of a group
    (micro = 1), where the dry warm-up passes add into the flat buffer and must be undone - a leaked pass doubles
    that group's gradient.  Bars: those of test_shape_bucketed_capture_matches_eager_steps (set for ten updates of
    these batches; here there are five)."""
    from test_gpu_engine import _shape_batches
    cfg = _cfg(dropout)
    batches = _shape_batches(cfg, 10)

    def run(bucketed):
        tr, model = _trainer(cfg, seed=9, lr=2e-4, accumulate=2)
        stepper = tr.bucketed(max_graphs=3, capture_on=2, warmup=1) if bucketed else None
        losses = []
        for i, b in enumerate(batches):
            assert tr.micro == i % 2
            nxt = batches[i + 1]["points"] if i + 1 < len(batches) else None
            l = stepper.step(b, next_points=nxt) if bucketed else tr.step(b)
            losses.append(float(l))
        _assert_group_closed(tr, 5)
        bufs = torch.cat([b.detach().double().reshape(-1) for b in model.buffers()])
        return losses, tr.opt.flat.clone().double(), bufs, stepper

    la, pa, ba, _ = run(False)
    lb, pb, bb, sc = run(True)
    roles = [(role, micro) for _, role, micro in sc.captures]
    print("captures:", roles, "stats:", sc.stats)
    assert any(micro >= 1 for _, micro in roles), "no capture fell inside an open group"
    assert {r for r, _ in roles} == {"accumulate", "last"}
    assert all((r == "last") == (micro == 1) for r, micro in roles)
    assert sc.stats["captured"] == len(roles) == len(sc.graphs) == 4 and sc.stats["eager"] == 3, sc.stats
    assert sc.stats["replayed"] == len(batches) - sc.stats["eager"] and sc.stats["evicted"] == 0
    assert len(sc.pipes) == 1, "all four graphs share the cloud shape's pre-pass pipeline"
    assert len({id(r.geo) for r in sc.graphs.values()}) == 1
    for i, (x, y) in enumerate(zip(la, lb)):
        tol = 2e-3 * (1 + i / 4) if i < 6 else 1.5e-2
        print("pass %d: eager %.6f bucketed %.6f rel %.2e (bar %.2e)" % (i, x, y, abs(x - y) / abs(x), tol))
    print("parameters rel-L2 %.3e, buffers rel-L2 %.3e" % (((pa - pb).norm() / pa.norm()).item(),
                                                         ((ba - bb).norm() / ba.norm()).item()))
    for i, (x, y) in enumerate(zip(la, lb)):
        tol = 2e-3 * (1 + i / 4) if i < 6 else 1.5e-2
        assert abs(x - y) <= tol * abs(x), (i, x, y)
    assert ((pa - pb).norm() / pa.norm()).item() < 6e-4
    assert ((ba - bb).norm() / ba.norm()).item() < 3e-3


def test_refusals_leave_the_state_alone(monkeypatch):
    ref = _mean_gradient()
    b0, b1 = ref["batches"][:2]
    tr, model = _trainer(ref["cfg"], lr=1e-4, accumulate=2)

    def snap():
        torch.cuda.synchronize()
        return (tr.micro, tr.accumulate, tr.opt.flat.clone(), tr.flat.flat.clone(), tr.opt.state.clone(),
                [b.clone() for b in model.buffers()])

    def same(a, b):
        return a[:2] == b[:2] and all(torch.equal(x, y) for x, y in zip(a[2:5], b[2:5])) and \
            all(torch.equal(x, y) for x, y in zip(a[5], b[5]))

    # every form documented as refusing accumulate > 1
    s0 = snap()
    with pytest.raises(RuntimeError, match="capture_double"):
        tr.capture_double(b0, b1)
    monkeypatch.setenv("DEMF_GEO_AT_BWD", "1")
    with pytest.raises(RuntimeError, match="DEMF_GEO_AT_BWD"):
        tr.capture(b0, warmup=1)
    monkeypatch.delenv("DEMF_GEO_AT_BWD")
    tr.allreduce_stub_us, tr.allreduce_overlap = 50, True
    with pytest.raises(RuntimeError, match="overlapped"):
        tr.step(b0)
    with pytest.raises(RuntimeError, match="overlapped"):
        tr.capture(b0, warmup=1)
    tr.allreduce_stub_us, tr.allreduce_overlap = 0, None
    with pytest.raises(ValueError, match="role"):
        tr.capture(b0, warmup=1, role="first")
    assert same(s0, snap())
    # a 'last' graph at micro = 0, an 'accumulate' graph at micro = 1
    last = tr.capture(b0, warmup=1, role="last")
    acc = tr.capture(b1, warmup=1)                       # (role from micro = 0)
    assert (last.role, acc.role) == ("last", "accumulate")
    assert same(s0, snap()), "captures are dry"
    with pytest.raises(RuntimeError, match="micro = 0"):
        last()
    assert same(s0, snap())
    acc()
    s1 = snap()
    assert s1[0] == 1 and tr.opt.t == 0 and bool(tr.flat.flat.any())
    with pytest.raises(RuntimeError, match="micro = 1"):
        acc()
    assert same(s1, snap())
    last()
    _assert_group_closed(tr, 1)
    # accumulate changed after the capture
    s2 = snap()
    tr.accumulate = 3
    s3 = snap()
    for r in (acc, last):
        with pytest.raises(RuntimeError, match="accumulate = 2.*accumulate = 3"):
            r()
    assert same(s3, snap()) and s3[0] == s2[0] == 0


# ---- the runner ---------------------------------------------------------------------------------------------------
SIX = [(6000, (53, 73), 3), (5000, (53, 73), 0), (7000, (53, 73), 4), (4500, (53, 73), 2), (5500, (53, 73), 1),
       (6500, (53, 73), 5)]
_RUNS = {}


def _dataset(tmp_path_factory):
    if "ds" not in _RUNS:
        import pipeline_reference as pref
        from demf_amd.dataset import SUNRGBDDataset
        root = str(tmp_path_factory.mktemp("accumulate"))
        ann, _ = pref.write_dataset(root, SIX, jpeg=True)
        _RUNS["ds"] = dict(root=root, ann=ann, ds=SUNRGBDDataset(root, ann))
    return _RUNS["ds"]


def _kwargs(**kw):
    """3 batches per pass x 3 passes = 9 batches per runner epoch, accumulate = 2: 4 steps, 1 batch discarded, and
    groups that run across the passes."""
    from test_gpu_train import _fit_kwargs
    return _fit_kwargs(**dict(dict(repeat=3, accumulate=2), **kw))


def _fit(tmp_path_factory, name, **kw):
    from demf_amd import train
    from test_gpu_train import _detector
    d = _dataset(tmp_path_factory)
    work = os.path.join(d["root"], name)
    steps = []
    out = train.fit(_detector(), d["ds"], work, on_step=lambda info: steps.append(
        (info["epoch"], info["iter"], info["micro"], info["indices"], info["loss"].clone())), **_kwargs(**kw))
    torch.cuda.synchronize()
    return dict(work=work, steps=steps, out=out)


@pytest.mark.parametrize("graphs", [False, True])
def test_runner_counts_optimizer_steps(tmp_path_factory, graphs):
    from demf_amd import train
    from test_gpu_train import _log
    run = _fit(tmp_path_factory, "graphs" if graphs else "eager", graphs=graphs)
    _RUNS[graphs] = run
    per_pass = 3
    steps, dropped = train.accumulation_plan(per_pass, 3, 2)
    assert (steps, dropped) == (4, 1)
    out = run["out"]
    assert out["iter"] == 2 * steps and out["trainer"].opt.t == 2 * steps and out["meter"].next_t == 2 * steps
    assert out["trainer"].micro == 0
    lines = [l for l in _log(run["work"]) if l["mode"] == "train"]
    print(json.dumps(lines))
    assert [(l["epoch"], l["iter"]) for l in lines] == [(1 + i // steps, i + 1) for i in range(2 * steps)]
    assert [l.get("discarded") for l in lines] == ([None] * (steps - 1) + [dropped]) * 2
    # on_step: once per micro-step, 9 per epoch, the last of each epoch belongs to the abandoned group
    seen = run["steps"]
    assert len(seen) == 2 * per_pass * 3
    want = []
    for e in range(2):
        for k in range(per_pass * 3):
            want.append((e + 1, e * steps + k // 2 + 1, k % 2))
    assert [(e, i, m) for e, i, m, _, _ in seen] == want
    # log_interval = 1: a line is one optimizer step, its loss the mean of the two losses on_step saw
    for n, l in enumerate(lines):
        pair = [float(loss) for e, i, m, _, loss in seen if i == n + 1 and e == l["epoch"]][:2]
        mean = (np.float64(pair[0]) + np.float64(pair[1])) / 2
        assert abs(l["loss"] - mean) <= 4 * U * abs(mean), (n, l["loss"], pair)
    ckpt = train.load_checkpoint_file(os.path.join(run["work"], "latest.pth"))
    assert ckpt["meta"]["accumulate"] == 2 and ckpt["meta"]["iter"] == 2 * steps
    if graphs:
        sc = out["stepper"]
        assert {r for _, r, _ in sc.captures} == {"accumulate", "last"} and sc.stats["replayed"] > len(sc.captures)


def test_runner_resume_and_command_line(tmp_path_factory, capsys):
    from demf_amd import train
    from test_gpu_pipeline import IMG_SCALE
    from test_gpu_train import SEED, _detector, _log
    d = _dataset(tmp_path_factory)
    whole = _RUNS.get(False) or _fit(tmp_path_factory, "eager_whole", graphs=False)
    first = _fit(tmp_path_factory, "resumed", graphs=False, max_epochs=1)
    latest = os.path.join(first["work"], "latest.pth")
    assert first["out"]["trainer"].opt.t == 4 and train.load_checkpoint_file(latest)["meter"] == dict(next_t=4)
    with pytest.raises(ValueError, match=r"accumulate = 2.*accumulate = 1"):
        train.fit(_detector(), d["ds"], first["work"], resume_from=latest, **_kwargs(graphs=False, accumulate=1))
    steps = list(first["steps"])
    second = train.fit(_detector(seed=9), d["ds"], first["work"], resume_from=latest, on_step=lambda info: steps.append(
        (info["epoch"], info["iter"], info["micro"], info["indices"], info["loss"].clone())), **_kwargs(graphs=False))
    torch.cuda.synchronize()
    assert [s[:4] for s in steps] == [s[:4] for s in whole["steps"]]
    assert second["iter"] == whole["out"]["iter"] == 8 and second["trainer"].opt.t == whole["out"]["trainer"].opt.t == 8
    assert second["meter"].next_t == 8
    assert [(l["epoch"], l["iter"]) for l in _log(first["work"])] == [(1 + i // 4, i + 1) for i in range(8)]
    # the command line
    work = os.path.join(d["root"], "work_cli")
    capsys.readouterr()
    train.main(["--data-root", d["root"], "--ann-file", os.path.basename(d["ann"]), "--work-dir", work, "--no-graphs",
                "--batch-size", "2", "--epochs", "1", "--seed", str(SEED), "--workers", "4", "--log-interval", "1",
                "--accumulate", "2", "--autoscale-lr"],
               model=_detector(), num_points=2048, img_scale=IMG_SCALE, repeat=3)
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["iter"] for l in printed] == [1, 2, 3, 4] and printed[-1]["discarded"] == 1
    assert all(l["lr"] == pytest.approx(0.008 * 2 / 8, rel=1e-6) for l in printed)
