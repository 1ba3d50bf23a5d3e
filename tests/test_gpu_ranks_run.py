"""The multi-rank runners on one GPU, as tests/test_gpu_multirank.py runs the engine: two ranks started with mp.spawn
share cuda:0 (DEMF_SHARE_DEVICE=1) and talk through gloo (DEMF_DIST_BACKEND=gloo), so that everything above the
transport - the loader shards, the merged detection store, the merged step meter, rank-0 log and checkpoints, the
buffer broadcast before validation, resume - runs on hardware.  One spawn per test; results come back through files.
This proves the software path; no run on more than one GPU exists."""
import json
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

WORLD = 2
SEED = 5
# (n_points, image (h, w), n_gt): ONE image size, so that a captured shape repeats; one scene without ground truth
FIVE = [(6000, (53, 73), 3), (5000, (53, 73), 0), (7000, (53, 73), 4), (4500, (53, 73), 2), (5500, (53, 73), 1)]
EIGHT = FIVE + [(6500, (53, 73), 2), (4800, (53, 73), 3), (5200, (53, 73), 1)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dump(obj, path):
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _write(root, specs):
    import pipeline_reference as pref
    ann, _ = pref.write_dataset(root, specs, jpeg=True)
    return ann


def _sets(root):
    from demf_amd.dataset import SUNRGBDDataset
    ann = os.path.join(root, "sunrgbd_infos_train.pkl")
    return SUNRGBDDataset(root, ann), SUNRGBDDataset(root, ann, test_mode=True)


def _detector():
    from test_gpu_train import _detector as make
    return make()


def _test_detector():
    """The same detector with its head widened as tests/test_gpu_detections.py widens it: on bare seeded weights no
    box holds points and the test pass detects nothing, which would compare empty stores."""
    from test_gpu_detections import _detector as make
    return make()


def _fit_kwargs(**kw):
    from test_gpu_pipeline import IMG_SCALE
    out = dict(batch_size=2, num_points=2048, img_scale=IMG_SCALE, max_epochs=1, repeat=1, log_interval=1,
               eval_interval=1, seed=SEED, workers=2, echo=False)
    out.update(kw)
    return out


def _results(store):
    return [(r["boxes_3d"].tensor, r["scores_3d"], r["labels_3d"]) for r in store.results()]


def _same_results(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) and x.dtype == y.dtype for ra, rb in zip(a, b)
                                    for x, y in zip(ra, rb))


def _run_test(root):
    from demf_amd import infer
    from test_gpu_pipeline import IMG_SCALE
    _, val = _sets(root)
    store = infer.run_test(_test_detector().cuda(), val, batch_size=1, workers=2, num_points=2048, img_scale=IMG_SCALE,
                           seed=SEED)
    return val, store


def _same_dict(a, b):
    """Equality of two evaluation dicts in which an AP without ground truth is NaN on both sides."""
    return a is not None and b is not None and json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def _log(work):
    with open(os.path.join(work, "train.log.json")) as f:
        return [json.loads(l) for l in f if l.strip()]


def _replica(out):
    torch.cuda.synchronize()
    return dict(flat=out["trainer"].opt.flat.clone().cpu(),
                sd={k: v.clone().cpu() for k, v in out["trainer"].model.state_dict().items()})


# ---- what a rank runs -----------------------------------------------------------------------------------------------
def _job_test(rank, root):
    val, store = _run_test(root)
    _dump(dict(results=_results(store), scenes=len(store), ev=val.evaluate(store) if rank == 0 else None),
          os.path.join(root, f"test_r{rank}.pkl"))


def _job_fit(rank, root):
    from demf_amd import train
    ds, val = _sets(root)
    steps = []
    out = train.fit(_detector(), ds, os.path.join(root, "work"), val_set=val, graphs=False,
                    on_step=lambda info: steps.append((info["epoch"], info["iter"], info["indices"])), **_fit_kwargs())
    _dump(dict(steps=steps, val=out["val"], iter=out["iter"], t=out["trainer"].opt.t, next_t=out["meter"].next_t,
               **_replica(out)), os.path.join(root, f"fit_r{rank}.pkl"))


def _job_resume(rank, root):
    from demf_amd import train
    ds, val = _sets(root)
    work = os.path.join(root, "work")
    steps = []
    on_step = lambda info: steps.append((info["epoch"], info["iter"], info["indices"]))     # noqa: E731
    first = train.fit(_detector(), ds, work, val_set=val, graphs=True, on_step=on_step, **_fit_kwargs())
    replayed = [first["stepper"].stats["replayed"]]
    mid = _replica(first)
    del first
    second = train.fit(_detector(), ds, work, val_set=val, graphs=True, on_step=on_step,
                       resume_from=os.path.join(work, "latest.pth"), **_fit_kwargs(max_epochs=2))
    replayed.append(second["stepper"].stats["replayed"])
    _dump(dict(steps=steps, replayed=replayed, mid=mid, iter=second["iter"], t=second["trainer"].opt.t,
               next_t=second["meter"].next_t, **_replica(second)), os.path.join(root, f"resume_r{rank}.pkl"))


def _worker(rank, world, port, root, job):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DEMF_SHARE_DEVICE="1", DEMF_DIST_BACKEND="gloo",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from demf_amd import engine, ranks
    engine.init_distributed()
    assert dist.get_backend() == "gloo" and torch.cuda.current_device() == 0
    assert (ranks.world(), ranks.rank()) == (world, rank)
    globals()["_job_" + job](rank, root)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def _spawn(root, job):
    mp.spawn(_worker, args=(WORLD, _free_port(), root, job), nprocs=WORLD, join=True)
    return [_load(os.path.join(root, f"{job}_r{r}.pkl")) for r in range(WORLD)]


# ---- 1. the sharded test pass ---------------------------------------------------------------------------------------
def test_sharded_test_pass_equals_the_single_process_one(tmp_path):
    root = str(tmp_path)
    _write(root, FIVE)
    # the precondition, on code this layer does not touch: one-scene batches give the same bits run after run
    val, store = _run_test(root)
    single = _results(store)
    assert _same_results(single, _results(_run_test(root)[1])), "the single-process test pass is not reproducible"
    assert len(single) == 5 and sum(len(r[1]) for r in single) > 0
    ev = val.evaluate(store)
    r0, r1 = _spawn(root, "test")
    assert r0["scenes"] == r1["scenes"] == 5
    assert _same_results(r0["results"], single)          # shards 0-2 and 3-4, merged in dataset order, bit for bit
    assert _same_results(r1["results"], r0["results"])   # the merged store is on every rank
    assert _same_dict(r0["ev"], ev) and r1["ev"] is None


# ---- 2. a two-rank fit ----------------------------------------------------------------------------------------------
def _accumulate_run(root, tag):
    from demf_amd import train
    ds, _ = _sets(root)
    steps = []
    work = os.path.join(root, "work_" + tag)
    train.fit(_detector(), ds, work, graphs=False, accumulate=WORLD,
              on_step=lambda info: steps.append((info["iter"], info["micro"], info["indices"])), **_fit_kwargs())
    torch.cuda.synchronize()
    return _log(work), steps


def test_two_rank_fit(tmp_path):
    """Measured on MI355X: the spread of line 1's terms between two single-process accumulate = 2
    runs, and the distance of the two-rank line from them, are printed below before they are compared."""
    from demf_amd import infer, meter, train
    root = str(tmp_path)
    _write(root, EIGHT)
    (log_a, steps_a), (log_b, _) = _accumulate_run(root, "a"), _accumulate_run(root, "b")
    r0, r1 = _spawn(root, "fit")
    work = os.path.join(root, "work")
    lines = _log(work)
    # the log is written once: two train lines (four chunks over two ranks are two steps) and one val line
    assert [(l["mode"], l["epoch"], l["iter"]) for l in lines] == [("train", 1, 1), ("train", 1, 2), ("val", 1, 2)]
    assert sorted(f for f in os.listdir(work) if not f.endswith(".json")) == ["epoch_1.pth", "latest.pth"]
    assert train.load_checkpoint_file(os.path.join(work, "latest.pth"))["meta"]["world"] == 2
    for r in (r0, r1):
        assert r["iter"] == r["t"] == r["next_t"] == 2
    assert _same_dict(r0["val"], r1["val"])
    assert _same_dict(r0["val"], {k: v for k, v in lines[2].items() if k not in ("mode", "epoch", "iter")})
    # replicas: bit-equal to each other and to the checkpoint
    assert torch.equal(r0["flat"], r1["flat"])
    assert set(r0["sd"]) == set(r1["sd"])
    for k, v in r0["sd"].items():
        assert torch.equal(v, r1["sd"][k]), k
    fresh = _detector()
    infer.load_checkpoint(fresh, os.path.join(work, "latest.pth"))
    got = fresh.state_dict()
    assert set(got) == set(r0["sd"])
    for k, v in r0["sd"].items():
        assert torch.equal(got[k].cpu(), v), k
    # the ranks' batches of iteration i are together group i of the single-process accumulate = 2 run
    for i in (1, 2):
        group = [idx for it, micro, idx in sorted(steps_a) if it == i]
        ranks_i = [[idx for _, it, idx in r["steps"] if it == i] for r in (r0, r1)]
        assert all(len(x) == 1 for x in ranks_i) and len(group) == 2
        assert [ranks_i[0][0], ranks_i[1][0]] == group
    # line 1: the same forward at the same weights on the same batches
    names = [n for n in meter.loss_names() if n != "_total"] + ["loss"]
    assert set(names) <= set(lines[0]) and set(lines[0]) == set(log_a[0]) - {"discarded"}
    report = {}
    for k in names:
        a, b, got = log_a[0][k], log_b[0][k], lines[0][k]
        report[k] = dict(spread=abs(a - b), distance=abs(got - a), value=a)
    print("two-rank line 1 vs accumulate = 2:", json.dumps(report))
    for k in names:
        s, d, v = report[k]["spread"], report[k]["distance"], report[k]["value"]
        assert d <= max(10 * s, 1e-6 * abs(v)), (k, report[k])


# ---- 3. captured steps and resume -----------------------------------------------------------------------------------
def test_captured_steps_and_resume_on_two_ranks(tmp_path):
    from demf_amd import train
    root = str(tmp_path)
    _write(root, EIGHT)
    r0, r1 = _spawn(root, "resume")
    work = os.path.join(root, "work")
    for r in (r0, r1):
        assert all(n > 0 for n in r["replayed"]), r["replayed"]          # both runs replayed a captured step
        assert [(e, i) for e, i, _ in r["steps"]] == [(1, 1), (1, 2), (2, 3), (2, 4)]    # iterations continue at 3
        assert r["iter"] == r["t"] == 4 and r["next_t"] == 4
    for part in (lambda r: r["mid"], lambda r: r):                       # after the first run and after the resumed one
        a, b = part(r0), part(r1)
        assert torch.equal(a["flat"], b["flat"])
        for k, v in a["sd"].items():
            assert torch.equal(v, b["sd"][k]), k
    assert not torch.equal(r0["mid"]["flat"], r0["flat"])                # the resumed epoch trained
    lines = _log(work)
    assert [(l["mode"], l["epoch"], l["iter"]) for l in lines] == [
        ("train", 1, 1), ("train", 1, 2), ("val", 1, 2), ("train", 2, 3), ("train", 2, 4), ("val", 2, 4)]
    assert all(np.isfinite(v) for l in lines if l["mode"] == "train" for k, v in l.items() if k != "mode")
    # the file belongs to a two-rank run: a single process refuses it
    ds, _ = _sets(root)
    with pytest.raises(ValueError, match="world = 2 ranks, this run has world = 1"):
        train.fit(_detector(), ds, os.path.join(root, "work_single"), graphs=False,
                  resume_from=os.path.join(work, "latest.pth"), **_fit_kwargs(max_epochs=2))
