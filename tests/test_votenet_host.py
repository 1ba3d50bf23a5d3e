"""Host logic of the points-only baseline's runners: which model ``--model`` builds, which loss names the meter and
the log lines carry, what the loader's host half does without an image, what a points-only batch's shape key is."""
import numpy as np
import pytest
import torch


def test_model_loss_names_come_from_the_head():
    from demf_amd import meter, train
    from demf_amd.modules import VoteNet

    class WithImage:                                         # (any model without a CAVoteHead: the meter's own names)
        pass
    names = train.model_loss_names(VoteNet())
    assert names == ("objectness_loss", "dir_class_loss", "dir_res_loss", "size_res_loss", "semantic_loss", "iou_loss",
                     "vote_loss", "_total")
    assert "center_loss" not in names and "center_loss" in meter.loss_names()
    assert train.model_loss_names(WithImage()) == meter.loss_names()
    rows = [dict({k: 1.0 + i for k in names}, t=i, lr_factor=1.0, grad_norm=2.0, clip=1.0, nonfinite=[]) for i in range(2)]
    line = train.format_log(rows, 1, 2, 0.008, 0.5, names)
    assert "center_loss" not in line and "_total" not in line and line["loss"] == 1.5 and line["vote_loss"] == 1.5
    assert set(line) == {"mode", "epoch", "iter", "lr", "loss", "grad_norm", "time"} | set(names[:-1])


def test_model_argument_of_both_command_lines():
    from demf_amd import infer, train
    base = ["--data-root", "r", "--ann-file", "a"]
    assert train.parse_args(base + ["--work-dir", "w"]).model == "demf"
    assert train.parse_args(base + ["--work-dir", "w", "--model", "votenet"]).model == "votenet"
    assert infer.parse_args(base + ["--checkpoint", "c"]).model == "demf"
    assert infer.parse_args(base + ["--checkpoint", "c", "--model", "votenet"]).model == "votenet"
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--work-dir", "w", "--model", "imvotenet"])


def test_points_only_batch_has_no_pyramid_in_its_shape_key():
    from demf_amd import engine
    pts = torch.zeros(2, 64, 4)
    gt = [torch.zeros(3, 7), torch.zeros(0, 7)]
    key = engine.StepCache.key(dict(points=pts, gt_bboxes_3d=gt, gt_labels_3d=None))
    assert key[0] == (2, 64, 4) and key[1] is None
    with_img = engine.StepCache.key(dict(points=pts, gt_bboxes_3d=gt, gt_labels_3d=None,
                                         img_features=[torch.zeros(2, 8, 4, 4)], img_metas=[{}, {}]))
    assert with_img[0] == key[0] and with_img[1] == ((2, 8, 4, 4),) and with_img[2] == key[2]


@pytest.mark.parametrize("mode", ["train", "test"])
def test_pipeline_host_half_without_images(tmp_path, mode, monkeypatch):
    """``ScenePipeline.load`` with and without the image: the same records, random draws, seeds, boxes and 3-D metadata;
    without it no image file is opened (the files are removed first) and the metas carry no image entry."""
    import os

    import pipeline_reference as pref
    from demf_amd import pipeline as pl
    from demf_amd.dataset import SUNRGBDDataset
    ann, _ = pref.write_dataset(str(tmp_path), [(600, (53, 73), 3), (500, (43, 56), 0)], jpeg=True)
    ds = SUNRGBDDataset(str(tmp_path), ann, test_mode=mode == "test")
    a = pl.ScenePipeline(ds, mode, img_scale=(200, 120), num_points=128, seed=3)
    b = pl.ScenePipeline(ds, mode, img_scale=(200, 120), num_points=128, seed=3, with_img=False)
    want = [a.load(i, epoch=2) for i in range(2)]
    for i in range(2):
        os.remove(ds.get_data_info(i)["img_filename"])
    got = [b.load(i, epoch=2) for i in range(2)]
    for x, y in zip(want, got):
        assert y["img"] is None and x["img"] is not None
        assert x["seed"] == y["seed"] and x["index"] == y["index"]
        assert np.array_equal(pl.param_row(x["params"]), pl.param_row(y["params"]))
        assert np.array_equal(x["raw"], y["raw"]) and np.array_equal(x["gt_bboxes_3d"], y["gt_bboxes_3d"])
        assert (x["gt_labels_3d"] is None) == (y["gt_labels_3d"] is None)
        if x["gt_labels_3d"] is not None:
            assert np.array_equal(x["gt_labels_3d"], y["gt_labels_3d"])
        assert not {"img_shape", "img_filename", "depth2img", "scale_factor"} & set(y["meta"])
        for k in ("pcd_horizontal_flip", "pcd_scale_factor", "transformation_3d_flow", "sample_idx"):
            assert x["meta"].get(k) == y["meta"].get(k), k
