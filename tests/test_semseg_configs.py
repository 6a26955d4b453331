"""CPU: the reference's SHIPPED ScanNet semantic-segmentation configs build through this package's registries: DefaultSegmentorV2 with
the reference's state-dict keys and shapes, optimizer groups from param_dicts, OneCycleLR, the DefaultTrainer and every hook but
PreciseEvaluator.  The evaluated configs (`_base_` merged) and the reference model's key -> shape maps are data in
tests/golden/semseg_configs.txt and tests/golden/semseg.npz (tests/golden/make_golden_semseg.py wrote them from the reference tree).

  configs/scannet/semseg-gs-scannet-all-w-normal-fixed-xyz.py      (20 classes)
  configs/scannet/semseg-gs-scannet200-all-w-normal-fixed-xyz.py   (200 classes)
"""
import ast
import os

import numpy as np
import pytest
import torch

CONFIGS = ["configs/scannet/semseg-gs-scannet-all-w-normal-fixed-xyz.py",
           "configs/scannet/semseg-gs-scannet200-all-w-normal-fixed-xyz.py"]


def load_config(golden_dir, rel):
    with open(os.path.join(golden_dir, "semseg_configs.txt")) as f:
        return ast.literal_eval(f.read())[rel]


@pytest.mark.parametrize("i,rel", list(enumerate(CONFIGS)))
def test_shipped_semseg_config_builds_through_the_registries(i, rel, tmp_path, golden_dir):
    from scenesplat_amd.pointcept_api import HOOKS, MODELS, TRAINERS, engine
    cfg = load_config(golden_dir, rel)
    fx = np.load(os.path.join(golden_dir, "semseg.npz"))
    num_classes = 20 if i == 0 else 200
    assert cfg["model"]["num_classes"] == num_classes == cfg["data"]["num_classes"] and cfg["data"]["ignore_index"] == -1
    assert len(cfg["data"]["names"]) == num_classes
    assert [c["type"] for c in cfg["model"]["criteria"]] == ["CrossEntropyLoss", "LovaszLoss"]
    # ---- model: the reference's keys and shapes, in the reference's order, and its parameter count
    model = MODELS.build(cfg["model"])
    assert type(model).__name__ == "DefaultSegmentorV2"
    sd = model.state_dict()
    assert list(sd.keys()) == list(fx[f"sd{i}_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(fx[f"sd{i}_shapes"])
    assert sum(p.numel() for p in model.parameters()) == int(fx[f"sd{i}_nparam"])
    assert tuple(model.seg_head.weight.shape) == (num_classes, 64)
    crit = model.criteria.criteria
    assert [type(c).__name__ for c in crit] == ["CrossEntropyLoss", "LovaszLoss"]
    assert crit[0].ignore_index == -1 and crit[1].ignore_index == -1 and crit[1].class_seen is None
    # ---- optimizer: AdamW, names containing "block" at the lower learning rate (utils/optimizer.py:13-48)
    opt = engine.build_optimizer(cfg["optimizer"], model, cfg["param_dicts"])
    names = [n for n, _ in model.named_parameters()]
    n_block = sum("block" in n for n in names)
    groups = [(g["lr"], len(g["params"])) for g in opt.param_groups]
    assert groups == [(0.006, len(names) - n_block), (0.0006, n_block)], groups
    ids0 = {id(p) for p in opt.param_groups[0]["params"]}
    assert id(model.seg_head.weight) in ids0 and id(model.seg_head.bias) in ids0
    assert all(g["weight_decay"] == 0.05 for g in opt.param_groups)
    # ---- scheduler: OneCycleLR, div_factor 10, peak at pct_start 0.05
    sched = engine.build_scheduler(dict(cfg["scheduler"], total_steps=1000), opt)
    assert [round(g["lr"], 8) for g in opt.param_groups] == [0.0006, 0.00006]
    for _ in range(50):
        opt.step(); sched.step()
    assert abs(opt.param_groups[0]["lr"] - 0.006) < 1e-6 and abs(opt.param_groups[1]["lr"] - 0.0006) < 1e-7
    # ---- trainer type and hooks: everything but PreciseEvaluator is covered
    assert cfg["train"]["type"] == "DefaultTrainer" and cfg["evaluate"] is True
    covered = [h for h in cfg["hooks"] if h["type"] in HOOKS.module_dict]
    missing = sorted({h["type"] for h in cfg["hooks"]} - {h["type"] for h in covered})
    assert [h["type"] for h in covered] == ["CheckpointLoader", "IterationTimer", "InformationWriter", "SemSegEvaluator",
                                           "CheckpointSaver"], covered
    assert missing == ["PreciseEvaluator"], missing
    run_cfg = {k: cfg[k] for k in ("model", "optimizer", "scheduler", "param_dicts", "enable_amp", "clip_grad", "mix_prob", "data")}
    run_cfg.update(device="cpu", eval_epoch=2, save_path=str(tmp_path), hooks=covered, find_unused_parameters=cfg["find_unused_parameters"])
    batches = [dict(feat=torch.zeros(1, 14))] * 5
    tr = TRAINERS.build(dict(type="DefaultTrainer", cfg=run_cfg, train_loader=batches, val_loader=batches[:2]))
    assert type(tr.model).__name__ == "DefaultSegmentorV2" and tr.val_loader is not None and len(tr.val_loader) == 2
    assert tr.scheduler.total_steps == 5 * 2
    ev = [h for h in tr.hooks if type(h).__name__ == "SemSegEvaluator"]
    assert len(ev) == 1 and ev[0].enable_voting is False and ev[0].vote_k == 25
    assert ev[0]._meta() == (num_classes, -1, cfg["data"]["names"])


def test_trainer_val_loader_defaults_to_none(tmp_path):
    from scenesplat_amd.pointcept_api import TRAINERS
    cfg = dict(model=dict(type="DefaultSegmentorV2", num_classes=4, backbone_out_channels=16,
                          backbone=dict(type="PT-v3m1", in_channels=6, enc_depths=(1, 1), enc_channels=(16, 16), enc_num_head=(1, 1),
                                        enc_patch_size=(16, 16), dec_depths=(1,), dec_channels=(16,), dec_num_head=(1,),
                                        dec_patch_size=(16,), stride=(2,)),
                          criteria=[dict(type="CrossEntropyLoss", ignore_index=-1)]),
               optimizer=dict(type="AdamW", lr=0.01), scheduler=dict(type="OneCycleLR", max_lr=0.01), device="cpu",
               save_path=str(tmp_path), hooks=[dict(type="SemSegEvaluator")])
    tr = TRAINERS.build(dict(type="DefaultTrainer", cfg=cfg, train_loader=[0, 1]))
    assert tr.val_loader is None
    tr.hooks[0].after_epoch()                 # nothing to evaluate: a no-op, no metric
    assert "current_metric_value" not in tr.comm_info


@pytest.mark.parametrize("kwargs", [dict(mode="binary"), dict(mode="multilabel"), dict(mode="multiclass", per_image=True)])
def test_lovasz_modes_outside_the_kernel_raise(kwargs):
    from scenesplat_amd.pointcept_api import LOSSES
    with pytest.raises(NotImplementedError, match="not implemented"):
        LOSSES.build(dict(type="LovaszLoss", ignore_index=-1, **kwargs))
    with pytest.raises(ValueError):
        LOSSES.build(dict(type="LovaszLoss", mode="softmax"))


@pytest.mark.parametrize("loss", [dict(type="CrossEntropyLoss", ignore_index=-1),
                                  dict(type="CrossEntropyLoss", ignore_index=-1, label_smoothing=0.1),
                                  dict(type="LovaszLoss", mode="multiclass", ignore_index=-1)])
def test_seg_losses_refuse_cpu_tensors(loss):
    from scenesplat_amd.pointcept_api import LOSSES
    crit = LOSSES.build(loss)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.randn(8, 5), torch.randint(0, 5, (8,)))


def test_cross_entropy_keeps_its_weight_on_the_host():
    from scenesplat_amd.pointcept_api import LOSSES
    ce = LOSSES.build(dict(type="CrossEntropyLoss", weight=[1.0, 2.0, 0.5], reduction="sum", ignore_index=-1))
    assert ce.weight.device.type == "cpu" and ce.weight.tolist() == [1.0, 2.0, 0.5] and ce.reduction == "sum"
