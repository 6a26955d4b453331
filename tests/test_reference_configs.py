"""CPU: the reference's SHIPPED language-pretraining configs must build through this package's registries unchanged: `model`,
`optimizer` + `param_dicts`, `scheduler`, the trainer type `train.type` (tools/train.py:14-17: TRAINERS.build(dict(type=cfg.train.type,
cfg=cfg))) and every hook this build covers.  The configs are plain assignments of literals; their evaluated values (with `_base_`
merged) are stored as data in tests/golden/lang_configs.txt (tests/golden/make_golden_configs.py wrote it from the reference tree).

  configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py   (BASELINE config 4: MultiDatasetTrainer)
  configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py                         (BASELINE config 3: DefaultTrainer)
"""
import ast
import os

import pytest
import torch

CONFIGS = ["configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py",
           "configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py"]


def load_config(golden_dir, rel):
    """The evaluated config (a Python literal: tuples stay tuples) as the reference's config loader returns it."""
    with open(os.path.join(golden_dir, "lang_configs.txt")) as f:
        return ast.literal_eval(f.read())[rel]


@pytest.mark.parametrize("rel", CONFIGS)
def test_shipped_lang_config_builds_through_the_registries(rel, tmp_path, golden_dir):
    from scenesplat_amd.pointcept_api import HOOKS, MODELS, TRAINERS, engine
    cfg = load_config(golden_dir, rel)
    assert cfg["mix_prob"] == 0.8 and cfg["enable_amp"] is True                     # Mix3D in 80 % of the training batches
    assert cfg["clip_grad"] == (1.0 if "concat_dataset" in rel else None)
    # ---- model: LangPretrainer(PT-v3m1, 3 criteria), 393 state-dict tensors, 91.71 M parameters
    model = MODELS.build(cfg["model"])
    assert type(model).__name__ == "LangPretrainer" and len(model.state_dict()) == 393
    nparam = sum(p.numel() for p in model.parameters())
    assert abs(nparam / 1e6 - 91.71) < 0.01, nparam
    # ---- optimizer: AdamW, names containing "block" at the lower learning rate (utils/optimizer.py:13-48)
    opt = engine.build_optimizer(cfg["optimizer"], model, cfg["param_dicts"])
    groups = [(g["lr"], len(g["params"])) for g in opt.param_groups]
    assert groups == [(0.006, 39), (0.0006, 324)], groups
    assert all(g["weight_decay"] == 0.05 for g in opt.param_groups)
    # ---- scheduler: OneCycleLR with per-group max_lr; cycle_momentum cycles AdamW's beta1 (utils/scheduler.py:100-134)
    sched = engine.build_scheduler(dict(cfg["scheduler"], total_steps=1000), opt)
    assert [round(g["lr"], 8) for g in opt.param_groups] == [0.0006, 0.00006]           # max_lr / div_factor at step 0
    assert abs(opt.param_groups[0]["betas"][0] - 0.95) < 1e-9
    for _ in range(50):
        opt.step(); sched.step()
    assert abs(opt.param_groups[0]["lr"] - 0.006) < 1e-6 and abs(opt.param_groups[0]["betas"][0] - 0.85) < 1e-6   # peak at pct_start
    # ---- trainer type and hooks
    ttype = cfg["train"]["type"]
    assert ttype in TRAINERS.module_dict, ttype
    assert ttype == ("MultiDatasetTrainer" if "concat_dataset" in rel else "DefaultTrainer")
    covered = [h for h in cfg["hooks"] if h["type"] in HOOKS.module_dict]
    missing = sorted({h["type"] for h in cfg["hooks"]} - {h["type"] for h in covered})
    # the zero-shot evaluators' metric code is out of scope; everything else the config names is registered
    assert [h["type"] for h in covered] == ["CheckpointLoader", "IterationTimer", "InformationWriter", "CheckpointSaver"], covered
    assert all(m in ("LangPretrainZeroShotSemSegEvalMulti", "LangPretrainZeroShotSemSegEval", "PreciseEvaluator") for m in missing), missing
    # ---- and the trainer itself, built the way tools/train.py does, from the config's own dicts (CPU: nothing is launched)
    run_cfg = {k: cfg[k] for k in ("model", "optimizer", "scheduler", "param_dicts", "enable_amp", "clip_grad", "mix_prob")}
    run_cfg.update(device="cpu", eval_epoch=2, save_path=str(tmp_path), hooks=covered, find_unused_parameters=cfg["find_unused_parameters"])
    batches = [dict(feat=torch.zeros(1, 11))] * 5
    loader = [(batches, 3), (batches[:2], 2)] if ttype == "MultiDatasetTrainer" else batches
    tr = TRAINERS.build(dict(type=ttype, cfg=run_cfg, train_loader=loader))
    assert type(tr.model).__name__ == "LangPretrainer"
    if ttype == "MultiDatasetTrainer":
        # 5 batches of the main dataset at ratio 3 -> one full round (3 + 2) + 2 left over (engines/train.py:358-365)
        assert tr.comm_info["iter_per_epoch"] == 7 == len(tr.train_loader) == len(list(tr.train_loader))
        assert tr.scheduler.total_steps == 7 * 2
    else:
        assert tr.scheduler.total_steps == 5 * 2
