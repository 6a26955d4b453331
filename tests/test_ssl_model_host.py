"""CPU: the host layer of the SimDINO pretraining model -- the numpy / fp64 restatements of tests/ssl_model_cases.py against the reference's
own outputs (tests/golden/ssl_model.npz, written by make_golden_ssl_model.py), the three shipped ssl-pretrain configs through MODELS /
PRETRAINERS, the state-dict key list, and the two schedules.  Construction needs no GPU; nothing here launches a kernel."""
import ast
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssl_model_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssl_model.npz")))


@pytest.fixture(scope="module")
def lits(golden_dir):
    with open(os.path.join(golden_dir, "ssl_model_configs.txt")) as f:
        return ast.literal_eval(f.read())


def case_tag(mtype, size):
    return "mask_%s_%s_" % (mtype, str(size).replace(".", "p"))


def recorded_draws(fx, tag):
    flags = fx[tag + "flag"].tolist()
    return [(f, fx.get(tag + "perm%d" % i), float(fx[tag + "rate"][i]) if f else None) for i, f in enumerate(flags)]


@pytest.mark.parametrize("mtype,size", sc.MASK_CASES)
def test_mask_restatement_reproduces_the_reference(fx, mtype, size):
    gc, offset = sc.mask_batch()
    assert np.array_equal(gc, fx["mask_gc"]) and np.array_equal(offset, fx["mask_offset"])
    tag = case_tag(mtype, size)
    ids, counts = sc.patch_ids(gc, offset, size)
    mask, w = sc.apply_draws(offset, ids, recorded_draws(fx, tag), mtype)
    assert np.array_equal(mask, fx[tag + "mask"])
    assert np.array_equal(w.view(np.uint16), fx[tag + "weights"].view(np.uint16))
    if mtype == "patch":
        # every point of a patch carries the same mask value; at 0.2 every voxel is its own patch, coarser sizes group
        begin = 0
        for b, end in enumerate(offset.tolist()):
            for p in range(counts[b]):
                assert len(set(mask[begin:end][ids[begin:end] == p].tolist())) == 1
            begin = end
        sizes = np.diff(np.concatenate([[0], offset]))
        assert (counts == sizes).all() if size == 0.2 else (counts[1:] < sizes[1:]).all()


@pytest.mark.parametrize("mtype,size", sc.MASK_CASES)
def test_mask_draw_order_replays_from_the_seed(fx, mtype, size):
    gc, offset = sc.mask_batch()
    tag = case_tag(mtype, size)
    s = int(fx[tag + "seed"])
    random.seed(s); np.random.seed(s); torch.manual_seed(s)
    counts = sc.patch_ids(gc, offset, size)[1] if mtype == "patch" else np.diff(np.concatenate([[0], offset]))
    draws = sc.draw_masks(offset, counts, mtype)
    for got, want in zip(draws, recorded_draws(fx, tag)):
        assert got[0] == want[0]
        if got[0]:
            assert np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_loss_restatements_reproduce_the_reference(fx):
    d = sc.mcr_loss64(fx["model_dino_student"], fx["model_dino_teacher"])
    # fp64 restatement of fp32 operands against the reference's fp32 result: the fp32 Cholesky of a 256 x 256 matrix carries ~1e-6 relative
    for k in ("loss", "comp_loss", "global_comp_loss", "expa_loss"):
        ref = float(fx["model_out_dino_mcr_" + k])
        assert abs(d[k] - ref) <= 2e-5 * max(1.0, abs(ref)), (k, d[k], ref)
    got = sc.cosine_patch64(fx["model_ibot_student"], fx["model_ibot_teacher"], fx["model_ibot_weight"])
    ref = float(fx["model_out_sim_ibot_patch_loss"])
    assert abs(got - ref) <= 2e-6 * abs(ref), (got, ref)
    total = float(fx["model_out_sim_dino_crops_loss"]) + ref + float(fx["model_out_global_mae_loss"])
    assert abs(total - float(fx["model_out_loss"])) <= 1e-6 * abs(total)


def test_project_losses_match_the_restatements_on_cpu(fx):
    from scenesplat_amd.pointcept_api import CosinePatchLoss, MCRLoss
    s, t = torch.from_numpy(fx["model_dino_student"]), torch.from_numpy(fx["model_dino_teacher"])
    loss, parts = MCRLoss(out_dim=256, expa_type=1, reduce_cov=0, eps=0.05, eps_end=-1, coeff=0.1)(list(s), list(t), no_diag=True)
    for k in ("loss", "comp_loss", "global_comp_loss", "expa_loss"):
        assert abs(float(parts[k]) - float(fx["model_out_dino_mcr_" + k])) <= 2e-6 * max(1.0, abs(float(parts[k]))), k
    pl, _ = CosinePatchLoss(patch_out_dim=32).forward_masked(torch.from_numpy(fx["model_ibot_student"]), torch.from_numpy(fx["model_ibot_teacher"]),
                                                           masks_weight=torch.from_numpy(fx["model_ibot_weight"]), view_nums=1)
    assert abs(float(pl) - float(fx["model_out_sim_ibot_patch_loss"])) <= 2e-6 * abs(float(pl))
    with pytest.raises(NotImplementedError):
        MCRLoss(out_dim=256, reduce_cov=1)


def test_shipped_configs_build_through_the_registries(lits):
    from scenesplat_amd.pointcept_api import MODELS, PRETRAINERS
    from scenesplat_amd.pointcept_api.ssl import PointTransformerV3_SIMDINO
    configs = [k for k in lits if k.endswith(".py")]
    assert len(configs) == 3
    for rel in configs:
        model = MODELS.build(lits[rel]["model"])
        assert isinstance(model.backbone_student, PointTransformerV3_SIMDINO) and model.backbone_student.do_mask
        assert hasattr(model, "backbone_teacher") == bool(lits[rel]["model"]["do_ema"])
        assert all(getattr(model.backbone_student.enc, "enc%d" % s).down.reduce == "max" for s in range(1, 5))
        assert PRETRAINERS.get(lits[rel]["train"]["type"]).__name__ == "DefaultSSLPreTrainer"
        if rel == "configs/scannet/ssl-pretrain-scannet-all-base.py":
            got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert got == [(k, tuple(s)) for k, s in lits["state_dict"]]
            assert not any(p.requires_grad for p in model.backbone_teacher.parameters())


def test_backbone_without_do_mask_has_no_decoder_and_no_token():
    from scenesplat_amd.pointcept_api import MODELS
    bb = MODELS.build(dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA))
    assert not hasattr(bb, "dec") and not hasattr(bb, "mask_token")
    bb = MODELS.build(dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA, do_mask=True))
    assert tuple(bb.mask_token.shape) == (1, sc.TINY["enc_channels"][0]) and next(iter(bb.state_dict())) == "mask_token"
    wins, _ = bb.plan_specs(with_dec=False)
    assert len(wins) == sum(sc.TINY["enc_depths"]) and len(bb.plan_specs()[0]) == len(wins) + sum(sc.TINY["dec_depths"])
    from scenesplat_amd.pointcept_api import DINOHead
    with pytest.raises(NotImplementedError):
        DINOHead(in_dim=8, out_dim=8, remove_last_layer=False)


def test_pretrainer_builds_on_the_host(fx):
    from scenesplat_amd.pointcept_api import PRETRAINERS
    cfg = dict(model=dict(type="DefaultContrastiverSimDinoV2", backbone_out_channels=64, enable_mae_loss=True,
                          backbone=dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA)),
               optimizer=dict(type="AdamW", lr=0.001, weight_decay=0.001, eps=1e-4),
               scheduler=dict(type="OneCycleLR", max_lr=[0.001, 0.0001], pct_start=0.05, anneal_strategy="cos", div_factor=10.0,
                              final_div_factor=1000.0),
               param_dicts=[dict(keyword="block", lr=0.0001)], eval_epoch=25, enable_amp=True, clip_grad=3.0, device="cpu")
    tr = PRETRAINERS.build(dict(type="DefaultSSLPreTrainer", cfg=cfg, train_loader=[{}, {}]))
    got_m = [tr.momentum_schedule.step() for _ in range(50)]
    got_t = [tr.teacher_temp_schedule.step() for _ in range(50)]
    assert np.array_equal(np.array(got_m), fx["sched_momentum"]) and np.array_equal(np.array(got_t), fx["sched_temp"])
    assert tr.scaler is None


def test_schedules_equal_the_reference_exactly(fx):
    from scenesplat_amd.pointcept_api import CosineScheduler
    mom = CosineScheduler(base_value=0.9, final_value=1, total_iters=50)
    temp = CosineScheduler(base_value=0.07, final_value=0.07, start_warmup_value=0.04, warmup_iters=30, total_iters=30)
    assert np.array_equal(np.array([mom.step() for _ in range(50)]), fx["sched_momentum"])
    assert np.array_equal(np.array([temp.step() for _ in range(50)]), fx["sched_temp"])
    assert mom.step() == 1 and temp.step() == 0.07
