"""PDNorm / PPT-v1m2 on the host: the state-dict contract against the reference's recorded key lists (tests/golden/pdnorm.npz,
written by tests/golden/make_golden_pdnorm.py), the decouple=False refusal, the C ABI, steady_key and the optimizer's keyword groups.
No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

TINY = dict(in_channels=11, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2),
            enc_depths=(1, 1, 2), enc_channels=(16, 32, 64), enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 16),
            dec_depths=(2, 1), dec_channels=(48, 32), dec_num_head=(1, 2), dec_patch_size=(64, 64))       # make_golden_rpe.TINY_CFG
CONDITIONS = ("A", "B", "C")


def backbone_cfg(adaptive=True, affine=True, **kw):
    return dict(type="PT-v3m1", **TINY, enable_flash=False, pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=adaptive,
                pdnorm_affine=affine, pdnorm_conditions=CONDITIONS, **kw)


def ppt_cfg(**kw):
    return dict(type="PPT-v1m2", backbone=backbone_cfg(), criteria=[dict(type="CrossEntropyLoss", ignore_index=-1)],
                backbone_out_channels=48, context_channels=256, conditions=CONDITIONS, num_classes=(5, 7, 4), **kw)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "pdnorm.npz"))


@pytest.mark.parametrize("adaptive,affine", [(False, True), (True, True), (True, False)])
def test_state_dict_keys_and_shapes_equal_the_reference(fx, adaptive, affine):
    from scenesplat_amd.pointcept_api import MODELS
    sd = MODELS.build(backbone_cfg(adaptive, affine)).state_dict()
    tag = f"ad{int(adaptive)}_aff{int(affine)}"
    assert list(sd.keys()) == fx[f"keys_{tag}"].tolist()
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == fx[f"shapes_{tag}"].tolist()
    keys = list(sd.keys())
    for probe in ("embedding.stem.norm.norm.0.running_mean", "enc.enc1.down.norm.0.norm.2.running_mean",
                  "dec.dec0.up.proj.1.norm.1.running_var", "dec.dec0.up.proj_skip.1.norm.0.num_batches_tracked"):
        assert probe in sd, probe
    assert ("enc.enc0.block0.norm1.0.norm.1.weight" in sd) == affine
    assert ("enc.enc0.block0.norm1.0.modulation.1.weight" in sd) == adaptive
    if adaptive:
        assert tuple(sd["enc.enc2.block0.cpe.2.modulation.1.weight"].shape) == (128, 256)      # context_channels is always 256 in PT-v3m1
    pd_affine = [k for k in keys if re.search(r"\.norm\.\d+\.(weight|bias)$", k)]           # weight / bias under a PDNorm's norm.{i}
    if affine:
        assert len(pd_affine) == 2 * 3 * (7 + 3 * 7)              # 7 BatchNorm + 3 LayerNorm x 7 blocks, three conditions each
    else:
        # affine=False: no weight / bias under norm.{i}; the BatchNorm buffers stay; the constant ones / zeros are not persistent
        assert not pd_affine, pd_affine[:3]
        assert not any(k.endswith("_ones") or k.endswith("_zeros") for k in keys)
    assert sum(k.endswith("running_mean") for k in keys) == 3 * 7          # stem + 2 down + 2 x (proj, proj_skip), three conditions each


def test_fixture_guard_figures(fx):
    """The stored outputs distinguish the conditions and feel the context (make_golden_pdnorm.py's guard): at least 0.3 of the RMS."""
    guards = [k for k in fx.files if k.startswith("guard_")]
    assert len(guards) == 8
    for k in guards:
        assert float(fx[k]) >= 0.3, (k, float(fx[k]))


def test_decouple_false_is_refused():
    from scenesplat_amd.pointcept_api import MODELS, MODULES
    from functools import partial
    with pytest.raises(ValueError, match="decouple"):
        MODELS.build(backbone_cfg(pdnorm_decouple=False))
    with pytest.raises(ValueError, match="decouple"):
        MODULES.build(dict(type="PDNorm", num_features=8, norm_layer=partial(torch.nn.LayerNorm), decouple=False))
    # every other combination builds
    for bn in (False, True):
        for ln in (False, True):
            for ad in (False, True):
                for aff in (False, True):
                    MODELS.build(dict(type="PT-v3m1", **TINY, enable_flash=False, pdnorm_bn=bn, pdnorm_ln=ln, pdnorm_adaptive=ad,
                                      pdnorm_affine=aff, pdnorm_conditions=CONDITIONS))


def test_pdnorm_module_contract():
    from functools import partial
    from scenesplat_amd.pointcept_api import MODULES, PDNorm
    m = MODULES.build(dict(type="PDNorm", num_features=8, norm_layer=partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01, affine=False),
                           conditions=CONDITIONS, adaptive=True))
    assert isinstance(m, PDNorm)
    assert list(m.state_dict().keys()) == [f"norm.{i}.{b}" for i in range(3) for b in ("running_mean", "running_var", "num_batches_tracked")] \
        + ["modulation.1.weight", "modulation.1.bias"]
    assert tuple(m.modulation[1].weight.shape) == (16, 256)
    assert m.index_of("B") == 1 and m.index_of(["C", "A"]) == 2
    with pytest.raises(AssertionError):
        m.index_of("ScanNet")
    with pytest.raises(AssertionError):
        m(dict(feat=torch.zeros(4, 8)))                                   # no condition
    with pytest.raises(AssertionError):
        m(dict(feat=torch.zeros(4, 8), condition="A"))                    # adaptive without context


def test_ppt_v1m2_builds_with_the_reference_keys(fx):
    from scenesplat_amd.pointcept_api import MODELS
    model = MODELS.build(ppt_cfg())
    sd = model.state_dict()
    assert list(sd.keys()) == fx["ppt_keys"].tolist()
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == fx["ppt_shapes"].tolist()
    assert tuple(sd["embedding_table.weight"].shape) == (3, 256)
    assert [tuple(sd[f"seg_heads.{i}.weight"].shape) for i in range(3)] == [(5, 48), (7, 48), (4, 48)]
    for other in ("SpUNet-v1m1", "PT-v3m2", "DefaultSegmentorV2"):
        cfg = ppt_cfg()
        cfg["backbone"] = dict(cfg["backbone"], type=other)
        with pytest.raises(AssertionError):
            MODELS.build(cfg)


def test_c_abi_declares_and_exports_the_pdnorm_entry_points():
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    header = open(build.HEADER).read()
    for s in ("ss_pdnorm_mod_fwd", "ss_pdnorm_mod_bwd", "ss_pdnorm_channels_per_workgroup"):
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(lib, s) and s in _lib.PROTOTYPES
    assert lib.ss_pdnorm_channels_per_workgroup() == 16


def test_steady_key_carries_the_condition():
    from scenesplat_amd.pointcept_api import MODELS
    ppt = MODELS.build(ppt_cfg())
    assert ppt.steady_key(dict(condition=["A"])) != ppt.steady_key(dict(condition=["B"]))
    assert ppt.steady_key(dict(condition=["B"])) == ppt.steady_key(dict(condition=["B"]))
    crit = [dict(type="CosineSimilarity", reduction="mean", loss_weight=1.0)]
    lang = MODELS.build(dict(type="LangPretrainer", backbone=backbone_cfg(adaptive=False), criteria=crit))
    seg = MODELS.build(dict(type="DefaultSegmentorV2", num_classes=5, backbone_out_channels=48, backbone=backbone_cfg(adaptive=False),
                            criteria=[dict(type="CrossEntropyLoss")]))
    for m in (lang, seg):
        a, b = m.steady_key(dict(condition=["A"], epoch_progress=0.1)), m.steady_key(dict(condition="C", epoch_progress=0.1))
        assert a != b and a == m.steady_key(dict(condition="A", epoch_progress=0.1))
    # a backbone without PDNorm layers keeps the key it had
    plain = MODELS.build(dict(type="LangPretrainer", backbone=dict(type="PT-v3m1", **TINY), criteria=crit))
    assert plain.steady_key(dict(condition=["A"], epoch_progress=0.1)) == plain.steady_key(dict(condition=["B"], epoch_progress=0.1)) == (None,)


def test_build_optimizer_keyword_groups():
    from scenesplat_amd.pointcept_api import MODELS, engine
    model = MODELS.build(ppt_cfg())
    opt = engine.build_optimizer(dict(type="AdamW", lr=1e-3, weight_decay=0.05), model, param_dicts=[dict(keyword="block", lr=1e-4)])
    names = dict(model.named_parameters())
    low = {id(p) for p in opt.param_groups[1]["params"]}
    rest = {id(p) for p in opt.param_groups[0]["params"]}
    assert opt.param_groups[1]["lr"] == 1e-4 and opt.param_groups[0]["lr"] == 1e-3
    assert id(names["backbone.enc.enc0.block0.norm1.0.modulation.1.weight"]) in low
    assert id(names["embedding_table.weight"]) in rest
    assert id(names["backbone.embedding.stem.norm.modulation.1.weight"]) in rest       # a modulation outside any block
    assert len(low) + len(rest) == len(names) and not (low & rest)
