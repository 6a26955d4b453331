"""CPU: the relative-position-encoding mode of PT-v3m1 (enable_rpe=True, enable_flash=False) -- construction, state-dict
contract and the discriminating power of the fixture tests/golden/attention_rpe*.npz (make_golden_rpe.py)."""
import glob
import os

import numpy as np
import pytest
import torch

MODULE_CASES = ("r_h2d16", "r_h2d48", "r_short")


def load_rpe_fixture(golden_dir):
    """attention_rpe.npz and its continuation files (one key space, split to keep every file below 1 MiB)"""
    fx = {}
    for fn in sorted(glob.glob(os.path.join(golden_dir, "attention_rpe*.npz"))):
        with np.load(fn) as z:
            fx.update({k: z[k] for k in z.files})
    return fx


def tiny_rpe_cfg(fx):
    cfg = {}
    for k, v in fx.items():
        if k.startswith("tiny_cfg_"):
            cfg[k[9:]] = tuple(v.tolist()) if v.ndim else v.item()
    return cfg


def test_tiny_config_with_rpe_has_the_reference_state_dict(golden_dir):
    from scenesplat_amd.pointcept_api import MODELS
    fx = load_rpe_fixture(golden_dir)
    model = MODELS.build(dict(type="PT-v3m1", **tiny_rpe_cfg(fx), drop_path=0.0, shuffle_orders=False, enable_rpe=True,
                              enable_flash=False))
    sd = model.state_dict()
    keys = [str(k) for k in fx["tiny_keys"]]
    assert list(sd.keys()) == keys and len(keys) == 181
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in fx["tiny_shapes"]]
    tables = [k for k in keys if k.endswith("attn.rpe.rpe_table")]
    assert [tuple(sd[k].shape) for k in tables] == [(75, 1), (75, 2), (45, 4), (45, 4), (75, 2), (75, 1), (75, 1)]
    assert tuple(sd["enc.enc2.block1.attn.rpe.rpe_table"].shape) == (45, 4)
    assert all(sd[k].dtype == torch.float32 and 0 < sd[k].abs().max() < 0.2 for k in tables)   # trunc_normal_(std=0.02): nonzero and small
    assert all(isinstance(p, torch.nn.Parameter) for n, p in model.named_parameters() if n.endswith("rpe_table"))


def test_rpe_with_flash_is_refused():
    from scenesplat_amd.pointcept_api import MODELS
    from scenesplat_amd.pointcept_api.ptv3 import SerializedAttention
    with pytest.raises(AssertionError, match="enable_rpe"):
        SerializedAttention(32, 2, 64, enable_rpe=True, enable_flash=True)
    with pytest.raises(AssertionError, match="enable_rpe"):
        MODELS.build(dict(type="PT-v3m1", enable_rpe=True))        # enable_flash defaults to True, as in the reference
    att = SerializedAttention(32, 2, 64, enable_rpe=False, enable_flash=False)
    assert att.rpe is None and "rpe.rpe_table" not in att.state_dict()


@pytest.mark.parametrize("patch,pos_bnd", [(16, 7), (48, 11), (64, 12), (128, 15), (256, 20), (1024, 31), (2048, 40)])
def test_pos_bnd_is_the_reference_expression(patch, pos_bnd):
    from scenesplat_amd.pointcept_api.ptv3 import RPE
    r = RPE(patch, 3)
    assert r.pos_bnd == pos_bnd and r.rpe_num == 2 * pos_bnd + 1
    assert tuple(r.rpe_table.shape) == (3 * r.rpe_num, 3) and r.rpe_table.dtype == torch.float32


def test_rpe_window_size_follows_the_smallest_batch_element():
    from scenesplat_amd.pointcept_api.ptv3 import SerializedAttention

    class Lv:
        def __init__(self, counts):
            self.counts = counts

    att = SerializedAttention(32, 2, 64, enable_rpe=True, enable_flash=False)
    assert att.rpe_window_size(Lv([300, 576])) == 64
    assert att.rpe_window_size(Lv([40, 170])) == 40
    assert att.rpe_window_size(Lv([700, 64])) == 64
    with pytest.raises(ValueError):
        att.rpe_window_size(Lv([0, 10]))


@pytest.mark.parametrize("name", MODULE_CASES)
def test_fixture_discriminates_a_missing_bias(golden_dir, name):
    """the output with the table differs from the output with a zero table by 10 bf16 tolerances: a kernel that drops the bias
    cannot pass the module cases"""
    fx = load_rpe_fixture(golden_dir)
    y, y0 = fx[f"{name}_y"], fx[f"{name}_y_zero"]
    gap = float(np.abs(y - y0).max())
    print(name, "gap", gap)
    assert gap >= 10 * 3e-2 * max(1.0, float(np.abs(y).max()))
    assert int(fx[f"{name}_K"]) == {"r_h2d16": 64, "r_h2d48": 128, "r_short": 40}[name]
    assert f"{name}_grad_rpe.rpe_table" in fx and f"{name}_sd_rpe.rpe_table" in fx
