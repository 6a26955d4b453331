"""GPU: the bf16 copies kept beside the fp32 parameters (functional.register_shadows / register_transposed / register_mirrored):
the tap-mirrored conv copy bit for bit, one refresh keeping all copies of a parameter together, and the model's copy plan
(PointTransformerV3._copy_plan) following the execution knobs on a live model."""
import pytest
import torch

from test_hip_block_tail import _tiny, _tiny_data

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _mirror_ref(w):
    cout, cin = w.shape[0], w.shape[-1]
    return w.detach().to(BF).reshape(cout, 27, cin).flip(1).permute(2, 1, 0).contiguous()


@pytest.mark.parametrize("cout,cin", [(8, 8), (16, 8)])
def test_mirrored_copy_is_bit_exact_and_follows_the_parameter(cout, cin):
    from scenesplat_amd import functional as SF
    w = torch.nn.Parameter(torch.randn(cout, 3, 3, 3, cin, generator=torch.Generator().manual_seed(cout)).cuda())
    src, dst = SF.register_shadows([w])
    SF.register_mirrored([w])
    assert SF.mirrored_of(w) is None                           # allocated, never written
    SF.refresh_shadows(src, dst)
    assert SF.mirrored_of(w).shape == (cin, 27, cout) and torch.equal(SF.mirrored_of(w), _mirror_ref(w))
    with torch.no_grad():
        w.add_(1)
    assert SF.mirrored_of(w) is None                           # stale: the conv dgrad mirrors on the fly
    SF.refresh_shadows(src, dst)
    assert torch.equal(SF.mirrored_of(w), _mirror_ref(w))


def test_a_width_that_needs_padding_keeps_no_mirrored_copy():
    from scenesplat_amd import functional as SF
    w = torch.nn.Parameter(torch.randn(8, 3, 3, 3, 6).cuda())
    src, dst = SF.register_shadows([w])
    SF.register_mirrored([w])
    SF.refresh_shadows(src, dst)
    assert SF.bf16_of(w) is dst[0] and SF.mirrored_of(w) is None


def test_one_refresh_keeps_all_copies_of_an_entry_together():
    from scenesplat_amd import functional as SF
    lin = torch.nn.Linear(48, 80).cuda()
    src, dst = SF.register_shadows([lin.weight, lin.bias])
    SF.register_transposed([lin.weight])
    SF.refresh_shadows(src, dst)
    assert SF.bf16_of(lin.weight) is dst[0] and SF.bf16_t_of(lin.weight) is not None
    with torch.no_grad():
        lin.weight.add_(1)
    fresh = SF.bf16_of(lin.weight)
    assert fresh is not dst[0] and torch.equal(fresh, lin.weight.detach().to(BF)) and SF.bf16_t_of(lin.weight) is None
    SF.refresh_shadows(src, dst)
    assert SF.bf16_of(lin.weight) is dst[0] and torch.equal(dst[0], lin.weight.detach().to(BF))
    assert torch.equal(SF.bf16_t_of(lin.weight), lin.weight.detach().to(BF).t().contiguous())


def _step(model, data):
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF):
        out = model(dict(data)).feat
    out.float().square().sum().backward()
    bad = [k for k, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not bad, bad


def _copies(model):
    from scenesplat_amd import functional as SF
    named = list(model.named_parameters())
    return ({k for k, p in named if SF.bf16_t_of(p) is not None}, {k for k, p in named if SF.mirrored_of(p) is not None})


@pytest.mark.parametrize("width", [dict(enc_channels=(128, 128), enc_num_head=(8, 8)), dict()], ids=["c128", "c64"])
@pytest.mark.parametrize("knob,before,after", [("dgrad_nt", True, False), ("dgrad_nt", False, True),
                                               ("conv_dtype", BF, "bf16x3"), ("conv_split_max_channels", 0, 256)])
def test_knob_changes_re_plan_the_copies_of_a_live_model(width, knob, before, after):
    """A model that has run under one setting and then runs under another keeps exactly the transposed and mirrored copies of a
    model built afresh from the same state dict and run once under the new setting.  (Registry state, not outputs: the small
    levels' conv accumulates with atomics.)"""
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import RUNTIME
    data = _tiny_data()
    old = dict(RUNTIME)
    try:
        RUNTIME.update(attn_impl=nv.ATTN_MFMA, conv_dtype=BF, conv_split_max_channels=0)
        RUNTIME[knob] = before
        live = _tiny(**width)
        _step(live, data)
        RUNTIME[knob] = after
        _step(live, data)
        fresh = _tiny(**width)
        fresh.load_state_dict(live.state_dict())
        _step(fresh, data)
        assert _copies(live) == _copies(fresh)
    finally:
        RUNTIME.clear(); RUNTIME.update(old)
