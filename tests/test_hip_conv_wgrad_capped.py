"""The capped, persistent form of the gathered weight-gradient kernel (csrc/wgrad8.hip: k_wgrad8_conv_capped, items handed out by a
ticket) and the deferred launch of the deferring stages' SubMConv3d weight gradients on the side stream (functional.py:
CONV_WGRAD_OVERLAP)."""
import pytest
import torch

from test_hip_round2 import CRIT, TINY, _Runtime

TAPS = 27
CHANNELS = [(8, 8), (256, 256), (264, 520)]        # (cin, cout): one partial tile; one full tile; ragged, two tiles by three
LEVELS = ["n1", "n63", "n65", "isolated", "room"]
# seven stages of the benchmark in backward order, (name, rows, width)
BENCH_STAGES = [("dec0", 102400, 768), ("dec1", 25600, 512), ("dec2", 6400, 256), ("enc3", 1600, 256), ("enc2", 6400, 128),
                ("enc1", 25600, 64), ("enc0", 102400, 32)]
_CACHE = {}


def _line_rulebook(n):
    """n voxels on a line along x: tap (dx, dy, dz) of site i is i + dx where dy = dz = 0 and that site exists."""
    nbr = torch.full((TAPS, n), -1, dtype=torch.int32)
    i = torch.arange(n, dtype=torch.int32)
    for dx in (-1, 0, 1):
        t = (dx + 1) * 9 + 4
        j = i + dx
        nbr[t] = torch.where((j >= 0) & (j < n), j, torch.full_like(j, -1))
    return nbr


def _level(name):
    """-> (nbr (27, n) int32, rowperm (n) int32) on the device; cached, never written"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "room":
        from scenesplat_amd.plan import build_plan
        from scenesplat_amd.synthetic import room_chunk
        data = room_chunk(64, 0, lang_dim=0)
        lv = build_plan(data["grid_coord"].cuda(), data["offset"].cuda(), ("z", "z-trans", "hilbert", "hilbert-trans"), ()).levels[0]
        nbr, perm = lv.neighbors(3).contiguous(), lv.conv_rowperm().contiguous()
    else:
        if name == "isolated":                     # 200 sites without neighbours: only the centre tap has pairs
            n = 200
            nbr = torch.full((TAPS, n), -1, dtype=torch.int32)
            nbr[13] = torch.arange(n, dtype=torch.int32)
        else:
            nbr = _line_rulebook(int(name[1:]))
        g = torch.Generator().manual_seed(nbr.shape[1])
        perm = torch.randperm(nbr.shape[1], generator=g).to(torch.int32)
        nbr, perm = nbr.cuda().contiguous(), perm.cuda().contiguous()
    _CACHE[name] = (nbr, perm)
    return _CACHE[name]


def _definition(x, g, nbr):
    """dW (cout, taps, cin) in fp32: per tap, gather + matmul (test_full_level_conv_c768_values)"""
    xf, gf = x.float(), g.float()
    dw = torch.zeros(g.shape[1], TAPS, x.shape[1], device=x.device)
    for t in range(TAPS):
        j = nbr[t].long()
        rows = torch.nonzero(j >= 0).squeeze(1)
        if rows.numel():
            dw[:, t, :] = gf[rows].t() @ xf[j[rows]]
    return dw


def _forms(nbr, perm):
    """(label, rowperm | None, blocks, nbr_walk | None): the rulebook plain and in walk order, with and without a row permutation"""
    from scenesplat_amd import native as nv
    out = []
    for label, p in (("perm", perm), ("noperm", None)):
        blocks = nv.subm_block_lists(nbr, p)
        out.append((label, p, blocks, None))
        out.append((label + "+walk", p, blocks, nv.subm_walk_rulebook(nbr, p)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("level", LEVELS)
def test_capped_conv_wgrad_equals_the_definition_and_the_plain_launch(level, cin, cout):
    """Integer-valued operands (exact in bf16, sums below 2^24): every form, cap and share length gives the fp32 definition and the
    plain launch's result bit for bit, whatever order the tickets were drawn in, and so does a second launch right behind the first
    (a ticket counter that was not zeroed again would hand out no items).  Normal random operands: within 1e-4 of the definition."""
    from scenesplat_amd import native as nv
    lib = nv.lib()
    nbr, perm = _level(level)
    n = nbr.shape[1]
    g_ = torch.Generator(device="cuda").manual_seed(1000 * cin + n)
    x = torch.randint(-2, 3, (n, cin), device="cuda", generator=g_).to(torch.bfloat16)
    g = torch.randint(-2, 3, (n, cout), device="cuda", generator=g_).to(torch.bfloat16)
    xr = torch.randn(n, cin, device="cuda", generator=g_).to(torch.bfloat16)
    gr = torch.randn(n, cout, device="cuda", generator=g_).to(torch.bfloat16)
    ref, refr = _definition(x, g, nbr), _definition(xr, gr, nbr)
    assert float(ref.abs().max()) < 2 ** 24
    forms = _forms(nbr, perm)
    assert torch.equal(nv.subm_conv_wgrad_pipe(x, g, nbr, perm, forms[0][2]), ref)
    if level == "isolated":
        cnt = forms[0][2][0].cpu()
        assert int(cnt[13]) == (n + 63) // 64 and int(cnt.sum()) == int(cnt[13])       # 26 taps without an active block
    # share lengths: the plain launch's (8 K-tiles at these sizes); on the room level 8 stated outright (many short items per workgroup)
    # and 80 (one share of the centre tap crosses the 60-K-tile index chunk)
    pers = [8, 80] if level == "room" else [0]
    if level == "room":
        assert (n + 63) // 64 > 80 and int(forms[0][2][0].max()) > 60
    for min_per in pers:
        items = int(lib.ss_subm_conv_wgrad_pipe_items(n, cin, cout, TAPS, min_per))
        tiles = -(-cin // 256) * -(-cout // 256)
        assert items == TAPS * tiles * -(-((n + 63) // 64) // min(max(min_per, 8), (n + 63) // 64))
        caps = sorted({1, 2, max(1, items - 1), items, items + 7})
        for label, p, blocks, walk in forms:
            for cap in caps:
                for again in (0, 1):
                    dw = nv.subm_conv_wgrad_capped(x, g, nbr, p, blocks, nbr_walk=walk, max_workgroups=cap, min_per=min_per)
                    assert torch.equal(dw, ref), (label, cap, min_per, again, float((dw - ref).abs().max()))
            for cap in (2, items):
                out = torch.zeros(cout, TAPS, cin, device="cuda")
                dw = nv.subm_conv_wgrad_capped(xr, gr, nbr, p, blocks, out=out, nbr_walk=walk, max_workgroups=cap, min_per=min_per)
                assert dw.data_ptr() == out.data_ptr()
                err = float((dw - refr).norm() / refr.norm().clamp_min(1e-30))
                assert err <= 1e-4, (label, cap, min_per, err)


@pytest.mark.gpu
def test_capped_conv_wgrad_refuses_bad_arguments():
    from scenesplat_amd import native as nv
    from scenesplat_amd._lib import NativeError
    nbr, perm = _level("n65")
    n = nbr.shape[1]
    x = torch.zeros(n, 8, device="cuda", dtype=torch.bfloat16)
    blocks = nv.subm_block_lists(nbr, perm)
    with pytest.raises(NativeError):
        nv.subm_conv_wgrad_capped(x, x, nbr, perm, blocks, max_workgroups=0)
    with pytest.raises(NativeError):
        nv.subm_conv_wgrad_capped(x, x, nbr, perm, blocks, max_workgroups=4, min_per=-1)
    assert nv.lib().ss_subm_conv_wgrad_pipe_items(n, 12, 8, TAPS, 0) == 0         # cin no multiple of 8: not eligible


# ---- the model's step ---------------------------------------------------------------------------------------------------------
# TINY with decoder widths of 128: the cpe convs of dec0 and dec1 (128 -> 128) run the pipeline weight gradient
WIDE = dict(TINY, enc_channels=(32, 64, 128), enc_num_head=(2, 4, 8), dec_channels=(128, 128), dec_num_head=(8, 8))
BAR = 2e-3           # test_model_gradients_with_the_overlap_equal_those_without: |a - b| <= 2e-3 |b| + 1e-7


def _wide_lang():
    from scenesplat_amd.pointcept_api import MODELS
    torch.manual_seed(5)
    return MODELS.build(dict(type="LangPretrainer", backbone=dict(type="PT-v3m1", **WIDE, drop_path=0.0, shuffle_orders=False),
                             criteria=CRIT)).cuda()


def _wide_input():
    from scenesplat_amd.synthetic import room_chunk
    d = {k: v.cuda() for k, v in room_chunk(n_side=40, seed=2, lang_dim=128, num_classes=4).items()}
    d["epoch_progress"] = 0.6
    return d


def _lang_step(model, d, **extra):
    from scenesplat_amd import native as nv
    with _Runtime(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA):
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(dict(d, **extra))
        out["loss"].backward()
    return out


def _lower_thresholds(monkeypatch, SF, rows):
    assert rows[0] > rows[1] > rows[2]
    monkeypatch.setattr(SF, "WGRAD_DEFER_MIN_ROWS", rows[1])        # levels 0 and 1 are "large", level 2 is the coarse chain
    monkeypatch.setattr(SF, "LINEAR_WGRAD_MIN_ROWS", 64)
    monkeypatch.setattr(SF, "CONV_IM2COL_MAX_SITES", rows[2])       # levels 0 and 1 run the implicit-GEMM conv, not the im2col form
    # ... and run it in ONE pass: at these sizes the dispatcher takes the split-K form, whose fp32 atomics make the forward differ from
    # run to run, and "bit-equal with the overlap on and off" would say nothing.  Wide convs: the pipeline kernel; the narrow ones of
    # the stem and the encoder, which it does not take: neighbour rows side by side and one matmul (the im2col form's arithmetic).
    from scenesplat_amd import native as nv

    def one_pass(x, w, bias, nbr, rowperm, out_dtype=torch.bfloat16, nbr_walk=None):
        (n, cin), (cout, taps) = x.shape, w.shape[:2]
        if nv.lib().ss_gemm8_ok(n, cin, cout, taps):
            return nv.subm_conv_fwd_pipe(x, w, bias, nbr, rowperm, out_dtype)
        out = nv.subm_im2col(x, nbr).float() @ w.reshape(cout, -1).float().t()
        return (out if bias is None else out + bias).to(out_dtype)
    monkeypatch.setattr(nv, "subm_conv_fwd", one_pass)
    monkeypatch.setattr(SF, "WGRAD_OVERLAP_FREE_CUS", 32)
    monkeypatch.setattr(SF, "WGRAD_OVERLAP", True)


def _nothing_queued(SF):
    o = SF._OVERLAP
    return not o["items"] and not o["convs"] and not o["held"] and not o["pairs"] and o["flight"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("join", ["end", "large"])
def test_model_gradients_with_the_conv_overlap_equal_those_without(monkeypatch, join):
    """dec0 and dec1 defer: their two cpe convs queue their weight gradients and run capped on the side stream.  Forward bit-equal,
    every parameter gradient within the bar of the Linear overlap's test, nothing left queued; a second backward into EXISTING
    gradients accumulates and does not defer; with a backward cut nothing defers; the Linear overlap's counters read what its own
    test expects."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    d = _wide_input()
    rows = [lv.n for lv in _wide_lang().backbone.prepare_plan(d).levels]
    print("rows per level:", rows)
    assert nv.lib().ss_subm_conv_wgrad_uses_pipe(rows[1], 128, 128, TAPS) == 1
    _lower_thresholds(monkeypatch, SF, rows)
    monkeypatch.setattr(SF, "WGRAD_OVERLAP_JOIN", join)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(SF, "CONV_WGRAD_OVERLAP", on)
        stats, cstats = dict(SF.OVERLAP_STATS), dict(SF.CONV_OVERLAP_STATS)
        model = _wide_lang().train()
        out = _lang_step(model, d)
        torch.cuda.synchronize()
        assert {k: SF.OVERLAP_STATS[k] - stats[k] for k in stats} == dict(deferred=2, launched=1, joined=1)
        took = {k: SF.CONV_OVERLAP_STATS[k] - cstats[k] for k in cstats}
        assert took == (dict(deferred=2, capped=2, inline=0) if on else dict(deferred=0, capped=0, inline=0)), took
        assert _nothing_queued(SF)
        res[on] = (out["loss"].detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
        if on:
            stats, cstats = dict(SF.OVERLAP_STATS), dict(SF.CONV_OVERLAP_STATS)
            _lang_step(model, d)                                    # .grad exists now: nothing defers
            torch.cuda.synchronize()
            assert SF.OVERLAP_STATS == stats and SF.CONV_OVERLAP_STATS == cstats and _nothing_queued(SF)
            twice = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert torch.equal(res[True][0], res[False][0])
    for k, b in res[False][1].items():
        a = res[True][1][k]
        err = float((a - b).norm() / b.norm().clamp_min(1e-30))
        print(f"conv overlap on / off {k}: {err:.2e}")
        assert a.dtype == b.dtype and (a - b).norm() <= BAR * b.norm() + 1e-7, (k, err)
        assert (twice[k] - 2 * b).norm() <= BAR * (2 * b).norm() + 2e-7, (k, float((twice[k] - 2 * b).norm() / (2 * b).norm()))
    # a backward cut: nothing defers
    monkeypatch.setattr(SF, "CONV_WGRAD_OVERLAP", True)
    stats, cstats = dict(SF.OVERLAP_STATS), dict(SF.CONV_OVERLAP_STATS)
    model = _wide_lang().train()
    from scenesplat_amd.pointcept_api.ptv3 import backward_tail
    cut = []
    with _Runtime(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA):
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(dict(d, backward_cut=cut))
        out["loss"].backward()
        assert len(cut) == 2
        backward_tail(cut)
    torch.cuda.synchronize()
    assert SF.OVERLAP_STATS == stats and SF.CONV_OVERLAP_STATS == cstats
    for k, p in model.named_parameters():
        b = res[False][1][k]
        assert (p.grad - b).norm() <= BAR * b.norm() + 1e-7, k


@pytest.mark.gpu
def test_conv_overlap_inside_a_captured_step(monkeypatch):
    """The wide tiny backbone through SteadyStateStep with dec0 and dec1 deferring Linears and convs: the capture ends cleanly, three
    replays give the eager step's gradients (the ticket counters are zeroed inside the step), and a forward that raises, followed by
    reset_state(), leaves nothing queued."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import MODELS
    from scenesplat_amd.steady_state import SteadyStateStep
    d = _wide_input()
    with _Runtime(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA):
        torch.manual_seed(11)
        model = MODELS.build(dict(type="PT-v3m1", **WIDE, drop_path=0.0, shuffle_orders=False)).cuda().train()
        perms = model.draw_perms()
        rows = [lv.n for lv in model.prepare_plan(d, perms=perms).levels]
        _lower_thresholds(monkeypatch, SF, rows)
        monkeypatch.setattr(SF, "CONV_WGRAD_OVERLAP", True)
        boom = []

        def fn(plan, t):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = model(dict(feat=t["feat"], grid_coord=d["grid_coord"], offset=d["offset"], plan=plan))
                if boom:
                    raise RuntimeError("injected failure in the forward")
            out.feat.float().square().mean().backward()
            return {"feat": out.feat}

        def grads():
            torch.cuda.synchronize()
            return {k: p.grad.clone() for k, p in model.named_parameters()}
        params = list(model.parameters())
        ref = {}
        for on in (False, True):                                  # eager: the conv overlap off, then on
            monkeypatch.setattr(SF, "CONV_WGRAD_OVERLAP", on)
            model.zero_grad(set_to_none=True)
            cstats = dict(SF.CONV_OVERLAP_STATS)
            fn(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
            assert SF.CONV_OVERLAP_STATS["capped"] - cstats["capped"] == (2 if on else 0)
            ref[on] = grads()
        for k, b in ref[False].items():
            assert (ref[True][k] - b).norm() <= BAR * b.norm() + 1e-7, k
        steady = SteadyStateStep(fn, params, warmup=0)
        for it in range(5):                                       # sync-checked eager step, capture + replay, three more replays
            model.zero_grad(set_to_none=True)
            steady(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
            assert steady.refused is None and steady.poisoned is None, steady.refused
            assert _nothing_queued(SF)
            got = grads()
            for k, b in ref[False].items():
                err = float((got[k] - b).norm() / b.norm().clamp_min(1e-30))
                assert (got[k] - b).norm() <= BAR * b.norm() + 1e-7, (it, k, err)
        assert steady.replays == 4 and steady.eager_steps == 1
        assert nv.stream_capture_status() == 0
        boom.append(1)
        with pytest.raises(RuntimeError, match="injected"):
            fn(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
        SF.reset_state()
        assert _nothing_queued(SF) and not SF._OVERLAP["stages"] and not SF._OVERLAP["armed"]


# ---- host only ------------------------------------------------------------------------------------------------------------------
def test_join_rule_on_the_benchmark_stages():
    """overlap_join_due on the benchmark's seven stages, backward order; dec0 and dec1 defer, the filler starts behind dec1.
    "large" joins at enc2's flush (enc1, 25,600 rows, comes next); "end" joins at no flush at all (the end of the backward does)."""
    from scenesplat_amd import functional as SF
    min_rows = 16384
    defers = {"dec0", "dec1"}
    joins = {"large": [], "end": []}
    for mode in joins:
        for i, (name, rows, _) in enumerate(BENCH_STAGES[2:], start=2):          # the stages that flush while the filler is in flight
            nxt = BENCH_STAGES[i + 1] if i + 1 < len(BENCH_STAGES) else None
            if SF.overlap_join_due(mode, rows, nxt[1] if nxt else None, name in defers, bool(nxt) and nxt[0] in defers, min_rows):
                joins[mode].append(name)
    assert joins["large"][0] == "enc2" and joins["end"] == []
    # a deferring stage that flushes with a filler in flight (a second decoder behind the first): both modes join
    assert SF.overlap_join_due("end", 102400, 6400, True, False, min_rows) and SF.overlap_join_due("large", 102400, 6400, True, False, min_rows)
    assert SF.overlap_join_due("end", 6400, 102400, False, True, min_rows)


def test_the_header_declares_the_capped_conv_entry():
    import ctypes
    from scenesplat_amd import _lib
    res, args = _lib.PROTOTYPES["ss_subm_conv_wgrad_pipe_capped"]
    assert res is ctypes.c_int and len(args) == 16 and args[7] is ctypes.c_void_p and args[8] is ctypes.c_int64
    assert _lib.PROTOTYPES["ss_subm_conv_wgrad_pipe_items"][0] is ctypes.c_int64
