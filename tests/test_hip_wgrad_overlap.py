"""The capped, persistent form of the grouped nn.Linear weight-gradient launch (csrc/wgrad8.hip: k_wgrad8_group_capped) and the
deferred launch of the full-resolution decoder stages' weight gradients beside the coarse levels' backward
(functional.py: WGRAD_OVERLAP)."""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_round2 import TINY, _Runtime, _tiny_input, _tiny_lang

# (m, k_in, n_out): one K-tile; ten K-tiles; 32 K-tiles with a partial last one; ragged in all three dimensions (two tiles each
# way, a partial K-tile)
SHAPES = [(257, 264, 520), (64, 8, 8), (2047, 64, 192), (640, 8, 16), (2047, 64, 192)]
FLOOR = 8          # K-tiles of 64 rows per share (wgrad8.hip)
GROUPS = [SHAPES[:n] for n in range(1, 6)]


def _plan(shapes, cap):
    """-> (descriptor rows with words 5..7 filled by the capped planner, items per problem)"""
    from scenesplat_amd import native as nv
    lib = nv.lib()
    tiles = sum(lib.ss_linear_wgrad_tiles(k, n) for _, k, n in shapes)
    desc = np.zeros((len(shapes), 8), dtype=np.int64)
    counts = []
    for j, (m, k, n) in enumerate(shapes):
        counts.append(lib.ss_linear_wgrad_group_plan_capped(m, k, n, tiles, cap, ctypes.c_void_p(desc[j].ctypes.data)))
        assert counts[-1] > 0, (m, k, n, cap)
    return desc, counts


def _caps(shapes):
    """1, 2, items - 1, items, items + 7 with items = the item count of a launch planned for a cap that does not bind"""
    items = sum(_plan(shapes, 4096)[1])
    return sorted({1, 2, max(1, items - 1), items, items + 7})


def _problems(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i, (m, k, n) in enumerate(shapes):
        x = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(m, n, device="cuda", generator=g).to(torch.bfloat16)
        out.append((x, dy, i % 2 == 0))                         # bias on every second problem
    return out


def _zeros(probs):
    return [(x, dy, torch.zeros(dy.shape[1], x.shape[1], device="cuda"), torch.zeros(dy.shape[1], device="cuda") if b else None)
            for x, dy, b in probs]


def _launch_capped(items, plan_cap, launch_cap):
    """The capped entry point on a plan made for plan_cap workgroups, launched on launch_cap."""
    from scenesplat_amd import grouped
    desc, counts = _plan([(x.shape[0], x.shape[1], dy.shape[1]) for x, dy, _, _ in items], plan_cap)
    for j, (x, dy, dw, db) in enumerate(items):
        desc[j, :5] = (x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else 0, x.shape[0])
    grouped.launch("ss_linear_wgrad_group_capped", desc, grouped.starts(counts), items[0][0].device, int(launch_cap))
    return sum(counts)


@pytest.fixture(scope="module")
def problems():
    """The operands and fp32 products of the largest group, made once (the smaller groups are its prefixes)."""
    probs = _problems(SHAPES, 3)
    refs = [(dy.float().t() @ x.float(), dy.float().sum(0)) for x, dy, _ in probs]
    return probs, refs


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [1, 2, 3, 4, 5])
def test_capped_group_matches_fp32_product(problems, nprob):
    """ss_linear_wgrad_group_capped against the fp32 product, bars of test_linear_wgrad_group_matches_fp32_reference, for every
    cap; and a plan of MANY short shares walked by one and by two workgroups (stale accumulators, LDS re-staged under a reader
    and an unbalanced wave-row stagger show up there)."""
    from scenesplat_amd import native as nv
    probs, refs = problems
    probs, refs = probs[:nprob], refs[:nprob]
    runs = [("wrapper", cap, cap) for cap in _caps(GROUPS[nprob - 1])] + [("shares", 4096, 1), ("shares", 4096, 2)]
    for form, plan_cap, cap in runs:
        items = _zeros(probs)
        if form == "wrapper":
            nv.linear_wgrad_group(items, max_workgroups=cap)
        else:
            _launch_capped(items, plan_cap, cap)
        torch.cuda.synchronize()
        for (x, dy, dw, db), (rw, rb) in zip(items, refs):
            ew = float((dw - rw).norm() / rw.norm())
            eb = float((db - rb).norm() / rb.norm()) if db is not None else 0.0
            print(f"nprob {nprob} {form} cap {cap}: {tuple(x.shape)} x {dy.shape[1]}: dw {ew:.2e} db {eb:.2e}")
            assert (dw - rw).norm() <= 1e-5 * rw.norm(), (form, cap, x.shape, dy.shape, ew)
            if db is not None:
                assert (db - rb).norm() <= 1e-5 * rb.norm(), (form, cap, x.shape, dy.shape, eb)


@pytest.mark.gpu
def test_capped_group_with_a_cap_that_does_not_bind_equals_the_plain_group():
    """Every problem one share (m <= 512), as many workgroups as items: every element of dW / db is ONE atomic add onto zero in
    both launches -- bit-equal."""
    from scenesplat_amd import native as nv
    shapes = [(257, 264, 520), (64, 8, 8), (512, 64, 192), (384, 8, 16), (129, 520, 264)]
    probs = _problems(shapes, 5)
    desc, counts = _plan(shapes, 4096)
    assert all((int(w) & 0xffffffff) == 1 for w in desc[:, 7])                  # one share each
    for cap in (sum(counts), sum(counts) + 7, 4096):
        a, b = _zeros(probs), _zeros(probs)
        nv.linear_wgrad_group(a)
        nv.linear_wgrad_group(b, max_workgroups=cap)
        torch.cuda.synchronize()
        for (_, _, dw0, db0), (_, _, dw1, db1) in zip(a, b):
            assert torch.equal(dw0, dw1)
            assert (db0 is None) == (db1 is None) and (db0 is None or torch.equal(db0, db1))


@pytest.mark.parametrize("nprob", [1, 2, 3, 4, 5])
def test_capped_plan_covers_k_once_with_even_shares(nprob):
    """The descriptor words of ss_linear_wgrad_group_plan_capped alone (no launch): the shares of every tile cover the K-tiles
    0 .. ceil(m / 64) exactly once, as the kernel reads them; no share is below the floor unless the problem is; the items a
    workgroup gets differ by at most one.  Also at the caps of a real launch (224 of 256 CUs) with large m."""
    groups = [(GROUPS[nprob - 1], cap) for cap in _caps(GROUPS[nprob - 1]) + [224]]
    if nprob == 5:
        groups += [([(102400, 64, 192), (102400, 256, 64), (25600, 128, 384), (25600, 512, 128), (6401, 8, 8)], cap) for cap in (1, 208, 224, 240)]
    for shapes, cap in groups:
        desc, counts = _plan(shapes, cap)
        for (m, k, n), row, cnt in zip(shapes, desc, counts):
            w5, w6, w7 = (int(w) & 0xffffffffffffffff for w in row[5:8])
            assert (w5 & 0xffffffff, w5 >> 32) == (k, n)
            ntn, ntiles = w6 & 0xffffffff, w6 >> 32
            assert ntn == -(-k // 256) and ntiles == ntn * -(-n // 256)
            nshares, min_per = w7 & 0xffffffff, w7 >> 32
            assert cnt == nshares * ntiles
            nblocks = -(-m // 64)
            per = max(-(-nblocks // nshares), min_per)                          # w8_body
            spans = [(s * per, min(nblocks, s * per + per)) for s in range(nshares)]
            assert spans[0][0] == 0 and spans[-1][1] == nblocks, (shapes, cap, spans)
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (shapes, cap, spans)
            assert all(e - b >= min(FLOOR, nblocks) for b, e in spans), (shapes, cap, spans)
        total = sum(counts)
        grid = min(total, cap)
        per_wg = [len(range(b, total, grid)) for b in range(grid)]
        assert max(per_wg) - min(per_wg) <= 1
        assert total <= max(4 * cap, sum(int(w) >> 32 for w in desc[:, 6]))     # at most four rounds (or one share per tile)


def _lang_step(model, d):
    from scenesplat_amd import native as nv
    with _Runtime(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA):
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(dict(d))
        out["loss"].backward()
    return out


def _level_rows(model, d):
    plan = model.backbone.prepare_plan(d)
    return [lv.n for lv in plan.levels]


@pytest.mark.gpu
def test_model_gradients_with_the_overlap_equal_those_without(monkeypatch):
    """Tiny LangPretrainer, the threshold lowered so that dec0 and dec1 defer: forward bit-equal, every parameter gradient within the
    bar of test_grouped_stage_wgrads_equal_per_layer_launches, nothing left deferred; a second backward into EXISTING gradients
    accumulates (and does not defer); with a backward cut nothing defers."""
    from scenesplat_amd import functional as SF
    d = _tiny_input(40, 2)
    rows = _level_rows(_tiny_lang(), d)
    assert rows[0] > rows[1] > rows[2]
    print("rows per level:", rows)
    monkeypatch.setattr(SF, "WGRAD_DEFER_MIN_ROWS", rows[1])        # levels 0 and 1 are "large", level 2 is the coarse chain
    monkeypatch.setattr(SF, "LINEAR_WGRAD_MIN_ROWS", 64)            # every level of the tiny model queues its weight gradients
    monkeypatch.setattr(SF, "WGRAD_OVERLAP_FREE_CUS", 32)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(SF, "WGRAD_OVERLAP", on)
        stats = dict(SF.OVERLAP_STATS)
        model = _tiny_lang().train()
        out = _lang_step(model, d)
        torch.cuda.synchronize()
        took = {k: SF.OVERLAP_STATS[k] - stats[k] for k in stats}
        assert took == (dict(deferred=2, launched=1, joined=1) if on else dict(deferred=0, launched=0, joined=0)), took
        assert not SF._OVERLAP["items"] and not SF._OVERLAP["held"] and not SF._OVERLAP["pairs"] and SF._OVERLAP["flight"] is None
        res[on] = (out["loss"].detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
        if on:
            stats = dict(SF.OVERLAP_STATS)
            _lang_step(model, d)                                    # .grad exists now: autograd reads what it is handed, nothing defers
            torch.cuda.synchronize()
            assert SF.OVERLAP_STATS == stats
            twice = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert torch.equal(res[True][0], res[False][0])
    for k, b in res[False][1].items():
        a = res[True][1][k]
        err = float((a - b).norm() / b.norm().clamp_min(1e-30))
        print(f"overlap on / off {k}: {err:.2e}")
        assert a.dtype == b.dtype and (a - b).norm() <= 2e-3 * b.norm() + 1e-7, (k, err)
        assert (twice[k] - 2 * b).norm() <= 2e-3 * (2 * b).norm() + 2e-7, (k, float((twice[k] - 2 * b).norm() / (2 * b).norm()))
    # a backward cut: dec0's gradients must be final when the backward leaves dec0 -- nothing defers
    monkeypatch.setattr(SF, "WGRAD_OVERLAP", True)
    stats = dict(SF.OVERLAP_STATS)
    model = _tiny_lang().train()
    from scenesplat_amd import native as nv
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
    assert SF.OVERLAP_STATS == stats
    for k, p in model.named_parameters():
        b = res[False][1][k]
        assert (p.grad - b).norm() <= 2e-3 * b.norm() + 1e-7, k


@pytest.mark.gpu
def test_overlap_inside_a_captured_step(monkeypatch):
    """The tiny backbone through SteadyStateStep with dec0 and dec1 deferring: the capture (two parallel branches) ends cleanly,
    two replays give the eager step's gradients, and a step that raises in its forward leaves nothing deferred."""
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    from scenesplat_amd.pointcept_api import MODELS
    from scenesplat_amd.steady_state import SteadyStateStep
    d = _tiny_input(40, 2)
    with _Runtime(conv_dtype=torch.bfloat16, attn_impl=nv.ATTN_MFMA):
        torch.manual_seed(11)
        model = MODELS.build(dict(type="PT-v3m1", **TINY, drop_path=0.0, shuffle_orders=False)).cuda().train()
        perms = model.draw_perms()
        rows = [lv.n for lv in model.prepare_plan(d, perms=perms).levels]
        print("rows per level:", rows)
        monkeypatch.setattr(SF, "WGRAD_DEFER_MIN_ROWS", rows[1])
        monkeypatch.setattr(SF, "LINEAR_WGRAD_MIN_ROWS", 64)
        monkeypatch.setattr(SF, "WGRAD_OVERLAP", True)
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
        model.zero_grad(set_to_none=True)
        stats = dict(SF.OVERLAP_STATS)
        fn(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
        assert {k: SF.OVERLAP_STATS[k] - stats[k] for k in stats} == dict(deferred=2, launched=1, joined=1)
        ref = grads()
        steady = SteadyStateStep(fn, params, warmup=0)
        for it in range(4):                                       # sync-checked eager step, capture + replay, two more replays
            model.zero_grad(set_to_none=True)
            steady(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
            assert steady.refused is None and steady.poisoned is None, steady.refused
            assert SF._OVERLAP["flight"] is None and not SF._OVERLAP["items"] and not SF._OVERLAP["held"]
            got = grads()
            for k, b in ref.items():
                err = float((got[k] - b).norm() / b.norm().clamp_min(1e-30))
                print(f"step {it} (replays so far {steady.replays}) {k}: {err:.2e}")
                assert (got[k] - b).norm() <= 2e-3 * b.norm() + 1e-7, (it, k, err)
        assert steady.replays == 3 and steady.eager_steps == 1
        assert nv.stream_capture_status() == 0
        # a forward that raises: the caller resets the state, nothing stays deferred or armed
        boom.append(1)
        with pytest.raises(RuntimeError, match="injected"):
            fn(model.prepare_plan(d, perms=perms), dict(feat=d["feat"]))
        SF.reset_state()
        assert not SF._OVERLAP["items"] and not SF._OVERLAP["held"] and not SF._OVERLAP["stages"] and not SF._OVERLAP["armed"]
