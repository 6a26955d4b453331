"""GPU: the SimDINO pretraining model -- the mask generator, mask token and grouped EMA kernels (csrc/ssl_model.hip), the PT-v3m1-simdino
backbone, DefaultContrastiverSimDinoV2 and DefaultSSLPreTrainer -- against the reference's own outputs (tests/golden/ssl_model.npz) and,
at sizes without a golden, against the restatements of tests/ssl_model_cases.py (themselves checked against the goldens on the host).

MEASURED (MI355X, the maxima the tests print before asserting; also in profiles/ssl_model.md):
  mask generator         masks, row indices and fp16 weights bit-equal to golden (i) and to the restatement at every edge size
  mask token             forward / dx bit-equal; dtoken within L 2^-24 sum|g| at every size; two runs: same bits
  EMA                    worst error / bound (2^-22 max(|t|, |s|)): 0.47 (m = 0.9), 0.49 (m = 0.999), 0 (m = 1.0: bit-identical)
  backbone vs (ii)       cosine distance max 1.2e-7 (eval) / 2.4e-7 (train) at the encoder, 1.8e-7 at the decoder; abs max 4.7e-6 / 8.8e-6
                         (encoder), 8.3e-6 (decoder); gradient norms within 3.3e-6 relative
  whole model vs (iii)   scalars: |err| <= 1.4e-5 (loss -3.2002139 vs -3.2001996; the reference's own fp32 - fp64 gap is 1.7e-6), bounds
                         4.5e-4 .. 6.4e-3; gradients 7e-7 .. 3.5e-5 relative, dino_head.mlp.4.bias 5.4e-4 (bound 3e-3)
  teacher after update   worst error / bound 0.50
"""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssl_model_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssl_model.npz")))


def seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def get_state():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def set_state(st):
    random.setstate(st[0]); np.random.set_state(st[1]); torch.set_rng_state(st[2])


def tiny_model(**kw):
    from scenesplat_amd.pointcept_api import MODELS
    args = dict(type="DefaultContrastiverSimDinoV2", backbone_out_channels=64, local_crop_num=3, enable_mae_loss=True,
                backbone=dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA))
    args.update(kw)
    return MODELS.build(args)


def tiny_backbone():
    from scenesplat_amd.pointcept_api import MODELS
    bb = MODELS.build(dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA, do_mask=True))
    bb.load_state_dict(sc.backbone_state(31), strict=True)
    return bb.cuda()


# ---- mask generator ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def masker():
    return tiny_model()          # (the mask generator reads no parameter: the model stays on the host)


def run_masker(model, gc, offset, mtype, size, probability=0.5, ratio=sc.RATIO):
    model.mask_type, model.mask_grid_size = mtype, size
    model.mask_sample_probability, model.mask_ratio_min_max = probability, ratio
    mask, w, idx = model.mask_generator(torch.from_numpy(offset).cuda(), torch.from_numpy(gc).int().cuda(), return_index=True)
    assert mask.dtype == torch.bool and w.dtype == torch.float16 and idx.dtype == torch.int32
    mask, idx = mask.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(idx, np.nonzero(mask)[0])          # the ascending row index of the masked points
    return mask, w.cpu().numpy()


@pytest.mark.parametrize("mtype,size", sc.MASK_CASES)
def test_mask_generator_matches_the_reference(fx, masker, mtype, size):
    tag = "mask_%s_%s_" % (mtype, str(size).replace(".", "p"))
    seed(int(fx[tag + "seed"]))
    mask, w = run_masker(masker, fx["mask_gc"], fx["mask_offset"], mtype, size)
    assert np.array_equal(mask, fx[tag + "mask"])
    assert np.array_equal(w.view(np.uint16), fx[tag + "weights"].view(np.uint16))


def restated(gc, offset, mtype, size, probability, ratio):
    """the restatement on the draws the model is about to make (the generators are put back)"""
    st = get_state()
    ids, counts = sc.patch_ids(gc, offset, size)
    tokens = np.diff(np.concatenate([[0], offset]))
    draws = sc.draw_masks(offset, counts if mtype == "patch" else tokens, mtype, probability, ratio)
    set_state(st)
    return ids, counts, draws, sc.apply_draws(offset, ids, draws, mtype)


MASK_EDGES = {
    "one_point": dict(sizes=(1,), side=4, mtype="patch", size=0.2),                       # B = 1, n = 1: k = int(1 * rate) = 0
    "single_patch": dict(sizes=(40, 60), side=4, mtype="patch", size=100.0, probability=1.0),   # every sample is ONE patch: k = 0
    "k_zero": dict(sizes=(200, 300), side=8, mtype="patch", size=0.2, probability=1.0, ratio=(0.0, 0.001)),
    "none_flagged": dict(sizes=(100, 150, 90), side=8, mtype="patch", size=2.0, probability=0.0),
    "all_flagged": dict(sizes=(100, 150, 90), side=8, mtype="patch", size=2.0, probability=1.0),
    "all_flagged_splats": dict(sizes=(100, 1, 90), side=8, mtype="splats", size=0.2, probability=1.0),
    "many_blocks": dict(sizes=(30000, 1, 40000), side=42, mtype="patch", size=2.0, probability=1.0),      # n = 70,001
    "past_a_full_grid": dict(sizes=(131072, 131329), side=65, mtype="patch", size=3.0, probability=1.0),   # n = 262,401 > 1024 x 256
}


@pytest.mark.parametrize("name", sorted(MASK_EDGES))
def test_mask_generator_matches_the_restatement(masker, name):
    from scenesplat_amd import native as nv
    c = dict(MASK_EDGES[name])
    gc, offset = sc.mask_batch(c.pop("sizes"), c.pop("side"), seed=11)
    mtype, size = c.pop("mtype"), c.pop("size")
    probability, ratio = c.pop("probability", 0.5), c.pop("ratio", sc.RATIO)
    seed(123)
    ids, counts, draws, (want_mask, want_w) = restated(gc, offset, mtype, size, probability, ratio)
    mask, w = run_masker(masker, gc, offset, mtype, size, probability, ratio)
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(w.view(np.uint16), want_w.view(np.uint16))
    if name in ("one_point", "single_patch", "k_zero", "none_flagged"):
        assert not mask.any() and len(w) == 0
    if name.startswith("all_flagged") or name in ("many_blocks", "past_a_full_grid"):
        assert all(d[0] for d in draws) and mask.any()
    if mtype == "patch":
        pid, start, cnt = nv.mask_patches(torch.from_numpy(gc).int().cuda(), torch.from_numpy(offset).int().cuda(), size)
        assert np.array_equal(pid.cpu().numpy(), ids) and cnt.tolist() == counts.tolist() + [0]
        assert start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
        # every point of a patch carries the same mask value
        key = np.repeat(np.arange(len(offset)), np.diff(np.concatenate([[0], offset]))) * (ids.max() + 1) + ids
        per_patch = np.zeros(key.max() + 1, np.int64); np.add.at(per_patch, key, mask)
        sizes = np.bincount(key, minlength=key.max() + 1)
        assert ((per_patch == 0) | (per_patch == sizes)).all()


def test_mask_generator_refuses_cells_outside_the_key(masker):
    gc = np.array([[0, 0, 0], [30000, 0, 0]], np.int64)          # 30000 / 0.2 = 150000 >= 2^17
    with pytest.raises(RuntimeError, match="2\\^17"):
        run_masker(masker, gc, np.array([2], np.int64), "patch", 0.2, 1.0)


# ---- mask token -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 48])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_mask_token_forward_backward(n, C):
    from scenesplat_amd import functional as SF
    from scenesplat_amd import native as nv
    g_ = torch.Generator().manual_seed(n * 100 + C)
    x0 = torch.randn(n, C, generator=g_).cuda()
    cot = torch.randn(n, C, generator=g_).cuda()
    tok0 = (torch.randn(1, C, generator=g_) * 0.1).cuda()
    lib = nv.lib()
    # L: the longest chain of fp32 additions behind one dtoken[c], from the kernel as written (csrc/ssl_model.hip): a row slot adds every
    # R-th row of its workgroup's span in order (ceil(span / R) additions), a channel adds its R = 256 // C slots in order (R - 1), the
    # finish adds the nb workgroup partials in order (nb - 1).  A sum of L terms added one by one in fp32 is within
    # gamma_{L-1} sum|g| <= L 2^-24 sum|g| of the exact sum (Higham, Accuracy and Stability, eq. 4.4; L (L - 1) 2^-24 <= 1 here).
    R, nb, span = 256 // C, lib.ss_mask_token_bwd_blocks(n), lib.ss_mask_token_bwd_span(n)
    L = -(-span // R) + (R - 1) + (nb - 1)
    assert L * (L - 1) * 2.0 ** -24 <= 1
    masks = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "random": torch.rand(n, generator=g_) < 0.4}
    for name, mask in masks.items():
        mask = mask.cuda()
        x, tok = x0.clone().requires_grad_(True), tok0.clone().requires_grad_(True)
        out = SF.mask_token(x, mask, tok)
        assert torch.equal(out, torch.where(mask[:, None], tok0, x0)), name
        out.backward(cot)
        assert torch.equal(x.grad, torch.where(mask[:, None], torch.zeros_like(cot), cot)), name
        exact = (cot.double() * mask[:, None]).sum(0)
        bound = L * 2.0 ** -24 * (cot.double().abs() * mask[:, None]).sum(0)
        err = (tok.grad.double()[0] - exact).abs()
        assert tok.grad.shape == tok0.shape and (err <= bound).all(), (name, (err / bound.clamp_min(1e-300)).max().item())
        dx2, dt2 = nv.mask_token_bwd(cot, mask)
        assert torch.equal(dt2, tok.grad[0]) and torch.equal(dx2, x.grad), name          # two runs, the same bits
    xb = x0.to(torch.bfloat16)
    mask = masks["random"].cuda()
    assert torch.equal(nv.mask_token_fwd(xb, mask, tok0[0].contiguous()), torch.where(mask[:, None], tok0.to(torch.bfloat16), xb))


# ---- grouped EMA --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0.9, 0.999, 1.0])
def test_ema_group_matches_fp64(m):
    from scenesplat_amd import native as nv
    g_ = torch.Generator().manual_seed(3)
    sizes = (1, 255, 4097, 65537)
    base = torch.randn(4097 + 3, generator=g_).cuda()
    teacher = [torch.randn(k, generator=g_).cuda() for k in sizes]
    teacher[2] = base[1:4098]                        # a contiguous slice at an odd element offset: no 16-byte lanes
    assert teacher[2].data_ptr() % 16 != 0 and teacher[2].is_contiguous()
    student = [torch.randn(k, generator=g_).cuda() for k in sizes]
    before = [t.clone() for t in teacher]
    guard = base.clone()
    nv.ema_group(teacher, student, m)
    assert base[0] == guard[0] and torch.equal(base[4098:], guard[4098:])
    worst = 0.0
    for t, t0, s in zip(teacher, before, student):
        exact = m * t0.double() + (1.0 - m) * s.double()
        bound = 2.0 ** -22 * torch.maximum(t0.abs(), s.abs()).double()
        err = (t.double() - exact).abs()
        worst = max(worst, (err / bound).max().item())
        assert (err <= bound).all()
        if m == 1.0:
            assert torch.equal(t, t0)
    print("ema m=%s: worst error / bound %.3f" % (m, worst))


def test_update_teacher_pairs_and_version_bump():
    model = tiny_model()
    model.load_state_dict(sc.model_state(model), strict=True)
    model = model.cuda().eval()
    frozen = "enc.enc1.down.proj.weight"
    dict(model.backbone_student.named_parameters())[frozen].requires_grad = False
    t0 = {k: v.clone() for k, v in model.backbone_teacher.state_dict().items()}
    s0 = {k: v.clone() for k, v in model.backbone_student.state_dict().items()}
    v = {k: t.cuda() for k, t in sc.view((300, 421), 11, 12, 60).items()}
    perms = model.backbone_teacher.draw_perms()

    def teacher_forward(bb):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            enc, dec = bb(dict(v), return_dec=True, perms=perms)
        return enc.feat.float(), dec.feat.float()
    stale = teacher_forward(model.backbone_teacher)              # (writes the version-stamped bf16 shadows)
    model.update_teacher(0.5)
    t1 = model.backbone_teacher.state_dict()
    params = dict(model.backbone_teacher.named_parameters())
    for k in t1:
        if k == "mask_token" or k == frozen or k not in params:          # the token, a frozen parameter, the BatchNorm buffers
            assert torch.equal(t1[k], t0[k]), k
        else:
            exact = 0.5 * t0[k].double() + 0.5 * s0[k].double()
            assert ((t1[k].double() - exact).abs() <= 2.0 ** -22 * torch.maximum(t0[k].abs(), s0[k].abs()).double()).all(), k
            assert not torch.equal(t1[k], t0[k]), k
    assert all(torch.equal(a, b) for a, b in zip(model.backbone_student.state_dict().values(), s0.values()))
    got = teacher_forward(model.backbone_teacher)
    fresh = tiny_backbone()
    fresh.load_state_dict(t1, strict=True)
    want = teacher_forward(fresh.eval())
    # the same kernels on the same operands; the weights moved half-way to the student's, so stale shadows are off by O(1)
    for a, b, c in zip(got, want, stale):
        assert (a - b).abs().max() <= 1e-6 * b.abs().max(), (a - b).abs().max()
        assert (c - b).abs().max() > 1e-2 * b.abs().max()


# ---- backbone -----------------------------------------------------------------------------------------------------------------------------
def coarse_rows(plan, fx):
    """reference row of every row of our coarsest level, by (sample, grid_coord)"""
    ref = {(int(b), tuple(c)): i for i, (b, c) in enumerate(zip(fx["bb_enc_batch"].tolist(), fx["bb_enc_gc"].tolist()))}
    lv = plan.levels[-1]
    return torch.tensor([ref[(int(b), tuple(c))] for b, c in zip(lv.batch.tolist(), lv.grid_coord.tolist())])


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_backbone_matches_reference(fx, mode, dec):
    bb = tiny_backbone()
    bb.train(mode == "train")
    v = sc.view((300, 421), 11, 12, 60)
    feat = v["feat"].cuda().requires_grad_(True)
    given = torch.from_numpy(fx["bb_mask"]).cuda()
    torch.manual_seed(77)                      # the reference drew its pooling shuffles from this seed
    enc, pdec = bb(dict(coord=v["coord"].cuda(), grid_coord=v["grid_coord"].cuda(), feat=feat, offset=v["offset"].cuda()),
                   mask=given, return_dec=bool(dec))
    tag = "bb_%s_%d_" % (mode, dec)
    rows = coarse_rows(enc.plan, fx)
    assert sorted(rows.tolist()) == list(range(len(fx[tag + "enc"]))) and enc.offset.tolist() == fx[tag + "enc_offset"].tolist()
    built = [k for k in enc.plan.levels[0]._windows if k[0] != "layout"]
    assert (pdec is None) == (not dec) and len(built) == (2 if dec else 1)      # dec0's second block is the only user of curve 1 at level 0
    ref_enc = torch.from_numpy(fx[tag + "enc"])[rows]
    cot_e = torch.randn(fx[tag + "enc"].shape, generator=torch.Generator().manual_seed(5))[rows]
    loss = (enc.feat * cot_e.cuda()).sum()
    pairs = [("enc", enc.feat.detach().cpu(), ref_enc)]
    if dec:
        cot_d = torch.randn(fx[tag + "dec"].shape, generator=torch.Generator().manual_seed(6))
        loss = loss + (pdec.feat * cot_d.cuda()).sum()
        pairs.append(("dec", pdec.feat.detach().cpu(), torch.from_numpy(fx[tag + "dec"])))
    loss.backward()
    for name, y, ref in pairs:
        cosd = (1 - F.cosine_similarity(y, ref, dim=1)).max().item()
        print("%s%s: cosine distance max %.3e, abs max %.3e" % (tag, name, cosd, (y - ref).abs().max().item()))
        assert cosd < 1e-5 and torch.allclose(y, ref, atol=2e-3, rtol=2e-3)
    r = torch.from_numpy(fx[tag + "dfeat"])
    assert (feat.grad.cpu() - r).norm() <= 3e-3 * r.norm() + 1e-5
    for k, p in bb.named_parameters():
        if tag + "grad_" + k in fx:
            r = torch.from_numpy(fx[tag + "grad_" + k])
            rel = ((p.grad.cpu() - r).norm() / r.norm()).item()
            print("%sgrad %s: %.3e" % (tag, k, rel))
            assert (p.grad.cpu() - r).norm() <= 3e-3 * r.norm() + 1e-5, k
        elif k.startswith("dec.") and not dec:
            assert p.grad is None, k
    assert tag + "grad_mask_token" in fx


def test_pt_v3m1_outputs_unchanged(golden_dir):
    from oracle import ptv3 as optv3
    from scenesplat_amd.pointcept_api import MODELS
    t = np.load(os.path.join(golden_dir, "ptv3_tiny.npz"))
    cfg = {k[4:]: (tuple(t[k].tolist()) if t[k].ndim else t[k].item()) for k in t.files if k.startswith("cfg_")}
    model = MODELS.build(dict(type="PT-v3m1", **cfg, drop_path=0.0, shuffle_orders=False)).cuda().eval()
    model.load_state_dict(optv3.init_state_dict(cfg, seed=11), strict=True)
    torch.manual_seed(77)
    with torch.no_grad():
        y = model(dict(feat=torch.from_numpy(t["feat"]).cuda(), grid_coord=torch.from_numpy(t["gc"]).cuda(),
                       offset=torch.from_numpy(t["offset"]).cuda())).feat.cpu()
    ref = torch.from_numpy(t["eval_y"])
    assert (1 - F.cosine_similarity(y, ref, dim=1)).max() < 1e-5 and torch.allclose(y, ref, atol=2e-3, rtol=2e-3)


# ---- whole model ------------------------------------------------------------------------------------------------------------------------------
def test_whole_model_matches_reference(fx):
    model = tiny_model(mask_grid_size=2.0)
    state = sc.model_state(model)
    model.load_state_dict(state, strict=True)
    model = model.cuda().train()
    inp = {k: t.cuda() for k, t in sc.model_inputs().items()}
    seed(1234)
    out = model(inp, 0.05)
    out["loss"].backward()
    assert sorted(out) == fx["model_scalar_names"].tolist()
    fails = []
    for k in sorted(out):
        ref, ref64 = float(fx["model_out_" + k]), float(fx["model_out_" + k + "_f64"])
        bound = max(4 * abs(ref - ref64), 2e-3 * abs(ref))
        err = abs(float(out[k].detach()) - ref)
        print("scalar %-34s ours %+.7f ref %+.7f f64 %+.7f  |err| %.2e  bound %.2e" % (k, float(out[k].detach()), ref, ref64, err, bound))
        if not err <= bound:
            fails.append(k)
    params = dict(model.named_parameters())
    for k in fx:
        if k.startswith("model_grad_"):
            g, r = params[k[11:]].grad.cpu(), torch.from_numpy(fx[k])
            print("grad %-52s rel %.3e" % (k[11:], ((g - r).norm() / r.norm()).item()))
            if not (g - r).norm() <= 3e-3 * r.norm() + 1e-5:
                fails.append(k)
        elif k.startswith("model_gradnorm_"):         # |‖g‖ - ‖r‖| <= ‖g - r‖: the same bound on the norms of ALL gradients
            g, r = params[k[15:]].grad.double().norm().item(), float(fx[k])
            if not abs(g - r) <= 3e-3 * r + 1e-5:
                fails.append(k)
    assert all(p.grad is None for p in model.backbone_teacher.parameters())
    model.update_teacher(0.99)
    worst = 0.0
    for k, t in model.backbone_teacher.named_parameters():
        t0, s0 = state["backbone_teacher." + k].reshape(-1)[:128], state["backbone_student." + k].reshape(-1)[:128]
        bound = 2.0 ** -22 * torch.maximum(t0.abs(), s0.abs()).double()
        err = (t.detach().cpu().reshape(-1)[:128].double() - torch.from_numpy(fx["model_teacher_head_" + k]).double()).abs()
        if k == "mask_token":
            assert torch.equal(t.detach().cpu(), state["backbone_teacher." + k])
        worst = max(worst, (err / bound.clamp_min(1e-30)).max().item())
        if not (err <= bound).all():
            fails.append("teacher " + k)
    print("teacher after update_teacher(0.99): worst error / bound %.3f" % worst)
    assert not fails, fails


# ---- trainer ------------------------------------------------------------------------------------------------------------------------------------
def test_pretrainer_two_steps(fx):
    from scenesplat_amd.pointcept_api import PRETRAINERS
    cfg = dict(model=dict(type="DefaultContrastiverSimDinoV2", backbone_out_channels=64, enable_mae_loss=True, mask_grid_size=2.0,
                          backbone=dict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA)),
               optimizer=dict(type="AdamW", lr=0.001, weight_decay=0.001, eps=1e-4),
               scheduler=dict(type="OneCycleLR", max_lr=[0.001, 0.0001], pct_start=0.05, anneal_strategy="cos", div_factor=10.0,
                              final_div_factor=1000.0),
               param_dicts=[dict(keyword="block", lr=0.0001)], eval_epoch=25, enable_amp=True, clip_grad=3.0, steady_state=True)
    lines = []
    tr = PRETRAINERS.build(dict(type="DefaultSSLPreTrainer", cfg=cfg, train_loader=[sc.model_inputs(), sc.model_inputs()], logger=lines.append))
    assert any("steady_state is ignored" in ln for ln in lines) and tr.scheduler.total_steps == 50
    tr.model.load_state_dict(sc.model_state(tr.model), strict=True)
    s0 = {k: v.clone() for k, v in tr.model.backbone_student.state_dict().items()}
    t0 = {k: v.clone() for k, v in tr.model.backbone_teacher.state_dict().items()}
    tr.model.train()
    seed(5)
    for i, batch in enumerate(tr.train_loader):
        tr.comm_info["iter"], tr.comm_info["input_dict"] = i, batch
        tr.run_step()
        out = tr.comm_info["model_output_dict"]
        assert all(torch.isfinite(v).all() for v in out.values()), {k: float(v) for k, v in out.items()}
    assert tr.last_momentum == fx["sched_momentum"][1]
    assert tr.optimizer.param_groups[0]["weight_decay"] != 0.001
    s1, t1 = tr.model.backbone_student.state_dict(), tr.model.backbone_teacher.state_dict()
    k = "enc.enc1.block0.attn.qkv.weight"
    assert not torch.equal(s1[k], s0[k]) and not torch.equal(t1[k], t0[k])
    assert not torch.equal(s1["mask_token"], s0["mask_token"]) and torch.equal(t1["mask_token"], t0["mask_token"])
