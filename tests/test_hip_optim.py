"""GPU: FusedAdamW (csrc/optim.hip) against clip_grad_norm_ + torch.optim.AdamW.

One set of inputs, three runs of it, shared by the tests below (module fixture, never modified):
  reference  clip_grad_norm_ + torch.optim.AdamW(foreach=False) in fp64,
  yardstick  clip_grad_norm_ + torch.optim.AdamW (torch's default fp32 path) -- what the Trainer ran before FusedAdamW existed,
  fused      FusedAdamW(max_grad_norm=1.0) in fp32.
The bar: for each of p, exp_avg, exp_avg_sq the max abs error of `fused` against the fp64 reference is at most 2x the yardstick's
max abs error against that same reference.  The factor 2 covers FMA contraction and the last-bit differences of a reordered
expression; an approximate sqrt or divide would break it.

Inputs: numel in {1, 7, 8, 8191, 8192, 8193, 3*8192+5} (one workgroup owns 8,192 elements; 16-byte lanes of 8 with a scalar
tail), 300 tensors of 3 elements (the descriptor search), one parameter whose gradient is a view at element offset 1 of a flat
buffer (only 4-byte aligned: the one-element-per-lane path, 2 workgroups), one parameter that never gets a gradient; two groups
(lr 6e-3 / wd 0.05 and lr 6e-4 / wd 0), betas (0.9, 0.999), eps 1e-8; five steps of seeded normal gradients, step 1 scaled x10,
the later ones x0.01.  With these 58,268 gradient elements the x0.01 steps have a norm of about 2.4, so max_grad_norm = 1.0 clips in
every step (coef about 4e-4, then about 0.41); the regime where the clip is inactive and coef == 1 exactly has its own test
(test_inactive_clip_is_bitwise_no_clip)."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

NUMELS = [1, 7, 8, 8191, 8192, 8193, 3 * 8192 + 5]
N_SMALL = 300
UNALIGNED_NUMEL = 8192 + 3
STEPS = 5
GROUPS = [dict(lr=6e-3, weight_decay=0.05), dict(lr=6e-4, weight_decay=0.0)]
BETAS, EPS, CLIP = (0.9, 0.999), 1e-8, 1.0


def _inputs(steps=STEPS, scales=None):
    """Seeded CPU tensors: initial parameters, per-step gradients (None for the parameter that never gets one), group of each."""
    gen = torch.Generator().manual_seed(1234)
    shapes = [(n,) for n in NUMELS] + [(3,)] * N_SMALL + [(UNALIGNED_NUMEL,), (10,)]
    unaligned, never = len(shapes) - 2, len(shapes) - 1
    init = [torch.randn(s, generator=gen) for s in shapes]
    scales = scales or [10.0] + [0.01] * (steps - 1)
    grads = [[None if i == never else torch.randn(s, generator=gen) * scales[k] for i, s in enumerate(shapes)] for k in range(steps)]
    group_of = [i % 2 for i in range(len(shapes))]
    return dict(init=init, grads=grads, group_of=group_of, unaligned=unaligned, never=never)


def _build(kind, params, group_of, clip):
    from scenesplat_amd.optim import FusedAdamW
    groups = [dict(params=[p for p, g in zip(params, group_of) if g == j], **GROUPS[j]) for j in range(2)]
    if kind == "fused":
        return FusedAdamW(groups, betas=BETAS, eps=EPS, max_grad_norm=clip)
    if kind == "torch64":
        return torch.optim.AdamW(groups, betas=BETAS, eps=EPS, foreach=False)
    return torch.optim.AdamW(groups, betas=BETAS, eps=EPS)


def _run(inp, kind, clip=CLIP, steps=None, handoff=None):
    """-> dict(p, exp_avg, exp_avg_sq: lists of fp64 tensors (None without state), norms: per-step total norm (device tensors),
    params, opt, grads_untouched).  handoff=k: k steps of torch.optim.AdamW, then its state_dict moves into `kind` for the rest."""
    dev = torch.device("cuda")
    dtype = torch.float64 if kind == "torch64" else torch.float32
    params = [nn.Parameter(t.to(dev, dtype)) for t in inp["init"]]
    first = "torch" if handoff else kind
    opt = _build(first, params, inp["group_of"], clip)
    norms, untouched = [], True
    for k, step_grads in enumerate(inp["grads"][:steps]):
        if handoff and k == handoff:
            nxt = _build(kind, params, inp["group_of"], clip)
            nxt.load_state_dict(opt.state_dict())
            opt = nxt
        fused = type(opt).__name__ == "FusedAdamW"
        for i, (p, g) in enumerate(zip(params, step_grads)):
            if g is None:
                p.grad = None
            elif fused and i == inp["unaligned"]:
                flat = torch.zeros(g.numel() + 5, dtype=dtype, device=dev)
                flat[1:1 + g.numel()] = g.to(dev, dtype)
                p.grad = flat[1:1 + g.numel()].view(g.shape)
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = g.to(dev, dtype)
        if fused:
            before = [None if p.grad is None else p.grad.clone() for p in params]
            opt.step()
            untouched = untouched and all(b is None or torch.equal(b, p.grad) for b, p in zip(before, params))
            if clip is not None:
                norms.append(opt.last_grad_norm.clone())
        else:
            if clip is not None:
                norms.append(torch.nn.utils.clip_grad_norm_(params, clip))
            opt.step()
    out = dict(params=params, opt=opt, norms=norms, grads_untouched=untouched)
    out["p"] = [p.detach().double() for p in params]
    for key in ("exp_avg", "exp_avg_sq"):
        out[key] = [opt.state[p][key].double() if p in opt.state else None for p in params]
    return out


def _err(run, ref, key):
    return max(float((a - b).abs().max()) for a, b in zip(run[key], ref[key]) if b is not None)


def _assert_bar(run, yard, ref, what):
    ratios = {}
    for key in ("p", "exp_avg", "exp_avg_sq"):
        e, y = _err(run, ref, key), _err(yard, ref, key)
        ratios[key] = e / y if y > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{what}: {key}: fused max abs err {e:.3e}, torch fp32 max abs err {y:.3e}, ratio {ratios[key]:.3f}")
    for key, r in ratios.items():
        assert r <= 2.0, (what, key, r)


@pytest.fixture(scope="module")
def runs():
    inp = _inputs()
    return dict(inp=inp, ref=_run(inp, "torch64"), yard=_run(inp, "torch"), fused=_run(inp, "fused"))


def test_error_against_fp64_within_twice_torchs_own(runs):
    _assert_bar(runs["fused"], runs["yard"], runs["ref"], "clip + AdamW, 5 steps")


def test_last_grad_norm_matches_fp64_norm(runs):
    assert len(runs["fused"]["norms"]) == STEPS
    for k, (a, b) in enumerate(zip(runs["fused"]["norms"], runs["ref"]["norms"])):
        assert a.dim() == 0 and a.dtype == torch.float32 and a.is_cuda
        rel = abs(float(a) - float(b)) / float(b)
        print(f"step {k}: norm {float(a):.6e} vs fp64 {float(b):.6e}, rel {rel:.2e}")
        assert rel <= 1e-6, (k, rel)
    assert float(runs["ref"]["norms"][0]) > 1000 and 1.0 < float(runs["ref"]["norms"][1]) < 5.0      # the clip was active throughout


def test_gradients_are_left_untouched(runs):
    assert runs["fused"]["grads_untouched"]


def test_parameter_without_gradient_is_skipped(runs):
    inp, fused = runs["inp"], runs["fused"]
    p = fused["params"][inp["never"]]
    assert p not in fused["opt"].state
    assert torch.equal(p.detach().cpu(), inp["init"][inp["never"]]) and p._version == 0
    assert all(float(fused["opt"].state[q]["step"]) == STEPS for q in fused["params"] if q is not p)
    assert all(q._version > 0 for q in fused["params"] if q is not p)


def test_two_runs_are_bitwise_identical(runs):
    again = _run(runs["inp"], "fused")
    for key in ("p", "exp_avg", "exp_avg_sq"):
        assert all(b is None or torch.equal(a, b) for a, b in zip(again[key], runs["fused"][key]))
    assert all(torch.equal(a, b) for a, b in zip(again["norms"], runs["fused"]["norms"]))


def test_without_clipping_matches_plain_adamw(runs):
    inp = runs["inp"]
    steps = 3
    ref, yard, fused = (_run(inp, k, clip=None, steps=steps) for k in ("torch64", "torch", "fused"))
    assert fused["opt"].last_grad_norm is None
    _assert_bar(fused, yard, ref, "AdamW without clipping, 3 steps")


def test_inactive_clip_is_bitwise_no_clip():
    """Gradients whose global norm is below max_grad_norm: coef == 1 exactly, so the run equals the one without clipping bit for bit."""
    inp = _inputs(steps=2, scales=[1e-3, 1e-3])
    a, b = _run(inp, "fused", clip=CLIP), _run(inp, "fused", clip=None)
    assert 0.0 < float(a["norms"][0]) < 1.0
    for key in ("p", "exp_avg", "exp_avg_sq"):
        assert all(y is None or torch.equal(x, y) for x, y in zip(a[key], b[key]))


def test_zero_gradients_move_parameters_by_weight_decay_only():
    inp = _inputs(steps=1)
    inp["grads"] = [[None if g is None else torch.zeros_like(g) for g in inp["grads"][0]]]
    out = _run(inp, "fused")
    assert float(out["norms"][0]) == 0.0
    for i, (p, p0) in enumerate(zip(out["params"], inp["init"])):
        grp = GROUPS[inp["group_of"][i]]
        want = p0.cuda() if i == inp["never"] else p0.cuda() * (1 - grp["lr"] * grp["weight_decay"])
        assert torch.equal(p.detach(), want), i
        if i != inp["never"]:
            st = out["opt"].state[p]
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()


def test_checkpoint_interchange_with_torch_adamw(runs):
    """Two steps of torch.optim.AdamW, its state_dict loaded into FusedAdamW, two more steps on each."""
    inp = runs["inp"]
    ref, yard = _run(inp, "torch64", steps=4), _run(inp, "torch", steps=4)
    fused = _run(inp, "fused", steps=4, handoff=2)
    assert type(fused["opt"]).__name__ == "FusedAdamW"
    assert all(float(fused["opt"].state[p]["step"]) == 4 for p in fused["params"] if p in fused["opt"].state)
    _assert_bar(fused, yard, ref, "state handed from torch AdamW after 2 of 4 steps")
    # and back: torch.optim.AdamW continues from FusedAdamW's state
    back = _build("torch", fused["params"], inp["group_of"], CLIP)
    back.load_state_dict(fused["opt"].state_dict())
    assert float(back.state[fused["params"][0]]["step"]) == 4


def test_step_bumps_versions_so_bf16_shadows_refresh():
    from scenesplat_amd import functional as F
    inp = _inputs(steps=2)
    dev = torch.device("cuda")
    params = [nn.Parameter(t.to(dev)) for t in inp["init"]]
    opt = _build("fused", params, inp["group_of"], CLIP)
    src, dst = F.register_shadows(params)
    F.refresh_shadows(src, dst)
    assert all(torch.equal(d, p.detach().bfloat16()) for p, d in zip(src, dst))
    versions = [p._version for p in params]
    for p, g in zip(params, inp["grads"][0]):
        p.grad = None if g is None else g.to(dev)
    opt.step()
    for i, p in enumerate(params):
        assert (p._version == versions[i]) if i == inp["never"] else (p._version > versions[i]), i
    F.refresh_shadows(src, dst)
    changed = sum(not torch.equal(a.detach().cpu(), b) for a, b in zip(params, inp["init"]))
    assert changed == len(params) - 1
    assert all(torch.equal(d.view(torch.int16), p.detach().bfloat16().view(torch.int16)) for p, d in zip(src, dst))


def test_step_reads_nothing_on_the_host():
    inp = _inputs(steps=2)
    dev = torch.device("cuda")
    params = [nn.Parameter(t.to(dev)) for t in inp["init"]]
    opt = _build("fused", params, inp["group_of"], CLIP)
    grads = [[None if g is None else g.to(dev) for g in step] for step in inp["grads"]]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in grads:                       # the first step creates the state, the second runs on existing state
            for p, g in zip(params, step):
                p.grad = g
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(opt.last_grad_norm) > 0


def test_unsupported_tensors_raise():
    from scenesplat_amd.optim import FusedAdamW
    dev = torch.device("cuda")
    ok = nn.Parameter(torch.ones(4, device=dev)); ok.grad = torch.ones_like(ok)
    half = nn.Parameter(torch.ones(4, device=dev, dtype=torch.bfloat16)); half.grad = torch.ones_like(half)
    with pytest.raises(RuntimeError, match="parameter 1"):
        FusedAdamW([ok, half]).step()
    strided = nn.Parameter(torch.ones(4, 6, device=dev)); strided.grad = torch.ones(6, 4, device=dev).t()
    with pytest.raises(RuntimeError, match="parameter 1"):
        FusedAdamW([ok, strided]).step()
    assert torch.equal(ok.detach(), torch.ones(4, device=dev))         # refused before anything was updated


def test_native_bindings_directly():
    """native.grad_norm_group / adamw_group and the C entry points under them: null record, empty input, null tables."""
    import ctypes
    import math
    from scenesplat_amd import native as nv
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(5)
    n = 8192 + 9
    p0, g, m0, v0 = (torch.randn(n, generator=gen).to(dev) for _ in range(4))
    v0 = v0.abs()
    lr, wd, b1, b2, eps, t = 1e-2, 0.1, 0.9, 0.999, 1e-8, 3
    scal = (1 - lr * wd, 1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, lr / (1 - b1 ** t))

    def want(coef):
        gd, pd, md, vd = (x.double() for x in (g * coef, p0, m0, v0))
        pd = pd * (1 - lr * wd); md = md + (gd - md) * (1 - b1); vd = vd * b2 + (1 - b2) * gd * gd
        return pd - lr / (1 - b1 ** t) * (md / (vd.sqrt() / math.sqrt(1 - b2 ** t) + eps)), md, vd

    # record = None: no clipping
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    nv.adamw_group([(p, g, m, v, scal), (torch.empty(0, device=dev),) * 4 + (scal,)], None)
    for got, ref in zip((p, m, v), want(1.0)):
        assert float((got.double() - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max())      # a few fp32 roundings
    # a record from grad_norm_group: norm, coef, and g * coef inside the update
    rec = nv.grad_norm_group([g, torch.empty(0, device=dev)], 1.0)
    norm = float(g.double().norm())
    assert abs(float(rec[0]) - norm) <= 1e-6 * norm and abs(float(rec[1]) - 1.0 / (norm + 1e-6)) <= 1e-6 / norm
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    nv.adamw_group([(p, g, m, v, scal)], rec)
    for got, ref in zip((p, m, v), want(float(rec[1]))):
        assert float((got.double() - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max())
    # no gradients at all: norm 0, coef 1
    rec = nv.grad_norm_group([], 1.0, rec)
    assert float(rec[0]) == 0.0 and float(rec[1]) == 1.0
    # validation: wrong dtype / size / device are refused by name before any launch
    with pytest.raises(RuntimeError, match=r"rows\[0\]\.m"):
        nv.adamw_group([(p, g, m[:-1], v, scal)], None)
    with pytest.raises(RuntimeError, match=r"grads\[1\]"):
        nv.grad_norm_group([g, g.double()], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.adamw_group([(p.cpu(), g, m, v, scal)], None)
    # C ABI: SS_OK (0) for empty input, SS_ERR_ARG (1) for null tables; nothing is launched in either case
    lib, null, st = nv.lib(), ctypes.c_void_p(0), nv._stream()
    assert lib.ss_optim_group_elems_per_workgroup() == 8192
    assert lib.ss_adamw_group(null, null, 0, 0, null, st) == 0 and lib.ss_grad_sqnorm_group(null, null, 0, 0, null, st) == 0
    assert lib.ss_adamw_group(null, null, 1, 1, null, st) == 1 and lib.ss_grad_sqnorm_group(null, null, 1, 1, null, st) == 1
    assert lib.ss_grad_norm_finish(null, 0, 1.0, null, st) == 1
    torch.cuda.synchronize()


# ---- the Trainer: clip_grad handed to the optimizer, OneCycleLR cycling lr and beta1 ------------------------------------------------
class _Stub(nn.Module):
    def __init__(self, dtype="float32"):
        super().__init__()
        self.stem = nn.Linear(16, 32)
        self.block0 = nn.Linear(32, 4)
        self.to(getattr(torch, dtype))

    def forward(self, d):
        x = d["feat"].to(self.stem.weight.dtype)
        return dict(loss=self.block0(torch.tanh(self.stem(x))).pow(2).mean() * 100.0)


def _trainer(opt_type, dtype, tmp):
    from scenesplat_amd.pointcept_api import MODELS, engine
    if "OptimGpuStub" not in MODELS.module_dict:
        MODELS.register_module("OptimGpuStub", module=_Stub)

    class Betas(engine.HookBase):
        seen = []

        def before_step(self):
            self.seen.append((self.trainer.optimizer.param_groups[0]["lr"], self.trainer.optimizer.param_groups[0]["betas"][0]))

    spy = Betas()
    spy.seen = []
    gen = torch.Generator().manual_seed(7)
    loader = [dict(feat=torch.randn(64, 16, generator=gen)) for _ in range(3)]
    cfg = dict(model=dict(type="OptimGpuStub", dtype=dtype), device="cuda", eval_epoch=1, save_path=str(tmp), enable_amp=False,
               clip_grad=1.0, optimizer=dict(type=opt_type, lr=6e-3, weight_decay=0.05), param_dicts=[dict(keyword="block", lr=6e-4)],
               scheduler=dict(type="OneCycleLR", max_lr=[6e-3, 6e-4], total_steps=6, pct_start=0.5, div_factor=10.0, final_div_factor=100.0),
               hooks=[spy], gc_freeze=False)
    torch.manual_seed(11)
    tr = engine.Trainer(cfg, train_loader=loader)
    tr.train()
    tr.seen = spy.seen
    return tr


def test_trainer_with_fused_adamw_matches_adamw(tmp_path):
    from scenesplat_amd.optim import FusedAdamW
    ref, yard, fused = _trainer("AdamW", "float64", tmp_path), _trainer("AdamW", "float32", tmp_path), _trainer("FusedAdamW", "float32", tmp_path)
    assert type(fused.optimizer) is FusedAdamW and fused.optimizer.max_grad_norm == 1.0 and type(yard.optimizer) is torch.optim.AdamW
    assert float(fused.optimizer.last_grad_norm) > 1.0                               # the clip took part
    assert len(fused.seen) == 3 and fused.seen == yard.seen                          # lr and beta1 followed the cycle, step by step
    assert fused.seen[0][1] == pytest.approx(0.95) and fused.seen[2][1] == pytest.approx(0.85) and fused.seen[2][0] == pytest.approx(6e-3)
    for key in ("p", "exp_avg", "exp_avg_sq"):
        def get(tr, p):
            return (p.detach() if key == "p" else tr.optimizer.state[p][key]).double()
        e = max(float((get(fused, p) - get(ref, q)).abs().max()) for p, q in zip(fused.model.parameters(), ref.model.parameters()))
        y = max(float((get(yard, p) - get(ref, q)).abs().max()) for p, q in zip(yard.model.parameters(), ref.model.parameters()))
        print(f"Trainer, 3 steps: {key}: fused max abs err {e:.3e}, AdamW max abs err {y:.3e}, ratio {e / y:.3f}")
        assert e <= 2.0 * y, (key, e, y)
