"""Golden vectors of the SimDINO pretraining model from the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ssl_model.py

make_golden.py's stub loader plus: torch_geometric.nn.pool.voxel_grid (torch_cluster's documented grid index, x fastest, extents
max + 1: neither package is installed, so this order is NOT pinned by a run of theirs; the partition does not depend on it), plyfile,
timm.models.layers, a conv stub that casts its input to the weight dtype and ignores .float() (the reference forces its convs to fp32;
the fp64 run keeps them in fp64), and Tensor.cuda as the identity (mask_generator calls .cuda() on an arange).

Tensor.half is the identity as well.  The reference's Block stores the normalised features as fp16 in front of the attention
(point_transformer_v3m1_ssl.py:330-331) and the model feeds the local crops as .half(); outside fp16 autocast its Linear layers then
refuse the mixed dtypes, so the reference cannot run in fp32 with those casts in place.  The goldens are the reference's arithmetic
WITHOUT that storage rounding inside the blocks; the fixture inputs are fp16-representable, so the crops' own .half() changes no value.
Data only, no reference source:

  ssl_model.npz
    (i)   mask_<case>_*: DefaultContrastiverSimDinoV2.mask_generator on ssl_model_cases.mask_batch() (B = 3: 1, 255, 257 points) for
          `patch` at mask_grid_size 0.2 / 2.0 / 3.0 and `splats`: the seed, the recorded draws (flag, rate, perm per sample), the mask and
          the fp16 weights.
    (ii)  bb_<mode>_<dec>_*: PT-v3m1-simdino on the tiny config (do_mask, pooling_reduce="max", drop_path 0), eval / train, return_dec
          both ways, with a given mask: encoder features with their rows' (batch, grid_coord) keys and cotangent, decoder features,
          dfeat, the mask_token gradient and a handful of parameter gradients.
    (iii) model_*: one training forward + backward of DefaultContrastiverSimDinoV2 on that backbone (B = 2, ssl_model_cases.model_inputs)
          under seed 1234: every output scalar (and `_f64`: the same run with the model and the features in fp64 -- it runs through
          the stubs), the operands of the two losses (`model_dino_*`, `model_ibot_*`), gradients of one parameter per part and the norm of every gradient, and of every teacher parameter after
          update_teacher(0.99) the first 128 elements and the fp64 sum.
    (iv)  sched_momentum / sched_temp: CosineScheduler over 50 steps (class body taken from engines/pretrain.py by ast, run here).
  ssl_model_configs.txt
    (v)   the evaluated `model` / `train` dicts of the three ssl-pretrain configs and the state-dict keys with shapes of the full-size
          model, as literals.
"""
import ast
import glob
import importlib
import os
import pprint
import random
import sys
import textwrap

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
R = "/root/reference/"

import make_golden as mg  # noqa: E402
import ssl_model_cases as sc  # noqa: E402


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def get_state():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def set_state(st):
    random.setstate(st[0])
    np.random.set_state(st[1])
    torch.set_rng_state(st[2])


def voxel_grid(pos, size, start=None, end=None, batch=None):
    """torch_cluster.grid_cluster by its documented formula: cell = floor((pos - start) / size) per axis, extents from `end` (the
    per-axis maximum), index = x + y * ex + z * ex * ey."""
    pos = pos.double()
    start = pos.new_zeros(pos.shape[1]) + (0 if start is None else start)
    end = pos.max(0)[0] if end is None else pos.new_zeros(pos.shape[1]) + end
    cell = torch.floor((pos - start) / size).long()
    ext = torch.floor((end - start) / size).long() + 1
    index, stride = torch.zeros(len(pos), dtype=torch.long), 1
    for a in range(pos.shape[1]):
        index += cell[:, a] * stride
        stride *= int(ext[a])
    return index


class CastConv(mg.SubMConv3d):
    def float(self):
        return self

    def forward(self, x):
        return super().forward(x.replace_feature(x.features.to(self.weight.dtype)))


def install():
    mg.install_stubs()
    import spconv.pytorch as spp
    spp.SubMConv3d = CastConv
    spp.modules.is_spconv_module = lambda m: isinstance(m, mg.SubMConv3d)
    tm = mg.stubpkg("timm.models"); tml = mg.stubpkg("timm.models.layers"); tm.layers = tml
    tml.DropPath = lambda p=0.0: torch.nn.Identity()
    mg.stubpkg("plyfile").PlyData = object; sys.modules["plyfile"].PlyElement = object
    mg.stubpkg("torch_geometric"); mg.stubpkg("torch_geometric.nn")
    mg.stubpkg("torch_geometric.nn.pool").voxel_grid = voxel_grid
    losses = sys.modules["pointcept.models.losses"]
    losses.build_criteria = importlib.import_module("pointcept.models.losses.builder").build_criteria
    mg.stubpkg("pointcept.models.point_transformer_v3_ssl", R + "pointcept/models/point_transformer_v3_ssl")
    importlib.import_module("pointcept.models.point_transformer_v3_ssl.point_transformer_v3m1_ssl")
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.half = lambda self, *a, **k: self
    return importlib.import_module("pointcept.models.simdinov2")


def backbone_cfg():
    return mg.ADict(type="PT-v3m1-simdino", **sc.TINY, **sc.TINY_EXTRA)


def scheduler_class():
    src = open(R + "pointcept/engines/pretrain.py").read()
    node = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "CosineScheduler"][0]
    ns = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), "pretrain.py", "exec"), ns)
    return ns["CosineScheduler"]


def literal_file(name, value):
    txt = "{\n" + "".join("%r:\n%s,\n" % (k, textwrap.indent(pprint.pformat(v, width=116, sort_dicts=False), "    "))
                          for k, v in value.items()) + "}"
    assert ast.literal_eval(txt) == value, "a config value is not a plain literal"
    with open(os.path.join(HERE, name), "w") as f:
        f.write(txt + "\n")


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(plain(x) for x in v)
    return v


def main():
    sd_mod = install()
    fx = {}

    # ---- (i) mask generator ---------------------------------------------------------------------------------------------------
    model = sd_mod.DefaultContrastiverSimDinoV2(backbone_out_channels=64, backbone=backbone_cfg(), local_crop_num=3, enable_mae_loss=True)
    gc, offset = sc.mask_batch()
    fx["mask_gc"], fx["mask_offset"] = gc, offset
    for ci, (mtype, size) in enumerate(sc.MASK_CASES):
        model.mask_type, model.mask_grid_size = mtype, size
        ids, counts = sc.patch_ids(gc, offset, size)
        tokens = np.diff(np.concatenate([[0], offset]))
        s = 900 + 10 * ci
        while True:
            # the reference divides by the number of masked patches: a flagged sample that rounds to none (the 1-point sample) raises
            # ZeroDivisionError there, so the golden takes the first seed whose draws leave that sample alone
            seed(s)
            st = get_state()
            draws = sc.draw_masks(offset, counts if mtype == "patch" else tokens, mtype)
            set_state(st)
            try:
                mask, w = model.mask_generator(torch.from_numpy(offset), torch.from_numpy(gc).int())
                break
            except ZeroDivisionError:
                s += 1
        tag = "mask_%s_%s_" % (mtype, str(size).replace(".", "p"))
        fx[tag + "seed"] = np.int64(s)
        fx[tag + "mask"], fx[tag + "weights"] = mask.numpy(), w.numpy()
        fx[tag + "flag"] = np.array([d[0] for d in draws]); fx[tag + "rate"] = np.array([d[2] if d[0] else -1.0 for d in draws])
        for i, d in enumerate(draws):
            if d[0]:
                fx[tag + "perm%d" % i] = d[1]
        m2, w2 = sc.apply_draws(offset, ids, draws, mtype)
        assert np.array_equal(m2, mask.numpy()) and np.array_equal(w2.view(np.uint16), w.numpy().view(np.uint16)), tag

    # ---- (ii) tiny backbone -----------------------------------------------------------------------------------------------------------
    ssl_mod = sys.modules["pointcept.models.point_transformer_v3_ssl.point_transformer_v3m1_ssl"]
    bb = ssl_mod.PointTransformerV3_SIMDINO(**sc.TINY, **sc.TINY_EXTRA, do_mask=True)
    bb.load_state_dict(sc.backbone_state(31), strict=True)
    sd0 = {k: v.clone() for k, v in bb.state_dict().items()}
    v = sc.view((300, 421), 11, 12, 60)
    g = torch.Generator().manual_seed(61)
    given = torch.rand(len(v["feat"]), generator=g) < 0.3
    fx["bb_mask"] = given.numpy()
    names = ("mask_token", "embedding.stem.norm.weight", "enc.enc1.down.proj.weight", "enc.enc2.block1.attn.proj.weight",
             "enc.enc0.block0.norm1.0.bias", "dec.dec0.block1.mlp.0.fc1.weight", "dec.dec1.up.proj_skip.0.weight")
    for mode in ("eval", "train"):
        for dec in (0, 1):
            bb.load_state_dict(sd0)
            bb.train(mode == "train")
            bb.zero_grad()
            f = v["feat"].clone().requires_grad_(True)
            torch.manual_seed(77)
            enc, pdec = bb(dict(coord=v["coord"], grid_coord=v["grid_coord"], feat=f, offset=v["offset"]), mask=given, return_dec=bool(dec))
            assert (pdec is None) == (not dec)
            tag = "bb_%s_%d_" % (mode, dec)
            cot_e = torch.randn(enc.feat.shape, generator=torch.Generator().manual_seed(5))
            loss = (enc.feat * cot_e).sum()
            if dec:
                cot_d = torch.randn(pdec.feat.shape, generator=torch.Generator().manual_seed(6))
                loss = loss + (pdec.feat * cot_d).sum()
                fx[tag + "dec"] = pdec.feat.detach().numpy()
            loss.backward()
            # the rows of the coarsest level are identified by (sample, grid_coord at that level): its row ORDER is not part of the contract
            depth = len(sc.TINY["stride"])
            keys = {}
            batch = torch.searchsorted(v["offset"], torch.arange(len(f)), right=True)
            for b_, c_ in zip(batch.tolist(), (v["grid_coord"] >> depth).tolist()):
                keys.setdefault((b_, tuple(c_)), len(keys))
            assert len(keys) == enc.feat.shape[0] and enc.offset.tolist()[-1] == len(keys)
            fx[tag + "enc"] = enc.feat.detach().numpy()      # (cotangents: torch.randn under Generator seeds 5 (enc) / 6 (dec), in the reference's row order)
            fx[tag + "enc_offset"] = enc.offset.numpy()
            fx[tag + "dfeat"] = f.grad.numpy()
            params = dict(bb.named_parameters())
            for pn in names:
                if params[pn].grad is not None:
                    fx[tag + "grad_" + pn] = params[pn].grad.numpy()
    # the key of every coarsest-level row, from the reference's own pooled grid_coord (recomputed by one more forward with a hook)
    rec = {}
    hook = bb.enc.register_forward_hook(lambda mod, i, o: rec.update(gc=o.grid_coord.clone(), batch=o.batch.clone()))
    bb.eval()
    torch.manual_seed(77)
    with torch.no_grad():
        bb(dict(coord=v["coord"], grid_coord=v["grid_coord"], feat=v["feat"], offset=v["offset"]), mask=given, return_dec=False)
    hook.remove()
    fx["bb_enc_gc"], fx["bb_enc_batch"] = rec["gc"].numpy(), rec["batch"].numpy()

    # ---- (iii) whole model ---------------------------------------------------------------------------------------------------------------
    picks = ("backbone_student.enc.enc1.block0.attn.qkv.weight", "backbone_student.dec.dec0.block0.mlp.0.fc2.weight",
             "dino_head.mlp.4.bias", "ibot_head.mlp.0.weight", "mae_head.0.weight", "backbone_student.mask_token")

    def run(dtype, rec):
        m = sd_mod.DefaultContrastiverSimDinoV2(backbone_out_channels=64, backbone=backbone_cfg(), local_crop_num=3, enable_mae_loss=True,
                                                mask_grid_size=2.0)
        m.load_state_dict(sc.model_state(m), strict=True)
        m = m.to(dtype).train()
        inp = sc.model_inputs()
        inp = {k: (t.to(dtype) if k.endswith("_feat") else t) for k, t in inp.items()}
        dino, ibot = m.dino_loss.forward, m.ibot_patch_loss.forward_masked        # the operands of the two losses, for the restatements

        def dino_rec(s_, t_, **kw):
            rec["model_dino_student"], rec["model_dino_teacher"] = torch.stack(s_).detach().numpy(), torch.stack(t_).detach().numpy()
            return dino(s_, t_, **kw)

        def ibot_rec(s_, t_, masks_weight, view_nums):
            rec["model_ibot_student"], rec["model_ibot_teacher"] = s_.detach().numpy(), t_.detach().numpy()
            rec["model_ibot_weight"] = masks_weight.numpy()
            return ibot(s_, t_, masks_weight=masks_weight, view_nums=view_nums)
        m.dino_loss.forward, m.ibot_patch_loss.forward_masked = dino_rec, ibot_rec
        seed(1234)
        out = m(inp, 0.05)
        out["loss"].backward()
        return m, out

    m, out = run(torch.float32, fx)
    fx["model_scalar_names"] = np.array(sorted(out))
    for k, t in out.items():
        fx["model_out_" + k] = np.float64(t.detach().double().item())
    params = dict(m.named_parameters())
    for pn in picks:
        fx["model_grad_" + pn] = params[pn].grad.numpy()
    for k, t in params.items():           # and the norm of every gradient (the 2048-wide dino_head matrices are too large to store)
        if t.grad is not None:
            fx["model_gradnorm_" + k] = np.float64(t.grad.double().norm().item())
    assert all(p.grad is None for p in m.backbone_teacher.parameters())
    m.update_teacher(0.99)
    for k, t in m.backbone_teacher.named_parameters():
        fx["model_teacher_head_" + k] = t.detach().reshape(-1)[:128].numpy().copy()
        fx["model_teacher_sum_" + k] = np.float64(t.detach().double().sum().item())
    try:
        _, out64 = run(torch.float64, {})
        for k, t in out64.items():
            fx["model_out_" + k + "_f64"] = np.float64(t.detach().double().item())
    except Exception as err:            # stated in the docstring of the tests if it happens
        print("fp64 run failed:", repr(err))

    # ---- (iv) schedules -------------------------------------------------------------------------------------------------------------------
    CS = scheduler_class()
    total = 50
    mom = CS(base_value=0.9, final_value=1, total_iters=total)
    temp = CS(base_value=0.07, final_value=0.07, start_warmup_value=0.04, warmup_iters=int(0.6 * total), total_iters=int(0.6 * total))
    fx["sched_momentum"] = np.array([mom.step() for _ in range(total)], np.float64)
    fx["sched_temp"] = np.array([temp.step() for _ in range(total)], np.float64)
    np.savez_compressed(os.path.join(HERE, "ssl_model.npz"), **fx)

    # ---- (v) config literals ------------------------------------------------------------------------------------------------------------------
    import make_golden_configs as mc
    lit = {}
    for p in sorted(glob.glob(R + "configs/*/ssl-pretrain-*.py")):
        rel = os.path.relpath(p, R)
        cfg = mc.load_config(R, rel)
        lit[rel] = dict(model=plain(cfg["model"]), train=plain(cfg["train"]))
    first = lit["configs/scannet/ssl-pretrain-scannet-all-base.py"]["model"]       # (do_ema and do_ibot: teacher, student and all heads)
    full = sd_mod.DefaultContrastiverSimDinoV2(**{k: (mg.ADict(v, enable_flash=False) if k == "backbone" else v) for k, v in first.items()
                                                  if k not in ("type", "code_weight")})     # (two configs pass code_weight, which the constructor does not take)
    lit["state_dict"] = [(k, tuple(v.shape)) for k, v in full.state_dict().items()]
    literal_file("ssl_model_configs.txt", lit)
    print("written: ssl_model.npz (%d arrays, %.0f KiB), ssl_model_configs.txt" % (
        len(fx), os.path.getsize(os.path.join(HERE, "ssl_model.npz")) / 1024))


if __name__ == "__main__":
    main()
