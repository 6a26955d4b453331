"""Generator of the semantic-segmentation fixtures, by running the REFERENCE's own Python (container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semseg.py <path of the reference tree>

Uses make_golden.py's stubs (addict, timm, spconv, torch_scatter) and writes, as data only:

  semseg_configs.txt  the two ScanNet semseg configs evaluated with `_base_` merged (their one import, the ScanNet200 class-name
                      constants, is resolved from the reference's constants file), {config path: {key: value}}
  semseg.npz          1. the reference DefaultSegmentorV2's state-dict key -> shape map per config (sd_<cfg>_keys / _shapes)
                      2. CrossEntropyLoss + LovaszLoss(multiclass) values and d logits (reference autograd; 128 seeded rows per
                         case) at C = 20 / 100 / 200, with ignored rows, a subset of classes present, class_seen, n = 1, and a
                         tie-heavy lattice case
                      3. DefaultSegmentorV2 at the ScanNet config's widths on a 6,400-Gaussian room with 14 features (flash off,
                         drop_path 0): eval logits (1,024 seeded rows in full, arg-max and top-2 margin of every row), the eval and
                         train-mode losses and the leading 4,096 elements of six parameter gradients
                      4. intersection_and_union_gpu (run on the CPU) on fixed predictions
Every input (logits, labels, point cloud, weights) is regenerated from the seeds of semseg_inputs.py; the fixture holds a checksum
of each one instead.
"""
import ast
import importlib
import os
import pprint
import sys
import textwrap

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import semseg_inputs as si  # noqa: E402

CONFIGS = ["configs/scannet/semseg-gs-scannet-all-w-normal-fixed-xyz.py",
           "configs/scannet/semseg-gs-scannet200-all-w-normal-fixed-xyz.py"]
KEYS = ("model", "optimizer", "scheduler", "param_dicts", "enable_amp", "clip_grad", "mix_prob", "find_unused_parameters",
        "train", "hooks", "evaluate")
DATA_KEYS = ("num_classes", "ignore_index", "names")
CONSTANTS = "pointcept/datasets/preprocessing/scannet/meta_data/scannet200_constants.py"

_BUILTINS = {k: __builtins__[k] if isinstance(__builtins__, dict) else getattr(__builtins__, k)
             for k in ("dict", "list", "tuple", "range", "len", "int", "float", "str", "bool", "min", "max", "sum", "round", "abs")}


def load_config(ref, rel):
    """Evaluate a config as data: its `from <constants> import NAMES` is served from the constants file (literals only)."""
    consts = {}
    exec(compile(open(os.path.join(ref, CONSTANTS)).read(), CONSTANTS, "exec"), {"__builtins__": _BUILTINS}, consts)  # noqa: S102

    def run(path, ns):
        tree = ast.parse(open(path).read(), path)
        local = {"__builtins__": _BUILTINS}
        body = []
        for node in tree.body:
            if isinstance(node, ast.ImportFrom) and node.module.endswith("scannet200_constants"):
                for a in node.names:
                    local[a.asname or a.name] = consts[a.name]
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                raise AssertionError("config imports something other than the class-name constants")
            else:
                body.append(node)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), local)  # noqa: S102
        for base in local.pop("_base_", []):
            run(os.path.normpath(os.path.join(os.path.dirname(path), base)), ns)
        ns.update({k: v for k, v in local.items() if not k.startswith("__")})
    ns = {}
    run(os.path.join(ref, rel), ns)
    return ns


def write_configs(ref):
    out = {}
    for rel in CONFIGS:
        cfg = load_config(ref, rel)
        d = {k: cfg[k] for k in KEYS}
        d["data"] = {k: cfg["data"][k] for k in DATA_KEYS}
        out[rel] = d
    txt = "{\n" + "".join("%r:\n%s,\n" % (rel, textwrap.indent(pprint.pformat(cfg, width=116, sort_dicts=False), "    "))
                          for rel, cfg in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(os.path.join(HERE, "semseg_configs.txt"), "w") as f:
        f.write(txt + "\n")
    return out


def main(ref):
    mg.R = ref.rstrip("/") + "/"
    mg.install_stubs()
    importlib.import_module("pointcept.models.point_transformer_v3.point_transformer_v3m1_base")
    lb = importlib.import_module("pointcept.models.losses.builder")
    importlib.import_module("pointcept.models.losses.misc")
    importlib.import_module("pointcept.models.losses.lovasz")
    sys.modules["pointcept.models.losses"].build_criteria = lb.build_criteria
    default = importlib.import_module("pointcept.models.default")
    from pointcept.utils.misc import intersection_and_union_gpu
    cfgs = write_configs(ref)
    fx = {}

    # ---- 1. state-dict maps -------------------------------------------------------------------------------------------
    for i, rel in enumerate(CONFIGS):
        mcfg = dict(cfgs[rel]["model"])
        mcfg.pop("type")
        bb = dict(mcfg["backbone"], enable_flash=False)
        bb.pop("type")
        model = default.DefaultSegmentorV2(mcfg["num_classes"], mcfg["backbone_out_channels"], dict(type="PT-v3m1", **bb),
                                           mcfg["criteria"])
        sd = model.state_dict()
        fx[f"sd{i}_keys"] = np.array(list(sd.keys()))
        fx[f"sd{i}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[f"sd{i}_nparam"] = np.int64(sum(p.numel() for p in model.parameters()))

    # ---- 2. the loss pair ---------------------------------------------------------------------------------------------
    names = []
    for name, logits, labels, seen in si.loss_cases():
        crit = lb.build_criteria([dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                                  dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1, class_seen=seen)])
        x = logits.clone().requires_grad_(True)
        ce = crit.criteria[0](x, labels)
        lov = crit.criteria[1](x, labels)
        total = ce + lov
        total.backward()
        rows = si.dlogit_rows(name, len(logits))
        fx.update({f"loss_{name}_checksum": si.checksum(logits, labels), f"loss_{name}_ce": ce.detach().numpy(),
                   f"loss_{name}_lov": lov.detach().numpy(), f"loss_{name}_total": total.detach().numpy(),
                   f"loss_{name}_rows": rows, f"loss_{name}_dlogits": x.grad.numpy()[rows],
                   f"loss_{name}_seen": np.array(seen if seen is not None else [], dtype=np.int64)})
        names.append(name)
    fx["loss_cases"] = np.array(names)

    # ---- 3. DefaultSegmentorV2 end to end at the ScanNet widths ---------------------------------------------------------
    mcfg = dict(cfgs[CONFIGS[0]]["model"])
    bb = dict(mcfg["backbone"], enable_flash=False, drop_path=0.0, shuffle_orders=False)
    bb.pop("type")
    model = default.DefaultSegmentorV2(mcfg["num_classes"], mcfg["backbone_out_channels"], dict(type="PT-v3m1", **bb),
                                       mcfg["criteria"])
    assert {k: bb[k] for k in si.SCANNET_BACKBONE} == si.SCANNET_BACKBONE
    model.load_state_dict(si.model_state(), strict=True)
    inp = si.model_inputs()
    assert np.array_equal(inp["grid_coord"].numpy(), mg.room(64, 4))
    n = len(inp["feat"])
    fx.update({"model_checksum": si.checksum(inp["grid_coord"], inp["feat"], inp["segment"], inp["offset"]),
               "model_seeds": np.array([si.MODEL_SEED, si.HEAD_SEED, si.POOL_SEED])})
    model.eval()
    torch.manual_seed(si.POOL_SEED)
    with torch.no_grad():
        out = model(dict(inp))
    logits = out["seg_logits"]
    rows = si.eval_rows(n)
    top2 = logits.topk(2, dim=1).values
    fx.update({"model_eval_rows": rows, "model_eval_logits": logits.numpy()[rows],
               "model_eval_argmax": logits.argmax(1).numpy().astype(np.int8),
               "model_eval_margin": (top2[:, 0] - top2[:, 1]).numpy().astype(np.float16),
               "model_eval_loss": out["loss"].numpy()})
    model.train()
    torch.manual_seed(si.POOL_SEED)
    out = model(dict(inp))
    out["loss"].backward()
    fx["model_train_loss"] = out["loss"].detach().numpy()
    params = dict(model.named_parameters())
    for k in si.GRAD_KEYS:
        fx["model_grad_" + k] = params[k].grad.reshape(-1)[:si.GRAD_ELEMS].numpy()
    fx["model_grad_keys"] = np.array(si.GRAD_KEYS)

    # ---- 4. intersection_and_union_gpu on the CPU ----------------------------------------------------------------------
    pred, tgt = si.iou_inputs()
    inter, union, target = intersection_and_union_gpu(pred.clone().float(), tgt.clone().float(), 20, -1)
    fx.update({"iou_checksum": si.checksum(pred, tgt), "iou_counts": torch.stack([inter, union, target]).round().long().numpy()})
    np.savez_compressed(os.path.join(HERE, "semseg.npz"), **fx)
    print("wrote semseg.npz and semseg_configs.txt; model n =", n, "train loss", float(out["loss"].detach()))


if __name__ == "__main__":
    main(sys.argv[1])
