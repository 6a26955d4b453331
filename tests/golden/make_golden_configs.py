"""Generator of tests/golden/lang_configs.txt: the reference's shipped language-pretraining configs, evaluated as DATA.

    python tests/golden/make_golden_configs.py <path of the reference tree>

The config files are plain assignments of literals; each one is evaluated with a handful of builtins, nothing imported, its
`_base_` files first (pointcept/utils/config.py merges them).  The keys tests/test_reference_configs.py reads are written
out as one Python literal, {config path: {key: value}}, which the test reads back with ast.literal_eval (data only; no
reference source)."""
import ast
import os
import pprint
import sys
import textwrap

CONFIGS = ["configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py",
           "configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py"]
KEYS = ("model", "optimizer", "scheduler", "param_dicts", "enable_amp", "clip_grad", "mix_prob", "find_unused_parameters",
        "train", "hooks")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lang_configs.txt")

_BUILTINS = {k: __builtins__[k] if isinstance(__builtins__, dict) else getattr(__builtins__, k)
             for k in ("dict", "list", "tuple", "range", "len", "int", "float", "str", "bool", "min", "max", "sum", "round", "abs")}


def load_config(ref, rel):
    def run(path, ns):
        src = open(path).read()
        if "import " in src:
            raise AssertionError("config with an import statement: not data")
        local = {"__builtins__": _BUILTINS}
        exec(compile(src, path, "exec"), local)              # noqa: S102 -- literals only, builtins restricted to the list above
        for base in local.pop("_base_", []):
            bpath = os.path.normpath(os.path.join(os.path.dirname(path), base))
            if not os.path.exists(bpath):
                # reference quirk: configs/scannet/lang-pretrain-...py names "../../_base_/..." (one level too many for where the
                # file is shipped); the file it means is configs/_base_/...
                bpath = os.path.join(ref, "configs", base[base.index("_base_"):])
            run(bpath, ns)
        ns.update({k: v for k, v in local.items() if not k.startswith("__")})
    ns = {}
    run(os.path.join(ref, rel), ns)
    return ns


def main(ref):
    out = {}
    for rel in CONFIGS:
        cfg = load_config(ref, rel)
        out[rel] = {k: cfg[k] for k in KEYS}
    txt = "{\n" + "".join("%r:\n%s,\n" % (rel, textwrap.indent(pprint.pformat(cfg, width=116, sort_dicts=False), "    "))
                          for rel, cfg in out.items()) + "}"
    assert ast.literal_eval(txt) == out, "a config value is not a plain literal"
    with open(OUT, "w") as f:
        f.write(txt + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
