"""CPU: the host side of the open-vocabulary test stage (scenesplat_amd/pointcept_api/tester.py): the TESTERS registry, the
reference's shipped `test` dicts (tests/golden/tester_configs.txt, written by tests/golden/make_golden_tester.py) building a
ZeroShotSemSegTester, the label-mapping table, the records and the metrics.  Nothing is launched."""
import ast
import os

import numpy as np
import pytest
import torch

CONFIGS = ["configs/concat_dataset/lang-pretrain-concat-scan-ppv2-matt-mcmc-wo-normal-contrastive.py",
           "configs/scannet/lang-pretrain-scannet-mcmc-wo-normal-contrastive.py"]
SS_OK, SS_ERR_ARG = 0, 1


def load_configs(golden_dir):
    with open(os.path.join(golden_dir, "tester_configs.txt")) as f:
        return ast.literal_eval(f.read())


def shipped_cases(golden_dir):
    """(config path, index | None, test dict, data.test dict) of every tester the two configs name"""
    out = []
    for rel, cfg in load_configs(golden_dir).items():
        if isinstance(cfg["test"], list):
            assert len(cfg["test"]) == len(cfg["data"]["test"])
            out += [(rel, i, t, d) for i, (t, d) in enumerate(zip(cfg["test"], cfg["data"]["test"]))]
        else:
            out.append((rel, None, cfg["test"], cfg["data"]["test"]))
    return out


class StubModel:
    calls = 0

    def eval(self):
        return self

    def __call__(self, input_dict, chunk_size=None):
        self.calls += 1
        return dict(point_feat=dict(feat=input_dict["feat"]))


def write_meta(tmp_path, names, dim=16, rows=None, tag=""):
    cn = tmp_path / f"labels{tag}.txt"
    cn.write_text("\n".join(names) + "\n\n")
    te = tmp_path / f"text{tag}.pt"
    torch.save(torch.randn(len(names) if rows is None else rows, dim, generator=torch.Generator().manual_seed(0)) * 3.0, te)
    return str(cn), str(te)


def test_tester_is_registered():
    from scenesplat_amd import pointcept_api as api
    assert "ZeroShotSemSegTester" in api.TESTERS.module_dict
    assert api.TESTERS.get("ZeroShotSemSegTester") is api.ZeroShotSemSegTester and issubclass(api.ZeroShotSemSegTester, api.TesterBase)
    with pytest.raises(KeyError):
        api.TESTERS.build(dict(type="SemSegTester", cfg={}))                       # out of scope: not registered


def test_existing_pins_still_hold():
    from scenesplat_amd.pointcept_api import HOOKS, TRANSFORMS
    for name in ("PreciseEvaluator", "BeginningEvaluator", "LangPretrainZeroShotSemSegEval", "LangPretrainZeroShotSemSegEvalMulti"):
        assert name not in HOOKS.module_dict
    with pytest.raises(NotImplementedError):
        TRANSFORMS.build(dict(type="GridSample", mode="test"))
    assert "GSGaussianBlurVoxelGPU" not in TRANSFORMS.module_dict


def test_shipped_test_dicts_build_a_tester(golden_dir, tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cases = shipped_cases(golden_dir)
    assert len(cases) == 6 and all(t["type"] == "ZeroShotSemSegTester" for _, _, t, _ in cases)
    full = load_configs(golden_dir)
    names = ["wall", "floor", "cabinet", "bed", "ceiling", "chair", "other furniture"]
    cn, te = write_meta(tmp_path, names)
    for rel, index, t, d in cases:
        cfg = dict(full[rel], save_path=str(tmp_path), device="cpu")
        # the shipped dicts, with only the two meta-data paths pointed at files that exist here
        patch = dict(t, class_names=cn, text_embeddings=te)
        cfg["test"] = patch if index is None else [patch if i == index else x for i, x in enumerate(cfg["test"])]
        model, loader = StubModel(), [[dict(fragment_list=[], name="s")]]
        kw = {} if index is None else dict(index=index)
        tester = TESTERS.build(dict(type=t["type"], cfg=cfg, model=model, test_loader=loader, **kw))
        assert tester.model is model and tester.test_loader is loader
        assert tester.vote_k == t["vote_k"] == 25 and tester.enable_voting is t["enable_voting"] is True
        assert tester.confidence_threshold == t["confidence_threshold"] == 0.1 and tester.ignore_index == -1
        assert tester.save_feat == t.get("save_feat", False) and tester.skip_eval == t.get("skip_eval", False)
        assert tester.pred_label_mapping == t.get("pred_label_mapping")
        assert tester.cfg["data"]["test"] == d and tester.data_type == d["type"]
        assert tester.class_names == names and tester.num_classes == 7
        exc = [i for i, n in enumerate(names) if n in t["excluded_classes"]]
        assert tester.excluded_indices == exc
        assert tester.keep_indices == ([i for i in range(7) if i not in exc] if exc else [])
        assert tester.num_keep_classes == len(tester.keep_indices)
        emb = tester.text_embeddings
        assert emb.shape == (7, 16) and torch.allclose(emb.norm(dim=1), torch.ones(7), atol=1e-6)      # F.normalize'd
    assert full[CONFIGS[0]]["test"][4].get("pred_label_mapping") == {4: 1, 5: 2}       # the HoliCity entry carries a mapping


def test_options_fall_back_to_the_constructor_arguments(tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cn, te = write_meta(tmp_path, ["a", "b", "c"])
    cfg = dict(save_path=str(tmp_path), device="cpu", test=dict(type="ZeroShotSemSegTester", vote_k=7),
               data=dict(test=dict(type="ScanNetGSDataset", split="val")))
    t = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=StubModel(), test_loader=[1], class_names=cn, text_embeddings=te,
                           vote_k=3, enable_voting=True, confidence_threshold=0.3, excluded_classes=["b"], ignore_index=255))
    assert (t.vote_k, t.enable_voting, t.confidence_threshold, t.ignore_index) == (7, True, 0.3, 255)      # cfg["test"] wins
    assert t.excluded_indices == [1] and t.keep_indices == [0, 2]


def test_class_count_mismatch_raises(tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cn, te = write_meta(tmp_path, ["a", "b", "c"], rows=4)
    cfg = dict(save_path=str(tmp_path), device="cpu", test=dict(type="ZeroShotSemSegTester", class_names=cn, text_embeddings=te),
               data=dict(test=dict(type="ScanNetGSDataset")))
    with pytest.raises(AssertionError, match="Mismatch in class names and text embeddings"):
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=StubModel(), test_loader=[1]))
    # the reference's two ways past the check (test.py:186-189)
    for extra in (dict(skip_eval=True), dict(pred_label_mapping={3: 0})):
        cfg2 = dict(cfg, test=dict(cfg["test"], **extra))
        assert TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg2, model=StubModel(), test_loader=[1])).num_classes == 3


def test_missing_loader_and_missing_checkpoint_raise(tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cn, te = write_meta(tmp_path, ["a", "b", "c"])
    cfg = dict(save_path=str(tmp_path), device="cpu", test=dict(type="ZeroShotSemSegTester", class_names=cn, text_embeddings=te),
               data=dict(test=dict(type="ScanNetGSDataset")), weight=str(tmp_path / "nope.pth"),
               model=dict(type="LangPretrainer", criteria=[],
                          backbone=dict(type="PT-v3m1", in_channels=4, enc_depths=(1, 1), enc_channels=(8, 16), enc_num_head=(1, 1),
                                        enc_patch_size=(16, 16), stride=(2,), dec_depths=(1,), dec_channels=(8,), dec_num_head=(1,),
                                        dec_patch_size=(16,))))
    with pytest.raises(ValueError, match="test_loader"):
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=StubModel()))
    with pytest.raises(RuntimeError, match="No checkpoint found at"):
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, test_loader=[1]))
    # a checkpoint saved from a DDP wrapper ("module." keys) loads at world size 1
    from scenesplat_amd.pointcept_api import MODELS
    ref = MODELS.build(cfg["model"])
    torch.save(dict(epoch=3, state_dict={"module." + k: v for k, v in ref.state_dict().items()}), cfg["weight"])
    t = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, test_loader=[1]))
    got = t.model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in ref.state_dict().items())


def reference_loop(pred, mapping):
    pred = pred.copy()
    for key, item in mapping.items():                  # engines/test.py:392-394
        pred[pred == key] = item
    return pred


@pytest.mark.parametrize("mapping", [{4: 1, 5: 2}, {1: 2, 2: 3}, {2: 3, 1: 2}, {0: 5, 5: 0}, {9: 1, -7: 2}, {-1: 3}, {3: -1, -1: 0}, {}, None])
def test_label_map_lut_is_the_sequential_loop(mapping):
    from scenesplat_amd.pointops import label_map_lut
    C, ignore = 6, -1
    lut = label_map_lut(mapping, C, ignore)
    assert lut.dtype == torch.int32 and lut.shape == (C + 1,)
    domain = np.array([ignore] + list(range(C)))
    assert np.array_equal(lut.numpy(), reference_loop(domain, mapping or {}))


def test_label_map_lut_on_random_mappings():
    from scenesplat_amd.pointops import label_map_lut
    g = np.random.RandomState(0)
    for _ in range(200):
        C = int(g.randint(1, 12))
        ignore = int(g.choice([-1, 255]))
        pairs = {int(k): int(v) for k, v in zip(g.randint(-2, C + 2, g.randint(0, 6)), g.randint(-1, C, 6))}
        pred = np.concatenate([g.randint(0, C, 50), [ignore] * 5])
        lut = label_map_lut(pairs, C, ignore).numpy()
        assert np.array_equal(lut[np.where(pred == ignore, 0, pred + 1)], reference_loop(pred, pairs))


def test_final_metrics_are_the_reference_formulas(golden_dir):
    from scenesplat_amd.pointcept_api import final_metrics
    fx = np.load(os.path.join(golden_dir, "tester.npz"))
    rec = {"a": dict(intersection=fx["s1_k1_inter"], union=fx["s1_k1_union"], target=fx["s1_k1_target"]),
           "b": dict(intersection=fx["s1_k3_inter"], union=fx["s1_k3_union"], target=fx["s1_k3_target"])}
    keep = [1, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    m = final_metrics(rec, keep)
    i = (fx["s1_k1_inter"] + fx["s1_k3_inter"]).astype(np.float64)
    u = (fx["s1_k1_union"] + fx["s1_k3_union"]).astype(np.float64)
    t = (fx["s1_k1_target"] + fx["s1_k3_target"]).astype(np.float64)
    assert i.sum() > 0 and (u > 0).all()
    iou, acc = i / (u + 1e-10), i / (t + 1e-10)
    assert m["mIoU"] == np.mean(iou[u != 0]) and m["mAcc"] == np.mean(acc[t != 0]) and m["allAcc"] == i.sum() / (t.sum() + 1e-10)
    assert m["fg_mIoU"] == np.mean(iou[keep][u[keep] != 0]) and m["fg_mAcc"] == np.mean(acc[keep][t[keep] != 0])
    assert m["fg_allAcc"] == i[keep].sum() / (t[keep].sum() + 1e-10)
    assert np.array_equal(m["iou_class"], iou) and np.array_equal(m["accuracy_class"], acc)
    assert "fg_mIoU" not in final_metrics(rec) and "fg_mIoU" not in final_metrics(rec, [])
    # classes nobody predicted and nobody carries stay out of the means
    z = dict(intersection=np.array([2, 0, 0]), union=np.array([4, 0, 3]), target=np.array([3, 0, 0]))
    m = final_metrics({"z": z})
    assert m["mIoU"] == np.mean([2 / (4 + 1e-10), 0.0]) and m["mAcc"] == 2 / (3 + 1e-10)


def test_merge_records_drops_a_repeated_scene():
    from scenesplat_amd.pointcept_api import final_metrics, merge_records
    a = dict(intersection=np.array([1, 2]), union=np.array([3, 4]), target=np.array([2, 3]))
    b = dict(intersection=np.array([5, 0]), union=np.array([6, 1]), target=np.array([5, 1]))
    merged = merge_records([{"scene0": a, "scene1": b}, {"scene0": a}, None, {}])      # rank 1 repeats scene0 (DistributedSampler padding)
    assert sorted(merged) == ["scene0", "scene1"]
    assert final_metrics(merged)["allAcc"] == final_metrics({"scene0": a, "scene1": b})["allAcc"] == 8 / (11 + 1e-10)


def test_entry_points_refuse_bad_arguments():
    """every call returns before a launch: no GPU"""
    from scenesplat_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()

    def vf(n=5, C=3, k=1, m=5):
        return lib.ss_vocab_finish(None, n, C, k, 0.0, -1, None, m, None, None, None, 0, None)
    assert vf(C=257) == SS_ERR_ARG and vf(C=0) == SS_ERR_ARG and vf(k=4) == SS_ERR_ARG and vf(k=0) == SS_ERR_ARG
    assert vf(C=256, k=9) == SS_ERR_ARG and vf(n=-1) == SS_ERR_ARG
    assert vf(n=0) == SS_OK and vf(n=0, C=256, k=8) == SS_OK
    assert vf() == SS_ERR_ARG                                                         # null buffers with rows to do

    def cv(m=5, ni=2, C=3):
        return lib.ss_cluster_vote(None, None, m, ni, C, -1, None, None, 0, None)
    assert cv(C=257) == SS_ERR_ARG and cv(C=0) == SS_ERR_ARG and cv(ni=-1) == SS_ERR_ARG and cv(m=-1) == SS_ERR_ARG
    assert cv(m=0) == SS_OK and cv() == SS_ERR_ARG
    assert lib.ss_vocab_finish_workspace_bytes(1000, 3, 5000) >= 1000 * 3 * 4
    assert lib.ss_cluster_vote_workspace_bytes(300, 200) >= 300 * 201 * 4 + 300 * 4


def test_host_wrappers_refuse_cpu_tensors():
    from scenesplat_amd import native as nv, pointops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.vocab_finish(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nv.cluster_vote(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 1, 3, -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.clustering_voting(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), -1, 3)
