"""GPU: the open-vocabulary test stage.  csrc/tester.hip (ss_vocab_finish, ss_cluster_vote) against numpy, and
ZeroShotSemSegTester end to end against RECORDED OUTPUTS of the reference's own neighbor_voting / clustering_voting /
intersection_and_union (tests/golden/tester.npz, written by tests/golden/make_golden_tester.py).  Everything here is integer
valued, so every comparison is exact."""
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IGNORE = -1


# ---- ss_vocab_finish --------------------------------------------------------------------------------------------------------
def vocab_reference(pred, k, threshold, ignore, inverse=None, lut=None):
    lab = np.argsort(-pred, axis=1, kind="stable")[:, :k].astype(np.int64)          # descending value, equal values: lower class first
    if k == 1:
        lab[pred.max(1) < threshold] = ignore
    if lut is not None:
        lab = lut[np.where(lab == ignore, 0, lab + 1)]
    if inverse is not None:
        lab = lab[inverse]
    return lab.astype(np.int32)


def vocab_rows(n, C, seed):
    """half the rows on a grid of five values (equal values in and around the top k, maxima exactly at the threshold 0.75),
    half continuous; every seventh row all zeros"""
    g = np.random.RandomState(seed)
    p = g.rand(n, C).astype(np.float32) * 2.0
    q = (g.randint(0, 5, (n, C)) / 4.0).astype(np.float32)
    cap = g.rand(n) < 0.5
    q[cap] = np.minimum(q[cap], 0.75)
    rows = np.arange(n) % 2 == 0
    p[rows] = q[rows]
    p[np.arange(n) % 7 == 3] = 0.0
    return p


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 7, 64, 65, 200, 256])
def test_vocab_finish_matches_the_stable_argsort(C, k):
    from scenesplat_amd import native as nv
    if k > C:
        with pytest.raises(RuntimeError):
            nv.vocab_finish(torch.zeros(4, C, device="cuda"), k=k)
        return
    for n in (1, 63, 64, 65, 1000):
        p = vocab_rows(n, C, 100 * C + n)
        g = np.random.RandomState(n + C)
        lut = np.concatenate([[g.randint(-1, C)], g.randint(-1, C, C)]).astype(np.int32)
        inv_long = g.randint(0, n, 2 * n + 3).astype(np.int64)                        # m > n: rows repeat
        inv_short = g.permutation(n)[:max(1, n // 3)].astype(np.int64)                # m < n
        dp = torch.from_numpy(p).cuda()
        for thr in (0.75, 0.1):
            got = nv.vocab_finish(dp, k=k, threshold=thr, ignore_index=IGNORE)
            assert got.shape == (n, k) and got.dtype == torch.int32
            assert np.array_equal(got.cpu().numpy(), vocab_reference(p, k, thr, IGNORE)), (n, C, k, thr)
        if k == 1 and C > 1 and n >= 63:
            ref = vocab_reference(p, 1, 0.75, IGNORE)[:, 0]
            assert (ref == IGNORE).any() and (ref >= 0).any()
            assert ((p.max(1) == 0.75) & (ref >= 0)).any()                            # a maximum exactly at the threshold keeps its class
        for inv in (inv_long, inv_short):
            got = nv.vocab_finish(dp, k=k, threshold=0.75, ignore_index=IGNORE, inverse=torch.from_numpy(inv).cuda(),
                                  lut=torch.from_numpy(lut).cuda())
            assert got.shape == (len(inv), k)
            assert np.array_equal(got.cpu().numpy(), vocab_reference(p, k, 0.75, IGNORE, inv, lut)), (n, C, k, len(inv))
        ig = 255 if C <= 255 else 1000                     # an ignore_index above the classes (255 IS a class when C = 256)
        got = nv.vocab_finish(dp, k=k, threshold=0.75, ignore_index=ig, lut=torch.from_numpy(lut).cuda())
        assert np.array_equal(got.cpu().numpy(), vocab_reference(p, k, 0.75, ig, None, lut))
        got = nv.vocab_finish(dp, k=k, threshold=0.75, ignore_index=ig)
        assert np.array_equal(got.cpu().numpy(), vocab_reference(p, k, 0.75, ig))
        # rows that start 4 bytes off a 16-byte boundary: the scalar-load form also where C % 4 == 0
        flat = torch.zeros(n * C + 1, device="cuda")
        flat[1:] = dp.reshape(-1)
        off = flat[1:].view(n, C)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert np.array_equal(nv.vocab_finish(off, k=k, threshold=0.75).cpu().numpy(), vocab_reference(p, k, 0.75, IGNORE))


def test_vocab_finish_hand_cases():
    from scenesplat_amd import native as nv
    p = torch.tensor([[0.2, 0.9, 0.9, 0.1, 0.9],           # three equal maxima: 1, 2, 4
                      [0.0, 0.0, 0.0, 0.0, 0.0],           # zeros: classes 0, 1, 2; ignored for any positive threshold
                      [0.5, 0.1, 0.5, 0.3, 0.3],           # ties inside and at the edge of the top 3: 0, 2, 3
                      [0.1, 0.2, 0.3, 0.4, 0.5]], device="cuda")
    assert nv.vocab_finish(p, k=3).tolist() == [[1, 2, 4], [0, 1, 2], [0, 2, 3], [4, 3, 2]]
    assert nv.vocab_finish(p, k=1, threshold=0.5).reshape(-1).tolist() == [1, IGNORE, 0, 4]           # 0.5 == threshold: kept
    assert nv.vocab_finish(p, k=1, threshold=1e-30).reshape(-1).tolist() == [1, IGNORE, 0, 4]
    assert nv.vocab_finish(p, k=1, threshold=0.0).reshape(-1).tolist() == [1, 0, 0, 4]
    assert nv.vocab_finish(p, k=5)[3].tolist() == [4, 3, 2, 1, 0]
    empty = nv.vocab_finish(torch.zeros(0, 5, device="cuda"), k=3)
    assert empty.shape == (0, 3)
    assert nv.vocab_finish(p, k=3, inverse=torch.zeros(0, dtype=torch.int64, device="cuda")).shape == (0, 3)
    for bad in (dict(pred=torch.zeros(4, 257, device="cuda")), dict(pred=p, k=6), dict(pred=p, k=0), dict(pred=p.double()),
                dict(pred=p, lut=torch.zeros(5, dtype=torch.int32, device="cuda"))):
        with pytest.raises(RuntimeError):
            nv.vocab_finish(**bad)


# ---- ss_cluster_vote --------------------------------------------------------------------------------------------------------
def cluster_reference(pred, instance, ignore):
    """np.unique + argmax per instance (the smallest of the most frequent values wins)"""
    out = pred.copy()
    for i in np.unique(instance):
        if i == ignore:
            continue
        rows = instance == i
        vals, counts = np.unique(pred[rows], return_counts=True)
        out[rows] = vals[np.argmax(counts)]
    return out


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "tester.npz"))


@pytest.mark.parametrize("s", [0, 1])
def test_clustering_voting_matches_the_recorded_reference(fx, s):
    from scenesplat_amd import native as nv, pointops
    C = int(fx[f"s{s}_classes"])
    pred, inst, ref = fx[f"s{s}_k1_base"], fx[f"s{s}_origin_instance"], fx[f"s{s}_cv_out"]
    got = pointops.clustering_voting(torch.from_numpy(pred).cuda(), torch.from_numpy(inst).cuda(), IGNORE, C)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(cluster_reference(pred, inst, IGNORE), ref)                 # the test's own loop is the recorded function
    ids = np.unique(inst[inst != IGNORE])
    dense = np.where(inst == IGNORE, -1, np.searchsorted(ids, inst)).astype(np.int32)
    got = nv.cluster_vote(torch.from_numpy(pred).cuda(), torch.from_numpy(dense).cuda(), len(ids), C, IGNORE)
    assert np.array_equal(got.cpu().numpy(), ref)
    if s == 0:                                                                        # and the voted prediction of the recorded chain
        got = pointops.clustering_voting(torch.from_numpy(fx["s0_k1_voted"]).cuda(), torch.from_numpy(inst).cuda(), IGNORE, C)
        assert np.array_equal(got.cpu().numpy(), fx["s0_k1_final"])


@pytest.mark.parametrize("ignore,C", [(-1, 6), (255, 20), (-100, 256), (3, 6)])
@pytest.mark.parametrize("num_instances", [1, 2, 300])
def test_cluster_vote_matches_the_unique_loop(num_instances, ignore, C):
    from scenesplat_amd import native as nv
    for m in (1, 65, 600):
        g = np.random.RandomState(m + num_instances)
        pred = g.randint(0, min(C, 4), m).astype(np.int32)                            # few values: equal counts are common
        pred[g.rand(m) < 0.3] = ignore
        inst = g.randint(-1, num_instances, m).astype(np.int32)
        if m >= 65:
            inst[10:40] = np.sort(inst[10:40])                                        # runs of equal rows inside a wave
            pred[20:30] = pred[20]
        got = nv.cluster_vote(torch.from_numpy(pred).cuda(), torch.from_numpy(inst).cuda(), num_instances, C, ignore)
        assert np.array_equal(got.cpu().numpy(), cluster_reference(pred, inst, -1)), (m, num_instances, ignore, C)


def test_clustering_voting_hand_cases():
    from scenesplat_amd import native as nv, pointops
    dev = "cuda"
    pred = torch.tensor([-1, 3, 5, 3, -1, 2, 4, 4, 0], dtype=torch.int32, device=dev)
    inst = torch.tensor([70, 70, 70, 70, 70, 9, -1, 1000, -1], dtype=torch.int64, device=dev)
    # instance 70: two -1, two 3, one 5 -> -1 (the numerically smallest of the most frequent); 9 and 1000: one row each
    assert pointops.clustering_voting(pred, inst, -1, 6).tolist() == [-1, -1, -1, -1, -1, 2, 4, 4, 0]
    # ignore_index = 255 sorts above the classes: the same rows now go to class 3, and instance id 255 means "no instance"
    p255 = torch.where(pred < 0, torch.full_like(pred, 255), pred)
    i255 = torch.where(inst < 0, torch.full_like(inst, 255), inst)
    assert pointops.clustering_voting(p255, i255, 255, 6).tolist() == [3, 3, 3, 3, 3, 2, 4, 4, 0]
    none = torch.full((9,), -1, dtype=torch.int64, device=dev)
    assert torch.equal(pointops.clustering_voting(pred, none, -1, 6), pred)           # all rows without an instance
    assert torch.equal(nv.cluster_vote(pred, none.int(), 0, 6, -1), pred)
    with pytest.raises(ValueError, match="pred outside"):
        pointops.clustering_voting(pred, inst, -1, 5)                                 # class 5 with 5 classes
    with pytest.raises(ValueError, match="same shape"):
        pointops.clustering_voting(pred, inst[:4], -1, 6)
    assert pointops.clustering_voting(pred[:0], inst[:0], -1, 6).shape == (0,)


# ---- the tester on the recorded scenes ----------------------------------------------------------------------------------
DIM = 16


class StubModel:
    """point_feat.feat = a fixed function of the input feat (the identity)"""

    def __init__(self):
        self.calls = 0

    def eval(self):
        return self

    def __call__(self, input_dict, chunk_size=None):
        assert chunk_size == 600000 and not torch.is_grad_enabled()
        self.calls += 1
        return dict(point_feat=dict(feat=input_dict["feat"].clone()))


class Loader(list):
    batch_size = 1


def scene_features(abc):
    """normalize(1.0 t[a] + 0.6 t[b] + 0.3 t[c]) over orthonormal text rows (the unit vectors)"""
    f = np.zeros((len(abc), DIM))
    for col, w in zip(range(3), (1.0, 0.6, 0.3)):
        f[np.arange(len(abc)), abc[:, col]] = w
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def make_scene(fx, s, tmp_path, dtype, **test_opts):
    """-> (cfg, loader, model, info) of one recorded scene as the reference's loader would hand it over"""
    C = int(fx[f"s{s}_classes"])
    abc = fx[f"s{s}_abc"]
    feat = scene_features(abc)
    text = np.eye(C, DIM)
    frags = [fx[f"s{s}_frag0"], fx[f"s{s}_frag1"]]
    # unambiguous ranks (checked in fp64 before anything runs): the gap between the k-th and the (k+1)-th accumulated probability
    # is >= 0.02 on every row, ten times the per-term tolerance the scan is granted, and so is the distance to the threshold
    acc = np.zeros((len(abc), C))
    for idx in frags:
        acc[idx] += 1.0 / (1.0 + np.exp(-(feat[idx] @ text.T)))
    srt = -np.sort(-acc, axis=1)
    thr = float(fx["threshold"])
    assert (srt[:, :3] - srt[:, 1:4]).min() >= 0.02 and np.abs(srt[:, 0] - thr).min() >= 0.02
    assert np.array_equal(np.argsort(-acc, axis=1, kind="stable")[:, :3], abc)
    names = [f"c{i}" for i in range(C)]
    (tmp_path / "labels.txt").write_text("\n".join(names) + "\n")
    torch.save(torch.from_numpy(text).float() * 2.5, tmp_path / "text.pt")           # the tester normalises the rows
    mapping = {int(k): int(v) for k, v in zip(fx[f"s{s}_map_keys"], fx[f"s{s}_map_items"])}
    pts = fx[f"s{s}_grid_coord_pts"]
    fragment_list = []
    for j, idx in enumerate(frags):
        frag = dict(coord=pts[idx], grid_coord=np.floor(pts[idx] / 0.02).astype(np.int64), index=idx,
                    feat=feat[idx].astype(np.float32), offset=np.array([len(idx)]))
        if j == 1:                                         # entries may be numpy arrays or CPU / GPU tensors
            frag = {k: torch.from_numpy(v) for k, v in frag.items()}
            frag["feat"] = frag["feat"].cuda()
        fragment_list.append(frag)
    d = dict(fragment_list=fragment_list, name=f"scene{s}", segment=np.zeros(len(abc), np.int64), coord=pts,
             origin_segment=fx[f"s{s}_origin_segment"], inverse=torch.from_numpy(fx[f"s{s}_inverse"]),
             origin_coord=fx[f"s{s}_origin_coord"], origin_feat_mask=fx[f"s{s}_origin_feat_mask"],
             origin_instance=torch.from_numpy(fx[f"s{s}_origin_instance"]).cuda())
    if f"s{s}_pc_coord" in fx.files:
        d.update(pc_coord=fx[f"s{s}_pc_coord"], pc_segment=fx[f"s{s}_pc_segment"])
    loader = Loader([[d]])
    class2id = np.concatenate([np.arange(C) * 10 + 1, [0]])                            # class2id[-1]: the ignored rows
    loader.dataset = types.SimpleNamespace(class2id=class2id)
    test = dict(type="ZeroShotSemSegTester", class_names=str(tmp_path / "labels.txt"), text_embeddings=str(tmp_path / "text.pt"),
                excluded_classes=["c0", "c2"], enable_voting=True, vote_k=int(fx["vote_k"]), confidence_threshold=thr,
                pred_label_mapping=mapping)
    test.update(test_opts)
    cfg = dict(save_path=str(tmp_path / "out"), test=test, data=dict(test=dict(type=dtype, split="val")))
    return cfg, loader, StubModel(), dict(C=C, names=names, class2id=class2id, has_pc="pc_coord" in d, feat=feat)


def formulas(inter, union, target, keep):
    i, u, t = (np.asarray(x, np.float64) for x in (inter, union, target))
    iou, acc = i / (u + 1e-10), i / (t + 1e-10)
    return dict(mIoU=np.mean(iou[u != 0]), mAcc=np.mean(acc[t != 0]), allAcc=i.sum() / (t.sum() + 1e-10),
                fg_mIoU=np.mean(iou[keep][u[keep] != 0]), fg_mAcc=np.mean(acc[keep][t[keep] != 0]),
                fg_allAcc=i[keep].sum() / (t[keep].sum() + 1e-10))


@pytest.mark.parametrize("form,dtype", [("k1", "ScanNetGSDataset"), ("k3", "ScanNetPPGSDataset")])
@pytest.mark.parametrize("s", [0, 1])
def test_tester_reproduces_the_recorded_reference_chain(fx, tmp_path, s, form, dtype):
    from scenesplat_amd.pointcept_api import TESTERS
    cfg, loader, model, info = make_scene(fx, s, tmp_path, dtype)
    lines = []
    tester = TESTERS.build(dict(type=cfg["test"]["type"], cfg=cfg, model=model, test_loader=loader, logger=lines.append))
    metrics = tester.test()
    assert model.calls == 2
    C, rec = info["C"], {k: fx[f"s{s}_{form}_{k}"] for k in ("table", "voted", "final", "inter", "union", "target")}
    out = os.path.join(cfg["save_path"], f"result_{dtype}")
    # the saved prediction: the recorded output of neighbor_voting + clustering_voting on the mapped, expanded labels
    saved = np.load(os.path.join(out, f"scene{s}_pred.npy"))
    assert saved.shape == rec["final"].shape and np.array_equal(saved, rec["final"])
    if not info["has_pc"]:                                 # both votes changed labels
        assert (rec["voted"] != fx[f"s{s}_{form}_base"]).any() and (rec["final"] != rec["voted"]).any()
    # the submission: the labels before the voting
    sub = np.loadtxt(os.path.join(out, "submit", f"scene{s}.txt"), delimiter=",", dtype=np.int64)
    if form == "k3":
        assert np.array_equal(sub, rec["table"])
        assert re.fullmatch(r"-?\d+,-?\d+,-?\d+", open(os.path.join(out, "submit", f"scene{s}.txt")).readline().strip())
    else:
        assert np.array_equal(sub, info["class2id"][rec["table"]])
    # counts and metrics
    keep = [i for i in range(C) if i not in (0, 2)]
    exp = formulas(rec["inter"], rec["union"], rec["target"], keep)
    assert all(metrics[k] == exp[k] for k in exp), (metrics, exp)
    assert rec["inter"].sum() > 0
    txt = open(os.path.join(out, "eval_results.txt")).read().split("\n")
    assert txt[0] == "Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}".format(exp["mIoU"], exp["mAcc"], exp["allAcc"])
    assert txt[1] == "Foreground Val result (excluding 2 classes): mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}".format(
        exp["fg_mIoU"], exp["fg_mAcc"], exp["fg_allAcc"])
    assert txt[2:4] == ["", "Per-class results:"] and len(txt) == 4 + C + 4 + 1
    iou0 = rec["inter"][0] / (rec["union"][0] + 1e-10)
    acc0 = rec["inter"][0] / (rec["target"][0] + 1e-10)
    assert txt[4] == "Class_0-c0 Result: iou/accuracy {:.4f}/{:.4f}".format(iou0, acc0)
    assert txt[4 + C:] == ["", "Excluded classes:", "Class_0", "Class_2", ""]
    assert any("Neighbor voting enabled with k=5" in ln for ln in lines)
    # a second run on the same save_path: a scene without pc_coord is loaded from its file, the metrics are the same
    model2 = StubModel()
    again = TESTERS.build(dict(type=cfg["test"]["type"], cfg=cfg, model=model2, test_loader=loader)).test()
    assert model2.calls == (2 if info["has_pc"] else 0)
    assert all(again[k] == exp[k] for k in exp)
    assert np.array_equal(np.load(os.path.join(out, f"scene{s}_pred.npy")), rec["final"])


def test_tester_counts_per_scene_and_refuses_a_length_mismatch(fx, tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cfg, loader, model, info = make_scene(fx, 0, tmp_path, "ScanNetGSDataset", enable_voting=False)
    seen = {}
    tester = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=loader))
    tester._write_results = lambda m, p: seen.update(m)
    tester.test()
    # without the voting: the expanded, mapped arg-max labels themselves
    saved = np.load(os.path.join(cfg["save_path"], "result_ScanNetGSDataset", "scene0_pred.npy"))
    assert np.array_equal(saved, fx["s0_k1_base"])
    bad = dict(loader[0][0], name="short", origin_segment=fx["s0_origin_segment"][:-1])
    with pytest.raises(ValueError, match="rows"):
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=Loader([[bad]]))).test()


def test_tester_skip_eval_and_save_feat(fx, tmp_path):
    from scenesplat_amd.pointcept_api import TESTERS
    cfg, loader, model, info = make_scene(fx, 1, tmp_path, "Matterport3DGSDataset", skip_eval=True, save_feat=True)
    assert TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=loader)).test() is None
    out = os.path.join(cfg["save_path"], "result_Matterport3DGSDataset")
    assert model.calls == 2 and not os.path.exists(os.path.join(out, "scene1_pred.npy")) and not os.path.exists(os.path.join(out, "eval_results.txt"))
    # the mean over the fragments that saw a point (the same feature both times), L2-normalised, carried through inverse
    feat = torch.load(os.path.join(out, "feat", "scene1_feat.pth"), weights_only=True)
    exp = torch.from_numpy(info["feat"]).float()[torch.from_numpy(fx["s1_inverse"])]
    assert feat.shape == exp.shape and torch.allclose(feat, exp, atol=1e-6)
    # save_feat alone: evaluated as usual, and an existing prediction is not loaded while features are being saved
    cfg, loader, model, info = make_scene(fx, 0, tmp_path, "Matterport3DGSDataset", save_feat=True)
    for _ in range(2):
        model.calls = 0
        m = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=loader)).test()
        assert model.calls == 2
    assert m["allAcc"] == fx["s0_k1_inter"].sum() / (fx["s0_k1_target"].sum() + 1e-10)
    sub = np.loadtxt(os.path.join(out, "submit", "scene0.txt"), dtype=np.int64)
    assert np.array_equal(sub, fx["s0_k1_table"])
    assert os.path.exists(os.path.join(out, "feat", "scene0_feat.pth"))


def test_tester_without_a_valid_gaussian_keeps_or_ignores(fx, tmp_path):
    """no valid point to vote with: pred unchanged without pc_coord, all ignore_index with it (no prediction exists for the query set)"""
    from scenesplat_amd.pointcept_api import TESTERS
    for s in (0, 1):
        cfg, loader, model, info = make_scene(fx, s, tmp_path, "ScanNetGSDataset")
        d = loader[0][0]
        d["origin_feat_mask"] = np.zeros_like(d["origin_feat_mask"])
        d.pop("origin_instance")
        d["name"] = f"novalid{s}"
        TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=loader)).test()
        saved = np.load(os.path.join(cfg["save_path"], "result_ScanNetGSDataset", f"novalid{s}_pred.npy"))
        if info["has_pc"]:
            assert saved.shape == (len(fx["s1_pc_coord"]),) and (saved == IGNORE).all()
        else:
            assert np.array_equal(saved, fx["s0_k1_base"])


# ---- a real model ---------------------------------------------------------------------------------------------------------
def test_tester_labels_equal_the_fragment_loop_on_a_real_model(tmp_path):
    """The tester and gpu_transforms.open_vocab_fragments run the same model and the same scan kernel on the same fragments and
    seeds, so the accumulated buffers are bit-equal and the labels must be equal: arg-max with a threshold, and top-3."""
    from scenesplat_amd.gpu_transforms import grid_sample_test, open_vocab_fragments
    from scenesplat_amd.pointcept_api import MODELS, TESTERS
    from scenesplat_amd.synthetic import room_chunk
    bb = dict(in_channels=11, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2), enc_depths=(1, 1, 1), enc_channels=(16, 32, 48),
              enc_num_head=(1, 2, 3), enc_patch_size=(64, 64, 16), dec_depths=(1, 1), dec_channels=(48, 32), dec_num_head=(1, 2), dec_patch_size=(64, 64),
              shuffle_orders=False)
    torch.manual_seed(0)
    model = MODELS.build(dict(type="LangPretrainer", backbone=dict(type="PT-v3m1", **bb), criteria=[])).cuda().eval()
    d = room_chunk(n_side=32, seed=2, lang_dim=0)
    g = torch.Generator().manual_seed(4)
    coord = torch.cat([d["coord"], d["coord"][:900] + 0.004, d["coord"][:300] + 0.008]).cuda()
    feat = torch.cat([d["feat"], d["feat"][:900] * 0.9, d["feat"][:300] * 1.1]).cuda()
    text = torch.nn.functional.normalize(torch.randn(20, 48, generator=g), dim=1)
    names = [f"c{i}" for i in range(20)]
    (tmp_path / "labels.txt").write_text("\n".join(names) + "\n")
    torch.save(text, tmp_path / "text.pt")
    frag = grid_sample_test(coord, 0.02)
    P, nvox = frag["index"].shape
    assert P >= 3
    off = torch.tensor([nvox], device="cuda")
    fragment_list = [dict(coord=coord[frag["index"][p]], grid_coord=frag["grid_coord"], index=frag["index"][p],
                          feat=feat[frag["index"][p]].contiguous(), offset=off) for p in range(P)]
    segment = torch.randint(-1, 20, (coord.shape[0],), generator=g)
    for dtype, thr in (("ScanNetGSDataset", 0.55), ("ScanNetPPGSDataset", 0.1)):
        cfg = dict(save_path=str(tmp_path / "out"), enable_amp=True, data=dict(test=dict(type=dtype, split="val")),
                   test=dict(type="ZeroShotSemSegTester", class_names=str(tmp_path / "labels.txt"), text_embeddings=str(tmp_path / "text.pt"),
                             confidence_threshold=thr))
        loader = [dict(fragment_list=fragment_list, segment=segment, name="room")]
        tester = TESTERS.build(dict(type="ZeroShotSemSegTester", cfg=cfg, model=model, test_loader=loader))
        torch.manual_seed(9)                              # (SerializedPooling shuffles its curves with the host RNG)
        metrics = tester.test()
        assert tester.model_calls == P and 0.0 <= metrics["allAcc"] <= 1.0
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lab, pred = open_vocab_fragments(model, dict(coord=coord, feat=feat), tester.text_embeddings, 0.02,
                                             topk=3 if "PP" in dtype else None, confidence_threshold=thr)
        out = os.path.join(cfg["save_path"], f"result_{dtype}")
        saved = np.load(os.path.join(out, "room_pred.npy"))
        if "PP" in dtype:
            sub = np.loadtxt(os.path.join(out, "submit", "room.txt"), delimiter=",", dtype=np.int64)
            assert np.array_equal(sub, lab.cpu().numpy()) and np.array_equal(saved, lab[:, 0].cpu().numpy())
        else:
            assert np.array_equal(saved, lab.cpu().numpy())
            assert (saved == IGNORE).any() and (saved >= 0).any()
        from scenesplat_amd import native as nv
        counts = nv.seg_iou(segment.cuda(), 20, IGNORE, pred=torch.from_numpy(saved).cuda().int()).cpu().numpy()
        assert metrics["allAcc"] == counts[0].sum() / (counts[2].sum() + 1e-10)
