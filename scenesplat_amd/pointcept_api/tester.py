"""The open-vocabulary test stage (pointcept/engines/test.py:31-666): `TESTERS` holds `ZeroShotSemSegTester`, reached the way
tools/test.py reaches it,

    TESTERS.build(dict(type=cfg["test"]["type"], cfg=cfg, model=model, test_loader=loader)).test()

Per scene the prediction stays on the device from the fragments to the counts: fused scan + accumulate (csrc/scan.hip), top-k /
threshold / label mapping / pred[inverse] (ss_vocab_finish), kNN-grid neighbour voting + majority vote, per-instance voting
(ss_cluster_vote), intersection / union / target (ss_seg_iou).  It leaves the device once, for the files the reference writes:
`{name}_pred.npy`, `submit/{name}.txt`, `feat/{name}_feat.pth`, `eval_results.txt` -- and, with `save_pca` beside `save_feat`, the PCA
colours of the saved features, `feat/{name}_pca_colors.npy` (feature_pca.py; not in the reference's tester: its
tools/visualize_features_pca.py computes them from the saved file).

Differences from the reference, on purpose:
  * datasets are out of scope: `test_loader` is injected (any sized iterable of `[d]` or `d`, see `ZeroShotSemSegTester.test`);
  * a `*_pred.npy` found on disk is the scene's FINAL prediction (it was saved after the voting), so it is evaluated as it is
    and not voted on a second time; the ScanNet++ file holds the voted column, which is accepted 1-d or (m, 3);
  * `test()` returns the metrics on the main process (the reference only logs them).
The SemanticKITTI / NuScenes submission formats are not carried over."""
import copy
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from .. import native as nv
from .. import pointops
from .engine import create_ddp_model, get_world_size, is_main_process, synchronize
from .registry import MODELS, TESTERS

SCANNET_SUBMIT_TYPES = ("ScanNetDataset", "ScanNet200Dataset", "ScanNetGSDataset", "ScanNet200GSDataset")
CSV_SUBMIT_TYPES = ("HoliCityGSDataset", "Matterport3DGSDataset")


def merge_records(records):
    """Per-rank {scene name: counts} dicts -> one dict with ONE entry per scene name.  DistributedSampler pads the last round
    with repeated scenes; the reference's `final_record.update(r)` keeps one of the copies (test.py:553-559), which is why the
    counts must not be all-reduced."""
    merged = {}
    for r in records:
        for name, v in (r or {}).items():
            merged.setdefault(name, v)
    return merged


def gather_records(record):
    """This rank's {scene: counts} -> the merged record of all ranks on the main process, None elsewhere (test.py:549-559)."""
    records = [record]
    if get_world_size() > 1:
        synchronize()
        records = [None] * get_world_size()
        torch.distributed.all_gather_object(records, record)
    return merge_records(records) if is_main_process() else None


def final_metrics(record, keep_indices=None):
    """{scene: dict(intersection, union, target)} -> dict(mIoU, mAcc, allAcc, iou_class, accuracy_class [, fg_mIoU, fg_mAcc,
    fg_allAcc]) with the reference's masks (union != 0, target != 0) and 1e-10 terms (test.py:566-602).  keep_indices: the
    classes that are not excluded; None or empty = no foreground values."""
    inter = np.sum([np.asarray(v["intersection"]) for v in record.values()], axis=0)
    union = np.sum([np.asarray(v["union"]) for v in record.values()], axis=0)
    target = np.sum([np.asarray(v["target"]) for v in record.values()], axis=0)
    iou_class = inter / (union + 1e-10)
    acc_class = inter / (target + 1e-10)
    out = dict(mIoU=float(np.mean(iou_class[union != 0])), mAcc=float(np.mean(acc_class[target != 0])),
               allAcc=float(inter.sum() / (target.sum() + 1e-10)), iou_class=iou_class, accuracy_class=acc_class)
    if keep_indices is not None and len(keep_indices):
        keep = list(keep_indices)
        out["fg_mIoU"] = float(np.mean(iou_class[keep][union[keep] != 0]))
        out["fg_mAcc"] = float(np.mean(acc_class[keep][target[keep] != 0]))
        out["fg_allAcc"] = float(inter[keep].sum() / (target[keep].sum() + 1e-10))
    return out


def _dev(v, device, dtype=None):
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    t = t.to(device, non_blocking=True)
    return t if dtype is None else t.to(dtype)


class TesterBase:
    """engines/test.py:31-113.  cfg: mapping with save_path / model / weight / enable_amp / test / data["test"] [/ device]."""

    def __init__(self, cfg, model=None, test_loader=None, verbose=True, index=None, logger=None):
        self.cfg = cfg
        self.verbose = verbose
        self.logger = logger
        self.device = torch.device(cfg.get("device", "cuda"))
        if self.verbose:
            self.log(f"Save path: {cfg.get('save_path')}")
        self.model = self.build_model(index=index) if model is None else model
        if test_loader is None:
            raise ValueError("test_loader=None: datasets are outside this package; pass the loader (see ZeroShotSemSegTester.test)")
        self.test_loader = test_loader

    def log(self, msg):
        if self.logger is not None and is_main_process():
            self.logger(msg)

    def build_model(self, index=None):
        model = MODELS.build(self.cfg["model"])
        self.log(f"Num params: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
        model = create_ddp_model(model.to(self.device), broadcast_buffers=False,
                                 find_unused_parameters=self.cfg.get("find_unused_parameters", False))
        weight_path = self.cfg.get("weight")
        if not (weight_path and os.path.isfile(weight_path)):
            raise RuntimeError("=> No checkpoint found at '{}'".format(weight_path))
        checkpoint = torch.load(weight_path, map_location=self.device, weights_only=False)
        weight = OrderedDict()
        for key, value in checkpoint["state_dict"].items():
            if key.startswith("module."):
                if get_world_size() == 1:
                    key = key[7:]                      # module.xxx.xxx -> xxx.xxx
            elif get_world_size() > 1:
                key = "module." + key                  # xxx.xxx -> module.xxx.xxx
            weight[key] = value
        model.load_state_dict(weight, strict=True)
        self.log("=> Loaded weight '{}' (epoch {})".format(weight_path, checkpoint.get("epoch")))
        return model

    def test(self):
        raise NotImplementedError

    @staticmethod
    def collate_fn(batch):
        return batch


@TESTERS.register_module()
class ZeroShotSemSegTester(TesterBase):
    """engines/test.py:116-666.  Every option is overridden by `cfg["test"][...]`; with `index`, `cfg["test"]` and
    `cfg["data"]["test"]` are lists and entry `index` is used."""

    def __init__(self, cfg, model=None, test_loader=None, verbose=True, class_names=None, text_embeddings=None,
                 excluded_classes=None, enable_voting=False, vote_k=25, confidence_threshold=0.1, ignore_index=-1, save_feat=False,
                 skip_eval=False, pred_label_mapping=None, index=None, logger=None, save_pca=False):
        super().__init__(cfg, model, test_loader, verbose, index=index, logger=logger)
        if index is not None:                              # multi-dataset testing
            cfg = copy.copy(cfg)
            cfg["test"] = cfg["test"][index]
            cfg["data"] = dict(cfg["data"], test=cfg["data"]["test"][index])
        self.cfg = cfg
        tc = cfg["test"]
        self.enable_voting = tc.get("enable_voting", enable_voting)
        self.vote_k = tc.get("vote_k", vote_k)
        self.confidence_threshold = tc.get("confidence_threshold", confidence_threshold)
        self.save_feat = tc.get("save_feat", save_feat)
        self.save_pca = tc.get("save_pca", save_pca)       # with save_feat: feat/{name}_pca_colors.npy beside the features (feature_pca.py)
        self.skip_eval = tc.get("skip_eval", skip_eval)
        self.pred_label_mapping = tc.get("pred_label_mapping", pred_label_mapping)
        self.ignore_index = ignore_index
        class_names = tc.get("class_names", class_names)
        text_embeddings = tc.get("text_embeddings", text_embeddings)
        excluded_classes = tc.get("excluded_classes", excluded_classes)

        if class_names:
            with open(class_names, "r") as f:
                self.class_names = [line.strip() for line in f if line.strip()]
        else:
            self.class_names = []
        if text_embeddings:
            emb = torch.load(text_embeddings, weights_only=True).to(self.device)
            self.text_embeddings = F.normalize(emb.float(), p=2, dim=1)
        else:
            self.text_embeddings = None

        self.excluded_indices, self.keep_indices = [], []
        if excluded_classes:
            self.excluded_indices = [i for i, name in enumerate(self.class_names) if name in excluded_classes]
            self.keep_indices = [i for i in range(len(self.class_names)) if i not in self.excluded_indices]
        self.num_keep_classes = len(self.keep_indices)
        self.num_classes = len(self.class_names)
        if self.pred_label_mapping is None and not self.skip_eval:
            assert self.text_embeddings is not None and self.num_classes == self.text_embeddings.size(0), \
                "Mismatch in class names and text embeddings"
        self.model_calls = 0

    # ---- pieces of test() ------------------------------------------------------------------------------------------------
    @property
    def data_type(self):
        return self.cfg["data"]["test"]["type"]

    def _forward(self, input_dict, amp):
        self.model_calls += 1
        with torch.no_grad(), torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=amp):
            return self.model(input_dict, chunk_size=600000)["point_feat"]["feat"]

    def _infer(self, data_dict, fragment_list, num_points, feat_save_path, tag):
        """The fragment loop (test.py:300-394) -> (m, k) int32 labels on the device, or None with skip_eval."""
        dev = self.device
        amp = bool(self.cfg.get("enable_amp")) and dev.type == "cuda"
        text = None if self.skip_eval else self.text_embeddings.to(torch.bfloat16).contiguous()
        pred = None if self.skip_eval else torch.zeros((num_points, text.shape[0]), dtype=torch.float32, device=dev)
        feats = counts = None
        for i, frag in enumerate(fragment_list):
            inp = {k: (_dev(v, dev) if isinstance(v, (torch.Tensor, np.ndarray)) else v) for k, v in frag.items()}
            idx = inp["index"].reshape(-1)
            f = self._forward(inp, amp)
            if not self.skip_eval:
                nv.feat_text_scan(f, text, want_max=False, idx=idx.to(torch.int32).contiguous(), pred_accum=pred)
            if self.save_feat:
                if feats is None:
                    feats = torch.zeros((num_points, f.shape[1]), dtype=torch.float32, device=dev)
                    counts = torch.zeros(num_points, dtype=torch.float32, device=dev)
                feats.index_add_(0, idx.long(), f.float())
                counts.index_add_(0, idx.long(), torch.ones(idx.numel(), dtype=torch.float32, device=dev))
            self.log(f"Test: {tag}, Fragment batch: {i + 1}/{len(fragment_list)}")
        inverse = None
        if "origin_segment" in data_dict:
            assert "inverse" in data_dict, "Inverse mapping is required to map pred to full origin_coord"
            inverse = _dev(data_dict["inverse"], dev, torch.int64).contiguous()
        if self.save_feat and feats is not None:
            seen = counts > 0                              # mean over the fragments that saw a point
            feats[seen] /= counts[seen].unsqueeze(1)
            final = F.normalize(feats, p=2, dim=1)
            if inverse is not None:
                final = final[inverse]
            if self.save_pca:                              # on the device tensor itself: the colours the tool gives on the saved file
                from .feature_pca import pca_colors
                pca_path = feat_save_path[:-len("_feat.pth")] + "_pca_colors.npy"
                np.save(pca_path, pca_colors(final)["colors"].cpu().numpy())
                self.log(f"Saved PCA colors to {pca_path}")
            torch.save(final.cpu(), feat_save_path)
            self.log(f"Saved pred feature with shape {tuple(final.shape)} to {feat_save_path}")
        if self.skip_eval:
            return None
        lut = None
        if self.pred_label_mapping is not None:
            lut = pointops.label_map_lut(self.pred_label_mapping, pred.shape[1], self.ignore_index, device=dev)
        k = 3 if "ScanNetPP" in self.data_type else 1
        return nv.vocab_finish(pred, k=k, threshold=self.confidence_threshold, ignore_index=self.ignore_index, inverse=inverse, lut=lut)

    def _write_submit(self, save_path, name, table):
        """table (m, k) int32 numpy, after the mapping and before the voting (test.py:396-429)"""
        os.makedirs(os.path.join(save_path, "submit"), exist_ok=True)
        path = os.path.join(save_path, "submit", f"{name}.txt")
        t = self.data_type
        if t in SCANNET_SUBMIT_TYPES:
            class2id = getattr(getattr(self.test_loader, "dataset", None), "class2id", None)
            if class2id is not None:
                np.savetxt(path, np.asarray(class2id)[table[:, 0]].reshape([-1, 1]), fmt="%d")
        elif "ScanNetPP" in t:
            np.savetxt(path, table.astype(np.int32), delimiter=",", fmt="%d")
        elif t in CSV_SUBMIT_TYPES:
            np.savetxt(path, table[:, 0].astype(np.int32), delimiter=",", fmt="%d")

    def _vote(self, pred, data_dict):
        """test.py:470-502 on the device: neighbour voting over the valid Gaussians, then per-instance voting."""
        dev = self.device
        has_pc = "pc_coord" in data_dict and "pc_segment" in data_dict
        if has_pc or "origin_coord" in data_dict:
            coords = _dev(data_dict["origin_coord"], dev, torch.float32)
            mask = data_dict.get("origin_feat_mask", None)
            valid = torch.ones(coords.shape[0], dtype=torch.bool, device=dev) if mask is None else _dev(mask, dev).bool()
            query = _dev(data_dict["pc_coord"], dev, torch.float32) if has_pc else None
            if bool(valid.any()):
                pred = pointops.neighbor_voting(coords, pred, valid, self.vote_k, self.ignore_index, self.num_classes, query_coords=query)
            elif has_pc:                                   # nothing to vote with: the query set has no prediction at all
                pred = torch.full((query.shape[0],), self.ignore_index, dtype=torch.int32, device=dev)
        else:
            self.log("Neighbor voting requires 'origin_coord (3dgs)' or 'pc_coord (pc)' in data_dict, skipped..")
        if "origin_instance" in data_dict:
            inst = _dev(data_dict["origin_instance"], dev).reshape(-1)
            if inst.shape == pred.shape:
                pred = pointops.clustering_voting(pred, inst, self.ignore_index, self.num_classes)
            else:
                self.log("clustering_voting: prediction and instance arrays must have the same shape")
        return pred

    # ---- the stage -------------------------------------------------------------------------------------------------------
    def test(self):
        """Loader contract (datasets/defaults.py:136-183): each item is `[d]` or `d`; entries are numpy arrays or CPU / GPU tensors.
        d: fragment_list [, segment, name, origin_segment + inverse, origin_coord, origin_feat_mask, origin_instance,
        pc_coord + pc_segment]; a fragment is a Collect output: coord, grid_coord, index, feat, offset [, condition].
        -> the metrics dict of `final_metrics` on the main process (None elsewhere and with skip_eval)."""
        bs = getattr(self.test_loader, "batch_size", 1)
        assert bs in (1, None), "ZeroShotSemSegTester: batch size 1"
        dtest = self.cfg["data"]["test"]
        self.log(">>>>>>>>>>>>>> ZeroShotSemSegTester Start Evaluation >>>>>>>>>>>>>")
        self.log(f"Testing on {dtest.get('split')} split of {self.data_type}")
        if self.skip_eval:
            self.log("ZeroShotSemSegTester skipping evaluation...")
        else:
            self.log(f"ZeroShotSemSegTester loaded text embeddings with shape {tuple(self.text_embeddings.shape)}")
        if self.enable_voting:
            self.log("Neighbor voting enabled with k={}".format(self.vote_k))
        if hasattr(self.model, "eval"):
            self.model.eval()
        save_path = os.path.join(self.cfg["save_path"], f"result_{self.data_type}")
        if is_main_process():
            os.makedirs(os.path.join(save_path, "submit"), exist_ok=True)
            if self.save_feat:
                os.makedirs(os.path.join(save_path, "feat"), exist_ok=True)
        synchronize()
        dev = self.device
        record = {}
        total = len(self.test_loader)
        for idx, item in enumerate(self.test_loader):
            data_dict = dict(item[0] if isinstance(item, (list, tuple)) else item)
            fragment_list = data_dict.pop("fragment_list")
            segment = data_dict.pop("segment", None)
            name = data_dict.pop("name", "default")
            pred_save_path = os.path.join(save_path, f"{name}_pred.npy")
            feat_save_path = os.path.join(save_path, "feat", f"{name}_feat.pth") if self.save_feat else None
            has_pc = "pc_coord" in data_dict and "pc_segment" in data_dict
            loaded = os.path.isfile(pred_save_path) and not self.save_feat and "pc_coord" not in data_dict
            table = None
            if loaded:
                self.log(f"{name}: loaded existing pred")
                pred_np = np.load(pred_save_path)
                pred = torch.from_numpy(pred_np[:, 0] if pred_np.ndim > 1 else pred_np).to(dev, torch.int32).contiguous()
            else:
                if segment is not None:
                    num_points = int(np.prod(tuple(segment.shape)))
                else:
                    num_points = int(data_dict["coord"].shape[0])
                table = self._infer(data_dict, fragment_list, num_points, feat_save_path, f"{idx + 1}/{total}-{name}")
                if table is None:                          # skip_eval
                    continue
                pred = table[:, 0].contiguous()
                if self.enable_voting:
                    pred = self._vote(pred, data_dict)
            if self.skip_eval:
                continue
            if has_pc:
                segment = data_dict["pc_segment"]
            elif "origin_segment" in data_dict:
                segment = data_dict["origin_segment"]
            if segment is None:
                raise ValueError(f"{name}: no segment to evaluate against")
            target = _dev(segment, dev, torch.int64).reshape(-1).contiguous()
            if target.shape[0] != pred.shape[0]:
                raise ValueError(f"{name}: prediction has {pred.shape[0]} rows, the segment {target.shape[0]}")
            counts = nv.seg_iou(target, self.num_classes, self.ignore_index, pred=pred.to(torch.int32).contiguous())
            # the scene's one trip off the device: the labels before the voting (submission), after it (prediction file), the counts
            parts = [pred.to(torch.int64), counts.reshape(-1)] + ([] if loaded else [table.reshape(-1).to(torch.int64)])
            host = torch.cat(parts).cpu().numpy()
            m_rows, n_counts = pred.shape[0], 3 * self.num_classes
            if not loaded:
                self._write_submit(save_path, name, host[m_rows + n_counts:].reshape(tuple(table.shape)))
                np.save(pred_save_path, host[:m_rows])
            inter, union, tgt = host[m_rows:m_rows + n_counts].reshape(3, self.num_classes)
            record[name] = dict(intersection=inter, union=union, target=tgt)
            iou = float(np.mean((inter / (union + 1e-10))[union != 0])) if (union != 0).any() else float("nan")
            acc = float(inter.sum() / (tgt.sum() + 1e-10))
            self.log(f"Test: {name} [{idx + 1}/{total}]-{target.shape[0]} Accuracy {acc:.4f} mIoU {iou:.4f}")

        if self.skip_eval:
            self.log("<<<<<<<<<<<<<<<<< Tester End, Skipped Evaluation <<<<<<<<<<<<<<<<<")
            return None
        self.log("Syncing ...")
        final_record = gather_records(record)
        if final_record is None:
            return None
        metrics = final_metrics(final_record, self.keep_indices if self.excluded_indices else None)
        self._write_results(metrics, save_path)
        return metrics

    def _write_results(self, m, save_path):
        """eval_results.txt in the reference's format (test.py:623-664) + the same lines to the logger"""
        lines = ["Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}".format(m["mIoU"], m["mAcc"], m["allAcc"])]
        if self.excluded_indices:
            lines.append("Foreground Val result (excluding {} classes): mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}".format(
                len(self.excluded_indices), m["fg_mIoU"], m["fg_mAcc"], m["fg_allAcc"]))
        for ln in lines:
            self.log(ln)
        lines += ["", "Per-class results:"]
        iou, acc = m["iou_class"], m["accuracy_class"]
        for i in range(self.num_classes):
            if self.class_names:
                lines.append("Class_{}-{} Result: iou/accuracy {:.4f}/{:.4f}".format(i, self.class_names[i], iou[i], acc[i]))
            else:
                lines.append("Class_{} iou/accuracy {:.4f}/{:.4f}".format(i, iou[i], acc[i]))
        if self.excluded_indices:
            lines += ["", "Excluded classes:"]
            for i in self.excluded_indices:
                lines.append(f"Class_{i}-{self.class_names[i]}" if "names" in self.cfg["data"] else f"Class_{i}")
        with open(os.path.join(save_path, "eval_results.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        self.log("<<<<<<<<<<<<<<<<< End Evaluation <<<<<<<<<<<<<<<<<")
