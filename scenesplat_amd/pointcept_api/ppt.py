"""Point Prompt Training with decoupled segmentation heads: ``PPT-v1m2``.

Registry name, constructor kwargs, forward contract and state-dict keys follow the reference
(pointcept/models/point_prompt_training/point_prompt_training_v1m2_decoupled.py:15-76): a learned prompt vector per training
dataset (`embedding_table`), handed to the backbone's PDNorm layers as data_dict["context"], and one Linear head per dataset.
Only the "PT-v3m1" backbone exists here; the reference's assertion on the backbone's type is kept as it is.
"""
import torch
import torch.nn as nn

from .lang import build_criteria
from .pdnorm import condition_key
from .registry import MODELS
from .structure import Point


@MODELS.register_module("PPT-v1m2")
class PointPromptTraining(nn.Module):
    def __init__(self, backbone=None, criteria=None, backbone_out_channels=96, context_channels=256,
                 conditions=("Structured3D", "ScanNet", "S3DIS"), num_classes=(25, 20, 13), backbone_mode=False):
        super().__init__()
        assert len(conditions) == len(num_classes)
        assert backbone["type"] in ["SpUNet-v1m3", "PT-v2m3", "PT-v3m1"]
        self.backbone = MODELS.build(backbone)
        self.criteria = build_criteria(criteria)
        self.conditions = conditions
        self.embedding_table = nn.Embedding(len(conditions), context_channels)
        self.backbone_mode = backbone_mode
        self.seg_heads = nn.ModuleList([nn.Linear(backbone_out_channels, num_cls) for num_cls in num_classes])

    def steady_key(self, host):
        """The host-side decisions of a step (steady-state replay): the batch's condition selects the prompt, the head and -- inside
        the backbone -- the norm layers, all baked into a captured step."""
        if "condition" not in host:
            return ()
        return (list(self.conditions).index(host["condition"][0]),) + condition_key(self.backbone, host)

    def forward(self, data_dict):
        condition = data_dict["condition"][0]
        assert condition in self.conditions
        i = list(self.conditions).index(condition)
        # the embedding lookup of one known row is a slice: no index tensor is built on the host (a captured step stays capturable)
        # and the rows of the other conditions receive exactly zero gradient, as from nn.Embedding
        data_dict["context"] = self.embedding_table.weight[i:i + 1]
        point = self.backbone(data_dict)
        feat = point["feat"] if isinstance(point, Point) else point
        if self.backbone_mode:
            return feat                  # PPT as a multi-dataset backbone
        seg_head = self.seg_heads[i]
        if not torch.is_autocast_enabled() and feat.dtype != seg_head.weight.dtype:
            feat = feat.to(seg_head.weight.dtype)
        seg_logits = seg_head(feat)
        if self.training:
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]))
        if "segment" in data_dict.keys():
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)
