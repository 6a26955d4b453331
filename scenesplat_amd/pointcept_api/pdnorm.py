"""Prompt-driven normalisation (PDNorm), the backbone half of Point Prompt Training.

Same registry name, constructor and state-dict keys as the reference
(pointcept/models/point_prompt_training/prompt_driven_normalization.py:8-53): one norm layer per training dataset
(`condition`) in `norm.{i}`, and with `adaptive` a `modulation = Sequential(SiLU, Linear(context_channels, 2C))` whose output,
driven by the per-dataset prompt vector (`context`, (1, context_channels)), scales and shifts the normalised features:
    shift, scale = modulation(context).chunk(2, dim=1);   feat = norm(feat) * (1 + scale) + shift.
One prompt per batch makes scale and shift per-channel constants, so they fold into the affine pair of the selected norm,
    gamma_eff = gamma * (1 + scale),   beta_eff = beta * (1 + scale) + shift        (gamma = 1, beta = 0 when affine=False),
and the fused norm kernels (csrc/norm.hip) run unchanged on gamma_eff / beta_eff.  The prompt arithmetic of ALL PDNorm layers of a
model is one grouped launch forward and one backward (csrc/pdnorm.hip, functional.pdnorm_modulation).

`decouple=False` cannot run in the reference (it stores the un-called norm_layer factory and then calls it on the features, which
constructs a module from a tensor): it is refused at construction instead of being given invented semantics.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as SF
from .registry import MODULES


class PointModule(nn.Module):
    """Marker base class, as pointcept/models/modules.py:8-14."""


class ResolvedNorm:
    """What a norm call site reads from a PDNorm layer during one forward: the effective affine pair, eps and the SELECTED
    condition's module (its buffers, mode and momentum).  Looks like the nn.BatchNorm1d / nn.LayerNorm it stands for to
    functional.batch_norm_act / ln_add_ln; calling it is the unfused path (channel counts the fused kernels do not take, post-norm)."""

    affine = True

    def __init__(self, weight, bias, mod):
        self.weight, self.bias, self.mod = weight, bias, mod
        self.is_bn = isinstance(mod, nn.BatchNorm1d)

    eps = property(lambda self: self.mod.eps)
    training = property(lambda self: self.mod.training)
    momentum = property(lambda self: self.mod.momentum)
    track_running_stats = property(lambda self: self.mod.track_running_stats)
    running_mean = property(lambda self: self.mod.running_mean)
    running_var = property(lambda self: self.mod.running_var)
    num_batches_tracked = property(lambda self: self.mod.num_batches_tracked)

    def __call__(self, x):
        m = self.mod
        if not self.is_bn:
            return F.layer_norm(x, m.normalized_shape, self.weight.to(x.dtype), self.bias.to(x.dtype), m.eps)
        if m.training and m.track_running_stats and m.num_batches_tracked is not None:       # nn.BatchNorm1d.forward's bookkeeping
            m.num_batches_tracked.add_(1)
        mom = m.momentum if m.momentum is not None else (1.0 / float(m.num_batches_tracked) if m.training and m.track_running_stats else 0.0)
        use_batch = m.training or m.running_mean is None
        return F.batch_norm(x, m.running_mean if (not m.training or m.track_running_stats) else None,
                            m.running_var if (not m.training or m.track_running_stats) else None, self.weight, self.bias, use_batch, mom, m.eps)


@MODULES.register_module()
class PDNorm(PointModule):
    def __init__(self, num_features, norm_layer, context_channels=256, conditions=("ScanNet", "S3DIS", "Structured3D"),
                 decouple=True, adaptive=False):
        super().__init__()
        if not decouple:
            raise ValueError("PDNorm(decouple=False) cannot run in the reference either: it keeps the un-called norm_layer factory as "
                             "self.norm and then calls it on the features, which constructs a module from a tensor.  Refused here "
                             "instead of inventing semantics: use decouple=True")
        self.conditions, self.decouple, self.adaptive = conditions, decouple, adaptive
        self.num_features, self.context_channels = num_features, context_channels
        self.norm = nn.ModuleList([norm_layer(num_features) for _ in conditions])
        for m in self.norm:
            if not isinstance(m, (nn.BatchNorm1d, nn.LayerNorm)):
                raise NotImplementedError(f"PDNorm: norm_layer must build nn.BatchNorm1d or nn.LayerNorm, got {type(m).__name__}")
        if self.adaptive:
            self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(context_channels, 2 * num_features, bias=True))
        if self.norm[0].weight is None:
            # affine-free norms: the fused kernels take gamma / beta tensors; constants that stay out of the state dict
            self.register_buffer("_ones", torch.ones(num_features), persistent=False)
            self.register_buffer("_zeros", torch.zeros(num_features), persistent=False)

    def index_of(self, condition):
        """Index of a condition given as the reference takes it: a string, or a list whose first entry counts."""
        if not isinstance(condition, str):
            condition = condition[0]
        assert condition in self.conditions, f"[PDNorm] condition {condition} not in {self.conditions}"
        return list(self.conditions).index(condition)

    def row(self, i):
        """(W, b, gamma | None, beta | None) of condition i: this layer's row of a grouped modulation launch."""
        lin, m = self.modulation[1], self.norm[i]
        return lin.weight, lin.bias, m.weight, m.bias

    def resolve_static(self, i):
        """Without `adaptive`: the selected module itself (its own parameters, no kernel and no copy), or its buffers under
        constant ones / zeros when it has no affine pair."""
        m = self.norm[i]
        return m if m.weight is not None else ResolvedNorm(self._ones, self._zeros, m)

    def forward(self, point):
        """The reference's call on a Point (feat, condition[, context]); inside PT-v3m1, where the model has resolved every layer
        for the forward already, the unfused call sites pass the feature tensor itself."""
        if torch.is_tensor(point):
            return resolved(self)(point)
        assert {"feat", "condition"}.issubset(point.keys()), f"feat and condition must be in point.keys(): {point.keys()}"
        i = self.index_of(point["condition"])
        if self.adaptive:
            assert "context" in point.keys()
            (g, b), = SF.pdnorm_modulation(SF.PDNormGroup([self.row(i)]), point["context"])
            norm = ResolvedNorm(g, b, self.norm[i])
        else:
            norm = self.resolve_static(i)
        x = point["feat"]
        fused = x.is_cuda and x.dim() == 2 and x.shape[1] % 4 == 0 and x.shape[1] <= 1024      # what the fused norm kernels take
        if isinstance(getattr(norm, "mod", norm), nn.BatchNorm1d):
            point["feat"] = SF.batch_norm_act(x, norm, False) if fused and norm.track_running_stats else norm(x)
        else:
            point["feat"] = SF.layer_norm(x, norm.weight, norm.bias, norm.eps) if fused else norm(x)
        return point


def resolved(m):
    """The norm a call site works with: m itself unless it is a PDNorm layer, then what the model resolved it to for this forward."""
    if not isinstance(m, PDNorm):
        return m
    r = m.__dict__.get("_resolved")
    if r is None:
        raise RuntimeError("PDNorm: not resolved for this forward (inside a model, PT-v3m1's forward selects the condition; on its "
                           "own, call the layer with a Point that has feat and condition)")
    return r


def pdnorm_layers(model):
    return [m for m in model.modules() if isinstance(m, PDNorm)]


def condition_key(backbone, host):
    """Part of a model's steady_key: the index of the batch's condition when the backbone has PDNorm layers (a captured step has the
    selected norms baked in), else nothing."""
    pds = backbone.__dict__.get("_pdnorm_list")
    if pds is None:
        pds = pdnorm_layers(backbone)
    if not pds or "condition" not in host:
        return ()
    return (pds[0].index_of(host["condition"]),)
