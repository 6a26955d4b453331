"""SimDINO self-supervised pretraining on the HIP hot path: the `PT-v3m1-simdino` backbone, the projection heads, the coding-rate and
cosine patch losses and `DefaultContrastiverSimDinoV2` (reference: pointcept/models/simdinov2.py,
point_transformer_v3_ssl/point_transformer_v3m1_ssl.py:532-751, losses/sim_dino_clstoken_loss.py, losses/sim_ibot_patch_loss.py).

Same registry names, constructor arguments, output dict and state-dict keys as the reference, so its configs build and its checkpoints
load.  What runs differently:

  * the mask generator partitions every sample into patches ON the device (csrc/ssl_model.hip) and reads two small vectors per global
    view on the host (the patch counts, the number of masked rows) where the reference loops over the samples with several reads each.
    The random draws stay on the CPU generators in the reference's order (torch.randperm, np.random.uniform), so a seeded run selects
    the same patches;
  * the masked rows travel as ONE ascending int32 index: the mask token is a select kernel, and feat[mask], the MAE targets and the
    patch features are row gathers through that index (boolean indexing would sync each time);
  * update_teacher is one grouped launch over all parameter pairs;
  * the loss arithmetic (covariance, Cholesky, cosine similarity) runs in fp32 with autocast off: [views, B, 256] and 256 x 256
    matrices, torch ops.

One stated deviation: when global view 0 has no masked row the reference's indicator indexes an empty tensor and raises; here the
indicator is 0 and that view adds nothing to the patch loss."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as SF
from .. import native as nv
from .ptv3 import PointTransformerV3, _lin
from .registry import MODELS
from .structure import Point


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


# ---- backbone ---------------------------------------------------------------------------------------------------------------------
@MODELS.register_module("PT-v3m1-simdino")
class PointTransformerV3_SIMDINO(PointTransformerV3):
    """PT-v3m1 with a learnable mask token behind the embedding, `pooling_reduce` for the encoder's poolings, and a forward that
    returns (encoder point, decoder point | None).  The decoder and the mask token exist only with do_mask."""

    def __init__(self, *args, do_mask=False, pooling_reduce="max", **kwargs):
        names = ("in_channels", "order", "stride", "enc_depths", "enc_channels")
        kwargs.update(zip(names, args))
        if len(args) > len(names):
            raise TypeError("PT-v3m1-simdino: pass the arguments behind enc_channels by keyword")
        kwargs.pop("cls_mode", None)        # (the reference builds the decoder by do_mask alone)
        super().__init__(cls_mode=not do_mask, **kwargs)
        self.do_mask = bool(do_mask)
        if pooling_reduce not in ("mean", "sum", "min", "max"):
            raise ValueError(f"unknown pooling_reduce {pooling_reduce!r}")
        for s in range(1, self.num_stages):
            getattr(self.enc, f"enc{s}").down.reduce = pooling_reduce
        if self.do_mask:
            self.mask_token = nn.Parameter(torch.zeros(1, self.enc_channels[0]))
            nn.init.trunc_normal_(self.mask_token, std=0.02)

    def _embedded(self, x, plan):
        mask = self.__dict__.get("_mask")
        if mask is None:
            return x
        if not self.do_mask:
            raise RuntimeError("PT-v3m1-simdino: a mask needs do_mask=True (there is no mask token)")
        if mask.shape[0] != x.shape[0]:
            raise RuntimeError("mask: one entry per point")
        return SF.mask_token(x, mask, self.mask_token)

    def forward(self, data_dict, mask=None, return_dec=False, perms=None):
        if return_dec and not self.do_mask:
            raise RuntimeError("PT-v3m1-simdino: return_dec needs do_mask=True (there is no decoder)")
        point, feat, plan = self._begin_forward(data_dict, perms, with_dec=bool(return_dec))
        pds = self._pdnorm()
        if pds:
            self._resolve_pdnorm(point)
        self.__dict__["_mask"] = mask
        try:
            x, skips = self._forward_encoder(feat, plan)
            last = plan.levels[-1]
            enc_offset = torch.tensor(last.offsets[1:], dtype=torch.int64).to(feat.device, non_blocking=True)
            point_enc = Point(feat=x, offset=enc_offset, plan=plan, level=self.num_stages - 1)
            point_dec = None
            if return_dec:
                point_dec = Point(feat=self._forward_decoder(point, x, skips, plan), plan=plan, level=0)
                for k in ("coord", "grid_coord", "offset"):
                    if dict.__contains__(point, k):
                        point_dec[k] = point[k]
            return point_enc, point_dec
        finally:
            self.__dict__["_mask"] = None
            for m in pds:
                m.__dict__.pop("_resolved", None)


class _SampleSegments:
    """The samples of a level as CSR segments, in the shape SF.segment_mean reads a pooled level."""

    def __init__(self, level):
        self.n = len(level.offsets) - 1
        self.indices = None
        self.cluster = level.batch
        self.idx_ptr = torch.tensor(level.offsets, dtype=torch.int32).to(level.device, non_blocking=True)


def sample_mean(point):
    """Mean of point.feat over every sample (torch_scatter.segment_csr(reduce="mean") over the padded offset) -> (B, C)."""
    level = point["plan"].levels[point["level"]]
    return SF.segment_mean(point["feat"], _SampleSegments(level), mean=True)


# ---- heads and losses ---------------------------------------------------------------------------------------------------------------
def _build_mlp(nlayers, in_dim, bottleneck_dim, hidden_dim=None, use_bn=False, bias=True):
    if nlayers == 1:
        return nn.Linear(in_dim, bottleneck_dim, bias=bias)
    dims = [in_dim] + [hidden_dim] * (nlayers - 1)
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers.append(nn.Linear(a, b, bias=bias))
        if use_bn:
            layers.append(nn.BatchNorm1d(b, eps=1e-3))
        layers.append(nn.GELU())
    layers.append(nn.Linear(hidden_dim, bottleneck_dim, bias=bias))
    return nn.Sequential(*layers)


class DINOHead(nn.Module):
    """MLP + L2 normalisation (eps 1e-4).  Only the form the model builds: remove_last_layer=True (no weight-normed prototype layer)."""

    def __init__(self, in_dim, out_dim, use_bn=False, nlayers=3, hidden_dim=2048, bottleneck_dim=256, mlp_bias=True, normalize=True,
                 remove_last_layer=False):
        super().__init__()
        if not remove_last_layer:
            raise NotImplementedError("DINOHead: only remove_last_layer=True is supported (the SimDINO model builds no prototype layer)")
        self.mlp = _build_mlp(max(nlayers, 1), in_dim, bottleneck_dim, hidden_dim=hidden_dim, use_bn=use_bn, bias=mlp_bias)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.normalize, self.remove_last_layer = normalize, remove_last_layer

    def forward(self, x):
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1])
        mods = [self.mlp] if isinstance(self.mlp, nn.Linear) else list(self.mlp)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear) and i + 1 < len(mods) and type(mods[i + 1]) is nn.GELU:
                x = SF.linear_gelu(x, m.weight, m.bias)
                i += 2
            else:
                x = _lin(m, x) if isinstance(m, nn.Linear) else m(x)
                i += 1
        with torch.autocast("cuda", enabled=False):
            x = x.float()
            if self.normalize:
                x = F.normalize(x, dim=-1, p=2, eps=1e-4)
        return x.reshape(*lead, x.shape[-1])


def _half_logdet(X):
    return torch.linalg.cholesky_ex(X)[0].diagonal().log().sum()


class MCRLoss(nn.Module):
    """Coding-rate loss of SimDINO: -coeff * compression - expansion.  reduce_cov=0 only (the covariance is not all-reduced); the world
    size enters the expansion's scalar and balancing factor."""

    def __init__(self, out_dim, expa_type=0, reduce_cov=0, eps=0.05, coeff=1, center=False, **kwargs):
        super().__init__()
        if reduce_cov != 0:
            raise NotImplementedError("MCRLoss: reduce_cov=0 only")
        if expa_type not in (0, 1):
            raise ValueError("MCRLoss: expa_type 0 or 1")
        if center:
            raise NotImplementedError("MCRLoss: centering is not part of the SimDINO model")
        self.out_dim, self.expa_type, self.reduce_cov, self.eps, self.coeff = out_dim, expa_type, reduce_cov, eps, coeff

    @torch.autocast("cuda", enabled=False)
    def forward(self, student_feat_list, teacher_feat_list, no_diag=True, normalized=True):
        student = torch.stack([t.float() for t in student_feat_list])       # (crops, B, D)
        teacher = torch.stack([t.float() for t in teacher_feat_list])       # (2, B, D)
        if not normalized:
            student = F.normalize(student, p=2, dim=-1, eps=1e-4)
            teacher = F.normalize(teacher, p=2, dim=-1, eps=1e-4)
        comp, global_comp = self.calc_compression(student, teacher, no_diag)
        nt = teacher.shape[0]
        expa_feat = student[:nt] if self.expa_type == 0 else (student[:nt] + teacher) / 2
        expa = self.calc_expansion(expa_feat)
        loss = -self.coeff * comp - expa
        return loss, {"loss": loss.detach(), "comp_loss": comp.detach(), "global_comp_loss": global_comp.detach(),
                      "expa_loss": expa.detach()}

    def calc_compression(self, student, teacher, no_diag=True):
        ns, nt = student.shape[0], teacher.shape[0]
        sim = (teacher.unsqueeze(1) * student.unsqueeze(0)).sum(-1).mean(-1)       # (nt, ns) mean cosine similarity of every pair
        if no_diag:                                                                # a student and the teacher of the SAME view: dropped
            sim = sim * (1.0 - torch.eye(nt, ns, dtype=sim.dtype, device=sim.device))
        comp = sim.sum() / (nt * ns - min(nt, ns))
        global_comp = sim[:, :nt].detach().sum().div_(nt)
        return comp, global_comp

    def calc_expansion(self, feat):
        views, m, p = feat.shape
        cov = torch.einsum("nbc,nbd->ncd", feat, feat)
        N = _world_size()
        scalar = p / (m * N * self.eps)
        eye = torch.eye(p, device=feat.device)
        loss = sum(_half_logdet(eye + scalar * cov[i]) for i in range(views))
        loss = loss / views
        return loss * ((p + N * m) / (p * N * m))


class CosinePatchLoss(nn.Module):
    def __init__(self, patch_out_dim, center=False, center_momentum=0.9, **kwargs):
        super().__init__()
        if center:
            raise NotImplementedError("CosinePatchLoss: centering is not part of the SimDINO model")
        self.patch_out_dim = patch_out_dim

    @torch.autocast("cuda", enabled=False)
    def forward_masked(self, student_patch_tokens_masked, teacher_patch_tokens_masked, masks_weight, view_nums):
        cos = F.cosine_similarity(teacher_patch_tokens_masked.float(), student_patch_tokens_masked.float(), dim=-1)
        comp = -(cos * masks_weight).sum() / view_nums
        return comp, {"comp_loss": comp.detach()}


# ---- model ------------------------------------------------------------------------------------------------------------------------------
@MODELS.register_module()
class DefaultContrastiverSimDinoV2(nn.Module):
    def __init__(self, backbone_out_channels, backbone=None, local_crop_num=3, do_ema=True, do_ibot=True, enable_mae_loss=False,
                 mask_ratio_min_max=(0.1, 0.5), mask_sample_probability=0.5, dino_weight=1.0, ibot_weight=1.0, mae_weight=1.0,
                 mask_grid_size=0.2, mask_type="patch", code_weight=None):
        super().__init__()
        # code_weight: two of the three shipped ssl-pretrain configs pass it; nothing reads it (the reference's constructor as shipped
        # does not even take it).  Accepted so that those configs build, and ignored.
        assert mask_type in ("patch", "splats"), f"mask_type should be 'patch' or 'splats', but got {mask_type}"
        if do_ibot:
            assert do_ema, "do_ibot needs do_ema: without it there is only the student"
        self.do_ema, self.do_ibot, self.enable_mae_loss = do_ema, do_ibot, enable_mae_loss
        self.dino_weight, self.ibot_weight, self.mae_weight = dino_weight, ibot_weight, mae_weight
        self.local_crop_num = local_crop_num
        self.mask_ratio_min_max = tuple(mask_ratio_min_max)
        self.mask_sample_probability = mask_sample_probability
        self.mask_grid_size, self.mask_type = mask_grid_size, mask_type
        backbone = dict(backbone)
        backbone["do_mask"] = True
        if do_ema:
            self.backbone_teacher = MODELS.build(backbone)
            for p in self.backbone_teacher.parameters():
                p.requires_grad = False
        self.backbone_student = MODELS.build(backbone)
        # (read from the built backbone, so that a config may leave the backbone's defaults out)
        bb = self.backbone_student
        self.num_layers = bb.num_stages
        in_channels, enc_out, dec_out = bb.embedding.in_channels, bb.enc_channels[-1], bb.dec_channels_[0]
        if enable_mae_loss:
            self.using_coord = in_channels == 14
            self.mae_head = nn.Sequential(nn.Linear(dec_out, 32), nn.LayerNorm(32), nn.ReLU(inplace=True),
                                          nn.Linear(32, 11))
            for m in self.mae_head.modules():
                if isinstance(m, nn.Linear):
                    nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self.dino_head = DINOHead(in_dim=enc_out, out_dim=256, hidden_dim=2048, bottleneck_dim=256, nlayers=3,
                                  normalize=True, remove_last_layer=True)
        self.dino_loss = MCRLoss(out_dim=256, expa_type=1, reduce_cov=0, eps=0.05, eps_end=-1, coeff=0.1)
        self.ibot_head = DINOHead(in_dim=dec_out, out_dim=32, hidden_dim=256, bottleneck_dim=32, nlayers=3,
                                  normalize=True, remove_last_layer=True)
        self.ibot_patch_loss = CosinePatchLoss(patch_out_dim=32)

    # -- EMA teacher ------------------------------------------------------------------------------------------------------------------
    def _ema_pairs(self):
        """(teacher tensors, student tensors): the student's trainable parameters except the mask token, matched by name.  Buffers
        (BatchNorm running statistics) are not averaged: the teacher keeps its own."""
        pairs = self.__dict__.get("_ema_pair_cache")
        names = [n for n, p in self.backbone_student.named_parameters() if p.requires_grad and "mask_token" not in n]
        if pairs is None or pairs[0] != names:
            teacher = dict(self.backbone_teacher.named_parameters())
            student = dict(self.backbone_student.named_parameters())
            pairs = self.__dict__["_ema_pair_cache"] = (names, [teacher[n] for n in names], [student[n] for n in names])
        return pairs[1], pairs[2]

    @torch.no_grad()
    def update_teacher(self, m=0.999):
        """teacher = m * teacher + (1 - m) * student in ONE grouped launch (csrc/ssl_model.hip)."""
        teacher, student = self._ema_pairs()
        nv.ema_group(teacher, student, float(m), cache=self.__dict__.setdefault("_ema_launch_cache", {}))
        # the kernel wrote through raw pointers: the version-stamped bf16 shadows (functional._stamp) key on the counters
        torch.autograd.graph.increment_version(teacher)

    # -- masks ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def mask_generator(self, offset, view_origin_coord=None, return_index=False):
        """-> (mask (n) bool, weights (masked rows) fp16[, index (masked rows) int32 ascending]).  Two device -> host reads: the patch
        counts (token counts in `splats` mode) and the number of masked rows.  CPU-generator draws in the reference's order:
        torch.randperm(B) for the flagged samples, then per flagged sample torch.randperm(patches) and np.random.uniform(lo, hi)."""
        dev = offset.device
        B = offset.numel()
        off32 = offset.to(torch.int32).contiguous()
        n_flag = int(np.ceil(B * self.mask_sample_probability))
        flagged = torch.zeros(B, dtype=torch.long)
        flagged[:n_flag] = 1
        flagged = flagged[torch.randperm(B)].tolist()
        lo, hi = self.mask_ratio_min_max
        weights = torch.ones(B, dtype=torch.float16)
        if self.mask_type == "patch":
            gc = view_origin_coord.to(torch.int32).contiguous()
            n = gc.shape[0]
            patch_id, patch_start, counts = nv.mask_patches(gc, off32, self.mask_grid_size)
            counts = counts.tolist()                                               # host read 1
            if counts[B]:
                raise RuntimeError("mask generator: a mask cell lies outside [0, 2^17) on some axis")
            starts = np.concatenate([[0], np.cumsum(counts[:B])])
            selected = torch.zeros(max(int(starts[-1]), 1), dtype=torch.uint8)
            for i in range(B):
                if not flagged[i]:
                    continue
                perm = torch.randperm(counts[i])
                rate = np.random.uniform(lo, hi)
                k = int(counts[i] * rate)
                if k > 0:                                                          # (k == 0: no masked row, the weight is never read)
                    selected[int(starts[i]) + perm[:k]] = 1
                    weights[i] = (torch.ones(1, dtype=torch.float16) * (1 / k))[0]
            mask, index, weight, count = nv.mask_select(selected.to(dev), patch_id, patch_start, off32, weights.to(dev), n)
        else:
            ends = offset.tolist()                                                 # host read 1
            n = int(ends[-1]) if B else 0
            selected = torch.zeros(max(n, 1), dtype=torch.uint8)
            begin = 0
            for i in range(B):
                tokens = int(ends[i]) - begin
                if flagged[i]:
                    rate = np.random.uniform(lo, hi)
                    num = torch.tensor(tokens) * rate                              # fp32, as the reference's 0-d tensor times a float
                    k = int(num)
                    perm = torch.randperm(tokens)
                    selected[begin:begin + tokens] = (perm < k).to(torch.uint8)    # == (arange < k)[perm]
                    weights[i] = (torch.ones(1, dtype=torch.float16) * (1 / num))[0]
                begin = int(ends[i])
            mask, index, weight, count = nv.mask_select(selected[:n].to(dev) if n else selected.to(dev)[:0], None, None, off32,
                                                        weights.to(dev), n)
        m = int(count.item())                                                      # host read 2
        out = (mask, weight[:m])
        return out + (index[:m],) if return_index else out

    # -- forward ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _view(input_dict, name, half=False):
        d = dict(coord=input_dict[f"{name}_coord"], feat=input_dict[f"{name}_feat"], offset=input_dict[f"{name}_offset"],
                 grid_coord=input_dict[f"{name}_grid_coord"])
        if half:                # the reference feeds the local crops as .half(): the values are rounded through fp16
            d["coord"], d["feat"] = d["coord"].half().float(), d["feat"].half().float()
        return d

    def forward(self, input_dict, teacher_temp, visualize=False):
        if not self.training:
            raise ValueError("Not implemented yet")
        if visualize:
            raise NotImplementedError("visualize is outside this port")
        g0, g1 = self._view(input_dict, "global_crop0"), self._view(input_dict, "global_crop1")
        locals_ = [self._view(input_dict, f"local_crop{i}", half=True) for i in range(self.local_crop_num)]
        # CPU-generator order: mask of view 0, mask of view 1, teacher view 0 / 1, student view 0 / 1, student local crops
        mask0, w0, idx0 = self.mask_generator(g0["offset"], g0["grid_coord"], return_index=True)
        mask1, w1, idx1 = self.mask_generator(g1["offset"], g1["grid_coord"], return_index=True)
        if self.enable_mae_loss:
            with torch.no_grad():
                gt0 = SF.gather_rows(g0["feat"].float().contiguous(), idx0)
                if self.using_coord:
                    gt0 = gt0[:, 3:]
        out, loss_dict = {}, {}
        if self.do_ema:
            with torch.no_grad():
                t_enc0, t_dec0 = self.backbone_teacher(Point(g0), return_dec=True)
                t_enc1, t_dec1 = self.backbone_teacher(Point(g1), return_dec=True)
                t_pool = torch.stack([sample_mean(t_enc0), sample_mean(t_enc1)], dim=1)        # (B, 2, C)
                t_patch0, t_patch1 = SF.gather_rows(t_dec0.feat, idx0), SF.gather_rows(t_dec1.feat, idx1)
        s_enc0, s_dec0 = self.backbone_student(Point(g0), mask=mask0, return_dec=True)
        s_enc1, s_dec1 = self.backbone_student(Point(g1), mask=mask1, return_dec=True)
        s_pool = torch.stack([sample_mean(s_enc0), sample_mean(s_enc1)], dim=1)
        s_patch0, s_patch1 = SF.gather_rows(s_dec0.feat, idx0), SF.gather_rows(s_dec1.feat, idx1)
        local_pools = []
        for view in locals_:
            enc, _ = self.backbone_student(Point(view), return_dec=False)
            local_pools.append(sample_mean(enc))
        if self.do_ema:
            loss_dict.update(self.calculate_sim_dino_loss_pool(t_pool, s_pool, local_pools))
        if self.do_ibot:
            loss_dict.update(self.calculate_sim_dino_loss_patch(t_patch0, t_patch1, s_patch0, s_patch1, teacher_temp, w0, w1))
            if t_patch0.shape[0]:
                a, b = t_patch0[0].float(), t_patch0[-1].float()
                out["teacher_ibot_global_indicator"] = F.cosine_similarity(a, b, dim=-1).mean()
            else:
                out["teacher_ibot_global_indicator"] = t_patch0.new_zeros((), dtype=torch.float32)
        if self.enable_mae_loss:
            h = self.mae_head
            pred = _lin(h[3], h[2](h[1](_lin(h[0], s_patch0))))
            with torch.autocast("cuda", enabled=False):
                loss_dict["global_mae_loss"] = F.mse_loss(pred.float(), gt0.detach()) if gt0.shape[0] else pred.float().sum() * 0.0
        loss = 0.0
        if self.do_ema:
            loss = loss + self.dino_weight * loss_dict["sim_dino_crops_loss"]
        if self.do_ibot:
            loss = loss + self.ibot_weight * loss_dict["sim_ibot_patch_loss"]
        if self.enable_mae_loss:
            loss = loss + self.mae_weight * loss_dict["global_mae_loss"]
        out["loss"] = loss
        out.update(loss_dict)
        return out

    def calculate_sim_dino_loss_pool(self, teacher_pool, student_pool, student_local_pools):
        """teacher_pool / student_pool (B, 2, C), student_local_pools: local_crop_num x (B, C)."""
        def crops(x):          # head, then crop-major rows
            x = self.dino_head(x).permute(1, 0, 2)
            return x.reshape(-1, x.shape[-1])
        t = crops(teacher_pool).detach()
        s = crops(student_pool)
        sl = crops(torch.stack(student_local_pools, dim=1))
        loss, parts = self.dino_loss(tuple(s.chunk(2)) + tuple(sl.chunk(self.local_crop_num)), tuple(t.chunk(2)), no_diag=True)
        d = {"dino_mcr_" + k: v for k, v in parts.items()}
        d["sim_dino_crops_loss"] = loss
        return d

    def calculate_sim_dino_loss_patch(self, t0, t1, s0, s1, teacher_temp, global_mask_weight_0=None, global_mask_weight_1=None, view_num=1):
        t = self.ibot_head(torch.cat([t0, t1], dim=0)).detach()
        s = self.ibot_head(torch.cat([s0, s1], dim=0))
        w = torch.cat([global_mask_weight_0, global_mask_weight_1], dim=0)
        loss, parts = self.ibot_patch_loss.forward_masked(s, t, masks_weight=w, view_nums=view_num)
        d = {"ibot_" + k: v for k, v in parts.items()}
        d["sim_ibot_patch_loss"] = loss
        return d


class CosineScheduler:
    """Per-step value table: `freeze_iters` zeros, a linear warm-up from start_warmup_value to base_value, then half a cosine from
    base_value to final_value; final_value after the table ends (pointcept/engines/pretrain.py:363-392, same numpy arithmetic)."""

    def __init__(self, base_value, final_value, total_iters, warmup_iters=0, start_warmup_value=0, freeze_iters=0):
        self.final_value, self.total_iters = final_value, total_iters
        rest = np.arange(total_iters - warmup_iters - freeze_iters)
        cosine = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * rest / len(rest)))
        self.schedule = np.concatenate((np.zeros(freeze_iters), np.linspace(start_warmup_value, base_value, warmup_iters), cosine))
        self.current_iter = 0
        assert len(self.schedule) == self.total_iters

    def step(self):
        if self.current_iter >= self.total_iters:
            return self.final_value
        value = self.schedule[self.current_iter]
        self.current_iter += 1
        return value
