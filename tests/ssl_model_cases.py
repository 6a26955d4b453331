"""Fixtures and numpy / fp64 restatements shared by the SimDINO model tests and tests/golden/make_golden_ssl_model.py.

Nothing here runs project code: the restatements are checked against the reference's own outputs (golden (i) and (iii)) by
tests/test_ssl_model_host.py and then serve the GPU tests at sizes that have no golden."""
import numpy as np
import torch

TINY = dict(in_channels=11, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2),
            enc_depths=(1, 1, 2), enc_channels=(16, 32, 64), enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 16),
            dec_depths=(2, 1), dec_channels=(48, 32), dec_num_head=(1, 2), dec_patch_size=(64, 64))
TINY_EXTRA = dict(drop_path=0.0, shuffle_orders=False, enable_flash=False, upcast_attention=False, upcast_softmax=False, enable_rpe=False,
                  pooling_reduce="max")
MASK_CASES = (("patch", 0.2), ("patch", 2.0), ("patch", 3.0), ("splats", 0.2))
MASK_SIZES = (1, 255, 257)
RATIO = (0.1, 0.5)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def cloud(n, side, seed):
    """n distinct voxels of a side^3 cube, in a seeded random order -> (n, 3) int64"""
    g = np.random.default_rng(seed)
    cells = g.choice(side ** 3, size=n, replace=False)
    return np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).astype(np.int64)


def mask_batch(sizes=MASK_SIZES, side=12, seed=3):
    """-> grid_coord (n, 3) int64, offset (B) int64 for samples of the given sizes (each its own distinct voxels)"""
    gcs = [cloud(n, side, seed + 17 * i) for i, n in enumerate(sizes)]
    return np.concatenate(gcs), np.cumsum(sizes).astype(np.int64)


def view(sizes, channels, side, seed):
    """One view of the whole-model fixture: fp16-representable features"""
    gc, offset = mask_batch(sizes, side, seed)
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(len(gc), channels, generator=g).to(torch.float16).to(torch.float32)
    return dict(grid_coord=torch.from_numpy(gc), offset=torch.from_numpy(offset), feat=feat,
                coord=(torch.from_numpy(gc).float() * 0.0625))


def model_inputs(local_crop_num=3):
    """B = 2, about 1,500 points per global view and 600 per local crop"""
    d = {}
    views = [("global_crop0", (700, 811), 14, 40), ("global_crop1", (803, 690), 14, 41)]
    views += [(f"local_crop{i}", (290 + 7 * i, 311 - 5 * i), 10, 50 + i) for i in range(local_crop_num)]
    for name, sizes, side, seed in views:
        for k, v in view(sizes, TINY["in_channels"], side, seed).items():
            d[f"{name}_{k}"] = v
    return d


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def backbone_state(seed):
    from oracle import ptv3 as optv3
    sd = optv3.init_state_dict(TINY, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    sd["mask_token"] = torch.randn(1, TINY["enc_channels"][0], generator=g) * 0.1
    return sd


def head_state(shapes, seed):
    """shapes: ordered {key: shape} of the head parameters -> seeded values (weights ~ N(0, 1 / fan_in), biases and LayerNorm small)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        shape = tuple(shape)
        if len(shape) == 2:
            sd[k] = torch.randn(*shape, generator=g) * shape[1] ** -0.5
        elif k.endswith("1.weight"):                  # the LayerNorm of the MAE head
            sd[k] = 1 + 0.1 * torch.randn(*shape, generator=g)
        else:
            sd[k] = 0.05 * torch.randn(*shape, generator=g)
    return sd


def model_state(model):
    """Seeded state of a whole DefaultContrastiverSimDinoV2 on the TINY backbone (teacher and student differ)"""
    sd = {}
    for prefix, seed in (("backbone_teacher.", 21), ("backbone_student.", 22)):
        sd.update({prefix + k: v for k, v in backbone_state(seed).items()})
    rest = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith("backbone_")}
    sd.update(head_state(rest, 23))
    return sd


# ---- mask generator restated ------------------------------------------------------------------------------------------------------------
def patch_ids(grid_coord, offset, mask_grid_size):
    """-> (patch_id (n), patch_count (B)): per sample, the rank of floor(fp32(grid_coord) / fp32(size)) among the occupied cells, ordered
    by x + y * ex + z * ex * ey after the per-sample minimum is subtracted (torch_cluster's grid index, from its documented formula)."""
    gc = np.asarray(grid_coord)
    ids, counts, begin = np.zeros(len(gc), np.int64), [], 0
    for end in np.asarray(offset).tolist():
        cell = np.floor(gc[begin:end].astype(np.float32) / np.float32(mask_grid_size)).astype(np.int64)
        if len(cell):
            cell -= cell.min(0)
            ext = cell.max(0) + 1
            key = cell[:, 0] + cell[:, 1] * ext[0] + cell[:, 2] * ext[0] * ext[1]
            uniq, inv = np.unique(key, return_inverse=True)
            ids[begin:end] = inv
            counts.append(len(uniq))
        else:
            counts.append(0)
        begin = end
    return ids, np.asarray(counts, np.int64)


def draw_masks(offset, counts, mask_type, probability=0.5, ratio=RATIO):
    """The reference's draws from the CPU generators (torch.randperm(B); per flagged sample torch.randperm + np.random.uniform)
    -> per sample (flagged, perm | None, rate | None); `counts` = patches per sample (`patch`) or tokens per sample (`splats`)."""
    B = len(offset)
    n_flag = int(np.ceil(B * probability))
    flagged = torch.zeros(B, dtype=torch.long)
    flagged[:n_flag] = 1
    flagged = flagged[torch.randperm(B)].tolist()
    draws = []
    for i in range(B):
        if not flagged[i]:
            draws.append((0, None, None))
        elif mask_type == "patch":
            perm = torch.randperm(int(counts[i])).numpy()
            draws.append((1, perm, float(np.random.uniform(*ratio))))
        else:
            rate = float(np.random.uniform(*ratio))
            draws.append((1, torch.randperm(int(counts[i])).numpy(), rate))
    return draws


def apply_draws(offset, ids, draws, mask_type):
    """-> (mask (n) bool, weights (masked rows) fp16) from recorded draws"""
    offset = np.asarray(offset).tolist()
    n = offset[-1] if offset else 0
    mask, w, begin = np.zeros(n, bool), np.ones(n, np.float16), 0
    for i, end in enumerate(offset):
        flagged, perm, rate = draws[i]
        if flagged:
            if mask_type == "patch":
                k = int(len(perm) * rate)
                chosen = np.zeros(len(perm), bool)
                chosen[perm[:k]] = True
                mask[begin:end] = chosen[ids[begin:end]]
                if k:
                    w[begin:end] = (torch.ones(1, dtype=torch.float16) * (1 / k)).numpy()[0]
            else:
                num = torch.tensor(end - begin) * rate
                k = int(num)
                mask[begin:end] = perm < k
                w[begin:end] = (torch.ones(1, dtype=torch.float16) * (1 / num)).numpy()[0]
        begin = end
    return mask, w[mask]


# ---- losses restated in fp64 ---------------------------------------------------------------------------------------------------------
def mcr_loss64(student, teacher, expa_type=1, eps=0.05, coeff=0.1, no_diag=True, world=1):
    """student (crops, B, D), teacher (2, B, D), already normalised -> dict(loss, comp_loss, global_comp_loss, expa_loss)"""
    s, t = np.asarray(student, np.float64), np.asarray(teacher, np.float64)
    ns, nt = len(s), len(t)
    sim = (t[:, None] * s[None]).sum(-1).mean(-1)
    if no_diag:
        for i in range(min(nt, ns)):
            sim[i, i] = 0.0
    comp = sim.sum() / (nt * ns - min(nt, ns))
    gcomp = sim[:, :nt].sum() / nt
    feat = s[:nt] if expa_type == 0 else (s[:nt] + t) / 2
    views, m, p = feat.shape
    scalar = p / (m * world * eps)
    total = 0.0
    for i in range(views):
        total += 0.5 * np.linalg.slogdet(np.eye(p) + scalar * feat[i].T @ feat[i])[1]
    expa = total / views * ((p + world * m) / (p * world * m))
    return dict(loss=-coeff * comp - expa, comp_loss=comp, global_comp_loss=gcomp, expa_loss=expa)


def cosine_patch64(student, teacher, weight, view_nums=1, eps=1e-8):
    s, t = np.asarray(student, np.float64), np.asarray(teacher, np.float64)
    cos = (s * t).sum(-1) / (np.maximum(np.linalg.norm(s, axis=-1), eps) * np.maximum(np.linalg.norm(t, axis=-1), eps))
    return -(cos * np.asarray(weight, np.float64)).sum() / view_nums
