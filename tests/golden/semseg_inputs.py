"""Seeded inputs of the semantic-segmentation fixture (tests/golden/semseg.npz), shared by its generator
(make_golden_semseg.py) and the tests, so that the fixture holds outputs only: logits, labels, point clouds and weights are
regenerated from these seeds (as prod_inputs.py does for the language fixtures), and semseg.npz stores a checksum of each input
that the tests compare before they use it."""
import numpy as np
import torch

MODEL_SEED, HEAD_SEED, INPUT_SEED, POOL_SEED = 21, 22, 23, 77
DLOGIT_ROWS = 128          # rows of d logits stored per loss case (all rows of the smaller cases)
EVAL_ROWS = 1024           # rows of the eval logits stored in full (arg-max and top-2 margin are stored for every row)
GRAD_ELEMS = 4096          # leading elements of each stored parameter gradient
GRAD_KEYS = ("seg_head.weight", "seg_head.bias", "backbone.embedding.stem.conv.weight", "backbone.enc.enc2.block1.attn.qkv.weight",
             "backbone.dec.dec0.block1.mlp.0.fc2.weight", "backbone.dec.dec0.up.proj_skip.0.weight")
SCANNET_BACKBONE = dict(in_channels=14, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
                        enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
                        enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16),
                        dec_patch_size=(1024,) * 4, mlp_ratio=4)


def loss_cases():
    """[(name, logits (n, C) f32, labels (n) int64, class_seen | None)]"""
    cases = []
    for C, n, present in ((20, 3000, 15), (100, 2000, 60), (200, 2500, 120)):
        g = torch.Generator().manual_seed(1000 + C)
        logits = torch.randn(n, C, generator=g) * 2.0
        cls = torch.randperm(C, generator=g)[:present]
        labels = cls[torch.randint(0, present, (n,), generator=g)]
        labels[torch.rand(n, generator=g) < 0.1] = -1
        cases.append((f"c{C}", logits, labels, None))
    g = torch.Generator().manual_seed(2000)
    logits = torch.randn(2000, 20, generator=g)
    labels = torch.randint(0, 12, (2000,), generator=g)
    labels[torch.rand(2000, generator=g) < 0.2] = -1
    cases.append(("seen", logits, labels, [0, 2, 3, 5, 7, 11, 13]))      # 13 is seen but absent
    g = torch.Generator().manual_seed(2001)
    cases.append(("n1", torch.randn(1, 20, generator=g), torch.tensor([4]), None))
    # ties: 6 distinct lattice probability rows, each repeated, logits = log p (softmax gives p back up to rounding)
    g = torch.Generator().manual_seed(2002)
    base = torch.randint(1, 5, (6, 8), generator=g).float()
    base = base / base.sum(1, keepdim=True)
    pick = torch.randint(0, 6, (600,), generator=g)
    labels = torch.randint(0, 5, (600,), generator=g)
    labels[::7] = -1
    cases.append(("ties", torch.log(base[pick]), labels, None))
    return cases


def dlogit_rows(name, n):
    """The rows whose d logits the fixture stores (sorted)."""
    if n <= DLOGIT_ROWS:
        return np.arange(n)
    g = torch.Generator().manual_seed(4000 + n)
    return np.sort(torch.randperm(n, generator=g)[:DLOGIT_ROWS].numpy())


def room_gc(n_side=64, seed=4):
    """room: floor n x n + two walls n x (n*72//256), rows shuffled (= scenesplat_amd.synthetic.room_grid)."""
    h = max(2, n_side * 72 // 256)
    xs, ys = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    floor = np.stack([xs.ravel(), ys.ravel(), np.zeros(n_side * n_side, int)], 1)
    yy, zz = np.meshgrid(np.arange(n_side), np.arange(1, h + 1), indexing="ij")
    wa = np.stack([np.zeros(yy.size, int), yy.ravel(), zz.ravel()], 1)
    wb = np.stack([np.full(yy.size, n_side - 1), yy.ravel(), zz.ravel()], 1)
    gc = np.concatenate([floor, wa, wb]).astype(np.int64)
    return gc[torch.randperm(len(gc), generator=torch.Generator().manual_seed(seed)).numpy()]


def model_inputs():
    """The 6,400-Gaussian model input (CPU tensors): coord, grid_coord, feat (14), offset (two batch elements), segment."""
    gc = torch.from_numpy(room_gc())
    n = len(gc)
    g = torch.Generator().manual_seed(INPUT_SEED)
    feat = torch.randn(n, 14, generator=g)
    segment = torch.randint(0, 20, (n,), generator=g)
    segment[torch.rand(n, generator=g) < 0.1] = -1
    return dict(coord=gc.float() * 0.02, grid_coord=gc, feat=feat, offset=torch.tensor([n // 2, n]), segment=segment)


def model_state(num_classes=20):
    """DefaultSegmentorV2 state dict: the oracle's seeded PT-v3m1 initialiser for the backbone, a seeded Linear head."""
    from oracle import ptv3 as optv3
    sd = {"backbone." + k: v for k, v in optv3.init_state_dict(SCANNET_BACKBONE, seed=MODEL_SEED).items()}
    gh = torch.Generator().manual_seed(HEAD_SEED)
    sd["seg_head.weight"] = torch.randn(num_classes, 64, generator=gh) * 64 ** -0.5
    sd["seg_head.bias"] = torch.randn(num_classes, generator=gh) * 0.02
    return sd


def eval_rows(n):
    g = torch.Generator().manual_seed(4100)
    return np.sort(torch.randperm(n, generator=g)[:EVAL_ROWS].numpy())


def iou_inputs():
    """(pred, target) int64 of the intersection_and_union_gpu case: 20 classes, 15 % ignored targets."""
    g = torch.Generator().manual_seed(3000)
    tgt = torch.randint(0, 20, (10000,), generator=g)
    tgt[torch.rand(10000, generator=g) < 0.15] = -1
    pred = torch.where(torch.rand(10000, generator=g) < 0.6, tgt.clamp(min=0), torch.randint(0, 20, (10000,), generator=g))
    pred[:50] = 19
    return pred, tgt


def checksum(*tensors):
    """float64 [sum, sum of |x|] per tensor (numpy's pairwise summation: the same on every machine)."""
    out = []
    for t in tensors:
        a = t.detach().cpu().numpy().astype(np.float64).ravel()
        out += [a.sum(), np.abs(a).sum()]
    return np.array(out)
