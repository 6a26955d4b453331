"""Inputs shared by tests/test_hip_rows_edges.py (GPU) and tests/test_rows_host.py (CPU): CSR layouts, feature rows and the list of
row widths with the kernel form each one takes in csrc/rows.hip.  Everything is built on the CPU from seeded generators; nothing
here touches the library under test."""
import functools
import types

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

N_SEG = 301                                   # n_seg * chunks is no multiple of the 256-thread block for any width below
SEG_LENGTHS = (0, 1, 2, 7, 8, 9, 64, 257)
LONG_LEN, LONG_AT, ONE_AT = 5000, 77, 200     # one long segment, and a 1-row segment at a known place

# ---- row widths: (dtype, C, alignment of the base pointer in bytes) ---------------------------------------------------------
F32_WIDTHS = (1, 3, 5, 4, 8, 36)
BF16_WIDTHS = (1, 3, 2, 4, 6, 8, 24, 72)
ALIGNED = [(F32, C, 16) for C in F32_WIDTHS] + [(BF16, C, 16) for C in BF16_WIDTHS]
MISALIGNED = [(F32, 8, 4), (BF16, 8, 2)]      # base[1 : 1 + n * C].view(n, C) of a flat allocation: one element past 16-byte alignment


def row_bytes(dtype, C):
    return C * (4 if dtype == F32 else 2)


def gather_form(dtype, C, align):
    """lane width in bytes ss_gather_rows / ss_scatter_rows move a row with"""
    rb = row_bytes(dtype, C)
    for lane in (16, 4):
        if rb % lane == 0 and align % lane == 0:
            return lane
    return 2


def reduce_form(dtype, C, align):
    """'v16' (one thread per 16-byte chunk) or 'scalar' (one element per thread): ss_segment_reduce / _bcast / ss_gather_add_rows"""
    return "v16" if row_bytes(dtype, C) % 16 == 0 and align % 16 == 0 else "scalar"


def case_id(case):
    dtype, C, align = case
    return "%s-C%d%s" % ("f32" if dtype == F32 else "bf16", C, "" if align == 16 else "-off%d" % align)


# ---- CSR layouts ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_csr(permute=True, empty=True, seed=0, n_seg=N_SEG, long_len=LONG_LEN):
    """A `level`-like object: idx_ptr (n_seg + 1) int32, indices (n) int32 source row of every CSR position (None = identity),
    cluster (n) int32 segment of every source row, n = n_seg; plus lens / seg_of_pos (int64) and n_rows.  Lengths are drawn from
    SEG_LENGTHS (without 0 when empty=False) and one segment has long_len rows; with empty=True the first, the middle and the
    last segment are empty."""
    g = torch.Generator().manual_seed(1000 + seed)
    pool = torch.tensor(SEG_LENGTHS if empty else SEG_LENGTHS[1:])
    lens = pool[torch.randint(0, len(pool), (n_seg,), generator=g)]
    lens[3:3 + len(pool)] = pool                           # every length occurs
    if empty:
        lens[0] = 0; lens[n_seg // 2] = 0; lens[n_seg - 1] = 0
    lens[LONG_AT] = long_len
    lens[ONE_AT] = 1
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    n_rows = int(ptr[-1])
    seg_of_pos = torch.repeat_interleave(torch.arange(n_seg), lens)
    if permute:
        indices = torch.randperm(n_rows, generator=g)
        cluster = torch.empty(n_rows, dtype=torch.int64)
        cluster[indices] = seg_of_pos
    else:
        indices, cluster = None, seg_of_pos.clone()
    return types.SimpleNamespace(n=n_seg, n_rows=n_rows, lens=lens, ptr=ptr, seg_of_pos=seg_of_pos,
                                 idx_ptr=ptr.to(torch.int32), cluster=cluster.to(torch.int32),
                                 indices=None if indices is None else indices.to(torch.int32))


def rows_in_csr_order(csr):
    """(n_rows) int64: the source row at every CSR position"""
    return torch.arange(csr.n_rows) if csr.indices is None else csr.indices.long()


def features(n, C, dtype, seed, mean=1.0, std=0.1):
    """(n, C) rows of mean + std * randn in `dtype`: the non-zero mean makes a low-precision or truncated accumulation visible"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * C + (1 if dtype == BF16 else 0))
    return (mean + std * torch.randn(n, C, generator=g)).to(dtype)


def cotangent(n, C, dtype, seed):
    g = torch.Generator().manual_seed(104729 * seed + 17 * C + (3 if dtype == BF16 else 2))
    return torch.randn(n, C, generator=g).to(dtype)


# ---- duplicate-voxel runs ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_runs(seed=0, n_single=450):
    """(sorted_keys (n) int64, order (n) int32, key_of_row (n) int64) with a run of 3 at the very first sorted positions, a run of
    40, runs of 2 in between and a run of 2 that ends at the last sorted position; order is the stable argsort, so every run lists
    its rows ascending and its first entry is the winner."""
    g = torch.Generator().manual_seed(2000 + seed)
    counts = [3] + [1] * (n_single // 2) + [40] + [2] * 30 + [1] * (n_single - n_single // 2) + [2]
    keys = torch.repeat_interleave(torch.arange(len(counts)) * 5 + 2, torch.tensor(counts))
    key_of_row = keys[torch.randperm(len(keys), generator=g)]
    sorted_keys, order = torch.sort(key_of_row, stable=True)
    assert sorted_keys[0] == sorted_keys[2] and sorted_keys[-1] == sorted_keys[-2] and sorted_keys[-2] != sorted_keys[-3]
    return sorted_keys.contiguous(), order.to(torch.int32).contiguous(), key_of_row
