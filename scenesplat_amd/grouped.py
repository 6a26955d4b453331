"""Host side of the grouped launches: many small problems in ONE launch (the contract is stated in include/scenesplat_hip.h).

A wrapper builds `desc`, one row of int64 words per problem, and `starts(counts)`, the first workgroup of every problem; `launch`
uploads both through pinned memory without a stream sync and calls the entry point.  The subtle part is the upload: the pinned
sources must outlive their asynchronous copies, a thread whose stream is capturing must not query events, and inside a captured
step ONE copy of a pool (DescriptorPool) serves every table of the step."""
import ctypes
import itertools
import threading

import numpy as np
import torch

from . import _lib

_GROUP_KEEP = []      # (event, pinned sources, device copies) of grouped launches whose upload may still be in flight
_GROUP_LOCK = threading.Lock()
_NP2T = {"int64": torch.int64, "int32": torch.int32}
CAPTURE_POOL = None   # a DescriptorPool while a capture is open (steady_state.py sets and clears it)


class DescriptorPool:
    """Pinned host memory for the descriptors of grouped launches issued INSIDE a hipGraph capture (steady_state.py).
    The captured host-to-device copy re-reads its source on every replay, so the source must live, unchanged, as long as
    the graph does; and pinned memory cannot be allocated while a stream is capturing.  The pool is allocated before the
    capture begins and owned by the captured step.

    open_capture(device), called right after capture_begin, records ONE copy of the whole pool into a device mirror: a copy
    node reads its source at REPLAY time, so the tables that the step writes into the pool later in the capture are all
    uploaded by that single node (34 separate 5-us copies per step before)."""

    def __init__(self, nbytes=1 << 20):
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8).pin_memory()
        self.off = 0
        self.device_side = []
        self.mirror = None

    def open_capture(self, device):
        self.mirror = torch.empty(self.buf.numel(), dtype=torch.uint8, device=device)
        self.mirror.copy_(self.buf, non_blocking=True)

    def take(self, arr):
        """-> (pinned host view holding arr, device view of the same bytes in the mirror | None)"""
        nb = arr.nbytes
        off = (self.off + 63) & ~63
        if off + nb > self.buf.numel():
            raise RuntimeError("descriptor pool of the captured step is full")
        self.off = off + nb
        view = self.buf[off:off + nb]
        view.numpy()[:] = arr.reshape(-1).view("uint8")
        host = view.view(_NP2T[arr.dtype.name]).view(arr.shape)
        dev = None if self.mirror is None else self.mirror[off:off + nb].view(_NP2T[arr.dtype.name]).view(arr.shape)
        return host, dev


def starts(counts):
    """Workgroup counts of the problems (a list, or a numpy column computed from the descriptor rows) -> the first workgroup of
    each, and the launch's total last."""
    out = [0, *itertools.accumulate(counts.tolist() if isinstance(counts, np.ndarray) else counts)]
    if out[-1] >= 2 ** 31:
        raise RuntimeError("grouped launch: more than 2^31 workgroups")
    return out


def _upload_descriptors(desc, wg_start, dev):
    """(descriptor rows, first-workgroup table) -> device tensors through pinned memory, without a stream sync."""
    wg_start = np.asarray(wg_start, dtype=np.int32)
    if CAPTURE_POOL is not None and torch.cuda.is_current_stream_capturing():
        (d_host, d_dev), (s_host, s_dev) = CAPTURE_POOL.take(desc), CAPTURE_POOL.take(wg_start)
        if d_dev is None or d_dev.device != torch.device(dev):
            d_dev, s_dev = d_host.to(dev, non_blocking=True), s_host.to(dev, non_blocking=True)
            CAPTURE_POOL.device_side.append((d_dev, s_dev))
        return d_dev, s_dev
    d_host, s_host = torch.from_numpy(desc).pin_memory(), torch.from_numpy(wg_start).pin_memory()
    d_dev, s_dev = d_host.to(dev, non_blocking=True), s_host.to(dev, non_blocking=True)
    # the pinned sources must outlive their asynchronous copies: each upload is kept until an event recorded behind it has passed
    # (a thread whose stream is capturing must not query events: it only appends)
    ev = None
    with _GROUP_LOCK:                         # (grouped launches may come from more than one host thread)
        if not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event(); ev.record()
            while _GROUP_KEEP and _GROUP_KEEP[0][0] is not None and _GROUP_KEEP[0][0].query():
                _GROUP_KEEP.pop(0)
        _GROUP_KEEP.append((ev, d_host, s_host, d_dev, s_dev))
        if len(_GROUP_KEEP) > 4096:           # (never reached in practice: a stalled stream would have to hold thousands of launches)
            _GROUP_KEEP[0][0].synchronize() if _GROUP_KEEP[0][0] is not None else None
            _GROUP_KEEP.pop(0)
    return d_dev, s_dev


def relaunch(symbol, tables, total, *extra):
    """lib().<symbol>(desc, wg_start, nprob, total, *extra, stream) on device tables that an earlier `launch` returned."""
    d_dev, s_dev = tables
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    status = getattr(_lib.load(), symbol)(ctypes.c_void_p(d_dev.data_ptr()), ctypes.c_void_p(s_dev.data_ptr()), d_dev.shape[0], int(total),
                                          *extra, stream)
    _lib.check(status, symbol)


def launch(symbol, desc, wg_start, dev, *extra):
    """Upload desc (nprob rows) and wg_start (nprob + 1, from `starts`) and run the entry point `symbol` on the current stream.
    -> the device tables (a caller whose problems stay put may `relaunch` them)."""
    tables = _upload_descriptors(desc, wg_start, dev)
    relaunch(symbol, tables, wg_start[-1], *extra)
    return tables
