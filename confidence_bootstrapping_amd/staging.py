"""One staging buffer for the ragged-batch front doors (NoiseTransform.apply_noise_batch, sampling.randomize_position_batch,
evaluation.pose_metrics_batch): every host array of a launch goes into ONE pinned buffer of 4-byte words, is uploaded once, and the
kernel gets a pointer into the device copy per array.

`ptr` is the int32 prefix sum the CSR-like descriptions are made of, `layout` is the pure-numpy packing (no GPU), `upload` is the GPU
half.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch


def ptr(sizes) -> np.ndarray:
    """sizes [n] -> int32 [n + 1] prefix sum starting at 0"""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int32)


def layout(arrays):
    """`arrays`: ordered mapping name -> array or None.  -> (words int32 [total], offsets {name: word offset}).
    Every array is flattened and viewed as 4-byte words.  The parts of 8-byte items (fp64, uint64 pointer tables) are placed before all
    parts of 4-byte items, each group in the mapping's order, so every part starts at a multiple of its item size -- on the device as
    well, where the buffer's base is aligned far beyond 8 bytes.  A part that is None or empty gets no words and no offset."""
    flat = {}
    for name, a in arrays.items():
        if a is None or np.size(a) == 0:
            continue
        a = np.ascontiguousarray(a).reshape(-1)
        if a.dtype.itemsize not in (4, 8):
            raise TypeError(f"{name}: items of {a.dtype.itemsize} bytes ({a.dtype}); the staging buffer takes 4- and 8-byte items")
        flat[name] = a
    order = sorted(flat, key=lambda name: -flat[name].dtype.itemsize)      # stable: 8-byte parts first, the mapping's order within
    parts = [flat[name].view(np.int32) for name in order]
    offsets = dict(zip(order, ptr([len(p) for p in parts])[:-1].tolist()))
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


def upload(arrays, dev):
    """layout(arrays) into one pinned int32 tensor, one non_blocking upload to `dev`.  -> (staged, at): the device tensor (keep it alive
    until the kernel that reads it is enqueued on the current stream) and at(name) = c_void_p of the part on the device, None for a part
    that is absent or empty."""
    words, offsets = layout(arrays)
    with torch.cuda.device(dev):
        host = torch.empty(len(words), dtype=torch.int32, pin_memory=True)
        host.numpy()[:] = words
        staged = host.to(dev, non_blocking=True)
    base = staged.data_ptr()
    return staged, lambda name: C.c_void_p(base + 4 * offsets[name]) if name in offsets else None
