"""Model of ops.reuse_chunks (kernel K12), straight from its rule: record i puts the `len` source
bytes at dst[off:off + len], their Xet chunk hash at hashes[index] and len at sizes[index]; every
other byte and row keeps its value.  Shared by the CPU and GPU tests."""
from __future__ import annotations

import numpy as np

from zest_amd import _core

SENTINEL = 0xA5


def expect(chunks, dst_offs, index, dst_before: np.ndarray, hashes_before: np.ndarray, sizes_before: np.ndarray):
    """chunks: the source bytes of every record.  Returns (dst, hashes, sizes) after the call."""
    dst, hashes, sizes = dst_before.copy(), hashes_before.copy(), sizes_before.copy()
    for data, off, row in zip(chunks, dst_offs, index):
        data = bytes(data)
        dst[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        hashes[row] = np.frombuffer(_core.chunk_hash(data), dtype=np.uint8)
        sizes[row] = len(data)
    return dst, hashes, sizes


def layout(lens, dst_mis, rng, gap: int = 48):
    """Output offsets for records of `lens` bytes, in a shuffled order, record i at an offset that is
    dst_mis[i] mod 16, with at least `gap` sentinel bytes between neighbours.  Returns (offs, total)."""
    order = rng.permutation(len(lens))
    offs = np.zeros(len(lens), dtype=np.int64)
    pos = 0
    for i in order:
        pos += gap
        pos += (int(dst_mis[i]) - pos) % 16
        offs[i] = pos
        pos += int(lens[i])
    return offs, pos + gap
