"""Reference model of the serve-pack kernel (csrc/gpu/serve.hip): plain Python, byte-exact.

The serialized form of a run of chunks is, per chunk, the 8-byte scheme-0 header
`[0][len LE24][0][len LE24]` followed by the payload; a served window is that stream sliced
`[lo:hi]`.  Also the chunk families the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np


def header(n: int) -> bytes:
    return bytes([0]) + n.to_bytes(3, "little") + bytes([0]) + n.to_bytes(3, "little")


def serialize(chunks) -> bytes:
    return b"".join(header(len(c)) + bytes(c) for c in chunks)


def serve(chunks, lo: int, hi: int) -> bytes:
    return serialize(chunks)[lo:hi]


def ser_ends(chunks) -> list[int]:
    out, e = [], 0
    for c in chunks:
        e += len(c) + 8
        out.append(e)
    return out


# ---------------------------------------------------------------------------------------------
# Chunk families: each returns (arena, offsets, lens) -- chunk i is arena[offsets[i]:][:lens[i]].
# The arena is a uint8 numpy array; placing it at a 16-byte aligned address makes `offsets mod 16`
# the source alignment the kernel sees.
# ---------------------------------------------------------------------------------------------
def family_tiny(seed: int = 1):
    """Lengths 1..40 back to back: one 16-byte output vector holds several headers and payloads."""
    rng = np.random.default_rng(seed)
    lens = np.arange(1, 41)
    offs = np.cumsum(lens) - lens
    return rng.integers(0, 256, int(lens.sum()), dtype=np.uint8), offs, lens


def family_alignment(seed: int = 2):
    """4 KiB chunks at each of the 16 offsets mod 16, scattered and out of order in the arena, plus
    two entries that point at the same bytes."""
    rng = np.random.default_rng(seed)
    slot = 4096 + 64
    arena = rng.integers(0, 256, 16 * slot, dtype=np.uint8)
    order = rng.permutation(16)
    offs = [int(s) * slot + int(k) for k, s in enumerate(order)]  # chunk k at offset = k (mod 16)
    assert sorted(o % 16 for o in offs) == list(range(16))
    offs += [offs[3], offs[3]]
    return arena, np.asarray(offs), np.full(len(offs), 4096)


def family_edges(seed: int = 3):
    """64 chunks of 8 KiB .. 128 KiB (incl. exactly 65536, 65537 and 131072), odd source offsets."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(8192, 131073, 64)
    lens[5], lens[6], lens[40] = 65536, 65537, 131072
    gaps = rng.integers(0, 16, 64)
    offs = np.cumsum(lens + gaps) - lens
    return rng.integers(0, 256, int(offs[-1] + lens[-1]), dtype=np.uint8), offs, lens


def family_table(seed: int = 4):
    """4096 chunks of 24 bytes: a 16 KiB output tile sees 512 boundaries, more than any LDS cache."""
    rng = np.random.default_rng(seed)
    lens = np.full(4096, 24)
    offs = np.arange(4096) * 24
    return rng.integers(0, 256, 4096 * 24, dtype=np.uint8), offs, lens


FAMILIES = {"tiny": family_tiny, "alignment": family_alignment, "edges": family_edges, "table": family_table}


def chunks_of(arena, offs, lens) -> list[bytes]:
    return [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def boundary_windows(ends, total: int):
    """(lo, hi) windows that start and end +-1 and +-16 bytes around every chunk boundary."""
    pts = sorted({min(total, max(0, e + d)) for e in [0] + list(ends) for d in (-16, -1, 0, 1, 16)})
    out = []
    for i, a in enumerate(pts):  # every point as a start, paired with the next few points as ends
        for b in pts[i + 1:i + 7]:
            out.append((a, b))
    return out
