"""The publish rule in plain Python, written from the Xet format and not from zest_amd.publish: the
host chunker, one chunk hash per chunk, a dict for "the smallest equal row wins", greedy xorb
packing, Merkle xorb hashes, file hashes, and terms by merging runs.  The CPU and GPU tests compare
ops.dedup_chunks and zest_amd.publish against it."""
from __future__ import annotations

import numpy as np

from zest_amd import _core

MAX_XORB_CHUNKS = 8192


def first_rows(index_rows, new_rows) -> np.ndarray:
    """index_rows / new_rows: sequences of 32-byte keys (bytes, or uint8 [k, 32] arrays).  For every
    new row, the smallest row of (index rows, then new rows) that holds the same bytes."""
    seen: dict[bytes, int] = {}
    m = 0
    for m, row in enumerate(index_rows, 1):
        seen.setdefault(bytes(row), m - 1)
    out = []
    for j, row in enumerate(new_rows):
        out.append(seen.setdefault(bytes(row), m + j))
    return np.asarray(out, dtype=np.int64)


def home_slot(key: bytes, slots: int) -> int:
    return int.from_bytes(bytes(key)[:8], "little") & (slots - 1)


def expected(files: dict, index=(), max_xorb_bytes: int = 64 << 20):
    """files: {path: bytes}; index: [(chunk hash, xorb hex, chunk index), ...] in index row order.
    Returns (ref, manifest): the expected dedup result over all files' chunks in sorted path order
    and the expected manifest."""
    index = list(index)
    m = len(index)
    chunks = []  # (path, hash, length) in row order
    per_file = {}
    for path in sorted(files):
        data = files[path]
        prev, rows = 0, []
        for e in _core.chunk_ends(data):
            rows.append(len(chunks))
            chunks.append((path, _core.chunk_hash(data[prev:e]), e - prev))
            prev = e
        assert prev == len(data)
        per_file[path] = rows
    ref = first_rows([h for h, _, _ in index], [h for _, h, _ in chunks])
    new = [i for i in range(len(chunks)) if ref[i] == m + i]
    xorb_of = np.asarray(_core.plan_xorbs(np.asarray([chunks[i][2] + 8 for i in new], dtype=np.uint64),
                                          max_xorb_bytes, MAX_XORB_CHUNKS)) if new else np.zeros(0, np.int64)
    groups: list[list[int]] = []
    for i, x in zip(new, xorb_of.tolist()):
        if x == len(groups):
            groups.append([])
        groups[x].append(i)
    hexes = [_core.xet_hex(_core.merkle_root([(chunks[i][1], chunks[i][2]) for i in g])) for g in groups]
    loc = {}
    for g, hx in zip(groups, hexes):
        for c, i in enumerate(g):
            loc[i] = (hx, c)
    man_files = []
    for path in sorted(files):
        terms = []
        for i in per_file[path]:
            r = int(ref[i])
            hx, c = (index[r][1], index[r][2]) if r < m else loc[r - m]
            if terms and terms[-1][0] == hx and terms[-1][2] == c:
                terms[-1][2] += 1
                terms[-1][3] += chunks[i][2]
            else:
                terms.append([hx, c, c + 1, chunks[i][2]])
        man_files.append({"path": path, "size": len(files[path]),
                          "xet_hash": _core.xet_hex(_core.file_hash([(chunks[i][1], chunks[i][2])
                                                                     for i in per_file[path]])),
                          "terms": terms})
    manifest = {"version": 1, "files": man_files,
                "xorbs": {hx: {"chunk_lens": [chunks[i][2] for i in g]} for g, hx in zip(groups, hexes)}}
    return ref, manifest


def hub_index(hub, repo: str):
    """The index rows of a repo's Xet files as the hub laid them out, in the order
    ChunkIndex.from_weights lists them (files in listing order = sorted paths, chunks in file order)."""
    files = hub.repos[("model", repo)].files
    rows = []
    for path in sorted(files):
        f = files[path]
        if not f.xet_hash:
            continue
        data, prev = f.data, 0
        ends = list(_core.chunk_ends(data))
        locs = [(hub.xorbs[x].hash_hex, c) for x, c0, c1 in f.terms for c in range(c0, c1)]
        assert len(locs) == len(ends)
        for e, (hx, c) in zip(ends, locs):
            rows.append((_core.chunk_hash(data[prev:e]), hx, c))
            prev = e
    return rows
