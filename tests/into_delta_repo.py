"""Three revisions of a small model for the in-place delta pull tests (CPU and GPU): one repo id per
revision on one hub, so that a later revision's terms point into the earlier one's xorbs.

Revision 1: FILE3 (two tensors that revision 2 swaps), FILE1 (the largest; data_start is 8 mod 16)
and FILE2 (a run of fourteen 4 KB tensors that one chunk spans, and a zero-size tensor).
Revision 2: FILE1 with one tensor replaced and ~200 KB inside another replaced; FILE2 with the same
tensors behind a header that is 8 bytes longer; FILE3 with two tensors in swapped order; FILE_NEW.
Revision 3: revision 2 with one more tensor of FILE1 replaced."""
from __future__ import annotations

import json
import struct

import numpy as np

REPO1, REPO2, REPO3 = "org/into-delta-step1", "org/into-delta-step2", "org/into-delta-step3"
FILE3, FILE1, FILE2, FILE_NEW = ("model-a.safetensors", "model-b.safetensors", "model-c.safetensors",
                                 "model-d.safetensors")  # listing order: FILE3 is scattered before FILE1
ITEMSIZE = {"U8": 1, "I8": 1, "BF16": 2, "F16": 2, "I16": 2, "F32": 4, "I32": 4}
TINY = [f"c.tiny.{i:02d}" for i in range(14)]

# (name, dtype, shape) in file order
SPEC1 = [("b.embed", "BF16", [1024, 1536]), ("b.bias", "F32", [3, 5]), ("b.wide", "U8", [2_000_003]),
         ("b.gate", "BF16", [128, 1024]), ("b.down", "F16", [700, 1000]), ("b.tail", "I32", [40_000])]
SPEC2 = ([("c.first", "F32", [300, 250])] + [(n, "U8" if i % 2 else "I16", [4096] if i % 2 else [2048])
                                             for i, n in enumerate(TINY)]
         + [("c.empty", "F32", [0, 7]), ("c.mid", "U8", [777_777]), ("c.last", "BF16", [500, 600])])
SPEC3 = [("a.one", "U8", [300_001]), ("a.left", "F16", [200, 1000]), ("a.right", "I32", [90_000]),
         ("a.end", "U8", [300_000])]
TWINS = ("a.end", "c.first")  # as many bytes in two files: their destinations can be traded
SPEC_NEW = [("d.new", "BF16", [300, 500])]
REPLACED, PATCHED, REPLACED3 = "b.gate", "b.wide", "b.bias"
PATCH_AT, PATCH_LEN = 900_000, 200_000
SWAPPED = ("a.left", "a.right")


def nbytes(dt: str, shape) -> int:
    return int(np.prod(shape, dtype=np.int64)) * ITEMSIZE[dt]


def safetensors(spec, payload: dict, metadata: dict | None = None, hlen: int | None = None) -> bytes:
    """The file of `spec` with payload[name] as each tensor's bytes; the JSON header is padded with
    spaces to `hlen` bytes (default: the next multiple of 8)."""
    head, off = {}, 0
    if metadata:
        head["__metadata__"] = metadata
    for name, dt, shape in spec:
        n = nbytes(dt, shape)
        assert len(payload[name]) == n, name
        head[name] = {"dtype": dt, "shape": list(shape), "data_offsets": [off, off + n]}
        off += n
    hb = json.dumps(head, separators=(",", ":")).encode()
    want = len(hb) + (-len(hb) % 8) if hlen is None else hlen
    assert want >= len(hb) and want % 8 == 0
    hb += b" " * (want - len(hb))
    return struct.pack("<Q", len(hb)) + hb + b"".join(payload[name] for name, _, _ in spec)


def header(data: bytes):
    """(data_start, {name: (dtype, shape, file offset, bytes)}) of a safetensors file."""
    (hlen,) = struct.unpack("<Q", data[:8])
    meta = json.loads(data[8:8 + hlen])
    start = 8 + hlen
    return start, {n: (e["dtype"], e["shape"], start + e["data_offsets"][0], e["data_offsets"][1] - e["data_offsets"][0])
                   for n, e in meta.items() if n != "__metadata__"}


def tensor_bytes(files: dict) -> dict:
    """{tensor name: its bytes} over every safetensors file of a revision."""
    out = {}
    for path, data in files.items():
        if path.endswith(".safetensors"):
            for name, (_, _, off, n) in header(data)[1].items():
                out[name] = data[off:off + n]
    return out


def specs(files: dict) -> dict:
    """{tensor name: (dtype, shape, path)} of a revision."""
    return {name: (dt, shape, path) for path, data in files.items() if path.endswith(".safetensors")
            for name, (dt, shape, _, _) in header(data)[1].items()}


def _hlen16(spec, payload, metadata: dict | None = None) -> int:
    """The shortest header length that leaves data_start = 8 + hlen at 8 mod 16."""
    n = len(safetensors(spec, payload, metadata)) - sum(len(payload[name]) for name, _, _ in spec) - 8
    return n + (-n % 16)


def revisions(seed: int = 33):
    rng = np.random.default_rng(seed)
    raw = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    # new bytes are bf16 weights, which a hub with policy="auto" stores BG4 + LZ4 compressed
    bf16 = lambda n: (rng.normal(0, 0.02, n // 2).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()
    p1 = {name: raw(nbytes(dt, shape)) for name, dt, shape in SPEC1 + SPEC2 + SPEC3}
    f1 = safetensors(SPEC1, p1, hlen=_hlen16(SPEC1, p1))
    assert header(f1)[0] % 16 == 8
    meta2 = {"step": "2", "note": "a longer header"}
    h2 = _hlen16(SPEC2, p1, meta2)
    f2 = safetensors(SPEC2, p1, {"step": "1"}, hlen=h2)
    rev1 = {FILE3: safetensors(SPEC3, p1), FILE1: f1, FILE2: f2, "config.json": b'{"step": 1}'}

    p2 = dict(p1)
    p2[REPLACED] = bf16(len(p1[REPLACED]))
    w = p1[PATCHED]
    p2[PATCHED] = w[:PATCH_AT] + bf16(PATCH_LEN) + w[PATCH_AT + PATCH_LEN:]
    p2["d.new"] = bf16(nbytes("BF16", [300, 500]))
    i, j = (next(k for k, s in enumerate(SPEC3) if s[0] == n) for n in SWAPPED)
    spec3 = list(SPEC3)
    spec3[i], spec3[j] = spec3[j], spec3[i]
    f2b = safetensors(SPEC2, p2, meta2, hlen=h2 + 8)
    assert header(f2b)[0] == header(f2)[0] + 8
    rev2 = {FILE3: safetensors(spec3, p2), FILE1: safetensors(SPEC1, p2, hlen=_hlen16(SPEC1, p2)), FILE2: f2b,
            FILE_NEW: safetensors(SPEC_NEW, p2), "config.json": b'{"step": 2}'}

    p3 = dict(p2)
    p3[REPLACED3] = raw(len(p2[REPLACED3]))
    rev3 = dict(rev2)
    rev3[FILE1] = safetensors(SPEC1, p3, hlen=_hlen16(SPEC1, p3))
    rev3["config.json"] = b'{"step": 3}'
    return rev1, rev2, rev3
