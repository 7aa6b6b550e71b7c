"""Two revisions of a small model for the delta-pull tests (CPU and GPU), and the model that says
which reconstruction terms of the second can be reused from the first."""
from __future__ import annotations

import json
import struct

import numpy as np

REPO1, REPO2 = "org/delta-step1", "org/delta-step2"  # the hub keeps one file set per repo id
A, B, C = "model-a.safetensors", "model-b.safetensors", "model-c.safetensors"


def safetensors(payload: bytes, name: str) -> bytes:
    head = json.dumps({name: {"dtype": "U8", "shape": [len(payload)], "data_offsets": [0, len(payload)]}}).encode()
    head += b" " * (-len(head) % 8)
    return struct.pack("<Q", len(head)) + head + payload


def revisions(seed: int = 21):
    """(files of revision 1, files of revision 2).  Revision 2: file A with 10 KB inserted near the
    front (every later chunk shifts its file offset by an amount that is no multiple of 16) and one
    ~200 KB region replaced, file B unchanged, file C new."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, 3_000_000, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, 1_000_000, dtype=np.uint8).tobytes()
    ins = rng.integers(0, 256, 10_007, dtype=np.uint8).tobytes()
    # the new bytes are bf16 weights, which a hub with policy="auto" stores BG4 + LZ4 compressed
    bf16 = lambda n: (rng.normal(0, 0.02, n // 2).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()
    new, c = bf16(200_000), bf16(600_000)
    a2 = a[:50_000] + ins + a[50_000:1_500_000] + new + a[1_700_000:]
    rev1 = {A: safetensors(a, "a"), B: safetensors(b, "b"), "config.json": b'{"step": 1}'}
    rev2 = {A: safetensors(a2, "a"), B: safetensors(b, "b"), C: safetensors(c, "c"), "config.json": b'{"step": 2}'}
    return rev1, rev2


def xet_files(hub, repo, paths=None):
    return [f for p, f in hub.repos[("model", repo)].files.items()
            if f.xet_hash and (paths is None or p in paths)]


def model_counts(hub, base_paths=None, new_paths=None):
    """(reused terms, fetched terms, reused files) of a delta pull of REPO2 over REPO1: a term is
    reusable iff every chunk of it is referenced by the base's files."""
    have = {(x, c) for f in xet_files(hub, REPO1, base_paths) for x, c0, c1 in f.terms for c in range(c0, c1)}
    reused = fetched = files = 0
    for f in xet_files(hub, REPO2, new_paths):
        ok = [all((x, c) in have for c in range(c0, c1)) for x, c0, c1 in f.terms]
        reused += sum(ok)
        fetched += len(ok) - sum(ok)
        files += all(ok)
    return reused, fetched, files


def reused_term_of(hub, path):
    """(xorb index, c0, c1, byte offset in the file) of the first reusable term of REPO2's `path`."""
    have = {(x, c) for f in xet_files(hub, REPO1) for x, c0, c1 in f.terms for c in range(c0, c1)}
    (f,) = xet_files(hub, REPO2, {path})
    off = 0
    for x, c0, c1 in f.terms:
        if all((x, c) in have for c in range(c0, c1)):
            return x, c0, c1, off
        off += hub.xorbs[x].cum[c1] - hub.xorbs[x].cum[c0]
    raise AssertionError(f"{path} has no reusable term")


def assert_tensors(got: dict, files: dict) -> None:
    """Every tensor of a pull equals the published bytes (the files hold one U8 tensor each)."""
    want = {}
    for path, data in files.items():
        if path.endswith(".safetensors"):
            (hlen,) = struct.unpack("<Q", data[:8])
            (name,) = json.loads(data[8:8 + hlen])
            want[name] = data[8 + hlen:]
    assert set(got) == set(want)
    for name, data in want.items():
        assert got[name].cpu().numpy().tobytes() == data, name
