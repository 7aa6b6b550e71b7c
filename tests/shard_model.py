"""Reference model of the sharded pull, plain NumPy and the safetensors bytes alone: no offset
arithmetic shared with zest_amd.shard.plan_file or the slice-gather kernel.

  tensor_slice(data, name, dim, start, stop)  bytes of one tensor's slice (frombuffer, reshape, slice)
  gather_model(src, entries)                  what a slice table writes: {dst_off: bytes}
  build_repo()                                the end-to-end repository of the shard tests
"""
from __future__ import annotations

import json
import struct

import numpy as np

ITEMSIZE = {"BF16": 2, "F16": 2, "F32": 4, "F64": 8, "I64": 8, "I32": 4, "I16": 2, "I8": 1, "U8": 1, "BOOL": 1,
            "F8_E4M3": 1, "F8_E5M2": 1}


def header(data: bytes) -> tuple[int, dict]:
    (hlen,) = struct.unpack("<Q", data[:8])
    meta = json.loads(data[8:8 + hlen])
    meta.pop("__metadata__", None)
    return 8 + hlen, meta


def tensor_array(data: bytes, name: str) -> np.ndarray:
    """The tensor as an array of opaque items (dtype V<itemsize>), copied out of the file."""
    start, meta = header(data)
    ent = meta[name]
    a, b = ent["data_offsets"]
    raw = bytes(data[start + a:start + b])  # a copy: the start may be misaligned
    return np.frombuffer(raw, dtype=f"V{ITEMSIZE[ent['dtype']]}").reshape(ent["shape"])


def tensor_slice(data: bytes, name: str, dim=None, start=None, stop=None) -> tuple[bytes, list]:
    """(bytes, shape) of tensor[..., start:stop, ...] along `dim` (dim None: the whole tensor)."""
    t = tensor_array(data, name)
    if dim is not None:
        idx = [slice(None)] * t.ndim
        idx[dim] = slice(start, stop)
        t = t[tuple(idx)]
    return np.ascontiguousarray(t).tobytes(), list(t.shape)


def chunk_range(n: int, rank: int, world: int) -> tuple[int, int]:
    """Index range of torch.chunk(t, world, dim)[rank] for a dim of n items divisible by world."""
    assert n % world == 0
    return rank * (n // world), (rank + 1) * (n // world)


def gather_model(src: bytes, entries) -> dict[int, bytes]:
    """entries: (src_off, run_bytes, src_stride, n_runs, dst_off) -> {dst_off: output bytes} of the
    entries with any output."""
    out = {}
    for so, rb, st, nr, do in entries:
        b = b"".join(bytes(src[so + r * st: so + r * st + rb]) for r in range(nr))
        if b:
            out[do] = b
    return out


# ------------------------------------------------------------------------------------------------
# Kernel cases, shared by the CPU-path and the GPU tests
# ------------------------------------------------------------------------------------------------
RUN_BYTES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 2048, (16 << 10) + 2)
N_RUNS = (1, 2, 37)
STRIDES = {"contiguous": lambda rb: rb, "plus1": lambda rb: rb + 1, "times8": lambda rb: 8 * rb}
CANARY = 0xA5
GUARD = 512  # canary bytes before and after the arena


def lay_out(specs, dst_step: int = 256, gap: int = 3):
    """specs: (run_bytes, n_runs, src_stride) per tensor -> (entries, src_len, arena_len).  Tensors
    follow each other in the source `gap` bytes apart (so their alignments differ) and in the arena
    at the next multiple of `dst_step`."""
    entries, s, d = [], 0, 0
    for rb, nr, st in specs:
        entries.append((s, rb, st, nr, d))
        if rb and nr:
            s += (nr - 1) * st + rb + gap
            d = -(-(d + rb * nr) // dst_step) * dst_step
    last = max((e[4] + e[1] * e[3] for e in entries), default=0)
    return entries, max(s - gap, 0), last


def grid_specs(stride: str):
    return [(rb, nr, STRIDES[stride](rb)) for rb in RUN_BYTES for nr in N_RUNS]


def check_gather(ops, device, src: np.ndarray, entries, arena_len: int, align: int = 0) -> None:
    """Run ops.slice_gather on `device` and compare the whole destination, canaries included, with
    gather_model.  The source is placed `align` bytes past a 16-byte boundary, and so that its last
    byte is the last byte of its allocation's logical range."""
    import torch

    n = len(src)
    hold = torch.empty(align + n, dtype=torch.uint8, device=device)  # the logical range ends with the source
    assert hold.data_ptr() % 16 == 0  # torch allocations are at least 64-byte aligned
    s = hold[align:]
    s.copy_(torch.from_numpy(src))
    want = np.full(arena_len + 2 * GUARD, CANARY, dtype=np.uint8)
    for do, b in gather_model(src.tobytes(), entries).items():
        want[GUARD + do:GUARD + do + len(b)] = np.frombuffer(b, dtype=np.uint8)
    full = torch.full((arena_len + 2 * GUARD,), CANARY, dtype=torch.uint8, device=device)
    assert full.data_ptr() % 16 == 0
    table = np.array(entries, dtype=ops.SLICE_DTYPE)
    ops.slice_gather(s, table, full[GUARD:GUARD + arena_len])
    got = full.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at arena offset {int(bad[0]) - GUARD}"


# ------------------------------------------------------------------------------------------------
# The end-to-end repository: four safetensors files of 0.3-1.7 MB whose names the built-in
# "llama-tp" plan knows, BF16 / F32 / U8 / F8_E4M3, a scalar and an empty tensor; the second file's
# header is padded so that its data section starts at an odd offset.  Largest file first.
# ------------------------------------------------------------------------------------------------
REPO = "org/shard-e2e"
WORLD = 4
INDEX = "model.safetensors.index.json"


def _layer(i: int, dt_a: str, dt_b: str, dt_c: str, h: int = 256):
    p = f"model.layers.{i}."
    return [(p + "input_layernorm.weight", "F32", [h], None),
            (p + "self_attn.q_proj.weight", dt_a, [512, h], 0),
            (p + "self_attn.q_proj.bias", dt_a, [512], 0),
            (p + "self_attn.k_proj.weight", dt_b, [128, h], 0),
            (p + "self_attn.v_proj.weight", dt_b, [128, h], 0),
            (p + "self_attn.o_proj.weight", dt_a, [h, 512], 1),
            (p + "mlp.gate_proj.weight", dt_c, [256, h], 0),
            (p + "mlp.up_proj.weight", "BF16", [512, h], 0),
            (p + "mlp.down_proj.weight", "BF16", [h, 512], 1)]


# path -> [(name, dtype, shape, dim the built-in plan splits or None)], in header order
FILES = {
    "model-00001-of-00004.safetensors": [("model.embed_tokens.weight", "BF16", [512, 256], 0)]
    + _layer(0, "BF16", "BF16", "F32"),
    "model-00002-of-00004.safetensors": _layer(1, "U8", "F8_E4M3", "BF16")
    + [("model.layers.1.scale", "F32", [], None), ("model.layers.1.mlp.up_proj.bias", "BF16", [0, 4], 0),
       ("model.layers.4.mlp.up_proj.weight", "BF16", [512, 256], 0),
       ("model.layers.4.mlp.down_proj.weight", "F32", [256, 256], 1)],
    "model-00003-of-00004.safetensors": _layer(2, "BF16", "BF16", "F32"),
    "model-00004-of-00004.safetensors": [("model.norm.weight", "BF16", [256], None),
                                         ("model.layers.3.self_attn.k_proj.weight", "BF16", [64, 256], 0),
                                         ("lm_head.weight", "BF16", [512, 256], 0)],
}
ODD_START_FILE = "model-00002-of-00004.safetensors"
SPLIT_DIM = {name: dim for specs in FILES.values() for name, _, _, dim in specs}
FILE_OF = {name: path for path, specs in FILES.items() for name, _, _, _ in specs}


def safetensors_bytes(specs, rng, odd_start: bool = False) -> bytes:
    meta, pos, body = {}, 0, []
    for name, dt, shape, _ in specs:
        n = int(np.prod(shape, dtype=np.int64)) * ITEMSIZE[dt]
        meta[name] = {"dtype": dt, "shape": shape, "data_offsets": [pos, pos + n]}
        body.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        pos += n
    head = json.dumps(meta, separators=(",", ":")).encode()
    while (8 + len(head)) % 16 != (5 if odd_start else 0):
        head += b" "
    return struct.pack("<Q", len(head)) + head + b"".join(body)


def build_repo(seed: int = 11) -> dict[str, bytes]:
    rng = np.random.default_rng(seed)
    files = {p: safetensors_bytes(specs, rng, odd_start=(p == ODD_START_FILE)) for p, specs in FILES.items()}
    files[INDEX] = json.dumps({"metadata": {}, "weight_map": FILE_OF}).encode()
    files["config.json"] = b'{"model_type": "llama"}'
    return files


def expected_shard(files: dict[str, bytes], rank: int, world: int = WORLD) -> dict[str, tuple[bytes, list]]:
    """name -> (bytes, shape) of what the built-in plan leaves rank `rank`, by the model."""
    out = {}
    for name, dim in SPLIT_DIM.items():
        data = files[FILE_OF[name]]
        if dim is None:
            out[name] = tensor_slice(data, name)
        else:
            n = header(data)[1][name]["shape"][dim]
            out[name] = tensor_slice(data, name, dim, *chunk_range(n, rank, world))
    return out
