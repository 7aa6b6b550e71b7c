"""Shard planner of the sharded device pull: which bytes of a safetensors file one rank keeps.

    shard = Shard(rank=3, world=8)                       # built-in "llama-tp" plan
    shard = Shard(3, 8, {"*.experts.*": "drop", "*.o_proj.weight": 1})
    tensors = zest_amd.pull(repo, device="cuda:3", shard=shard)

Pure Python, no GPU: `plan_file` turns a safetensors header and a `Shard` into the table that
`ops.slice_gather` (K10, csrc/gpu/shard.hip) executes and the layout of the compact arena it fills;
`files_to_skip` decides from `model.safetensors.index.json` alone which files a rank never fetches.

Actions a plan gives a tensor:
  None                 keep it whole (replicated on every rank)
  "drop"               this rank does not keep it
  dim (int)            equal contiguous split of that dim; the rank keeps part `rank` of `world`,
                       identical to torch.chunk(t, world, dim)[rank]; the dim must divide by world
  (dim, start, stop)   an explicit index range of that dim (GQA K/V heads, uneven experts, ...)

A plan is a name ("llama-tp"), a dict of fnmatch patterns to actions (first match wins, no match:
keep whole), or a callable (name, shape, dtype) -> action.  dtype is the safetensors dtype string.
While a callable plan runs, `plan.shard` is the Shard asking (set before every call when the
callable accepts attributes), which is how it sees `rank` and `world`: pipeline stages and expert
placement are written that way.

Skipping whole files: the index has no shapes, so for that decision the plan is asked with
shape=None and dtype=None.  The built-in plan and dict plans never need the shape to say "drop".
A callable that returns anything but "drop" for shape=None (or cannot cope with it and raises
TypeError / AttributeError / IndexError) keeps the file; its tensors are then decided, with their
shapes, once the file's header is in hand.
"""
from __future__ import annotations

import fnmatch
import json
from dataclasses import dataclass, field

import numpy as np
import torch

from .device import ST_DTYPES
from .ops import SLICE_DTYPE

ARENA_ALIGN = 256  # every kept tensor starts at a multiple of this in its arena
INDEX_NAME = "model.safetensors.index.json"

# HF Llama / Mistral / Qwen2 tensor parallelism: column-parallel projections split their output
# rows (dim 0, weights and biases), row-parallel ones their input columns (dim 1), the embeddings
# their vocabulary rows.  Norms, row-parallel biases and everything else stay whole.
LLAMA_TP = {}
for _p in ("q_proj", "k_proj", "v_proj", "gate_proj", "up_proj"):
    LLAMA_TP[f"*.{_p}.weight"] = 0
    LLAMA_TP[f"*.{_p}.bias"] = 0
for _p in ("embed_tokens.weight", "lm_head.weight"):
    LLAMA_TP[f"*.{_p}"] = 0
    LLAMA_TP[_p] = 0
for _p in ("o_proj.weight", "down_proj.weight"):
    LLAMA_TP[f"*.{_p}"] = 1
PLANS = {"llama-tp": LLAMA_TP}


class Shard:
    """What one rank of `world` keeps of a checkpoint (see the module docstring for plans)."""

    def __init__(self, rank: int, world: int, plan="llama-tp"):
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"Shard: rank {rank} outside world of {world}")
        if isinstance(plan, str):
            if plan not in PLANS:
                raise ValueError(f"Shard: unknown plan {plan!r} (built in: {sorted(PLANS)})")
            plan = PLANS[plan]
        elif not isinstance(plan, dict) and not callable(plan):
            raise ValueError("Shard: plan is a name, a dict of patterns or a callable (name, shape, dtype)")
        self.rank, self.world, self.plan = rank, world, plan

    def __repr__(self):
        return f"Shard(rank={self.rank}, world={self.world})"

    def action(self, name: str, shape, dtype):
        """The plan's raw action for a tensor (shape None: only "drop" or not matters)."""
        if isinstance(self.plan, dict):
            for pat, act in self.plan.items():
                if fnmatch.fnmatchcase(name, pat):
                    return act
            return None
        try:
            self.plan.shard = self
        except AttributeError:  # builtins, bound methods: they have their own way to rank and world
            pass
        return self.plan(name, None if shape is None else tuple(shape), dtype)

    def resolve(self, name: str, shape, dtype):
        """None (whole), "drop", or (dim, start, stop) checked against `shape`."""
        act = self.action(name, shape, dtype)
        if act is None or (isinstance(act, str) and act == "drop"):
            return act
        shape = tuple(shape)
        if isinstance(act, (int, np.integer)) and not isinstance(act, bool):
            dim = _dim(name, int(act), shape)
            if shape[dim] % self.world:
                raise ValueError(f"{name}: dim {dim} of shape {list(shape)} is not divisible by world {self.world}")
            part = shape[dim] // self.world
            return dim, self.rank * part, (self.rank + 1) * part
        if isinstance(act, (tuple, list)) and len(act) == 3 and all(
                isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in act):
            dim = _dim(name, int(act[0]), shape)
            start, stop = int(act[1]), int(act[2])
            if not 0 <= start <= stop <= shape[dim]:
                raise ValueError(f"{name}: range [{start}, {stop}) outside dim {dim} of shape {list(shape)}")
            return dim, start, stop
        raise ValueError(f"{name}: plan action {act!r} is not None, 'drop', a dim or (dim, start, stop)")


def _dim(name: str, dim: int, shape: tuple) -> int:
    if not -len(shape) <= dim < len(shape):
        raise ValueError(f"{name}: dim {dim} out of range for shape {list(shape)}")
    return dim % len(shape)


def as_shard(shard) -> Shard:
    """A Shard, or (rank, world) as shorthand for the default plan."""
    if isinstance(shard, Shard):
        return shard
    if isinstance(shard, (tuple, list)) and len(shard) == 2:
        return Shard(shard[0], shard[1])
    raise ValueError("shard= takes a zest_amd.shard.Shard or (rank, world)")


@dataclass
class PlannedTensor:
    name: str
    dtype: str          # safetensors dtype string
    shape: tuple        # sliced shape
    dst_off: int        # byte offset in the arena (multiple of ARENA_ALIGN)
    nbytes: int


@dataclass
class FilePlan:
    table: np.ndarray                       # ops.SLICE_DTYPE, one entry per kept tensor, header order
    arena_bytes: int
    tensors: list = field(default_factory=list)  # PlannedTensor per table entry
    dropped: list = field(default_factory=list)  # names this rank does not keep

    def views(self, arena: torch.Tensor) -> dict:
        """Typed, sliced views into a filled arena (uint8, at least arena_bytes)."""
        out = {}
        for t in self.tensors:
            dt = ST_DTYPES[t.dtype]
            raw = arena[t.dst_off:t.dst_off + t.nbytes]
            v = raw.view(dt) if t.nbytes else torch.empty(0, dtype=dt, device=arena.device)
            out[t.name] = v.view(t.shape) if t.shape else v.reshape(())
        return out


def _itemsize(name: str, dtype: str) -> int:
    dt = ST_DTYPES.get(dtype)
    if dt is None:
        raise ValueError(f"{name}: unsupported dtype {dtype}")
    return torch.empty((), dtype=dt).element_size()


def _prod(xs) -> int:
    n = 1
    for x in xs:
        n *= int(x)
    return n


def tensor_runs(name: str, ent: dict, data_start: int, shard: Shard, file_size: int | None = None):
    """The runs `shard` keeps of one safetensors header entry: (sliced shape, src_off, run_bytes,
    src_stride, n_runs, nbytes) with src_off counted from the start of the file, or None when the
    plan drops the tensor.  The entry is checked first (dtype, data_offsets against shape and
    file_size).  Shared by `plan_file` (arena destinations) and `zest_amd.into` (the caller's)."""
    isz = _itemsize(name, ent["dtype"])
    shape = tuple(int(x) for x in ent["shape"])
    a, b = (int(x) for x in ent["data_offsets"])
    if any(x < 0 for x in shape) or a < 0 or b - a != _prod(shape) * isz:
        raise ValueError(f"{name}: data_offsets [{a}, {b}) do not match shape {list(shape)} of {ent['dtype']}")
    if file_size is not None and data_start + b > file_size:
        raise ValueError(f"{name}: data_offsets [{a}, {b}) reach past the file ({file_size} bytes)")
    act = shard.resolve(name, shape, ent["dtype"])
    if act == "drop":
        return None
    if act is None:
        out_shape, src_off, run, stride, n_runs = shape, data_start + a, b - a, b - a, 1
    else:
        dim, start, stop = act
        inner = _prod(shape[dim + 1:]) * isz
        out_shape = shape[:dim] + (stop - start,) + shape[dim + 1:]
        src_off = data_start + a + start * inner
        run, stride, n_runs = (stop - start) * inner, shape[dim] * inner, _prod(shape[:dim])
    nbytes = run * n_runs
    if nbytes == 0:
        run = stride = n_runs = 0
        src_off = data_start + a
    elif run == stride or n_runs == 1:  # the slice is contiguous in the file: one run
        run, stride, n_runs = nbytes, nbytes, 1
    return out_shape, src_off, run, stride, n_runs, nbytes


def plan_file(data_start: int, meta: dict, shard: Shard, file_size: int | None = None) -> FilePlan:
    """The slice table and arena layout of one safetensors file for `shard`.

    data_start, meta: as `device.parse_safetensors_header` returns them; file_size (when given)
    bounds every entry.  Kept tensors are placed in header order at ARENA_ALIGN-aligned offsets.
    Each entry's data_offsets must span exactly shape * itemsize bytes."""
    rows, tensors, dropped = [], [], []
    pos = 0
    for name, ent in meta.items():
        if name == "__metadata__":
            continue
        runs = tensor_runs(name, ent, data_start, shard, file_size)
        if runs is None:
            dropped.append(name)
            continue
        out_shape, src_off, run, stride, n_runs, nbytes = runs
        rows.append((src_off, run, stride, n_runs, pos))
        tensors.append(PlannedTensor(name, ent["dtype"], out_shape, pos, nbytes))
        pos = -(-(pos + nbytes) // ARENA_ALIGN) * ARENA_ALIGN
    arena = tensors[-1].dst_off + tensors[-1].nbytes if tensors else 0
    return FilePlan(np.array(rows, dtype=SLICE_DTYPE), arena, tensors, dropped)


def files_to_skip(index_json, file_names, shard: Shard) -> set:
    """The files of `file_names` this rank need not fetch: every tensor that the index's
    weight_map puts in them resolves to "drop".  index_json: the index as bytes, str or dict.
    Files the index does not mention are kept (see the module docstring for the shape=None rule)."""
    idx = index_json if isinstance(index_json, dict) else json.loads(index_json)
    by_file: dict[str, list] = {}
    for name, fn in idx.get("weight_map", {}).items():
        by_file.setdefault(fn, []).append(name)
    skip = set()
    for fn in file_names:
        names = by_file.get(fn)
        if not names:
            continue
        try:
            if all(_is_drop(shard.action(n, None, None)) for n in names):
                skip.add(fn)
        except (TypeError, AttributeError, IndexError):  # the plan needs shapes: decide with the header
            pass
    return skip


def _is_drop(act) -> bool:
    return isinstance(act, str) and act == "drop"
