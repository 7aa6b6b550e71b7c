"""Pull into tensors the caller already owns: `pull(repo, rev, device=..., into=target)`.

    model = build_model().to("cuda:0")                       # parameters at fixed addresses
    zest_amd.pull(repo, "v2", device="cuda:0", into=model)   # v2's bytes land in those parameters

    qkv = layer.qkv_proj.weight                              # a fused parameter: the caller names its parts
    zest_amd.pull(repo, device="cuda:0", into={"...q_proj.weight": qkv[:q], "...k_proj.weight": qkv[q:q + k],
                                                "...v_proj.weight": qkv[q + k:]})

The flow is the sharded pull's (zest_amd.direct._pull_sharded): files in which nothing is wanted (per
`model.safetensors.index.json`) are not fetched; the others are pulled and verified whole, group by
group, through one reused scratch; after a group verifies, one `ops.slice_scatter` launch per file
(K15, csrc/gpu/scatter.hip) copies the wanted tensors, or with `shard=` this rank's slices of them,
to the destinations' addresses.  Peak device memory is the model plus one scratch, where
`pull()` followed by `param.copy_()` holds two models.

    model = build_model().to("cuda:0", torch.bfloat16)       # served in bf16, the checkpoint is F32
    zest_amd.pull(repo, device="cuda:0", into=model, cast=True)

`cast=True`: a wanted tensor stored in another float dtype than its destination's is converted on the
way, F32 / F16 / BF16 to each other, round to nearest even.  The file is still verified in its stored
dtype (the Xet hash is over the stored bytes); the conversion is in the scatter: per verified file the
tensors whose dtype matches go through `ops.slice_scatter` untouched and the others through one
`ops.slice_scatter_cast` launch (K16, csrc/gpu/scatter_cast.hip), at most two launches per file, all
planning and every refusal before the first.  Peak device memory stays the model plus one scratch,
where `pull()` followed by a converting `param.copy_()` holds the whole checkpoint next to the model.

No byte of a file reaches a destination before that whole file has passed its Xet hash, and a file
whose tensors do not fit their destinations (dtype, sliced shape) writes nothing: a file that fails
leaves its destinations untouched, files before it stay written.  The bytes are written behind
autograd's back (version counters are not bumped), and nothing may run the model during the call.

Limits: one process (no collective form), no delta (`base=` is refused: every wanted file is
fetched), network bytes are those of a sharded pull, destinations must be contiguous, dtype
conversion only with `cast=True` and only among F32, F16 and BF16 (no F8, F64 or integer conversions,
no scaling).
"""
from __future__ import annotations

import os
import struct
import time

import numpy as np
import torch

from . import _core, ops
from . import device as zdev
from . import shard as zshard
from .direct import DEFAULT_SCRATCH, _groups, _slot

_ST_NAMES = {dt: name for name, dt in zdev.ST_DTYPES.items()}


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


class Target:
    """The destinations of an `into=` pull.  dests: {checkpoint name: tensor}, one name per distinct
    destination; aliases: {other name: that name} for names that share a destination's bytes (tied
    weights), which count as provided when the first name is written."""

    def __init__(self, into, dev: torch.device):
        if isinstance(into, torch.nn.Module):
            into = into.state_dict(keep_vars=True)
        if not isinstance(into, dict):
            raise ValueError("into= takes a {checkpoint tensor name: destination tensor} dict or a torch.nn.Module")
        self.given = into
        self.dests: dict[str, torch.Tensor] = {}
        self.aliases: dict[str, str] = {}
        seen = {}  # (address, bytes, dtype, shape) -> first name
        for name, t in into.items():
            if not isinstance(name, str) or not isinstance(t, torch.Tensor):
                raise ValueError(f"into=: {name!r} does not map a tensor name to a tensor")
            other_gpu = dev.type == "cuda" and dev.index is not None and t.device.index != dev.index
            if t.device.type != dev.type or other_gpu:
                raise ValueError(f"into=: {name} is on {t.device}, the pull goes to {dev}; move the destination or "
                                 f"pull with device={str(t.device)!r}")
            if not t.is_contiguous():
                raise ValueError(f"into=: {name} is not contiguous; pass contiguous views (a fused parameter as one "
                                 "view per checkpoint tensor)")
            if t.dtype not in _ST_NAMES:
                raise ValueError(f"into=: {name} has dtype {t.dtype}, which safetensors cannot hold")
            key = (t.data_ptr(), _nbytes(t), t.dtype, tuple(t.shape))
            if _nbytes(t) and key in seen:
                self.aliases[name] = seen[key]
                continue
            seen.setdefault(key, name)
            self.dests[name] = t
        live = sorted((t.data_ptr(), _nbytes(t), name) for name, t in self.dests.items() if _nbytes(t))
        for (a0, n0, name0), (a1, _, name1) in zip(live, live[1:]):
            if a1 < a0 + n0:
                raise ValueError(f"into=: the destinations of {name0} and {name1} overlap; each checkpoint tensor "
                                 "needs bytes of its own (tied weights: pass the same tensor under both names)")

    def shard(self, sh):
        """The plan of this pull as a Shard: every name that is not a destination is dropped, the rest
        is the caller's shard (kept whole without one)."""
        dests = self.dests

        def plan(name, shape, dtype):
            if name not in dests:
                return "drop"
            return None if sh is None else sh.action(name, shape, dtype)

        return zshard.Shard(0, 1, plan) if sh is None else zshard.Shard(sh.rank, sh.world, plan)


SAME = (1 << 64) - 1  # `kind` of a tensor that needs no conversion in a cast=True plan


def plan_file_into(data_start: int, meta: dict, wsh, dests: dict, file_size: int | None = None, cast: bool = False):
    """The scatter table of one safetensors file: (ops.SCATTER_DTYPE table, names, bytes written).
    wsh: `Target.shard(...)`.  Raises ValueError naming the tensor when a wanted tensor's dtype or
    (sliced) shape differs from its destination's; the run arithmetic is `shard.tensor_runs`.
    cast=True: the table is ops.CAST_DTYPE, its runs in stored (source) bytes; `kind` is the
    ops.CAST_KINDS code of a tensor whose dtype differs from its destination's and SAME for the
    others, and only pairs outside ops.CAST_KINDS are refused.  Bytes written are destination bytes."""
    rows, names, total = [], [], 0
    for name, ent in meta.items():
        if name == "__metadata__":
            continue
        runs = zshard.tensor_runs(name, ent, data_start, wsh, file_size)
        if runs is None:
            continue
        out_shape, src_off, run, stride, n_runs, nbytes = runs
        t = dests[name]
        kind = SAME
        if zdev.ST_DTYPES[ent["dtype"]] != t.dtype:
            if not cast:
                raise ValueError(f"{name}: the checkpoint holds {ent['dtype']}, the destination is {t.dtype} "
                                 "(into= converts nothing)")
            kind = ops.CAST_KINDS.get((ent["dtype"], _ST_NAMES[t.dtype]))
            if kind is None:
                raise ValueError(f"{name}: the checkpoint holds {ent['dtype']}, the destination is {t.dtype} "
                                 "(cast=True converts F32, F16 and BF16 to each other, nothing else)")
        if tuple(out_shape) != tuple(t.shape):
            raise ValueError(f"{name}: the checkpoint gives shape {list(out_shape)}, the destination has "
                             f"{list(t.shape)}")
        rows.append((src_off, run, stride, n_runs, t.data_ptr(), kind) if cast
                    else (src_off, run, stride, n_runs, t.data_ptr()))
        names.append(name)
        total += nbytes if kind == SAME else _nbytes(t)
    return np.array(rows, dtype=ops.CAST_DTYPE if cast else ops.SCATTER_DTYPE), names, total


def _scatter_file(buf: torch.Tensor, path: str, wsh, target: Target, written: dict, info: dict,
                  cast: bool = False) -> None:
    """Plan one verified file in `buf`, check it against the destinations and scatter it: one launch,
    with cast=True one for the tensors copied as they are and one for the converted ones.  Everything
    that can refuse the file runs before the first launch."""
    (hlen,) = struct.unpack("<Q", buf[:8].cpu().numpy().tobytes())
    start, meta = zdev.parse_safetensors_header(buf[:8 + hlen].cpu().numpy().tobytes())
    table, names, total = plan_file_into(start, meta, wsh, target.dests, buf.numel(), cast)
    for name in names:
        if name in written:
            raise ValueError(f"duplicate tensor {name} in {path}")
    bufs = [target.dests[n] for n in names]
    if cast:
        conv = table[table["kind"] != SAME]
        same = np.empty(len(table) - len(conv), dtype=ops.SCATTER_DTYPE)
        for f in ops.SCATTER_DTYPE.names:
            same[f] = table[f][table["kind"] == SAME]
        ops.check_scatter_cast(buf, conv, bufs)  # slice_scatter_cast itself would refuse only after the first launch
        ops.slice_scatter(buf, same, bufs)
        ops.slice_scatter_cast(buf, conv, bufs)
        info["cast_tensors"] += len(conv)
        info["cast_bytes_in"] += int((conv["run_bytes"] * conv["n_runs"]).sum())
    else:
        ops.slice_scatter(buf, table, bufs)
    for name in names:
        written[name] = target.dests[name]
    info["file_bytes"] += buf.numel()
    info["written_bytes"] += total
    info["tensors"] += len(names)


def pull_into(repo, revision, dev, into, sh, scratch_bytes, stats, strict, *, p2p, peers, tracker, dht, dht_bootstrap,
              repo_type, staging_bytes, threads, include, cast=False):
    """pull_to_device(into=...): see the module docstring.  Returns {name: destination} of what was
    written, after the device has finished the scatters."""
    target = Target(into, dev)  # refusals first: nothing is listed or fetched for a target that cannot be filled
    wsh = target.shard(sh)
    net = (p2p, list(peers or []), tracker, dht, list(dht_bootstrap or []))
    _, files = _core.list_repo_files(repo, revision, repo_type)
    has_index = any(f["path"] == zshard.INDEX_NAME for f in files)
    if include:
        files = [f for f in files if any(f["path"].endswith(x) for x in include)]
    st_files = [f for f in files if f["path"].endswith(".safetensors")]
    skipped: set = set()
    if has_index and st_files:  # which file holds which tensor, without fetching any of them
        r = _core.pull(repo, revision, *net, [zshard.INDEX_NAME], True, 0, repo_type)
        with open(os.path.join(r["snapshot_dir"], zshard.INDEX_NAME), "rb") as fh:
            skipped = zshard.files_to_skip(fh.read(), [f["path"] for f in st_files], wsh)
        st_files = [f for f in st_files if f["path"] not in skipped]
    xet = [f for f in st_files if f["xet_hash"]]
    plain = [f for f in st_files if not f["xet_hash"]]
    cuda = dev.type == "cuda"
    written: dict[str, torch.Tensor] = {}
    info = {"file_bytes": 0, "written_bytes": 0, "tensors": 0, "skipped_files": sorted(skipped), "missing": [],
            "groups": 0, "scratch_bytes": 0, "scatter_s": 0.0, "cast_tensors": 0, "cast_bytes_in": 0}
    if stats is not None:
        stats["into"] = info  # also what a pull that raises half way leaves behind
    timed = []  # cuda: (start, end) events around each group's scatters, read once at the end

    if xet:
        biggest = max(_slot(f["size"]) for f in xet)
        want = max(max(f["size"] for f in xet), DEFAULT_SCRATCH) if scratch_bytes is None else int(scratch_bytes)
        scratch_n = min(max(want, biggest), sum(_slot(f["size"]) for f in xet))  # never more than every file at once
        groups = _groups(xet, scratch_n)
        info["groups"], info["scratch_bytes"] = len(groups), scratch_n
        if cuda:
            dp = ops.hip().DeviceXetPull(repo, revision, repo_type, *net, dev.index or 0, staging_bytes, threads)
            with torch.cuda.device(dev):
                scratch = ops.padded_empty(scratch_n, dev)
                torch.cuda.synchronize(dev)  # the allocation is visible to the pull's private stream
                for g in groups:
                    # pull_files returns once every file of the group has passed its Merkle check (and
                    # raises otherwise): only then does any of their bytes move to a destination
                    dp.pull_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for f, o in g:
                        _scatter_file(scratch[o:o + f["size"]], f["path"], wsh, target, written, info, cast)
                    ev1.record()
                    timed.append((ev0, ev1))
                    dp.order_after(ev1.cuda_event)  # the next group overwrites the scratch these scatters read
                del scratch  # back to torch's allocator, which orders its reuse behind the scatters' stream
        else:
            hf = _core.HostXetFetcher(repo, revision, repo_type, *net, threads)
            scratch = torch.empty(scratch_n, dtype=torch.uint8)
            for g in groups:
                hf.fetch_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                t0 = time.perf_counter()
                for f, o in g:
                    _scatter_file(scratch[o:o + f["size"]], f["path"], wsh, target, written, info, cast)
                info["scatter_s"] += time.perf_counter() - t0
    if plain:  # non-Xet safetensors: the host route, then the same plan and scatter, file by file
        r = _core.pull(repo, revision, *net, [f["path"] for f in plain], True, 0, repo_type)
        for f in plain:
            buf = zdev.load_file(os.path.join(r["snapshot_dir"], f["path"]), dev)
            t0 = time.perf_counter()
            if cuda:
                with torch.cuda.device(dev):
                    _scatter_file(buf, f["path"], wsh, target, written, info, cast)
                    torch.cuda.current_stream(dev).synchronize()  # buf is freed before the next file loads
            else:
                _scatter_file(buf, f["path"], wsh, target, written, info, cast)
            info["scatter_s"] += time.perf_counter() - t0
            del buf
    if cuda:
        torch.cuda.synchronize(dev)  # the destinations hold their bytes when pull returns
        info["scatter_s"] += sum(a.elapsed_time(b) for a, b in timed) / 1e3
    info["missing"] = sorted(n for n in target.dests if n not in written)
    if strict and info["missing"]:
        raise KeyError(f"into=: no file of {repo}@{revision} provided {', '.join(info['missing'])}")
    out = dict(written)
    for name, first in target.aliases.items():
        if first in written:
            out[name] = target.given[name]
    return out
