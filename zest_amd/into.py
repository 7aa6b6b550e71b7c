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

    landed = zest_amd.pull(repo, "step-100", device="cuda:0", into=model)               # plus a record
    landed = zest_amd.pull(repo, "step-200", device="cuda:0", into=model, base=landed)  # only what changed

`pull(..., into=...)` returns a `Landed`: the {name: destination} dict, with `.record`, an
`IntoRecord` of what was written whole and unconverted (per Xet file its header bytes, chunk sizes,
reconstruction terms and the tensors' file ranges; plain data, no addresses).  `record.bind(dests)`
lays each file out over the destinations (header uploaded, every recorded tensor at its destination's
address, everything else a hole) and returns a `delta.ResidentSet`: chunks inside one tensor are read
where they lie, chunks that cross tensor boundaries are gathered into a seam arena at every bind,
chunks that touch a hole are not resident.  `base=` accepts a `Landed` (bound fresh) anywhere a
resident set is accepted.

With `into=` and `base=` together the model is updated in place (`_pull_xet_delta`).  Per file: (A) the
terms whose chunks are all resident are hashed where they lie (`ops.hash_chunks_at`), the others are
fetched into a compact patch scratch, and the file's Merkle root over all leaf hashes must equal its
Xet hash; (B) the header is read from the verified bytes and planned against the destinations; a
resident chunk that already lies at its place in its destination is kept, every other resident chunk
that overlaps a wanted tensor is moved: gathered and re-hashed into a bounce area
(`ops.reuse_chunks`); (C) `ops.slice_scatter` writes the fetched and the moved pieces.  Within a group
of files every gather is queued before the first scatter.  A file that misses its hash (destinations
modified since the record was taken) has written nothing and is pulled whole, as without a base.
Peak device memory above the model is the patch (the bytes fetched), the moved bytes, the seam arena
and small tables.

Limits: one process (no collective form); `base=` reuses whole terms only, needs the base on the
pull's device and is refused with `shard=` and `cast=True` (sliced or converted destinations do not
hold stored bytes, and are not recorded); a record covers only tensors loaded through `into=`;
network bytes without a base are those of a sharded pull; destinations must be contiguous; dtype
conversion only with `cast=True` and only among F32, F16 and BF16 (no F8, F64 or integer conversions,
no scaling).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import struct
import time
from dataclasses import dataclass

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


@dataclass
class FileRecord:
    """One Xet file an `into=` pull scattered.  header: the file's first data_start bytes; chunk_lens:
    its chunk sizes in file order; term_keys: [(xorb_hex, c0, c1), ...]; tensors: (name, file offset,
    bytes) of every tensor written whole and unconverted."""
    path: str
    xet_hash: str
    size: int
    header: bytes
    chunk_lens: np.ndarray
    term_keys: list
    tensors: list


def _norm(dev) -> torch.device:
    d = torch.device(dev)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class IntoRecord:
    """What an `into=` pull wrote, as plain data without addresses: `files`, a list of FileRecord."""

    def __init__(self, files=()):
        self.files = list(files)

    def state(self) -> dict:
        """A JSON-able form (`json.dumps`); the headers go as hex."""
        return {"version": 1, "files": [
            {"path": f.path, "xet_hash": f.xet_hash, "size": int(f.size), "header": f.header.hex(),
             "chunk_lens": [int(x) for x in f.chunk_lens], "term_keys": [[hx, int(a), int(b)] for hx, a, b in f.term_keys],
             "tensors": [[n, int(o), int(k)] for n, o, k in f.tensors]} for f in self.files]}

    @classmethod
    def from_state(cls, obj: dict) -> "IntoRecord":
        if not isinstance(obj, dict) or obj.get("version") != 1:
            raise ValueError("IntoRecord.from_state: not the state of an IntoRecord (version 1)")
        return cls(FileRecord(f["path"], f["xet_hash"], int(f["size"]), bytes.fromhex(f["header"]),
                              np.asarray(f["chunk_lens"], dtype=np.uint32),
                              [(hx, int(a), int(b)) for hx, a, b in f["term_keys"]],
                              [(n, int(o), int(k)) for n, o, k in f["tensors"]]) for f in obj["files"])

    def layout(self, f: FileRecord, dests: dict):
        """The segments of `f` over `dests` in file order: [(bytes, tensor name or "" for the header or
        None for a hole)].  A recorded tensor that `dests` lacks, or holds with another size, is a hole."""
        segs, pos = [(len(f.header), "")], len(f.header)
        for name, off, n in sorted(f.tensors, key=lambda r: (r[1], r[2])):
            if n == 0:
                continue
            if off < pos:
                raise ValueError(f"IntoRecord: {f.path}: {name} overlaps the bytes before it")
            if off > pos:
                segs.append((off - pos, None))
            t = dests.get(name)
            segs.append((n, name if isinstance(t, torch.Tensor) and t.is_contiguous() and _nbytes(t) == n else None))
            pos = off + n
        if pos > f.size:
            raise ValueError(f"IntoRecord: {f.path}: tensors reach past the file")
        if pos < f.size:
            segs.append((f.size - pos, None))
        return segs

    def bind(self, dests, device=None):
        """The record as a `delta.ResidentSet` over `dests` (the Landed itself, a {name: tensor} dict or
        a module) as they are now.  Per file the virtual layout is the header (uploaded to a small
        tensor) followed by each recorded tensor's bytes at its destination's address; every other byte
        range is a hole.  A chunk inside one segment keeps its address there; a chunk that crosses
        segment boundaries without touching a hole is gathered, one piece per segment it touches, into
        one seam arena for this bind (at most 128 KiB per boundary; on a GPU in one `ops.reuse_chunks`
        launch, on the CPU copied one by one); a chunk that touches a hole is not resident."""
        from .delta import ResidentSet
        from .publish import classify_chunks_with_holes
        from .seed import merge_chunk_refs

        if isinstance(dests, torch.nn.Module):
            dests = dests.state_dict(keep_vars=True)
        if not isinstance(dests, dict):
            raise ValueError("IntoRecord.bind takes a {tensor name: tensor} dict or a torch.nn.Module")
        tensors = [t for t in dests.values() if isinstance(t, torch.Tensor)]
        if device is None:
            if not tensors:
                raise ValueError("IntoRecord.bind: no tensors, and no device given")
            device = tensors[0].device
        dev = _norm(device)
        for name, t in dests.items():
            if isinstance(t, torch.Tensor) and _norm(t.device) != dev:
                raise ValueError(f"IntoRecord.bind: {name} is on {t.device}, the set is bound on {dev}")
        t_start = time.perf_counter()
        cuda = dev.type == "cuda"
        placed, seam_bytes = [], 0
        for f in self.files:
            segs = self.layout(f, dests)
            lens = np.asarray(f.chunk_lens, dtype=np.uint32)
            if int(lens.sum(dtype=np.uint64)) != f.size or sum(n for n, _ in segs) != f.size:
                raise ValueError(f"IntoRecord: {f.path}: chunks and segments do not add up to the file's {f.size} bytes")
            pl = classify_chunks_with_holes([n for n, _ in segs], [s is None for _, s in segs],
                                            np.cumsum(lens, dtype=np.uint64))
            placed.append((f, segs, lens, pl))
            seam_bytes += pl["seam_bytes"]
        with torch.cuda.device(dev) if cuda else contextlib.nullcontext():
            arena = None
            if seam_bytes:
                arena = ops.padded_empty(seam_bytes, dev) if cuda else torch.empty(seam_bytes, dtype=torch.uint8)
            buffers, refs, at, seam_chunks = [], {}, 0, 0
            p_src, p_len, p_dst = [], [], []
            for f, segs, lens, pl in placed:
                head = torch.frombuffer(bytearray(f.header), dtype=torch.uint8).to(dev)
                flat = [head if s == "" else None if s is None else ops._flat_u8(dests[s].detach()) for _, s in segs]
                buffers += [t for t in flat if t is not None]
                base = np.asarray([0 if t is None else t.data_ptr() for t in flat], dtype=np.uint64)
                if cuda:  # the pieces of every file are gathered in one launch after the loop
                    p_src.append(base[pl["piece_seg"]] + pl["piece_off"])
                    p_len.append(pl["piece_len"])
                    p_dst.append(np.uint64(at) + pl["piece_dst"])
                else:
                    for sg, so, ln, do in zip(pl["piece_seg"].tolist(), pl["piece_off"].tolist(),
                                              pl["piece_len"].tolist(), pl["piece_dst"].tolist()):
                        arena[at + do:at + do + ln].copy_(flat[sg][so:so + ln])
                addr = base[pl["seg"]] + pl["off"]
                if pl["seam_chunks"]:
                    addr[pl["seam"]] = np.uint64(arena.data_ptr() + at) + pl["arena_off"][pl["seam"]]
                at += pl["seam_bytes"]
                seam_chunks += pl["seam_chunks"]
                res, cur = pl["resident"], 0
                for hx, c0, c1 in f.term_keys:  # as seed.plan_resident_runs, cut at chunks that are not resident
                    k = int(c1) - int(c0)
                    if k <= 0 or cur + k > len(lens):
                        raise ValueError(f"IntoRecord: {f.path}: terms do not match the file's {len(lens)} chunks")
                    on = np.flatnonzero(res[cur:cur + k])
                    for run in np.split(on, np.flatnonzero(np.diff(on) != 1) + 1) if len(on) else []:
                        a, b = cur + int(run[0]), cur + int(run[-1]) + 1
                        refs.setdefault(hx, []).append((int(c0) + int(run[0]), addr[a:b], lens[a:b]))
                    cur += k
                if cur != len(lens):
                    raise ValueError(f"IntoRecord: {f.path}: terms cover {cur} chunks, the file has {len(lens)}")
            if p_src and sum(len(a) for a in p_src):
                # one K12 launch copies every piece (its hashes of the pieces are not used)
                n = sum(len(a) for a in p_src)
                ops.reuse_chunks(np.concatenate(p_src), np.concatenate(p_len), arena, np.concatenate(p_dst),
                                 torch.empty((n, 32), dtype=torch.uint8, device=dev), np.arange(n), buffers=buffers)
            rs = ResidentSet(merge_chunk_refs(refs), buffers + ([arena] if arena is not None else []), dev)
        rs.seam_chunks, rs.seam_bytes, rs.bind_s = seam_chunks, seam_bytes, time.perf_counter() - t_start
        return rs


class Landed(dict):
    """What `pull(..., into=...)` returns: {name: destination} of what was written, with `.record`
    (an IntoRecord) and `.device`.  As `base=` of a later pull it is bound to these destinations."""

    def __init__(self, written=(), record: IntoRecord | None = None, device=None):
        super().__init__(written)
        self.record = record if record is not None else IntoRecord()
        self.device = None if device is None else _norm(device)


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


def _whole_rows(table, names, meta: dict) -> list:
    """(name, file offset, bytes) of the plan rows that copy a stored tensor whole and unconverted."""
    out = []
    for row, name in zip(table, names):
        a, b = (int(x) for x in meta[name]["data_offsets"])
        conv = "kind" in table.dtype.names and int(row["kind"]) != SAME
        if not conv and int(row["run_bytes"]) * int(row["n_runs"]) == b - a:
            out.append((name, int(row["src_off"]), b - a))
    return out


def _record(records: list, f: dict, head: bytes, lens, keys, rows: list) -> None:
    """Append the FileRecord of a scattered Xet file, unless no tensor with bytes was written whole."""
    if any(n for _, _, n in rows):
        records.append(FileRecord(f["path"], f["xet_hash"], int(f["size"]), head, lens,
                                  [(hx, int(a), int(b)) for hx, a, b in keys], rows))


def _scatter_file(buf: torch.Tensor, path: str, wsh, target: Target, written: dict, info: dict,
                  cast: bool = False, rec=None) -> None:
    """Plan one verified file in `buf`, check it against the destinations and scatter it: one launch,
    with cast=True one for the tensors copied as they are and one for the converted ones.  Everything
    that can refuse the file runs before the first launch.  rec: (listing dict, chunk_lens, term_keys,
    list) of a Xet file; its FileRecord is appended to the list."""
    (hlen,) = struct.unpack("<Q", buf[:8].cpu().numpy().tobytes())
    head = buf[:8 + hlen].cpu().numpy().tobytes()
    start, meta = zdev.parse_safetensors_header(head)
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
    if rec is not None:
        f, chunk_lens, keys, records = rec
        lens = (np.frombuffer(chunk_lens, dtype="<u4") if isinstance(chunk_lens, (bytes, bytearray, memoryview))
                else np.asarray(chunk_lens)).astype(np.uint32)
        _record(records, f, head[:start], lens, keys, _whole_rows(table, names, meta))
    info["file_bytes"] += buf.numel()
    info["written_bytes"] += total
    info["tensors"] += len(names)


DELTA_KEYS = ("kept_terms", "kept_bytes", "moved_chunks", "moved_bytes", "fetched_terms", "fetched_bytes",
              "applied_bytes", "seam_chunks", "seam_bytes", "patch_bytes", "fallback_files", "fallback_bytes")


def _peek(addr: int, n: int, buffers, dev) -> bytes:
    """n bytes at an absolute address inside one of `buffers`, on the host."""
    if n == 0:
        return b""
    if dev.type != "cuda":
        return ctypes.string_at(addr, n)
    for b in buffers:
        off = addr - b.data_ptr()
        if 0 <= off and off + n <= _nbytes(b):
            return ops._flat_u8(b)[off:off + n].cpu().numpy().tobytes()
    raise ValueError(f"[{addr:#x}, {addr + n:#x}) lies in no buffer of the base")


class _DeltaFile:
    """One file of an in-place delta pull: `delta._FilePlan` (terms split into resident and fetched)
    with the fetched runs laid one after another in a patch, and, once the file has verified, the
    plan of step B: which resident chunks are kept or moved and what the scatters copy."""

    def __init__(self, plan):
        self.p = plan
        self.runs = []  # (t0, t1, offset in the file's patch)
        at = 0
        for t0, t1 in plan.runs(False):
            self.runs.append((t0, t1, at))
            at += int(plan.t_off[t1] - plan.t_off[t0])
        self.patch = at  # bytes to fetch

    def sources(self, patch_addr: int) -> None:
        """Per chunk: its offset in the file, whether it was fetched and the address of its bytes (in
        the patch at `patch_addr`, or where the base holds it).  After the fetch (chunk_lens is whole)."""
        p = self.p
        lens = p.chunk_lens.astype(np.int64)
        self.cend = np.cumsum(lens)
        self.coff = self.cend - lens
        self.fetched = np.zeros(p.nchunks, dtype=bool)
        self.caddr = np.zeros(p.nchunks, dtype=np.uint64)
        for t, a in p.src.items():
            self.caddr[p.t_chunk[t]:p.t_chunk[t + 1]] = a
        for t0, t1, at in self.runs:
            c0, c1 = int(p.t_chunk[t0]), int(p.t_chunk[t1])
            self.fetched[c0:c1] = True
            self.caddr[c0:c1] = (patch_addr + at + (self.coff[c0:c1] - int(p.t_off[t0]))).astype(np.uint64)

    def read(self, a: int, b: int, buffers, dev) -> bytes:
        """Bytes [a, b) of the verified file, from wherever its chunks lie."""
        out, c = [], int(np.searchsorted(self.cend, a, side="right"))
        while a < b:
            n = min(b, int(self.cend[c])) - a
            out.append(_peek(int(self.caddr[c]) + a - int(self.coff[c]), n, buffers, dev))
            a, c = a + n, c + 1
        return b"".join(out)

    def plan(self, wsh, target: Target, buffers, dev) -> None:
        """Step B on the host: header, `plan_file_into`, and per wanted tensor its kept chunks, moved
        chunks and the pieces to scatter.  Raises ValueError as `_scatter_file` does."""
        p, size = self.p, int(self.p.f["size"])
        if size < 8:
            raise ValueError(f"{p.f['path']}: too short for a safetensors file")
        (hlen,) = struct.unpack("<Q", self.read(0, 8, buffers, dev))
        if 8 + hlen > size:
            raise ValueError(f"{p.f['path']}: the header reaches past the file")
        self.head = self.read(0, 8 + hlen, buffers, dev)
        start, self.meta = zdev.parse_safetensors_header(self.head)
        self.head = self.head[:start]
        self.table, self.names, self.total = plan_file_into(start, self.meta, wsh, target.dests, size)
        self.kept = np.zeros(p.nchunks, dtype=bool)
        self.moved = np.zeros(p.nchunks, dtype=bool)
        r0 = np.asarray([int(p.t_off[t0]) for t0, _, _ in self.runs], dtype=np.int64)
        r1 = np.asarray([int(p.t_off[t1]) for _, t1, _ in self.runs], dtype=np.int64)
        self.patch_rows, self.moved_rows = [], []  # (offset in the patch, bytes, dst address) / (chunk, offset in it, ..)
        for row in self.table:
            a, n, da = int(row["src_off"]), int(row["run_bytes"]) * int(row["n_runs"]), int(row["dst_addr"])
            if n == 0:
                continue
            idx = np.arange(np.searchsorted(self.cend, a, side="right"), np.searchsorted(self.coff, a + n, side="left"))
            co, ce = self.coff[idx], self.cend[idx]
            res = ~self.fetched[idx]
            home = (np.uint64(da) + (co - a).astype(np.uint64))  # wraps for a chunk that starts before the tensor
            kept = res & (co >= a) & (ce <= a + n) & (self.caddr[idx] == home)
            self.kept[idx[kept]] = True
            self.moved[idx[res & ~kept]] = True
            for c, lo, hi in zip(idx[res & ~kept].tolist(), np.maximum(co, a)[res & ~kept].tolist(),
                                 np.minimum(ce, a + n)[res & ~kept].tolist()):
                self.moved_rows.append((c, lo - int(self.coff[c]), hi - lo, da + lo - a))
            for k in range(int(np.searchsorted(r1, a, side="right")), int(np.searchsorted(r0, a + n, side="left"))):
                lo, hi = max(int(r0[k]), a), min(int(r1[k]), a + n)
                self.patch_rows.append((self.runs[k][2] + lo - int(r0[k]), hi - lo, da + lo - a))

    def counters(self) -> dict:
        p = self.p
        lens = p.chunk_lens.astype(np.int64)
        kept_terms = sum(1 for t in p.src if self.kept[p.t_chunk[t]:p.t_chunk[t + 1]].any())
        return {"kept_terms": kept_terms, "kept_bytes": int(lens[self.kept].sum()),
                "moved_chunks": int(self.moved.sum()), "moved_bytes": int(lens[self.moved].sum()),
                "applied_bytes": sum(r[1] for r in self.patch_rows) + sum(r[2] for r in self.moved_rows)}


def _one_run_table(rows) -> np.ndarray:
    """SCATTER_DTYPE rows that each copy one run: rows = [(src_off, bytes, dst_addr)]."""
    tab = np.zeros(len(rows), dtype=ops.SCATTER_DTYPE)
    for i, (so, n, da) in enumerate(rows):
        tab[i] = (so, n, n, 1, da)
    return tab


def _pull_xet_delta(fetcher, xet: list, dev: torch.device, rs, target: Target, wsh, written: dict, info: dict,
                    scratch_bytes, records: list) -> None:
    """The Xet files of an `into=` pull with a base: see the module docstring.  fetcher: a
    `_hip.DeviceXetPull` (GPU, the caller has made `dev` current) or a `_core.HostXetFetcher` (CPU).

    Counters (info["delta"]): fetched_terms / fetched_bytes: the terms that are not wholly resident;
    kept_bytes: resident chunks that lie wholly inside a wanted tensor, at their place in its
    destination (not touched); moved_chunks / moved_bytes: every other resident chunk that overlaps a
    wanted tensor (gathered whole, re-hashed, its overlap scattered); kept_terms: resident terms with
    a kept chunk; applied_bytes: what the scatters wrote; kept and moved count files
    that went through, not files that fell back; check_s: wall time of the bind (also bind_s), the
    hashing in place, the Merkle check and the gathers, without the fetch."""
    from . import delta as zdelta

    cuda = dev.type == "cuda"
    d = dict.fromkeys(DELTA_KEYS, 0)
    d.update(seam_chunks=rs.seam_chunks, seam_bytes=rs.seam_bytes, check_s=rs.bind_s, bind_s=rs.bind_s, fetch_s=0.0,
             apply_s=0.0, files={})
    info["delta"] = d
    files = []
    for f in xet:  # the reconstructions: which terms the base holds
        df = _DeltaFile(zdelta._FilePlan(f, fetcher.term_keys(f["xet_hash"]), fetcher.term_shapes(f["xet_hash"]), 0, rs))
        files.append(df)
        d["fetched_terms"] += df.p.nterms - int(df.p.reused.sum())
        d["fetched_bytes"] += df.patch
        d["files"][f["path"]] = {"fetched_bytes": df.patch, "kept_bytes": 0, "moved_bytes": 0, "fallback": False}
    slots = [_slot(df.patch) for df in files]
    want = DEFAULT_SCRATCH if scratch_bytes is None else int(scratch_bytes)
    patch_n = min(max(want, max(slots)), sum(slots))  # never below one file's own patch
    groups = _groups([{"size": df.patch, "df": df} for df in files], patch_n)
    info["groups"], info["scratch_bytes"], d["patch_bytes"] = len(groups), patch_n, patch_n

    def alloc(n: int) -> torch.Tensor:
        return ops.padded_empty(n, dev) if cuda else torch.empty(n, dtype=torch.uint8)

    def sync() -> None:
        if cuda:
            torch.cuda.synchronize(dev)

    patch = alloc(patch_n)
    whole = None  # the scratch of the fallbacks: allocated on demand, reused
    timed = []
    for g in groups:
        g = [(e["df"], o) for e, o in g]
        # A: verify without writing
        t_a = time.perf_counter()
        leaf0 = 0
        for df, _ in g:
            df.p.leaf0 = leaf0
            leaf0 += df.p.nchunks
        hashes = torch.zeros((max(leaf0, 1), 32), dtype=torch.uint8, device=dev)
        sizes = torch.zeros(max(leaf0, 1), dtype=torch.int64, device=dev)
        which = [(i, t0, t1) for i, (df, _) in enumerate(g) for t0, t1, _ in df.runs]
        dst = [patch.data_ptr() + o + at for df, o in g for _, _, at in df.runs]
        fetch = zdelta._Fetch([df.p for df, _ in g], None, which, dev, dst)
        sync()  # the tables (and, first, the patch) are visible to the pull's private streams
        src = [(df.p.src[t], df.p.lens[t], np.arange(df.p.leaf0 + df.p.t_chunk[t], df.p.leaf0 + df.p.t_chunk[t + 1]))
               for df, _ in g for t in sorted(df.p.src)]
        if src:  # resident chunks are hashed where they lie, straight into the files' leaf rows
            ops.hash_chunks_at(np.concatenate([s[0] for s in src]), np.concatenate([s[1] for s in src]), hashes,
                               np.concatenate([s[2] for s in src]), sizes, buffers=rs.buffers)
        t_f = time.perf_counter()
        fetch.run(fetcher, hashes, sizes, False)
        d["fetch_s"] += time.perf_counter() - t_f
        t_f = time.perf_counter() - t_f
        sync()
        roots = ops.merkle_roots(hashes, sizes, [(df.p.leaf0, df.p.nchunks) for df, _ in g], file_hash=True).cpu().numpy()
        good = [_core.xet_hex(roots[i].tobytes()) == df.p.f["xet_hash"] for i, (df, _) in enumerate(g)]
        for (df, _), ok in zip(g, good):
            fetcher.settle(df.p.f["xet_hash"], ok)

        # B: plan on the verified bytes; every gather of the group before its first scatter
        refused, claimed = None, set()
        for i, (df, o) in enumerate(g):
            if not good[i]:
                continue
            df.sources(patch.data_ptr() + o)
            try:
                df.plan(wsh, target, rs.buffers + [patch], dev)
                for name in df.names:
                    if name in written or name in claimed:
                        raise ValueError(f"duplicate tensor {name} in {df.p.f['path']}")
                claimed.update(df.names)
            except ValueError as e:  # this file writes nothing; the files before it are still written
                refused, g, good = e, g[:i], good[:i]
                break
        moved = [(i, c) for i, (df, _) in enumerate(g) if good[i] for c in np.flatnonzero(df.moved).tolist()]
        bounce = None
        if moved:
            m_len = np.asarray([g[i][0].p.chunk_lens[c] for i, c in moved], dtype=np.int64)
            m_off = np.cumsum(m_len) - m_len
            where = {ic: int(o) for ic, o in zip(moved, m_off)}
            bounce = alloc(int(m_len.sum()))
            again = torch.zeros((len(moved), 32), dtype=torch.uint8, device=dev)
            ops.reuse_chunks(np.asarray([g[i][0].caddr[c] for i, c in moved], dtype=np.uint64), m_len, bounce, m_off,
                             again, np.arange(len(moved)), buffers=rs.buffers)
            rows = torch.from_numpy(np.asarray([g[i][0].p.leaf0 + c for i, c in moved], dtype=np.int64)).to(dev)
            same = (again == hashes.index_select(0, rows)).all(dim=1).cpu().numpy()
            for (i, _), ok in zip(moved, same):  # the bytes changed between the check and the gather
                good[i] = good[i] and bool(ok)
        d["check_s"] += time.perf_counter() - t_a - t_f

        # C: apply
        t_c = time.perf_counter()
        if cuda:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        for i, (df, o) in enumerate(g):
            if not good[i]:
                continue
            f, bufs = df.p.f, [target.dests[n] for n in df.names]
            ops.slice_scatter(patch[o:o + df.patch], _one_run_table(df.patch_rows), bufs)
            if df.moved_rows:
                ops.slice_scatter(bounce, _one_run_table([(where[(i, c)] + co, n, da) for c, co, n, da in df.moved_rows]),
                                  bufs)
            for name in df.names:
                written[name] = target.dests[name]
            _record(records, f, df.head, df.p.chunk_lens.copy(), df.p.keys, _whole_rows(df.table, df.names, df.meta))
            info["file_bytes"] += int(f["size"])
            info["written_bytes"] += df.total
            info["tensors"] += len(df.names)
            cnt = df.counters()
            for k, v in cnt.items():
                d[k] += v
            d["files"][f["path"]].update(kept_bytes=cnt["kept_bytes"], moved_bytes=cnt["moved_bytes"])
        if cuda:
            ev1.record()
            timed.append((ev0, ev1))
            fetcher.order_after(ev1.cuda_event)  # the next group overwrites the patch these scatters read
        else:
            d["apply_s"] += time.perf_counter() - t_c
        del bounce

        # a file that missed its hash wrote nothing: today's path for that file alone
        for i, (df, _) in enumerate(g):
            if good[i]:
                continue
            f = df.p.f
            if whole is None or whole.numel() < _slot(f["size"]):
                whole = None
                whole = alloc(_slot(f["size"]))
                sync()
            job = [(f["xet_hash"], whole.data_ptr(), f["size"])]
            (r,) = fetcher.pull_files(job) if cuda else fetcher.fetch_files(job)
            _scatter_file(whole[:f["size"]], f["path"], wsh, target, written, info, False,
                          (f, r["chunk_lens"], fetcher.term_keys(f["xet_hash"]), records))
            if cuda:
                ev = torch.cuda.Event()
                ev.record()
                fetcher.order_after(ev.cuda_event)  # a later fallback overwrites this scratch
            d["fallback_files"] += 1
            d["fallback_bytes"] += int(f["size"])
            d["files"][f["path"]]["fallback"] = True
        if refused is not None:
            sync()
            raise refused
    if cuda:
        torch.cuda.synchronize(dev)
        d["apply_s"] += sum(a.elapsed_time(b) for a, b in timed) / 1e3
    info["scatter_s"] += d["apply_s"]


def pull_into(repo, revision, dev, into, sh, scratch_bytes, stats, strict, *, p2p, peers, tracker, dht, dht_bootstrap,
              repo_type, staging_bytes, threads, include, cast=False, base=None):
    """pull_to_device(into=...): see the module docstring.  Returns a Landed, {name: destination} of what
    was written with the record of it, after the device has finished the scatters.  base: a
    `delta.ResidentSet` on `dev`; the Xet files are then updated in place (`_pull_xet_delta`)."""
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
    records: list[FileRecord] = []

    if xet and base is not None:
        if cuda:
            dp = ops.hip().DeviceXetPull(repo, revision, repo_type, *net, dev.index or 0, staging_bytes, threads)
            with torch.cuda.device(dev):
                _pull_xet_delta(dp, xet, dev, base, target, wsh, written, info, scratch_bytes, records)
        else:
            hf = _core.HostXetFetcher(repo, revision, repo_type, *net, threads)
            _pull_xet_delta(hf, xet, dev, base, target, wsh, written, info, scratch_bytes, records)
    elif xet:
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
                    res = dp.pull_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for (f, o), r in zip(g, res):
                        _scatter_file(scratch[o:o + f["size"]], f["path"], wsh, target, written, info, cast,
                                      (f, r["chunk_lens"], dp.term_keys(f["xet_hash"]), records))
                    ev1.record()
                    timed.append((ev0, ev1))
                    dp.order_after(ev1.cuda_event)  # the next group overwrites the scratch these scatters read
                del scratch  # back to torch's allocator, which orders its reuse behind the scatters' stream
        else:
            hf = _core.HostXetFetcher(repo, revision, repo_type, *net, threads)
            scratch = torch.empty(scratch_n, dtype=torch.uint8)
            for g in groups:
                res = hf.fetch_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                t0 = time.perf_counter()
                for (f, o), r in zip(g, res):
                    _scatter_file(scratch[o:o + f["size"]], f["path"], wsh, target, written, info, cast,
                                  (f, r["chunk_lens"], hf.term_keys(f["xet_hash"]), records))
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
    out = Landed(written, IntoRecord(records), dev)
    for name, first in target.aliases.items():
        if first in written:
            out[name] = target.given[name]
    return out
