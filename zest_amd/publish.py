"""Publish weights that are resident in memory as a new, deduplicated Xet revision.

    w0 = zest_amd.pull("org/model", "step-100", device="cuda:0")
    index = zest_amd.ChunkIndex.from_weights(w0)      # before the tensors change
    ...                                               # a training step updates w0's tensors in place
    pub = zest_amd.publish(w0, index=index, seed=True)
    pub.manifest                                      # files, reconstruction terms, new xorbs: JSON-able
    ...
    pub2 = zest_amd.publish(w0, index=pub.index)      # step -> step: the index comes from the last call

`publish` is the producing side of the delta pull (zest_amd.delta).  It chunks every file where it
lies (GearHash candidates K5 + the Xet min/max rule), hashes the chunks (K1), finds every chunk the
index already knows or that occurred earlier in the same call (`ops.dedup_chunks`, kernel K13: a
hash join on the device over the 32-byte chunk hashes), packs only the remaining, new chunks into
new xorbs (`_core.plan_xorbs`, xorb hashes by K2) and writes every file's reconstruction as terms
into old and new xorbs (file hashes by K2).  No byte is copied: the returned `.resident` set maps
every xorb chunk the revision references, new or old, to the address in the file buffers where its
bytes lie, and `seed=True` serves them from there as stored (scheme 0) chunks through the resident
seeder (`seed.ResidentSeedServer.from_plan`, K9).  A peer pulls the revision with
`pull(repo, rev, base=its old weights, peers=[publisher])` and fetches only the new chunks; a peer
without the old revision gets everything from the publisher.

A producer that holds loose tensors (a trainer, a merge: every parameter its own allocation)
publishes them where they lie, without packing them into a file first:

    pub = zest_amd.publish({"model.safetensors": zest_amd.TensorFile(model.state_dict())}, seed=True)

The file, byte for byte what `pack_safetensors` would build, then exists only as a list of segments
(a small header tensor, then each tensor's bytes): K14 (`ops.cdc_candidates_segments`) finds the
boundaries over the virtual concatenation, `ops.hash_chunks_at` hashes every chunk at its absolute
address, and only the chunks that cross a tensor boundary (at most one per boundary, 128 KiB each)
are copied, once, into a seam arena that the resident set keeps alive with the tensors.

Limits: a plain uint8 buffer without the 4 KiB tail pad of a pull's buffers is still copied once
per call (`ops._as_padded_u8`); a `TensorFile` on the CPU is packed in host memory; new chunks are
not compressed (resident serving is scheme 0); one device per call; the
manifest is handed to pullers by whoever runs the hub (`zest_amd.testing.FakeHub.add_manifest`):
uploading xorbs and shards to a real Hub CAS is not implemented; there is no CLI form, and an index
lives in its process.
"""
from __future__ import annotations

import contextlib
import json
import struct
import sys
import time
import types
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _core, ops
from . import device as zdev
from .delta import ResidentSet, _norm_device
from .seed import merge_chunk_refs

MAX_XORB_CHUNKS = 8192
HASH_LAUNCH_BYTES = 1 << 30  # chunk bytes per K1 launch, as ops.reuse_chunks: bounds the hash scratch


def _hash_chunks(buf: torch.Tensor, lens: np.ndarray) -> torch.Tensor:
    """Xet chunk hashes of consecutive chunks of `buf` (uint8 [n, 32] on its device), in launches of
    at most HASH_LAUNCH_BYTES."""
    lens = np.asarray(lens, dtype=np.uint32)
    cum = np.cumsum(lens, dtype=np.uint64)
    offs = cum - lens
    cuts = [0] + (np.flatnonzero(np.diff(cum // np.uint64(HASH_LAUNCH_BYTES))) + 1).tolist() + [len(lens)]
    parts = [ops.hash_ranges(buf, offs[a:b], lens[a:b]) for a, b in zip(cuts, cuts[1:]) if b > a]
    return torch.cat(parts) if len(parts) != 1 else parts[0]


class ChunkIndex:
    """What the swarm already has, chunk by chunk: `hashes` (uint8 [M, 32], on the device the join
    runs on), the parallel host arrays `xorb_id` / `chunk` (row r is chunk `chunk[r]` of xorb
    `xorbs[xorb_id[r]]`) and `xorbs`, the xorb hashes as Xet hex.  Rows need not be unique: the first
    row of a hash is the one `publish` refers to.  `a | b` unites two indexes, a's rows first."""

    def __init__(self, hashes: torch.Tensor, xorb_id, chunk, xorbs):
        if hashes.dtype != torch.uint8 or hashes.dim() != 2 or hashes.shape[1] != 32:
            raise ValueError("ChunkIndex: hashes must be a uint8 [M, 32] tensor")
        self.hashes = hashes.contiguous()
        self.xorb_id = np.ascontiguousarray(xorb_id, dtype=np.int64)
        self.chunk = np.ascontiguousarray(chunk, dtype=np.int64)
        self.xorbs = list(xorbs)
        m = self.hashes.shape[0]
        if self.xorb_id.shape != (m,) or self.chunk.shape != (m,):
            raise ValueError("ChunkIndex: xorb_id and chunk must have one entry per hash")
        if m and (self.xorb_id.min() < 0 or self.xorb_id.max() >= len(self.xorbs)):
            raise ValueError("ChunkIndex: xorb_id outside the xorb list")

    @classmethod
    def empty(cls, device) -> "ChunkIndex":
        return cls(torch.empty((0, 32), dtype=torch.uint8, device=device), [], [], [])

    @property
    def device(self) -> torch.device:
        return _norm_device(self.hashes.device)

    def __len__(self) -> int:
        return self.hashes.shape[0]

    def to(self, device) -> "ChunkIndex":
        return ChunkIndex(self.hashes.to(device), self.xorb_id, self.chunk, self.xorbs)

    def __or__(self, other: "ChunkIndex") -> "ChunkIndex":
        if not isinstance(other, ChunkIndex):
            return NotImplemented
        if other.device != self.device:
            raise ValueError(f"chunk indexes on different devices ({self.device}, {other.device}) do not merge: "
                             "move one with .to(device)")
        pos = {hx: i for i, hx in enumerate(self.xorbs)}
        xorbs = list(self.xorbs)
        remap = np.empty(len(other.xorbs), dtype=np.int64)
        for i, hx in enumerate(other.xorbs):
            if hx not in pos:
                pos[hx] = len(xorbs)
                xorbs.append(hx)
            remap[i] = pos[hx]
        return ChunkIndex(torch.cat([self.hashes, other.hashes]),
                          np.concatenate([self.xorb_id, remap[other.xorb_id] if len(other) else other.xorb_id]),
                          np.concatenate([self.chunk, other.chunk]), xorbs)

    @classmethod
    def from_weights(cls, w) -> "ChunkIndex":
        """The index of a direct pull's `Weights`: every chunk of its Xet files, re-hashed from the
        file buffers as they are now, located through the files' reconstruction terms.  Every file's
        Merkle file hash is then compared with the Xet hash the pull verified: an index of bytes that
        were modified since would point peers at xorb chunks that hold other bytes, so a file that no
        longer matches raises VerifyError.  Take the index before modifying the tensors."""
        if not isinstance(w, zdev.Weights) or w._device is None:
            raise ValueError("ChunkIndex.from_weights takes the Weights an unsharded direct pull returned "
                             "(device='cuda:N' or 'cpu')")
        if len(w._meta) != len(w._files):
            raise ValueError("these Weights do not record their files' paths and Xet hashes: pull them again")
        dev = w._device
        if not w._files:
            return cls.empty(dev)
        pos: dict[str, int] = {}
        xorbs, hashes, sizes, xid, cidx, jobs, leaf0 = [], [], [], [], [], [], 0
        for (path, _), (buf, chunk_lens, keys) in zip(w._meta, w._files):
            lens = (np.frombuffer(chunk_lens, dtype="<u4") if isinstance(chunk_lens, (bytes, bytearray, memoryview))
                    else np.asarray(chunk_lens)).astype(np.uint32)
            cur = 0
            for hx, c0, c1 in keys:
                if hx not in pos:
                    pos[hx] = len(xorbs)
                    xorbs.append(hx)
                k = int(c1) - int(c0)
                xid.append(np.full(k, pos[hx], dtype=np.int64))
                cidx.append(np.arange(int(c0), int(c1), dtype=np.int64))
                cur += k
            if cur != len(lens) or int(lens.sum(dtype=np.uint64)) != buf.numel():
                raise ValueError(f"{path}: terms cover {cur} chunks, the file has {len(lens)}")
            hashes.append(_hash_chunks(buf, lens))
            sizes.append(lens.astype(np.int64))
            jobs.append((leaf0, len(lens)))
            leaf0 += len(lens)
        hashes = torch.cat(hashes)
        sizes_d = torch.from_numpy(np.concatenate(sizes)).to(dev)
        roots = ops.merkle_roots(hashes, sizes_d, jobs, file_hash=True).cpu().numpy()
        for (path, want), root in zip(w._meta, roots):
            got = _core.xet_hex(root.tobytes())
            if got != want:
                raise zdev.VerifyError(f"{path}: the bytes in memory hash to {got}, the pull verified {want}: the "
                                       "tensors were modified since; take the index (ChunkIndex.from_weights) "
                                       "before modifying the tensors")
        return cls(hashes, np.concatenate(xid), np.concatenate(cidx), xorbs)


@dataclass
class Published:
    """What `publish` returns.  manifest: the revision's metadata, JSON-able; index: the ChunkIndex
    of every chunk of this revision (its hashes come from this call, so the next publish can take it
    although the tensors keep changing); resident: a `delta.ResidentSet` over the file buffers that
    covers every xorb chunk the revision references; stats: counters and seconds per phase; server:
    the resident seed server when `seed=` asked for one."""
    manifest: dict
    index: ChunkIndex
    resident: ResidentSet
    stats: dict = field(default_factory=dict)
    server: object = None

    @property
    def port(self):
        return self.server.port if self.server is not None else None

    def json(self) -> str:
        return json.dumps(self.manifest, separators=(",", ":"))


def _file_set(files):
    """[(path, buffer)] sorted by path and the device they are on."""
    if isinstance(files, zdev.Weights):
        if files._device is None or not files._files:
            raise ValueError("publish: these Weights hold no Xet file buffers (an empty file set): publish the "
                             "Weights of an unsharded direct pull, or a {path: uint8 tensor} dict")
        if len(files._meta) != len(files._files):
            raise ValueError("publish: these Weights do not record their files' paths: pull them again")
        items = [(path, buf) for (path, _), (buf, _, _) in zip(files._meta, files._files)]
    elif isinstance(files, dict):
        if not files:
            raise ValueError("publish: the file set is empty: pass {path: uint8 tensor holding the whole file} or "
                             "the Weights of a direct pull")
        items = list(files.items())
    else:
        raise ValueError(f"publish takes {{path: uint8 tensor}} or the Weights of a direct pull, got "
                         f"{type(files).__name__}")
    for path, buf in items:
        if isinstance(path, str) and isinstance(buf, TensorFile):
            continue  # validated when it was made
        if not isinstance(path, str) or not isinstance(buf, torch.Tensor):
            raise ValueError("publish: files must map path strings to tensors")
        if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
            raise ValueError(f"publish: {path} must be a contiguous 1-D uint8 tensor holding the whole file "
                             "(pack_safetensors builds one from loose tensors, TensorFile publishes them "
                             "where they lie)")
        if buf.numel() == 0:
            raise ValueError(f"publish: {path} is empty: an empty file has no chunks to publish; leave it out")
    devs = {_norm_device(b.device) for _, b in items}
    if len(devs) > 1:
        raise ValueError(f"publish: files on more than one device ({', '.join(sorted(map(str, devs)))}): one call "
                         "publishes from one device; move the files to one device or publish per device")
    return sorted(items, key=lambda it: it[0]), devs.pop()


def publish(files, *, index: ChunkIndex | None = None, seed=False, max_xorb_bytes: int = 64 << 20,
            stats: dict | None = None) -> Published:
    """Publish files that lie in memory as a new Xet revision, deduplicated against `index`.

    files: `{path: contiguous uint8 tensor holding the whole file, or a TensorFile of loose
    tensors}`, all on one device and freely mixed, or a
    `Weights`, whose file buffers and recorded paths are published in their current state (tensors
    updated in place are the normal case; only its Xet-backed files have buffers, small plain files
    of the repository are the hub's to carry over).  index: the `ChunkIndex` of what the swarm already has
    (None: nothing).  Files are processed in sorted path order, so the result is deterministic.  A
    chunk the index knows becomes a reference to its old xorb; a chunk repeated across or within the
    files is stored once; the rest is packed into new xorbs of at most `max_xorb_bytes` serialized
    bytes and 8192 chunks, uncompressed.  Nothing is copied, except, for a `TensorFile`, the few
    chunks that cross a tensor boundary (into a seam arena, at most 128 KiB per boundary).

    seed=True (or a port): `.resident` is served to BEP XET peers by a resident seed server,
    registered like a pull's (`zest_amd.seed.active()`, `stop_all()`).  The seeded buffers must stay
    read-only until the server stops, as for every resident seeder: bytes changed in place no longer
    match their chunk hashes and receivers drop them.  A training loop publishes clones, or stops
    the server before the next step.

    stats (and `.stats`): files, bytes, chunks, new / matched (found in the index) / duplicate
    (repeated in this call) chunks and bytes, new_xorbs, and seconds per phase (cdc, select, hash,
    dedup, plan, merkle).  With a `TensorFile` on a GPU also segments, seam_chunks, seam_bytes and
    the phase seam (classifying the chunks and copying the seam pieces)."""
    from . import seed as zseed

    items, dev = _file_set(files)
    cuda = dev.type == "cuda"
    port = zseed.seed_port(seed)
    if port is not None and not cuda:
        raise ValueError(f"publish: seed= serves from GPU memory, these files are on {dev}: publish from "
                         "device='cuda:N' tensors to seed, or hand the bytes to the hub yourself")
    if index is not None:
        if not isinstance(index, ChunkIndex):
            raise ValueError("publish: index= takes a ChunkIndex (ChunkIndex.from_weights, or an earlier "
                             "Published.index)")
        if index.device != dev:
            raise ValueError(f"publish: the index is on {index.device} but the files are on {dev}: the join runs on "
                             "one device; move the index with index.to(device)")
    if index is None:
        index = ChunkIndex.empty(dev)
    loose = any(isinstance(b, TensorFile) for _, b in items)
    if loose and not cuda:  # host memory is not the scarce resource: pack there, then the buffer path
        items, loose = [(p, b.pack() if isinstance(b, TensorFile) else b) for p, b in items], False
    sec = dict.fromkeys(("cdc", "select", "hash", "dedup", "plan", "merkle") + (("seam",) if loose else ()), 0.0)

    def lap(key: str, t0: float) -> float:
        if cuda:
            torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        sec[key] += t1 - t0
        return t1

    with torch.cuda.device(dev) if cuda else contextlib.nullcontext():
        # 1 + 2: chunk boundaries and chunk hashes, file by file.  A TensorFile is chunked over its
        # segment list (K14) and its chunks are placed and hashed after the loop, when the call's seam
        # arena and leaf table can be sized.
        lens_f, hashes_f, addr_f, segs_f, place_f = [], [], [], {}, {}
        for i, (path, buf) in enumerate(items):
            n = buf.numel()
            t = time.perf_counter()
            if isinstance(buf, TensorFile):
                segs_f[i] = segs = buf.segments()
                cands = ops.cdc_candidates_segments(segs)
                t = lap("cdc", t)
                ends = ops.select_chunks(cands, n)
                lens = np.diff(np.concatenate([[0], ends]).astype(np.uint64)).astype(np.uint32)
                t = lap("select", t)
                place_f[i] = classify_chunks([s.numel() for s in segs], ends)
                lap("seam", t)
                hashes_f.append(None)
                addr_f.append(None)
                lens_f.append(lens)
                continue
            if cuda:
                src = ops._as_padded_u8(buf)  # a pull's buffers are padded; others are copied once, for both kernels
                cands = ops.cdc_candidates(src)
                t = lap("cdc", t)
                ends = ops.select_chunks(cands, n)
            else:
                src = buf
                ends = np.asarray(_core.chunk_ends(buf.numpy()), dtype=np.uint64)  # the host chunker: scan + rule
                t = lap("cdc", t)
            lens = np.diff(np.concatenate([[0], ends]).astype(np.uint64)).astype(np.uint32)
            t = lap("select", t)
            hashes_f.append(_hash_chunks(src, lens))
            lap("hash", t)
            lens_f.append(lens)
            addr_f.append(np.uint64(buf.data_ptr()) + (np.cumsum(lens, dtype=np.uint64) - lens))
            del src
        counts = [len(ln) for ln in lens_f]
        leaf0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        lens = np.concatenate(lens_f)
        arena = None
        if loose:
            # seam chunks, the few that cross a segment boundary, are copied piece by piece into one arena
            # for the call; every other chunk keeps its address in its tensor
            t = time.perf_counter()
            seam_bytes = sum(pl["seam_bytes"] for pl in place_f.values())
            arena = ops.padded_empty(seam_bytes, dev) if seam_bytes else None
            at = 0
            for i, pl in place_f.items():
                segs = segs_f[i]
                for sg, so, ln, do in zip(pl["piece_seg"].tolist(), pl["piece_off"].tolist(),
                                          pl["piece_len"].tolist(), pl["piece_dst"].tolist()):
                    arena[at + do:at + do + ln].copy_(segs[sg][so:so + ln])
                base = np.asarray([s.data_ptr() for s in segs], dtype=np.uint64)
                addr = base[pl["seg"]] + pl["off"]
                if pl["seam_chunks"]:
                    addr[pl["seam"]] = np.uint64(arena.data_ptr() + at) + pl["arena_off"][pl["seam"]]
                addr_f[i] = addr
                at += pl["seam_bytes"]
            t = lap("seam", t)
            # the call's leaf table: rows of plain buffers are copied in, rows of loose files are hashed
            # at their addresses straight into it
            hashes = torch.empty((len(lens), 32), dtype=torch.uint8, device=dev)
            for i, h in enumerate(hashes_f):
                if h is not None:
                    hashes[int(leaf0[i]):int(leaf0[i + 1])].copy_(h)
            at_rows = np.concatenate([np.arange(leaf0[i], leaf0[i + 1], dtype=np.int64) for i in place_f])
            ops.hash_chunks_at(np.concatenate([addr_f[i] for i in place_f]),
                               np.concatenate([lens_f[i] for i in place_f]), hashes, at_rows,
                               buffers=[s for i in place_f for s in segs_f[i]] + ([arena] if arena is not None else []))
            del hashes_f
            lap("hash", t)
        else:
            hashes = torch.cat(hashes_f) if len(hashes_f) != 1 else hashes_f[0]
        N, m = len(lens), len(index)

        # 3: the join over (index, every file's chunks)
        t = time.perf_counter()
        ref = ops.dedup_chunks(index.hashes, hashes).cpu().numpy()
        t = lap("dedup", t)

        # 4: new rows, in order, into xorbs
        own = m + np.arange(N, dtype=np.int64)
        is_new, is_old = ref == own, ref < m
        new_rows = np.flatnonzero(is_new)
        xorb_of = np.asarray(_core.plan_xorbs(lens[new_rows].astype(np.uint64) + np.uint64(8), int(max_xorb_bytes),
                                              MAX_XORB_CHUNKS), dtype=np.int64)
        x_first = np.flatnonzero(np.concatenate([[True], xorb_of[1:] != xorb_of[:-1]])) if len(xorb_of) else \
            np.zeros(0, np.int64)
        x_count = np.diff(np.concatenate([x_first, [len(xorb_of)]]))
        t = lap("plan", t)

        # 5 + 6: xorb hashes over the compacted new rows, file hashes over each file's leaves
        sizes_d = torch.from_numpy(lens.astype(np.int64)).to(dev)
        if len(new_rows):
            sel = torch.from_numpy(new_rows).to(dev)
            xroots = ops.merkle_roots(hashes.index_select(0, sel), sizes_d.index_select(0, sel),
                                      [(int(a), int(k)) for a, k in zip(x_first, x_count)], file_hash=False)
            new_hex = [_core.xet_hex(r.tobytes()) for r in xroots.cpu().numpy()]
        else:
            new_hex = []
        froots = ops.merkle_roots(hashes, sizes_d, [(int(leaf0[i]), counts[i]) for i in range(len(items))],
                                  file_hash=True).cpu().numpy()
        t = lap("merkle", t)

    # where every chunk of the revision lives: (xorb, chunk index) per row
    xorbs = list(index.xorbs) + new_hex
    loc_x, loc_c = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.int64)
    loc_x[new_rows] = len(index.xorbs) + xorb_of
    loc_c[new_rows] = np.arange(len(new_rows), dtype=np.int64) - np.repeat(x_first, x_count)
    old_rows = np.flatnonzero(is_old)
    loc_x[old_rows], loc_c[old_rows] = index.xorb_id[ref[old_rows]], index.chunk[ref[old_rows]]
    dup_rows = np.flatnonzero(~is_new & ~is_old)  # an earlier fresh row, which is a new one
    loc_x[dup_rows], loc_c[dup_rows] = loc_x[ref[dup_rows] - m], loc_c[ref[dup_rows] - m]

    # 7: per file, terms as maximal runs of chunks that are consecutive in one xorb
    man_files, refs, bufs = [], {}, []
    for i, (path, buf) in enumerate(items):
        a, b = int(leaf0[i]), int(leaf0[i + 1])
        x, c, ln = loc_x[a:b], loc_c[a:b], lens[a:b]
        cuts = np.concatenate([[0], np.flatnonzero((x[1:] != x[:-1]) | (c[1:] != c[:-1] + 1)) + 1, [b - a]])
        terms = [[xorbs[int(x[s])], int(c[s]), int(c[e - 1]) + 1, int(ln[s:e].sum(dtype=np.uint64))]
                 for s, e in zip(cuts, cuts[1:])]
        man_files.append({"path": path, "size": int(buf.numel()), "xet_hash": _core.xet_hex(froots[i].tobytes()),
                          "terms": terms})
        cur = 0
        for hx, c0, c1, _ in terms:  # as seed.plan_resident_runs, over per-chunk addresses
            refs.setdefault(hx, []).append((c0, addr_f[i][cur:cur + c1 - c0], ln[cur:cur + c1 - c0]))
            cur += c1 - c0
        bufs += segs_f[i] if i in segs_f else [buf]
    manifest = {"version": 1, "files": man_files,
                "xorbs": {hx: {"chunk_lens": [int(v) for v in lens[new_rows[a:a + k]]]}
                          for hx, a, k in zip(new_hex, x_first, x_count)}}
    sec["plan"] += time.perf_counter() - t  # host work: locations, terms, manifest

    used, inv = np.unique(loc_x, return_inverse=True)  # the next index names only xorbs this revision references
    out_index = ChunkIndex(hashes, inv.reshape(-1), loc_c, [xorbs[int(u)] for u in used])
    resident = ResidentSet(merge_chunk_refs(refs), bufs + ([arena] if arena is not None else []), dev)
    nbytes = lambda rows: int(lens[rows].sum(dtype=np.uint64))
    info = {"files": len(items), "bytes": int(lens.sum(dtype=np.uint64)), "chunks": N,
            "new_chunks": len(new_rows), "matched_chunks": len(old_rows), "duplicate_chunks": len(dup_rows),
            "new_bytes": nbytes(new_rows), "matched_bytes": nbytes(old_rows), "duplicate_bytes": nbytes(dup_rows),
            "new_xorbs": len(new_hex), "seconds": sec}
    if loose:
        info.update(segments=sum(len(sg) for sg in segs_f.values()),
                    seam_chunks=sum(pl["seam_chunks"] for pl in place_f.values()),
                    seam_bytes=sum(pl["seam_bytes"] for pl in place_f.values()))
    if stats is not None:
        stats.update(info)
    pub = Published(manifest, out_index, resident, info)
    if port is not None:
        pub.server = zseed.ResidentSeedServer.from_plan(resident.plan, resident.buffers, dev, port)
        zseed._active.append(pub.server)
    return pub


_ST_NAMES = {v: k for k, v in zdev.ST_DTYPES.items()}


def _safetensors_header(tensors: dict, metadata: dict | None, what: str) -> tuple[bytes, int]:
    """The first bytes of the safetensors file of `tensors` in dict order (8-byte length, JSON header
    padded with spaces to a multiple of 8) and the size of the data that follows."""
    head, off = {}, 0
    if metadata:
        head["__metadata__"] = {str(k): str(v) for k, v in metadata.items()}
    for name, t in tensors.items():
        dt = _ST_NAMES.get(t.dtype)
        if dt is None:
            raise ValueError(f"{what}: {name}: dtype {t.dtype} has no safetensors name")
        n = t.numel() * t.element_size()
        head[name] = {"dtype": dt, "shape": list(t.shape), "data_offsets": [off, off + n]}
        off += n
    hb = json.dumps(head, separators=(",", ":")).encode()
    hb += b" " * (-len(hb) % 8)
    return struct.pack("<Q", len(hb)) + hb, off


def pack_safetensors(tensors: dict, metadata: dict | None = None) -> torch.Tensor:
    """One safetensors file in memory from loose tensors: a uint8 buffer on the tensors' device
    holding the header and every tensor's bytes in dict order (plain copies, no kernel; on a GPU the
    buffer is padded for the kernels that read it).  It costs a second copy of the tensors:
    `publish({path: TensorFile(tensors)})` publishes the same file from where the tensors lie."""
    if not tensors:
        raise ValueError("pack_safetensors: no tensors")
    devs = {_norm_device(t.device) for t in tensors.values()}
    if len(devs) > 1:
        raise ValueError("pack_safetensors: tensors on more than one device")
    dev = devs.pop()
    head, off = _safetensors_header(tensors, metadata, "pack_safetensors")
    total = len(head) + off
    buf = ops.padded_empty(total, dev) if dev.type == "cuda" else torch.empty(total, dtype=torch.uint8)
    buf[:len(head)].copy_(torch.frombuffer(bytearray(head), dtype=torch.uint8))
    at = len(head)
    for t in tensors.values():
        n = t.numel() * t.element_size()
        if n:
            buf[at:at + n].copy_(t.contiguous().reshape(-1).view(torch.uint8))
        at += n
    return buf


class TensorFile:
    """One safetensors file made of loose tensors, published where they lie.

    `publish({path: TensorFile(tensors, metadata)})` publishes the file `pack_safetensors(tensors,
    metadata)` would build, byte for byte (8-byte length, JSON header padded to 8, the tensors in
    dict order), without building it: on a GPU the file is a list of segments, one small device
    tensor for the header bytes and then every tensor's bytes at their own address.  Zero-element
    tensors contribute no segment; tensors that share storage (tied weights) are ordinary segments.
    The tensors must be contiguous, on one device and of dtypes safetensors can name.  On the CPU
    the file is packed in host memory, which is not the scarce resource, and goes down the buffer
    path."""

    def __init__(self, tensors: dict, metadata: dict | None = None):
        if not isinstance(tensors, dict) or not tensors:
            raise ValueError("TensorFile: no tensors: pass a non-empty {name: tensor} dict (an empty file has no "
                             "chunks to publish; leave it out)")
        for name, t in tensors.items():
            if not isinstance(name, str) or not isinstance(t, torch.Tensor):
                raise ValueError("TensorFile: tensors must map name strings to tensors")
            if not t.is_contiguous():
                raise ValueError(f"TensorFile: {name} is not contiguous: its bytes are published where they lie, so "
                                 "pass tensor.contiguous() (a copy of that tensor only) or the storage it is a view of")
        devs = {_norm_device(t.device) for t in tensors.values()}
        if len(devs) > 1:
            raise ValueError(f"TensorFile: tensors on more than one device ({', '.join(sorted(map(str, devs)))}): "
                             "one file is published from one device; move the tensors to one device")
        self.tensors = dict(tensors)
        self.metadata = dict(metadata) if metadata else None
        self.device = devs.pop()
        self.header, data = _safetensors_header(self.tensors, self.metadata, "TensorFile")
        self.nbytes = len(self.header) + data

    def numel(self) -> int:
        return self.nbytes

    def pack(self) -> torch.Tensor:
        """The file as one buffer (`pack_safetensors`): a copy."""
        return pack_safetensors(self.tensors, self.metadata)

    def segments(self) -> list:
        """The file as flat uint8 tensors in file order: a new tensor on the tensors' device holding
        the header bytes, then a view of every tensor that has bytes."""
        head = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(self.device)
        return [head] + [ops._flat_u8(t) for t in self.tensors.values() if t.numel()]


def classify_chunks(seg_lens, chunk_ends) -> dict:
    """Where the chunks of a segmented file lie.  seg_lens: the segments' sizes in file order
    (empty segments are allowed and hold nothing); chunk_ends: the chunks' sorted END offsets, the
    last one the file size.  Pure NumPy.

    A chunk whose bytes lie inside one segment is read there: `seg[c]`, `off[c]` = the segment of its
    first byte and its offset in it.  A chunk that crosses one or more segment boundaries is a seam
    chunk (`seam[c]`): its pieces `(piece_chunk, piece_seg, piece_off, piece_len, piece_dst)`, in file
    order, are to be copied to offsets `piece_dst` of an arena of `seam_bytes` bytes, where seam chunk
    c then lies in one piece at `arena_off[c]`.  A chunk that ends exactly on a boundary crosses
    nothing.  Every seam chunk crosses at least one boundary, no boundary is crossed by two chunks and
    a chunk is at most 128 KiB, so seam_bytes <= 128 KiB * (segments with bytes - 1)."""
    seg_lens = np.asarray(seg_lens, dtype=np.uint64).reshape(-1)
    ends = np.asarray(chunk_ends, dtype=np.uint64).reshape(-1)
    vend = np.cumsum(seg_lens, dtype=np.uint64)
    vstart = vend - seg_lens
    n = int(vend[-1]) if len(vend) else 0
    if len(ends) and (int(ends[-1]) != n or (np.diff(ends.astype(np.int64)) <= 0).any() or int(ends[0]) == 0):
        raise ValueError(f"classify_chunks: chunk ends must increase strictly up to the file size {n}")
    if not len(ends) and n:
        raise ValueError(f"classify_chunks: no chunks for a file of {n} bytes")
    starts = np.concatenate([np.zeros(1, np.uint64), ends[:-1]]) if len(ends) else ends
    # the segment that holds byte p: the last one that starts at or before p (an empty segment shares
    # its start with the next one, which is later in the list)
    first = np.searchsorted(vstart, starts, side="right").astype(np.int64) - 1
    last = np.searchsorted(vstart, ends - np.uint64(1), side="right").astype(np.int64) - 1
    seam = last > first
    rows = np.flatnonzero(seam)
    k = (last - first + 1)[rows]
    pc = np.repeat(rows, k)  # one piece per segment a seam chunk touches, empty segments included for now
    ps = np.repeat(first[rows], k) + (np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k))
    lo = np.maximum(starts[pc], vstart[ps])
    hi = np.minimum(ends[pc], vend[ps])
    live = hi > lo
    pc, ps, lo, hi = pc[live], ps[live], lo[live], hi[live]
    plen = hi - lo
    arena_off = np.zeros(len(ends), dtype=np.uint64)
    clen = (ends - starts)[rows]
    arena_off[rows] = np.cumsum(clen, dtype=np.uint64) - clen  # seam chunks back to back
    return {"seg": first, "off": starts - vstart[first] if len(ends) else starts, "seam": seam,
            "piece_chunk": pc, "piece_seg": ps, "piece_off": lo - vstart[ps], "piece_len": plen,
            "piece_dst": arena_off[pc] + (lo - starts[pc]), "arena_off": arena_off,
            "seam_chunks": int(seam.sum()), "seam_bytes": int(clen.sum(dtype=np.uint64))}


def classify_chunks_with_holes(seg_lens, seg_hole, chunk_ends) -> dict:
    """`classify_chunks` for a file of which only some segments are in memory.  seg_hole: per segment,
    True where its bytes are nowhere (a hole).  A chunk that touches a byte of a hole is not resident
    (`resident[c]` is False): it is no seam chunk, has no pieces and no arena bytes, and its `seg` /
    `off` mean nothing.  Every other chunk is placed as classify_chunks places it, the seam chunks back
    to back in an arena of `seam_bytes` bytes that counts resident seam chunks only, so the bound
    seam_bytes <= 128 KiB * (segment boundaries) still holds."""
    seg_lens = np.asarray(seg_lens, dtype=np.uint64).reshape(-1)
    hole = np.asarray(seg_hole, dtype=bool).reshape(-1)
    if len(hole) != len(seg_lens):
        raise ValueError("classify_chunks_with_holes: one hole flag per segment")
    pl = classify_chunks(seg_lens, chunk_ends)
    ends = np.asarray(chunk_ends, dtype=np.uint64).reshape(-1)
    starts = np.concatenate([np.zeros(1, np.uint64), ends[:-1]]) if len(ends) else ends
    vstart = np.cumsum(seg_lens, dtype=np.uint64) - seg_lens
    hole_len = np.where(hole, seg_lens, np.uint64(0))
    before = np.cumsum(hole_len, dtype=np.uint64) - hole_len  # hole bytes before each segment

    def hole_bytes_below(p):  # hole bytes in [0, p)
        s = np.maximum(np.searchsorted(vstart, p, side="right").astype(np.int64) - 1, 0)
        return before[s] + np.where(hole[s], np.minimum(p - vstart[s], seg_lens[s]), np.uint64(0))

    resident = hole_bytes_below(ends) == hole_bytes_below(starts) if len(ends) else np.zeros(0, dtype=bool)
    seam = pl["seam"] & resident
    keep = resident[pl["piece_chunk"]]
    rows = np.flatnonzero(seam)
    clen = (ends - starts)[rows]
    arena_off = np.zeros(len(ends), dtype=np.uint64)
    arena_off[rows] = np.cumsum(clen, dtype=np.uint64) - clen
    pc, lo = pl["piece_chunk"][keep], (pl["piece_off"] + vstart[pl["piece_seg"]])[keep]
    return {"seg": pl["seg"], "off": pl["off"], "seam": seam, "resident": resident,
            "piece_chunk": pc, "piece_seg": pl["piece_seg"][keep], "piece_off": pl["piece_off"][keep],
            "piece_len": pl["piece_len"][keep], "piece_dst": arena_off[pc] + (lo - starts[pc]), "arena_off": arena_off,
            "seam_chunks": int(seam.sum()), "seam_bytes": int(clen.sum(dtype=np.uint64))}


class _CallableModule(types.ModuleType):
    """`zest_amd.publish` names this module once it is imported and the function before: calling the
    module publishes, so `zest_amd.publish(files, ...)` works either way."""

    def __call__(self, *a, **kw):
        return publish(*a, **kw)


sys.modules[__name__].__class__ = _CallableModule
