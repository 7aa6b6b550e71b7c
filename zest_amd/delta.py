"""Delta device pull: reuse the chunks of another revision that are already resident on the device.

    w0 = zest_amd.pull("org/model", "step-100", device="cuda:0")
    w1 = zest_amd.pull("org/model", "step-200", device="cuda:0", base=w0)

Xet dedups chunk by chunk at upload, so the reconstruction of a new revision points into the old
revision's xorbs wherever the bytes did not change.  `ResidentSet` is the map of where those xorb
chunks sit in memory after a direct pull (`seed.plan_resident_runs`, the map resident seeding serves
from); `pull_files_delta` resolves every term of the new files against it.  A term whose whole chunk
range is resident is *reused*: its chunks are copied from the base's memory and re-hashed on the way
(`ops.reuse_chunks`, kernel K12).  Every other term is *fetched* through the usual waterfall
(`DeviceXetPull.pull_terms` / `HostXetFetcher.fetch_terms`).  The waterfall of a device pull becomes
resident -> cache -> P2P -> CDN.

Nothing about the base is trusted: every file's hash is re-derived (`ops.merkle_roots`) from the
hashes of the bytes that landed in the *new* buffers, reused chunks included, and compared with the
file's Xet hash.  A file that misses with reused terms (the base tensors were modified in place) has
exactly those terms fetched from the network and is checked again.

Limits: granularity is the whole term (the CAS cuts terms at every changed chunk); the base must be
on the pull's device (no peer reads); a plain delta pull writes new buffers, so peak memory is old + new
until the caller drops the base (`pull(..., into=model, base=landed)`, zest_amd.into, is the form that
updates a model's own tensors in place and writes only the changed chunks); a resident set does not
outlive its process, so the CLI has no `--base`.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import _core, ops
from . import device as zdev
from .seed import merge_chunk_refs, plan_resident_runs


def _norm_device(device) -> torch.device:
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class ResidentSet:
    """Where the xorb chunks of a finished direct pull sit in memory.

    plan: `{xorb_hex: [(first_chunk, addrs, lens), ...]}` as `seed.plan_resident_runs` returns it
    (runs sorted by first_chunk, uint64 addresses / uint32 sizes); buffers: the uint8 tensors the
    addresses point into, kept alive by the set; device: where they are."""

    def __init__(self, plan: dict, buffers, device):
        self.plan = {hx: sorted(((int(f), np.asarray(a, dtype=np.uint64), np.asarray(ln, dtype=np.uint32))
                                 for f, a, ln in runs), key=lambda r: r[0]) for hx, runs in plan.items()}
        self.buffers = list(buffers)
        self.device = _norm_device(device)
        # what binding an `into=` record cost (zest_amd.into.IntoRecord.bind); zero for every other set
        self.seam_chunks, self.seam_bytes, self.bind_s = 0, 0, 0.0

    @classmethod
    def from_files(cls, files, device) -> "ResidentSet":
        """files: per file `(buffer, chunk_lens, term_keys)`: the uint8 tensor holding the whole decoded
        file, its chunk sizes in file order and its reconstruction terms (see plan_resident_runs)."""
        files = [(b, lens, list(keys)) for b, lens, keys in files]
        return cls(plan_resident_runs([(b.data_ptr(), lens, keys) for b, lens, keys in files]),
                   [b for b, _, _ in files], device)

    def __len__(self) -> int:
        return sum(len(a) for runs in self.plan.values() for _, a, _ in runs)

    @property
    def nbytes(self) -> int:
        return sum(int(ln.sum(dtype=np.uint64)) for runs in self.plan.values() for _, _, ln in runs)

    def lookup(self, xorb_hex: str, c0: int, c1: int):
        """(addrs, lens) of chunks [c0, c1) of the xorb when all of them are resident, else None.  The
        range may be part of a run or span runs that are adjacent in chunk index."""
        runs = self.plan.get(xorb_hex)
        c0, c1 = int(c0), int(c1)
        if not runs or c1 <= c0:
            return None
        addrs, lens, cur = [], [], c0
        for first, a, ln in runs:
            if first > cur:
                return None  # a hole at `cur`
            end = first + len(a)
            if end <= cur:
                continue
            take = min(end, c1)
            addrs.append(a[cur - first:take - first])
            lens.append(ln[cur - first:take - first])
            cur = take
            if cur == c1:
                return np.concatenate(addrs), np.concatenate(lens)
        return None

    def __or__(self, other: "ResidentSet") -> "ResidentSet":
        if not isinstance(other, ResidentSet):
            return NotImplemented
        if other.device != self.device:
            raise ValueError(f"resident sets on different devices ({self.device}, {other.device}) do not merge")
        # a chunk both sets hold keeps this set's copy (the first reference)
        plan = merge_chunk_refs({hx: self.plan.get(hx, []) + other.plan.get(hx, [])
                                 for hx in {**self.plan, **other.plan}})
        seen, bufs = set(), []
        for b in self.buffers + other.buffers:
            if id(b) not in seen:
                seen.add(id(b))
                bufs.append(b)
        out = ResidentSet(plan, bufs, self.device)
        out.seam_chunks, out.seam_bytes = self.seam_chunks + other.seam_chunks, self.seam_bytes + other.seam_bytes
        out.bind_s = self.bind_s + other.bind_s
        return out


def as_resident_set(base, device) -> ResidentSet:
    """The `base=` keyword as one ResidentSet on `device`: a Weights, a ResidentSet, what
    `zest_amd.publish` returned (a Published), what `pull(..., into=...)` returned (a Landed, whose
    record is bound to its destinations as they are now) or a list of those.  Raises ValueError for
    anything else and for a base on another device."""
    dev = _norm_device(device)
    items = list(base) if isinstance(base, (list, tuple)) else [base]
    if not items:
        raise ValueError("base= is empty: pass the Weights of an earlier pull (or leave base= out)")
    from .into import Landed
    from .publish import Published

    out = None
    for b in items:
        if isinstance(b, Landed):
            if b.device != dev:
                raise ValueError(f"base= is resident on {b.device} but the pull targets {dev}: a delta pull copies "
                                 "inside one device; pull the base on that device first (reads from peer GPUs are "
                                 "not supported)")
            b = b.record.bind(b, dev)  # fresh: the seam arena is gathered from the destinations as they are
        rs = b.resident if isinstance(b, (zdev.Weights, Published)) else b
        if not isinstance(rs, ResidentSet):
            what = "Weights of a sharded or snapshot pull" if isinstance(b, zdev.Weights) else type(b).__name__
            raise ValueError(f"base= takes the Weights returned by an unsharded direct pull (device='cuda:N' or "
                             f"'cpu'), their .resident set, or a list of those; got {what}: a plain dict of tensors "
                             "does not say which xorb chunks its bytes are")
        if rs.device != dev:
            raise ValueError(f"base= is resident on {rs.device} but the pull targets {dev}: a delta pull copies "
                             "inside one device; pull the base on that device first (reads from peer GPUs are not "
                             "supported)")
        out = rs if out is None else out | rs
    return out


class _FilePlan:
    """One file of a delta pull: its terms split into reused and fetched."""

    def __init__(self, f: dict, keys, shapes, leaf0: int, rs: ResidentSet):
        self.f, self.keys, self.leaf0 = f, keys, leaf0
        self.nterms = len(keys)
        self.t_off = np.zeros(self.nterms + 1, dtype=np.int64)    # output offset of each term
        self.t_chunk = np.zeros(self.nterms + 1, dtype=np.int64)  # first chunk (file order) of each term
        self.reused = np.zeros(self.nterms, dtype=bool)
        self.src, self.lens = {}, {}  # per reused term: chunk addresses / sizes
        for t, ((hx, c0, c1), (ulen, nch)) in enumerate(zip(keys, shapes)):
            self.t_off[t + 1] = self.t_off[t] + int(ulen)
            self.t_chunk[t + 1] = self.t_chunk[t] + int(nch)
            hit = rs.lookup(hx, c0, c1) if int(c1) - int(c0) == int(nch) else None
            if hit is not None and int(hit[1].sum(dtype=np.uint64)) == int(ulen):
                self.reused[t] = True
                self.src[t], self.lens[t] = hit
        if int(self.t_off[-1]) != int(f["size"]):
            raise zdev.VerifyError(f"{f['path']}: reconstruction covers {int(self.t_off[-1])} bytes, the file has "
                                   f"{f['size']}")
        self.nchunks = int(self.t_chunk[-1])
        self.chunk_lens = np.zeros(self.nchunks, dtype=np.uint32)
        for t, ln in self.lens.items():
            self.chunk_lens[self.t_chunk[t]:self.t_chunk[t + 1]] = ln

    def runs(self, want: bool):
        """Maximal runs [t0, t1) of consecutive terms whose `reused` flag is `want`."""
        out, t = [], 0
        while t < self.nterms:
            if self.reused[t] != want:
                t += 1
                continue
            t1 = t
            while t1 < self.nterms and self.reused[t1] == want:
                t1 += 1
            out.append((t, t1))
            t = t1
        return out


class _Fetch:
    """Term runs `which` = [(file index, t0, t1), ...] of all files, fetched in ONE call (staging
    batches cross file boundaries) into place.  The fetch API wants the jobs' chunks at consecutive
    rows, so they land in a compact table that is then spread over the files' leaf rows.  The tables
    are allocated here and the fetch happens in run(): the caller synchronises the device in between
    (the pull's private streams must see the allocations) and may queue other work before run().
    dst: the address each run lands at, when that is not its place in its file's buffer (the in-place
    pull's compact patch, zest_amd.into); `bufs` is then unused."""

    def __init__(self, plans, bufs, which, dev, dst=None):
        self.plans, self.which, self.dev = plans, which, dev
        self.jobs, self.rows, at = [], [], 0
        for k, (fi, t0, t1) in enumerate(which):
            p = plans[fi]
            to = bufs[fi].data_ptr() + int(p.t_off[t0]) if dst is None else int(dst[k])
            self.jobs.append((p.f["xet_hash"], int(t0), int(t1), to, at))
            self.rows.append(np.arange(p.leaf0 + p.t_chunk[t0], p.leaf0 + p.t_chunk[t1], dtype=np.int64))
            at += int(p.t_chunk[t1] - p.t_chunk[t0])
        self.fh = torch.zeros((at, 32), dtype=torch.uint8, device=dev)
        self.fs = torch.zeros(at, dtype=torch.int64, device=dev)
        self.idx = torch.from_numpy(np.concatenate(self.rows)).to(dev) if which else None

    def run(self, fetcher, hashes, sizes, repair: bool) -> None:
        """share_runs: changed regions of one file are separate terms whose new chunks are neighbours
        in one new xorb, so the CAS covers them with one fetch entry; it is downloaded once."""
        if not self.which:
            return
        cuda = self.dev.type == "cuda"
        if cuda:
            res = fetcher.pull_terms(self.jobs, self.fh.data_ptr(), self.fs.data_ptr(), repair, True)
        else:
            res = fetcher.fetch_terms(self.jobs, self.fh.data_ptr(), repair, True)
        lens = [np.frombuffer(r["chunk_lens"], dtype="<u4") for r in res]
        for (fi, t0, t1), ln in zip(self.which, lens):
            p = self.plans[fi]
            if len(ln) != int(p.t_chunk[t1] - p.t_chunk[t0]):
                raise zdev.VerifyError(f"{p.f['path']}: terms [{t0}, {t1}) came back with {len(ln)} chunks")
            p.chunk_lens[p.t_chunk[t0]:p.t_chunk[t1]] = ln
        if not cuda:
            self.fs.copy_(torch.from_numpy(np.concatenate(lens).astype(np.int64)))
        # (pull_terms returns with its kernels done, so the current stream may read the tables)
        hashes.index_copy_(0, self.idx, self.fh)
        sizes.index_copy_(0, self.idx, self.fs)


def pull_files_delta(fetcher, xet: list, dev: torch.device, rs: ResidentSet, info: dict):
    """The Xet files `xet` (listing dicts) of a new revision into new buffers on `dev`, reusing what
    `rs` holds.  fetcher: a `_hip.DeviceXetPull` (GPU) or `_core.HostXetFetcher` (CPU) of the new
    revision.  Returns [(buffer, chunk_lens, term_keys), ...] per file, every file verified against its
    Xet hash; fills `info` (stats["delta"])."""
    cuda = dev.type == "cuda"
    info.update(reused_terms=0, fetched_terms=0, reused_bytes=0, fetched_bytes=0, reused_files=0, refetched_terms=0,
                reuse_s=0.0, fetch_s=0.0, verify_s=0.0)
    plans, leaf0 = [], 0
    for f in xet:
        p = _FilePlan(f, fetcher.term_keys(f["xet_hash"]), fetcher.term_shapes(f["xet_hash"]), leaf0, rs)
        plans.append(p)
        leaf0 += p.nchunks
        nr = int(p.reused.sum())
        info["reused_terms"] += nr
        info["fetched_terms"] += p.nterms - nr
        rb = sum(int(p.t_off[t + 1] - p.t_off[t]) for t in np.flatnonzero(p.reused))
        info["reused_bytes"] += rb
        info["fetched_bytes"] += int(f["size"]) - rb
        info["reused_files"] += int(nr == p.nterms)
    n_leaves = leaf0
    if cuda:
        bufs = [ops.padded_empty(f["size"], dev)[:f["size"]] for f in xet]
    else:
        bufs = [torch.empty(f["size"], dtype=torch.uint8) for f in xet]
    hashes = torch.zeros((max(n_leaves, 1), 32), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(max(n_leaves, 1), dtype=torch.int64, device=dev)

    fetch = _Fetch(plans, bufs, [(fi, a, b) for fi, p in enumerate(plans) for a, b in p.runs(False)], dev)
    if cuda:
        torch.cuda.synchronize(dev)  # buffers and tables are visible to the pull's private streams

    # reused terms: per file one table (a record's output offset is relative to its file's buffer),
    # queued on the current stream; they run on the GPU while the fetch below moves bytes on the
    # pull's own streams (the two write disjoint bytes and disjoint table rows)
    if cuda:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    t0 = time.perf_counter()
    for p, buf in zip(plans, bufs):
        ts = sorted(p.src)
        if not ts:
            continue
        lens = np.concatenate([p.lens[t] for t in ts]).astype(np.int64)
        offs = np.concatenate([p.t_off[t] + np.cumsum(p.lens[t], dtype=np.int64) - p.lens[t] for t in ts])
        rows = np.concatenate([np.arange(p.leaf0 + p.t_chunk[t], p.leaf0 + p.t_chunk[t + 1]) for t in ts])
        ops.reuse_chunks(np.concatenate([p.src[t] for t in ts]), lens, buf, offs, hashes, rows, sizes,
                         buffers=rs.buffers)
    if cuda:
        ev1.record()
    else:
        info["reuse_s"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    fetch.run(fetcher, hashes, sizes, False)
    info["fetch_s"] = time.perf_counter() - t0
    if cuda:
        torch.cuda.synchronize(dev)  # join: the reuse launches and the pull's streams
        info["reuse_s"] = ev0.elapsed_time(ev1) / 1e3

    def misses():
        roots = ops.merkle_roots(hashes, sizes, [(p.leaf0, p.nchunks) for p in plans], file_hash=True).cpu().numpy()
        return [fi for fi, p in enumerate(plans) if _core.xet_hex(roots[fi].tobytes()) != p.f["xet_hash"]]

    t0 = time.perf_counter()
    bad = misses() if plans else []
    if bad:
        # The new hashes disagree with the file's: if it has reused terms, the base's bytes are no
        # longer what their xorb chunks were (tensors modified in place).  Fetch exactly those terms.
        again = [(fi, a, b) for fi in bad for a, b in plans[fi].runs(True)]
        if again:
            info["refetched_terms"] = sum(b - a for _, a, b in again)
            refetch = _Fetch(plans, bufs, again, dev)
            if cuda:
                torch.cuda.synchronize(dev)
            refetch.run(fetcher, hashes, sizes, True)
            if cuda:
                torch.cuda.synchronize(dev)
            bad = misses()
    for fi, p in enumerate(plans):
        fetcher.settle(p.f["xet_hash"], fi not in bad)
    info["verify_s"] = time.perf_counter() - t0
    if bad:
        p = plans[bad[0]]
        raise zdev.VerifyError(f"{p.f['path']}: bytes do not hash to the file's Xet hash {p.f['xet_hash']}")
    return [(buf, p.chunk_lens, p.keys) for p, buf in zip(plans, bufs)]
